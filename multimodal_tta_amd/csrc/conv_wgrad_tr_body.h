// The body of wgrad_tr_kernel and wgrad_tr_raw_kernel (conv_wgrad.hip): included inside each kernel, which names TZ, TY, SI,
// GBF, DBF, TD, NB and the raw-staging flags RG, RD as compile-time constants and has the kernel argument `WArgs a`.  One text
// and no function in between: these kernels sit at their register limit, and wgrad_tr_kernel must compile to exactly what it
// was before the second kernel existed (conv_igemm_body.h does the same).  No include guard on purpose.
// RG / RD: the gathered / the dense operand is bf16-stored and takes no transform (host: wgrad_raw_bits) - its 16-byte items
// go to LDS as loaded, under their masks.  Every RG / RD site is an `if constexpr`.
// UPD (wgrad_tr_upd_kernel; MMTTA_OPT_WGRAD_EPILOGUE_UPDATE): the kernel also has `UpdArgs u`, `PSets ps` and the optimizer
// KIND, and ends in the fused update of its block instead of the slab stores.  One `if constexpr` at the end of the text.
  using G = WTGeo<TZ, TY, SI>;
  static_assert(TY % 2 == 0, "a k step is two rows of one z slice");
  static_assert((!RG || GBF) && (!RD || DBF), "raw staging copies bf16-stored items");
  constexpr bool NEEDC = TD ? !RD : !RG;      // the module-input side is transformed: its coefficients are fetched
  extern __shared__ float lds[];
  unsigned char* gl = reinterpret_cast<unsigned char*>(lds);
  unsigned char* dl = gl + G::G_BYTES;                  // NB dense images back to back
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, r = lane & 31;
  const int cg0 = blockIdx.y * 32, cd0 = blockIdx.z * 32 * NB;

  // operand addresses: lane part (group row q, 8-byte column chunk, row half) + tap (A only)
  const int lq = (lane & 15) >> 2, lp = lane & 3, lc = (lane >> 4) & 1;
  const unsigned char* dread = dl + (h * 8 + lq) * 64 + lc * 32 + lp * 8;
  const unsigned char* gread[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const int tap = min(wave + 4 * j, 26);
    gread[j] = gl + (h * SI * G::BX + lq) * 64 + lc * 32 + lp * 8 + G::tap_off(tap);
  }
  f32x16 acc[NB][7];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int j = 0; j < 7; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[nb][j][i] = 0.f;
  float dbs[NB][8];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int c = 0; c < 8; ++c) dbs[nb][c] = 0.f;
  const bool want_db = a.dbpart != nullptr && blockIdx.y == 0;

  // ---- staging roles (per-thread constants)
  const int rsub = min(tid / G::IPR, G::RPP - 1);                // box row inside a pass
  const int rem = tid % G::IPR, bx = rem >> 2, c8 = rem & 3;     // box x, 8-channel chunk
  const int bxm = SI == 1 ? bx : (bx & 1) * G::XH + (bx >> 1);
  unsigned char* gst = gl + (rsub * G::BX + bxm) * 64 + c8 * 16;  // + pass * RPP * BX * 64
  const int dvox0 = tid >> 2, d8 = tid & 3;                      // dense item p: voxel dvox0 + 64 p, chunk d8
  unsigned char* dst = dl + dvox0 * 64 + d8 * 16;                // + p * 4096
  const int dzl = dvox0 / (TY * 8), dyl = (dvox0 >> 3) % TY, dxl = dvox0 & 7;     // (pass p adds 64 / (TY * 8) to z)
  const int gcb = cg0 + 8 * c8, dcb = cd0 + 8 * d8;               // (dense column block nb: + 32 nb)
  // clamped (always valid) load channels; rows of bf16 tensors are padded to 8 channels, of fp32 tensors to 4
  const unsigned gc_lo = GBF ? min(gcb, (a.Cg - 1) & ~7) : min(gcb, (a.Cg - 1) & ~3), gc_hi = min(gcb + 4, (a.Cg - 1) & ~3);
  const unsigned dc_lo = DBF ? min(dcb, (a.Cd - 1) & ~7) : min(dcb, (a.Cd - 1) & ~3), dc_hi = min(dcb + 4, (a.Cd - 1) & ~3);
  // (column block 1 of a pair is whole: the host pairs blocks only when CDp / 32 is even and rows are padded to 8 channels)
  const unsigned dc_lo1 = DBF ? min(dcb + 32, (a.Cd - 1) & ~7) : min(dcb + 32, (a.Cd - 1) & ~3), dc_hi1 = min(dcb + 36, (a.Cd - 1) & ~3);
  const bool gtail = (a.Cg & 7) != 0, dtail = (a.Cd & 7) != 0;  // only then can a chunk hold channels past the last one
  auto pair_mask = [](int c, int C) { return (c < C ? 0xffffu : 0u) | (c + 1 < C ? 0xffff0000u : 0u); };
  const unsigned gsd = (unsigned)a.gsd, gsh = (unsigned)a.gsh, gsw = (unsigned)a.gsw;
  const unsigned dsd = (unsigned)a.dsd, dsh = (unsigned)a.dsh, dsw = (unsigned)a.dsw;

  // slab sx = slab (sx % S) of parameter set (sx / S): a set's slabs cover ITS batch items only, in the order a launch of
  // those items alone would use (the reduce kernels then sum a set's rows in that same order)
  const int sx = (int)xcd_contiguous_id(blockIdx.x, gridDim.x);
  const int qset = sx / a.S, sls = sx - qset * a.S;
  const int t0 = qset * a.tiles_set + sls * a.tiles_per_split;
  const int t1 = min((qset + 1) * a.tiles_set, t0 + a.tiles_per_split);
  const int tpn = a.tz * a.ty * a.tx;
  constexpr int GP = G::GP, DP = G::DP;
  constexpr int PREF = (GBF || DBF) ? 40 : 32;                         // registers the cross-loop prefetch may hold
  constexpr int PGmax = (PREF - NB * DP * (DBF ? 4 : 8)) / (GBF ? 4 : 8);
  constexpr int PG = PGmax < 0 ? 0 : (PGmax < GP ? PGmax : GP);        // box passes prefetched across the MFMA loop
  Oct8<GBF> gv[GP];
  Oct8<DBF> dq[NB * DP];
  unsigned pok = 0u;                             // bit p: box item of pass p lies inside the tensor
  unsigned dok = 0u;                             // bit p: dense item p lies inside the tensor
  int pn = -1, poz0 = 0, poy0 = 0, pox0 = 0;     // tile whose loads are in gv[0..PG) / dq
  int cn = -1;                                   // batch item the transform coefficients belong to
  float* coefl = reinterpret_cast<float*>(dl + NB * G::D_BYTES);     // [NB][2][32]: scale, shift of the module-input channels
  const float relu_lo = act_lo(TD ? a.td.relu : a.tg.relu);
  unsigned gxoff = 0u;                           // per tile: x / channel part of the box offsets, x in bounds
  bool gxok = false;

  auto tile_x = [&](int ix0) {
    const int ix = ix0 + bx;
    gxok = (unsigned)ix < (unsigned)a.Wgg;
    gxoff = __umul24((unsigned)min(max(ix, 0), a.Wgg - 1), gsw);
  };
  auto load_g = [&](auto pc, const float* gbase, int iz0, int iy0) {
    constexpr int P = decltype(pc)::value;
    constexpr int row0 = G::RPP * P, bz0 = row0 / G::BY, by0 = row0 % G::BY;
    constexpr bool can_wrap = by0 + G::RPP > G::BY;
    int by = by0 + rsub;
    bool wrap = false;
    if constexpr (can_wrap) {
      wrap = by >= G::BY;
      by = wrap ? by - G::BY : by;
    }
    const int izA = iz0 + bz0, izB = izA + 1;                    // wave-uniform candidates
    const unsigned zoA = __umul24((unsigned)min(max(izA, 0), a.Dgg - 1), gsd), zoB = __umul24((unsigned)min(max(izB, 0), a.Dgg - 1), gsd);
    const bool zkA = (unsigned)izA < (unsigned)a.Dgg, zkB = (unsigned)izB < (unsigned)a.Dgg;
    const unsigned zo = (can_wrap && wrap) ? zoB : zoA;
    const bool zk = (can_wrap && wrap) ? zkB : zkA;
    const int iy = iy0 + by;
    const bool ok = zk && gxok && (unsigned)iy < (unsigned)a.Hgg;
    pok |= (ok ? 1u : 0u) << P;
    const unsigned off = zo + __umul24((unsigned)min(max(iy, 0), a.Hgg - 1), gsh) + gxoff;
    gv[P] = oct8_ld<GBF>(gbase, off + gc_lo, off + gc_hi);
  };
  auto commit_g = [&](auto pc, const float (&sc)[8], const float (&sh)[8]) {
    constexpr int P = decltype(pc)::value;
    unsigned okm = ((pok >> P) & 1u) ? 0xffffffffu : 0u;
    uint4 pk;
    if constexpr (RG) {      // the item as loaded, under its masks
      // (a chunk past the module input's last one re-read the last valid chunk: the transform blanks it through zero
      // coefficients, here the mask does; a gradient operand keeps what it re-read in both kernels - those slab rows are
      // never reduced)
      if constexpr (!TD) okm = gcb < a.Cg ? okm : 0u;
      pk = gv[P].q;
      pk.x &= okm; pk.y &= okm; pk.z &= okm; pk.w &= okm;
    } else {
    float v[8];
    oct8_f8(gv[P], v);
    if constexpr (!TD) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = act_max(fmaf(v[j], sc[j], sh[j]), relu_lo);
    }
    pk.x = wpack2(v[0], v[1]) & okm; pk.y = wpack2(v[2], v[3]) & okm;
    pk.z = wpack2(v[4], v[5]) & okm; pk.w = wpack2(v[6], v[7]) & okm;
    }
    if (gtail) {
      pk.x &= pair_mask(gcb, a.Cg); pk.y &= pair_mask(gcb + 2, a.Cg); pk.z &= pair_mask(gcb + 4, a.Cg); pk.w &= pair_mask(gcb + 6, a.Cg);
    }
    *reinterpret_cast<uint4*>(gst + P * (G::RPP * G::BX * 64)) = pk;
  };
  auto issue = [&](int tile) {
    pn = tile / tpn;
    int t = tile % tpn;
    const int txi = t % a.tx; t /= a.tx;
    const int tyi = t % a.ty;
    const int tzi = t / a.ty;
    poz0 = tzi * TZ; poy0 = tyi * TY; pox0 = txi * 8;
    const float* dbase = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.dn) + (long long)pn * a.dsn * (DBF ? 2 : 4));
    const int oy = poy0 + dyl, ox = pox0 + dxl;
    const bool yxok = oy < a.Hd && ox < a.Wd;
    const unsigned yxoff = __umul24((unsigned)min(oy, a.Hd - 1), dsh) + __umul24((unsigned)min(ox, a.Wd - 1), dsw);
    dok = 0u;
#pragma unroll
    for (int p = 0; p < DP; ++p) {
      const int oz = poz0 + dzl + p * (64 / (TY * 8));
      dok |= ((yxok && oz < a.Dd) ? 1u : 0u) << p;
      const unsigned off = __umul24((unsigned)min(oz, a.Dd - 1), dsd) + yxoff;
      dq[p] = oct8_ld<DBF>(dbase, off + dc_lo, off + dc_hi);
      if constexpr (NB == 2) dq[DP + p] = oct8_ld<DBF>(dbase, off + dc_lo1, off + dc_hi1);
    }
    pok = 0u;
    tile_x(pox0 * SI - 1);
    const float* gbase = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.g) + (long long)pn * a.gsn * (GBF ? 2 : 4));
    static_for<0, PG>([&](auto pc) { load_g(pc, gbase, poz0 * SI - 1, poy0 * SI - 1); });
  };

  if (t0 < t1) issue(t0);
  for (int tile = t0; tile < t1; ++tile) {
    const int n = pn;
    // what the prefetch had no registers for comes in rounds of RB passes (all loads of a round in flight together);
    // the first round is requested before the prefetched part is committed
    constexpr int RB = GBF ? 12 : 4;
    constexpr int R1 = PG + RB < GP ? PG + RB : GP;
    const float* gbase = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.g) + (long long)n * a.gsn * (GBF ? 2 : 4));
    const int iz0 = poz0 * SI - 1, iy0 = poy0 * SI - 1;
    static_for<PG, R1>([&](auto pc) { load_g(pc, gbase, iz0, iy0); });
    if (NEEDC && n != cn) {       // per-(n, channel) transform, once per batch item; kept in LDS (16 registers across the MFMA loop
                         // cost more than four LDS reads per tile); every thread of a chunk writes the same values
      if constexpr (NB == 1) {
        float s8[8], h8[8];
        if constexpr (TD) nl_coeff_vec<8>(a.td, n, a.Cd, dcb, s8, h8);
        else nl_coeff_vec<8>(a.tg, n, a.Cg, gcb, s8, h8);
        const int k8 = TD ? d8 : c8;
#pragma unroll
        for (int j = 0; j < 8; ++j) { coefl[8 * k8 + j] = s8[j]; coefl[32 + 8 * k8 + j] = h8[j]; }
      } else {
#pragma unroll
      for (int nb = 0; nb < (TD ? NB : 1); ++nb) {
        float s8[8], h8[8];
        if constexpr (TD) nl_coeff_vec<8>(a.td, n, a.Cd, dcb + 32 * nb, s8, h8);
        else nl_coeff_vec<8>(a.tg, n, a.Cg, gcb, s8, h8);
        const int k8 = TD ? d8 : c8;
#pragma unroll
        for (int j = 0; j < 8; ++j) { coefl[64 * nb + 8 * k8 + j] = s8[j]; coefl[64 * nb + 32 + 8 * k8 + j] = h8[j]; }
      }
      }
      cn = n;
      __syncthreads();
    }
    float sc[8], sh[8];
    // (the one-block form is kept statement for statement: the register allocation of the two-workgroup kernels is at its
    // limit, and the paired form's loop nest around the same statements cost them 100 bytes more spills, 206 -> 295 us)
    if constexpr (NB == 1) {
    if constexpr (NEEDC) {
      const float4* cq = reinterpret_cast<const float4*>(coefl + 8 * (TD ? d8 : c8));
      const float4 s0 = cq[0], s1 = cq[1], h0 = cq[8], h1 = cq[9];
      sc[0] = s0.x; sc[1] = s0.y; sc[2] = s0.z; sc[3] = s0.w; sc[4] = s1.x; sc[5] = s1.y; sc[6] = s1.z; sc[7] = s1.w;
      sh[0] = h0.x; sh[1] = h0.y; sh[2] = h0.z; sh[3] = h0.w; sh[4] = h1.x; sh[5] = h1.y; sh[6] = h1.z; sh[7] = h1.w;
    }
#pragma unroll
    for (int p = 0; p < DP; ++p) {
      float v[8];
      if constexpr (!RD) oct8_f8(dq[p], v);
      if constexpr (TD && !RD) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = act_max(fmaf(v[j], sc[j], sh[j]), relu_lo);
      }
      const unsigned okm = ((dok >> p) & 1u) ? 0xffffffffu : 0u;
      if (want_db) {                                                  // bias gradient: fp32 sums of what is staged
        if constexpr (RD) oct8_f8(dq[p], v);                          // (raw: unpacked for these sums only, not repacked)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const unsigned cm = (dcb + j < a.Cd) ? okm : 0u;
          dbs[0][j] += __uint_as_float(__float_as_uint(v[j]) & cm);
        }
      }
      uint4 pk;
      if constexpr (RD) {
        const unsigned dm = (!TD || dcb < a.Cd) ? okm : 0u;      // (chunks past the module input's last one: see commit_g)
        pk = dq[p].q;
        pk.x &= dm; pk.y &= dm; pk.z &= dm; pk.w &= dm;
      } else {
      pk.x = wpack2(v[0], v[1]) & okm; pk.y = wpack2(v[2], v[3]) & okm;
      pk.z = wpack2(v[4], v[5]) & okm; pk.w = wpack2(v[6], v[7]) & okm;
      }
      if (dtail) {
        pk.x &= pair_mask(dcb, a.Cd); pk.y &= pair_mask(dcb + 2, a.Cd); pk.z &= pair_mask(dcb + 4, a.Cd); pk.w &= pair_mask(dcb + 6, a.Cd);
      }
      *reinterpret_cast<uint4*>(dst + p * 4096) = pk;
    }
    } else {
#define MMTTA_COEF_REGS(nb)                                                                                            \
    {                                                                                                                  \
      const float4* cq = reinterpret_cast<const float4*>(coefl + 64 * (nb) + 8 * (TD ? d8 : c8));                      \
      const float4 s0 = cq[0], s1 = cq[1], h0 = cq[8], h1 = cq[9];                                                     \
      sc[0] = s0.x; sc[1] = s0.y; sc[2] = s0.z; sc[3] = s0.w; sc[4] = s1.x; sc[5] = s1.y; sc[6] = s1.z; sc[7] = s1.w; \
      sh[0] = h0.x; sh[1] = h0.y; sh[2] = h0.z; sh[3] = h0.w; sh[4] = h1.x; sh[5] = h1.y; sh[6] = h1.z; sh[7] = h1.w; \
    }
    if constexpr (NEEDC && (!TD || NB == 1)) MMTTA_COEF_REGS(0)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
    if constexpr (NEEDC && TD && NB > 1) MMTTA_COEF_REGS(nb)
    const int dcn = dcb + 32 * nb;
#pragma unroll
    for (int p = 0; p < DP; ++p) {
      float v[8];
      if constexpr (!RD) oct8_f8(dq[nb * DP + p], v);
      if constexpr (TD && !RD) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = act_max(fmaf(v[j], sc[j], sh[j]), relu_lo);
      }
      const unsigned okm = ((dok >> p) & 1u) ? 0xffffffffu : 0u;
      if (want_db) {                                                  // bias gradient: fp32 sums of what is staged
        if constexpr (RD) oct8_f8(dq[nb * DP + p], v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const unsigned cm = (dcn + j < a.Cd) ? okm : 0u;
          dbs[nb][j] += __uint_as_float(__float_as_uint(v[j]) & cm);
        }
      }
      uint4 pk;
      if constexpr (RD) {
        const unsigned dm = (!TD || dcn < a.Cd) ? okm : 0u;
        pk = dq[nb * DP + p].q;
        pk.x &= dm; pk.y &= dm; pk.z &= dm; pk.w &= dm;
      } else {
      pk.x = wpack2(v[0], v[1]) & okm; pk.y = wpack2(v[2], v[3]) & okm;
      pk.z = wpack2(v[4], v[5]) & okm; pk.w = wpack2(v[6], v[7]) & okm;
      }
      if (dtail) {
        pk.x &= pair_mask(dcn, a.Cd); pk.y &= pair_mask(dcn + 2, a.Cd); pk.z &= pair_mask(dcn + 4, a.Cd); pk.w &= pair_mask(dcn + 6, a.Cd);
      }
      *reinterpret_cast<uint4*>(dst + nb * G::D_BYTES + p * 4096) = pk;
    }
    }
    }
    static_for<0, R1>([&](auto pc) { commit_g(pc, sc, sh); });
    if constexpr (R1 < GP) {
      constexpr int R2 = R1 + RB < GP ? R1 + RB : GP;
      static_for<R1, R2>([&](auto pc) { load_g(pc, gbase, iz0, iy0); });
      static_for<R1, R2>([&](auto pc) { commit_g(pc, sc, sh); });
      if constexpr (R2 < GP) {
        static_for<R2, GP>([&](auto pc) { load_g(pc, gbase, iz0, iy0); });
        static_for<R2, GP>([&](auto pc) { commit_g(pc, sc, sh); });
      }
    }
    __syncthreads();
    if (tile + 1 < t1) issue(tile + 1);                               // lands during the MFMAs below
    // ---- MFMAs.  Fragment f = (k step, tap slot) is read LA MFMAs before it multiplies (a ring of LA + 1 register sets;
    // a fence per MFMA, or the scheduler sinks every read to one MFMA ahead and the MFMA waits out the LDS latency)
    constexpr int LA = 3, NF = G::NK * 7;
    wbf16x8 ra[LA + 1], fb[2][NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) fb[0][nb] = MMTTA_TR_FRAG(dread, nb * G::D_BYTES);
#pragma unroll
    for (int f = 0; f < LA; ++f) ra[f] = MMTTA_TR_FRAG(gread[f % 7], G::row_off(f / 7));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int ks = f / 7, j = f % 7;
      if (f + LA < NF) ra[(f + LA) % (LA + 1)] = MMTTA_TR_FRAG(gread[(f + LA) % 7], G::row_off((f + LA) / 7));
      if (j == 2 && ks + 1 < G::NK) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) fb[(ks + 1) & 1][nb] = MMTTA_TR_FRAG(dread, nb * G::D_BYTES + (ks + 1) * 1024);
      }
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        acc[nb][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ra[f % (LA + 1)], fb[ks & 1][nb], acc[nb][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
  }
  if constexpr (UPD) {
    // One slab per set (host: wgrad_updates_in_epilogue): this workgroup holds the complete gradient of its 27 x 32 cg x
    // 32 NB cd block, so the slab, its read-back and wgrad_update27_kernel's launch are left out - the same optimizer and
    // image code runs here on the same LDS tile (the images are dead: the loop ended with a barrier), 8 cg at a time.
    float* tile = lds;                              // [32 cd][UPD_RS], then the two step scalars
    float* scal = lds + UPD_CD * UPD_RS;
    const int t0s = *u.step;
    if (tid == 0) optim_scalars(KIND, u.a, t0s, scal[0], scal[1]);
    const bool first = t0s == 0;
    const bool wd_on = u.a.wd != 0.f;
    const bool keep_m = KIND != 2 || u.a.momentum != 0.f;
    __syncthreads();
    const float step_size = scal[0], bc2_sqrt = scal[1];
    if (want_db) {                                  // the complete bias gradient of these 32 NB channels (see below)
      float* red8 = lds;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        if (nb) __syncthreads();
#pragma unroll
        for (int c = 0; c < 8; ++c) red8[tid * 8 + c] = dbs[nb][c];
        __syncthreads();
        const int cd = cd0 + 32 * nb + tid;
        if (tid < 32 && cd < a.Cd) {
          float sacc = 0.f;
#pragma unroll 8
          for (int q = 0; q < 64; ++q) sacc += red8[((q << 2) | (tid >> 3)) * 8 + (tid & 7)];
          // bias_rows_sum over this one row adds zeros to it: sacc is never -0 (it starts at +0), so that is sacc itself
          const float t = 0.f + sacc;
          const long long o = pset_bias_elems(ps, qset) + cd;
          float pi = u.bp[o], mi = 0.f, vi = 0.f;
          if (!first) {
            if (keep_m) mi = u.bm[o];
            if (KIND != 2) vi = u.bv[o];
          }
          optim_update<KIND>(pi, t, mi, vi, wd_on && u.b_decay, u.a, step_size, bc2_sqrt, first);
          u.bp[o] = pi;
          if (keep_m) u.bm[o] = mi;
          if (KIND != 2) u.bv[o] = vi;
        }
      }
      __syncthreads();
    }
    const bool decay = wd_on && u.w_decay;
    const long long wo = pset_weight_elems(ps, qset), rowst = (long long)a.Cg * 27;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      // accumulator rows 8 g + (i & 3) + 4 h, i = 4 g .. 4 g + 3, are cg group g of the block; the value is slab_sums4's for
      // one slab, 0.f + acc (a -0 does not survive there either)
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        const int tap = wave + 4 * j;
        if (tap < 27) {
#pragma unroll
          for (int i = 0; i < 4; ++i) tile[r * UPD_RS + (i + 4 * h) * 27 + tap] = 0.f + acc[nb][j][4 * g + i];
        }
      }
      __syncthreads();
      const int ucg0 = cg0 + 8 * g, ucd0 = cd0 + 32 * nb;
      const long long ob = wo + ((long long)ucd0 * a.Cg + ucg0) * 27;
      upd_optim4<KIND, 4>(u, ob, rowst, 0, ucd0, a.Cd, first, keep_m, decay, step_size, bc2_sqrt, tile);
      upd_optim4<KIND, 3>(u, ob, rowst, 4, ucd0, a.Cd, first, keep_m, decay, step_size, bc2_sqrt, tile);
      __syncthreads();
#pragma unroll
      for (int m = 0; m < 2; ++m) upd_repack(u.img[m], ps, qset, ucg0, ucd0, tile);
      __syncthreads();
    }
  } else {
  const int sl = sx;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const int tap = wave + 4 * j;
    if (tap < 27) {
      float* sb = a.slab + (((long long)sl * 27 + tap) * a.CGp + cg0) * a.CDp + cd0 + 32 * nb + r;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
        sb[(long long)row * a.CDp] = acc[nb][j][i];
      }
    }
  }
  if (want_db) {                                    // thread (voxel slot, chunk d8) holds channels 8 d8 .. 8 d8 + 7
    float* red8 = lds;                              // the images are dead: the loop ended with a barrier
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if (nb) __syncthreads();
#pragma unroll
      for (int c = 0; c < 8; ++c) red8[tid * 8 + c] = dbs[nb][c];
      __syncthreads();
      if (tid < 32) {
        float sacc = 0.f;
#pragma unroll 8
        for (int q = 0; q < 64; ++q) sacc += red8[((q << 2) | (tid >> 3)) * 8 + (tid & 7)];
        a.dbpart[(long long)sl * a.CDp + cd0 + 32 * nb + tid] = sacc;
      }
    }
  }
  }
