// The body of igemm_kernel and igemm_reuse_kernel (conv_igemm.hip): included inside each kernel, which names the tile
// (NB, MB, TZ, TY, TX, KCI, BF, OCC, ABF) and REUSE as constants.  One text, so that the two cannot drift apart, and no
// function in between, so that igemm_kernel compiles to exactly what it was before the second kernel existed.
// Expects in scope, as compile-time constants: int NB, MB, TZ, TY, TX, KCI, OCC; bool BF, ABF, REUSE, RAW; and the kernel
// argument `GArgs a`.  No include guard on purpose: it is included once per kernel.
// RAW (igemm_raw_kernel, igemm_reuse_raw_kernel): the input is bf16-stored, takes no norm-on-load and has whole 8-channel
// chunks only (the host asks: raw_staging), so a 16-byte item goes to LDS as it was loaded, under its halo / chunk mask -
// no unpack, no coefficients, no fma / max / repack.  Every RAW site is an `if constexpr`: the other kernels keep their text.
  extern __shared__ float lds[];
  static_assert(!REUSE || (NB == 1 && MB == 2 && TZ == 4 && TY == 8 && TX == 8 && KCI == 16 && BF && OCC > 2),
                "fragment reuse is built for the lean tile");
  static_assert(!RAW || (BF && ABF), "raw staging copies bf16-stored items");
  // LDS voxel stride: fp32: KCI+1 words (odd: the 32 rows of a fragment hit distinct banks);
  // bf16: KCI+8 halfwords (16-byte slots stay aligned for ds_read_b128)
  constexpr int VS = BF ? (KCI + 8) : (KCI + 1);
  static_assert(!BF || KCI % 16 == 0, "bf16 stages are multiples of the MFMA K=16");
  constexpr int MT = TZ * TY * TX;
  constexpr int MG = 4 / NB;
  static_assert(MT == 32 * MB * MG, "tile rows must equal 32*MB*(4/NB)");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cb = wave % NB, mg = wave / NB;
  const int h = lane >> 5, r = lane & 31;

  // workgroups are dealt round-robin over the 8 XCDs: give each XCD one CONTIGUOUS run of tiles (a z-slab of the
  // volume), so that the halo rows neighbouring tiles share are served by that XCD's L2 instead of being fetched again
  // (the whole 3-D grid is renumbered, tile index fastest: the tiles that stream the SAME weight panel - same column
  // group, same K split - then also share an XCD, which matters for the weight-bound 8^3 / 16^3 levels)
  const unsigned lflat = xcd_contiguous_id(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z),
                                           gridDim.x * gridDim.y * gridDim.z);
  const int bx = (int)(lflat % gridDim.x);
  const int lby = (int)((lflat / gridDim.x) % gridDim.y), lbz = (int)(lflat / (gridDim.x * gridDim.y));
  int cidx, t;
  class_of_tile(a, bx, cidx, t);
  const ClassInfo ci = a.cls[cidx];
  const int tile_in_n = t % (a.tz * a.ty * a.tx);
  const int txi = t % a.tx; t /= a.tx;
  const int tyi = t % a.ty; t /= a.ty;
  const int tzi = t % a.tz;
  const int n = t / a.tz;
  const float* wpn = pset_packed(a.ps, a.wp, n);        // this batch item's parameter set (workgroup-uniform)
  const float* biasn = pset_bias(a.ps, a.bias, n);
  const int gz0 = tzi * TZ, gy0 = tyi * TY, gx0 = txi * TX;
  const int BZ = (TZ - 1) * a.si + ci.zext + 1;
  const int BY = (TY - 1) * a.si + ci.yext + 1;
  const int BX = (TX - 1) * a.si + ci.xext + 1;
  const int boxvox = BZ * BY * BX;
  const int LP = (BF && a.si == 1) ? LDS_PITCH_BF16 : BX;      // LDS x-row pitch in voxels
  const int iz0 = gz0 * a.si + ci.zmin, iy0 = gy0 * a.si + ci.ymin, ix0 = gx0 * a.si + ci.xmin;

  const int colbase = (lby * NB + cb) * 32;
  const bool colact = REUSE || colbase < a.Np;

  int rowaddr[MB];   // LDS word address of (row's voxel, channel h) inside the box
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    int zl, yl, xl;
    row_to_local<TZ, TY, TX, BF>((mg * MB + mb) * 32 + r, zl, yl, xl);
    rowaddr[mb] = (((zl * a.si) * BY + yl * a.si) * LP + xl * a.si) * VS + (BF ? 8 * h : h);
    // both parity blocks: voxel (z = mg, y, x slot r & 3) of the box; the block and the tap are immediates (rfrag)
    if constexpr (REUSE) rowaddr[mb] = ((mg * (TY + 2) + (r >> 3) + 4 * ((r >> 2) & 1)) * LDS_PITCH_BF16 + (r & 3)) * VS + 8 * h;
  }

  f32x16 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[mb][i] = 0.f;

  const int ks0 = lbz * a.stages_per_split;
  const int ks1 = min(a.nstages, ks0 + a.stages_per_split);
  // batch item base: element offsets are applied by the storage helpers (the pointer itself is never advanced, so the
  // same code addresses 2-byte and 4-byte elements)
  const float* inb = a.in;
  const long long inoff = (long long)n * a.isn;

  // Row-structured loader of the bf16 3x3x3 stride-1 stages (the bulk of the network).  With several volumes in flight
  // the chip is bound by vector-ALU issue (profiles/r02c_sq_counters.md) and the generic walk below spends ~100 vector
  // instructions per 8-channel item on index decoding, bounds and 64-bit addressing.  Here an item's geometry is paid
  // ONCE PER TILE: a thread owns one (x, channel chunk) column of the box and walks the box rows RPP at a time, so its
  // 32-bit element offset of pass P (voff[P], channel base folded into the wave-uniform pointer) and its in-bounds bit
  // are the same for every stage, the LDS address is a per-thread constant plus an immediate, and a stage costs the
  // conversion / norm-on-load / pack only.  The first PG passes of stage ks+1 are requested during the MFMA phase of
  // stage ks - after its last weight-fragment request, because loads return in order - and land under it.
  constexpr int RCV8 = BF ? KCI / 8 : 1;                  // 8-channel chunks per voxel
  constexpr int RBY = TY + 2, RBZ = TZ + 2, RBX = TX + 2;
  constexpr int RIPR = RBX * RCV8;                        // items per box row
  constexpr int RRPP = 256 / RIPR;                        // box rows per pass (threads beyond repeat the last row)
  constexpr int RNROW = RBZ * RBY;
  constexpr int RGP = (RNROW + RRPP - 1) / RRPP;          // passes per stage
  constexpr int RPG = !BF ? 0 : (OCC > 2 ? 0 : (KCI == 16 ? (ABF ? 4 : 2) : 0));   // of which prefetched across the MFMA phase
  constexpr int RGPA = BF ? RGP : 1;
  const bool fast = REUSE || (BF && a.rowload && ci.ntaps == 27 && a.si == 1);      // workgroup-uniform: all 256 threads stage
  const bool pipe = fast && RPG > 0;
  Oct8<ABF> gv[RGPA];
  unsigned voff[RGPA];
  unsigned pok = 0u;
  // the 16-channel stages keep the offsets across the stages; the 32-channel stages have no registers to spare during
  // their MFMA phase (two weight-fragment sets of 40) and rebuild them per stage (~12 instructions per item, still 1/8 of
  // the generic walk) - `rrsub` goes through an opaque copy there, or the compiler hoists the rebuild out of the K loop
  constexpr bool RHOIST = KCI == 16;
  const int rrsub = min(tid / RIPR, RRPP - 1), rrem = tid % RIPR, rbx = rrem / RCV8, rcv = rrem % RCV8;
  auto geometry = [&]() {
    int rs = rrsub;
    if constexpr (!RHOIST) asm volatile("" : "+v"(rs));
    const int ix = ix0 + rbx;
    const bool xok = (unsigned)ix < (unsigned)a.Wi;
    const unsigned xoff = __umul24((unsigned)min(max(ix, 0), a.Wi - 1), (unsigned)a.isw) + rcv * 8;
    pok = 0u;
    static_for<0, RGP>([&](auto pc) {
      constexpr int P = decltype(pc)::value;
      const int row = min(RRPP * P + rs, RNROW - 1);
      const int bz = row / RBY, by = row - bz * RBY;
      const int iz = iz0 + bz, iy = iy0 + by;
      const bool ok = xok && (unsigned)iz < (unsigned)a.Di && (unsigned)iy < (unsigned)a.Hi;
      pok |= (ok ? 1u : 0u) << P;
      voff[P] = __umul24((unsigned)min(max(iz, 0), a.Di - 1), (unsigned)a.isd) + __umul24((unsigned)min(max(iy, 0), a.Hi - 1), (unsigned)a.ish) + xoff;
    });
  };
  unsigned short* lh0 = reinterpret_cast<unsigned short*>(lds);
  unsigned short* rst = lh0 + (rrsub * LDS_PITCH_BF16 + (REUSE ? reuse_xslot(rbx) : rbx)) * VS + rcv * 8;       // + P * RRPP * LDS_PITCH_BF16 * VS
  // norm-on-load coefficients of every channel this workgroup will stage, once, in LDS behind the box image (a
  // per-stage fetch from global memory would be an exposed round trip in front of every commit)
  float* coef = lds + a.coef_off;
  const int cbase = ks0 * KCI, nch = (ks1 - ks0) * KCI;
  if (fast) {
    if constexpr (!RAW) {
      for (int cch = tid; cch < nch; cch += 256) {
        float sc1 = 0.f, sh1 = 0.f;
        if (cbase + cch < a.Ci) nl_coeff(a.tin, n, a.Ci, cbase + cch, sc1, sh1);     // channels past the last one stage as zeros
        coef[cch] = sc1;
        coef[nch + cch] = sh1;
      }
    }
    if constexpr (RHOIST) geometry();
  }
  // channel part of an item's address: wave-uniform (folded into the pointer); the last stage of a Ci that is no multiple
  // of KCI clamps to the last valid chunk (its coefficients are zero)
  auto stage_base = [&](int ks) {
    return reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.in) + ((long long)n * a.isn + (long long)ks * KCI) * (ABF ? 2 : 4));
  };
  const int cmax8 = ABF ? ((a.Ci - 1) & ~7) : ((a.Ci - 1) & ~3);
  auto load_item = [&](auto pc, const float* sb, int c0) {
    constexpr int P = decltype(pc)::value;
    // chunks past the tensor's last one (partial last stage) re-read the last valid chunk; their coefficients are zero
    const int over = max(c0 + rcv * 8 - cmax8, 0), over_hi = max(c0 + rcv * 8 + 4 - cmax8, 0);
    gv[P] = oct8_ld<ABF>(sb, voff[P] - over, voff[P] + 4 - over_hi);
  };
  auto issue = [&](int ks) {
    const float* sb = stage_base(ks);
    static_for<0, RPG>([&](auto pc) { load_item(pc, sb, ks * KCI); });
  };
  if (fast && ks0 < ks1) {
    if (pipe) issue(ks0);
    if constexpr (!RAW) __syncthreads();      // coefficients visible
  }

  // Weight fragment of (tap t, 16-channel step k2) of the canonical stage: a wave-uniform 64-bit base (scalar registers:
  // parameter set, stage, slab - the slab walks up for the forward form, down for the mirrored input gradient) plus ONE
  // 32-bit per-lane byte offset, so a request costs two scalar adds instead of a 64-bit multiply-add per lane
  // (measured on the 64^3 32-channel layers: 7 scalar + 1 vector instruction per fragment before).
  // (compiled into the lean 64^3 tile only: beside the table-driven stage it costs the four-block tiles, which sit at the
  // 256-register limit, 200-450 bytes of spills)
  constexpr bool CANON_CFG = BF && OCC > 2;
  const long long wslab16 = (long long)(a.Kp / 8) * a.Np * 16;                    // bytes per tap slab
  const char* const wuni = reinterpret_cast<const char*>(wpn) + (a.flip27 ? 26 * wslab16 : 0);
  const long long wstep16 = a.flip27 ? -wslab16 : wslab16;
  const unsigned wlane16 = (unsigned)(h * a.Np + colbase + r) * 16u;
  auto wfrag27 = [&](int c0, int t, int k2) {
    const char* ub = wuni + ((long long)(c0 / 8) * a.Np + (long long)k2 * 2 * a.Np) * 16 + t * wstep16;
    return *reinterpret_cast<const uint4*>(ub + wlane16);
  };

  for (int ks = ks0; ks < ks1; ++ks) {
    const int stage = ks;
    const int c0 = ks * KCI;
    // the first group of weight fragments of this stage is requested before the staging pass, so its L2 round trip
    // hides behind the box loads instead of opening the MFMA phase (full 27-tap stages of the bf16 path only)
    constexpr int WG0 = BF ? (OCC > 2 ? 3 : (KCI == 16 ? 9 : 5)) : 1;
    constexpr int WKS = BF ? KCI / 16 : 1;
    uint4 wfirst[WG0][WKS];
    bool wfirst_ok = false;
    if constexpr (BF) {
      if (REUSE || (colact && ci.ntaps == 27 && ((min(KCI, a.Ci - c0) + 15) >> 4) == WKS)) {   // same test as the MFMA section
        wfirst_ok = true;
        const long long slabsz8 = (long long)(a.Kp / 8) * a.Np;
        if (CANON_CFG && fast) {
#pragma unroll
          for (int t = 0; t < WG0; ++t)
#pragma unroll
            for (int k2 = 0; k2 < WKS; ++k2) wfirst[t][k2] = wfrag27(c0, t, k2);
        } else {
          const uint4* wq0 = reinterpret_cast<const uint4*>(wpn) + (long long)(c0 / 8 + h) * a.Np + colbase + r;
#pragma unroll
          for (int t = 0; t < WG0; ++t)
#pragma unroll
            for (int k2 = 0; k2 < WKS; ++k2) wfirst[t][k2] = wq0[(a.slab + ci.tap0)[t] * slabsz8 + k2 * 2 * a.Np];
        }
      }
    }
    // ---------------- stage the input box (KCI channels) into LDS ----------------
    if constexpr (BF) {
      unsigned short* lh = reinterpret_cast<unsigned short*>(lds);
      if (fast) {
        const float* sb = stage_base(ks);
        // what the prefetch had no registers for comes in rounds of RB passes (all loads of a round in flight together);
        // the first round is requested before the prefetched passes are committed
        constexpr int RB = ABF ? 6 : 4;
        constexpr int R1 = RPG + RB < RGP ? RPG + RB : RGP;
        if constexpr (!RHOIST) geometry();
        static_for<RPG, R1>([&](auto pc) { load_item(pc, sb, c0); });
        float sc[8], sh[8];
        if constexpr (!RAW) {
          const float4* cq = reinterpret_cast<const float4*>(coef + (c0 - cbase) + rcv * 8);
          const float4* hq = reinterpret_cast<const float4*>(coef + nch + (c0 - cbase) + rcv * 8);
          const float4 s0 = cq[0], s1 = cq[1], h0 = hq[0], h1 = hq[1];
          sc[0] = s0.x; sc[1] = s0.y; sc[2] = s0.z; sc[3] = s0.w; sc[4] = s1.x; sc[5] = s1.y; sc[6] = s1.z; sc[7] = s1.w;
          sh[0] = h0.x; sh[1] = h0.y; sh[2] = h0.z; sh[3] = h0.w; sh[4] = h1.x; sh[5] = h1.y; sh[6] = h1.z; sh[7] = h1.w;
        }
        const float relu_lo = act_lo(a.tin.relu);
        auto commit_item = [&](auto pc) {
          constexpr int P = decltype(pc)::value;
          uint4 pk;
          if constexpr (RAW) {
            // the item as loaded, under the halo bit and - in a partial last stage, where the loader re-read the last valid
            // chunk - the chunk test, folded into one mask
            const unsigned okm = (((pok >> P) & 1u) && (REUSE || c0 + rcv * 8 < a.Ci)) ? 0xffffffffu : 0u;
            pk = gv[P].q;
            pk.x &= okm; pk.y &= okm; pk.z &= okm; pk.w &= okm;
          } else {
          float v[8];
          oct8_f8(gv[P], v);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = act_max(fmaf(v[j], sc[j], sh[j]), relu_lo);
          const unsigned okm = ((pok >> P) & 1u) ? 0xffffffffu : 0u;
          pk.x = pack_bf16x2(v[0], v[1]) & okm; pk.y = pack_bf16x2(v[2], v[3]) & okm;
          pk.z = pack_bf16x2(v[4], v[5]) & okm; pk.w = pack_bf16x2(v[6], v[7]) & okm;
          }
          if (RNROW % RRPP == 0 || P + 1 < RGP || RRPP * P + rrsub < RNROW)       // the last pass may be partial
            *reinterpret_cast<uint4*>(rst + P * (RRPP * LDS_PITCH_BF16 * VS)) = pk;
        };
        static_for<0, R1>(commit_item);
        static_for_step<R1, RGP, RB>([&](auto r0) {
          constexpr int A = decltype(r0)::value, B = A + RB < RGP ? A + RB : RGP;
          static_for<A, B>([&](auto pc) { load_item(pc, sb, c0); });
          static_for<A, B>(commit_item);
        });
      } else if (RAW || a.vec4) {          // (a raw launch has 16-byte items: the host asked)
        constexpr int CV8 = KCI / 8;
        const int cv = tid % CV8;          // 256 % CV8 == 0
        const int c = c0 + cv * 8;
        float sc[8], sh[8];
        constexpr int STEP = 256 / CV8;
        const int first_item = 0;
        if constexpr (!RAW) nl_coeff_vec<8>(a.tin, n, a.Ci, c, sc, sh);
        // U items per trip: all their global loads are issued before the first use (one exposed latency per
        // trip instead of one per item)
        // all of a thread's items in as few trips as the register budget allows: one exposed memory latency per trip
        constexpr int U = OCC > 2 ? 2 : 4;
        const bool tail = (a.Ci & 7) != 0;       // only then can lanes beyond Ci hold uninitialised padding
        for (int bv0 = tid / CV8 + first_item * STEP; bv0 < boxvox; bv0 += U * STEP) {
          float4 x0[U], x1[U];
          uint4 xq[U];                       // RAW: the item as loaded, zeros outside the tensor and past its last chunk
          bool ok[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int bv = bv0 + u * STEP;
            const int bz = (int)__umulhi((unsigned)bv, ci.mBXY), brem = bv - bz * ci.BXY;
            const int by = (int)__umulhi((unsigned)brem, ci.mBX), bx = brem - by * ci.BX;
            const int iz = iz0 + bz, iy = iy0 + by, ix = ix0 + bx;
            ok[u] = bv < boxvox && (unsigned)iz < (unsigned)a.Di && (unsigned)iy < (unsigned)a.Hi &&
                    (unsigned)ix < (unsigned)a.Wi && c < a.Ci;
            x0[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            x1[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (RAW) xq[u] = make_uint4(0u, 0u, 0u, 0u);
            if (ok[u]) {
              const long long so = inoff + (long long)iz * a.isd + (long long)iy * a.ish + (long long)ix * a.isw + c;
              if constexpr (RAW) xq[u] = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(inb) + so);
              else if constexpr (ABF) ld8_t<true>(inb, so, x0[u], x1[u]);      // rows of bf16 tensors are padded to 8 channels
              else {
                x0[u] = *reinterpret_cast<const float4*>(inb + so);
                if (c + 4 < a.Ci) x1[u] = *reinterpret_cast<const float4*>(inb + so + 4);
              }
            }
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int bv = bv0 + u * STEP;
            if (bv < boxvox) {
              uint4 pk = make_uint4(0u, 0u, 0u, 0u);
              if constexpr (RAW) pk = xq[u];
              else if (ok[u]) {
                const float xs[8] = {x0[u].x, x0[u].y, x0[u].z, x0[u].w, x1[u].x, x1[u].y, x1[u].z, x1[u].w};
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                  v[j] = nl_apply(xs[j], sc[j], sh[j], a.tin.relu);
                  if (tail && c + j >= a.Ci) v[j] = 0.f;
                }
                pk.x = pack_bf16x2(v[0], v[1]); pk.y = pack_bf16x2(v[2], v[3]);
                pk.z = pack_bf16x2(v[4], v[5]); pk.w = pack_bf16x2(v[6], v[7]);
              }
              const int bz = (int)__umulhi((unsigned)bv, ci.mBXY), brem = bv - bz * ci.BXY;
              const int by = (int)__umulhi((unsigned)brem, ci.mBX), bx = brem - by * ci.BX;
              *reinterpret_cast<uint4*>(lh + ((bz * BY + by) * LP + bx) * VS + cv * 8) = pk;
            }
          }
        }
      } else {
        const int cc = tid % KCI;
        const int c = c0 + cc;
        float sc, sh;
        nl_coeff_vec<1>(a.tin, n, a.Ci, c, &sc, &sh);
        for (int bv = tid / KCI; bv < boxvox; bv += 256 / KCI) {
          const int bz = (int)__umulhi((unsigned)bv, ci.mBXY), brem = bv - bz * ci.BXY;
          const int by = (int)__umulhi((unsigned)brem, ci.mBX), bx = brem - by * ci.BX;
          const int iz = iz0 + bz, iy = iy0 + by, ix = ix0 + bx;
          float v = 0.f;
          if ((unsigned)iz < (unsigned)a.Di && (unsigned)iy < (unsigned)a.Hi && (unsigned)ix < (unsigned)a.Wi &&
              c < a.Ci)
            v = nl_apply(ld1_t<ABF>(inb, inoff + (long long)iz * a.isd + (long long)iy * a.ish + (long long)ix * a.isw + c), sc, sh,
                         a.tin.relu);
          lh[((bz * BY + by) * LP + bx) * VS + cc] = __builtin_bit_cast(unsigned short, (__bf16)v);
        }
      }
    } else {
    if (a.vec4) {
      constexpr int CV = KCI / 4;
      const int cv = tid % CV;           // 256 % CV == 0: fixed channel group per thread
      const int c = c0 + cv * 4;
      float sc[4], sh[4];
      nl_coeff_vec<4>(a.tin, n, a.Ci, c, sc, sh);
      constexpr int U = 4, STEP = 256 / CV;
      for (int bv0 = tid / CV; bv0 < boxvox; bv0 += U * STEP) {
        float4 xin[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int bv = bv0 + u * STEP;
          const int bz = (int)__umulhi((unsigned)bv, ci.mBXY), brem = bv - bz * ci.BXY;
          const int by = (int)__umulhi((unsigned)brem, ci.mBX), bx = brem - by * ci.BX;
          const int iz = iz0 + bz, iy = iy0 + by, ix = ix0 + bx;
          ok[u] = bv < boxvox && (unsigned)iz < (unsigned)a.Di && (unsigned)iy < (unsigned)a.Hi &&
                  (unsigned)ix < (unsigned)a.Wi && c < a.Ci;
          xin[u] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (ok[u]) xin[u] = *reinterpret_cast<const float4*>(inb + inoff + iz * a.isd + iy * a.ish + ix * a.isw + c);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int bv = bv0 + u * STEP;
          if (bv < boxvox) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok[u]) {
              v.x = nl_apply(xin[u].x, sc[0], sh[0], a.tin.relu);
              v.y = (c + 1 < a.Ci) ? nl_apply(xin[u].y, sc[1], sh[1], a.tin.relu) : 0.f;
              v.z = (c + 2 < a.Ci) ? nl_apply(xin[u].z, sc[2], sh[2], a.tin.relu) : 0.f;
              v.w = (c + 3 < a.Ci) ? nl_apply(xin[u].w, sc[3], sh[3], a.tin.relu) : 0.f;
            }
            float* d = lds + bv * VS + cv * 4;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
          }
        }
      }
    } else {
      const int cc = tid % KCI;          // 256 % KCI == 0
      const int c = c0 + cc;
      float sc, sh;
      nl_coeff_vec<1>(a.tin, n, a.Ci, c, &sc, &sh);
      for (int bv = tid / KCI; bv < boxvox; bv += 256 / KCI) {
        const int bx = bv % BX, by = (bv / BX) % BY, bz = bv / (BX * BY);
        const int iz = iz0 + bz, iy = iy0 + by, ix = ix0 + bx;
        float v = 0.f;
        if ((unsigned)iz < (unsigned)a.Di && (unsigned)iy < (unsigned)a.Hi && (unsigned)ix < (unsigned)a.Wi &&
            c < a.Ci)
          v = nl_apply(inb[inoff + iz * a.isd + iy * a.ish + ix * a.isw + c], sc, sh, a.tin.relu);
        lds[bv * VS + cc] = v;
      }
    }
    }
    __syncthreads();

    // ---------------- MFMA over taps x channel blocks ----------------
    if constexpr (BF) {
      if (colact) {
        constexpr int KS = KCI / 16;
        const unsigned short* lh = reinterpret_cast<const unsigned short*>(lds);
        const int kreal = min(KCI, a.Ci - c0);
        const int nks = (kreal + 15) >> 4;         // 16-channel steps that carry data
        const uint4* wq = reinterpret_cast<const uint4*>(wpn);   // image [tap][Kp/8][Np][8 bf16]
        const long long slabsz8 = (long long)(a.Kp / 8) * a.Np;
        const uint4* wcol = wq + (long long)(c0 / 8 + h) * a.Np + colbase + r;
        const int np2 = 2 * a.Np;
        const int ntap = ci.ntaps;
        const int* tslab = a.slab + ci.tap0;
        const int* ttoff = a.toff + ci.tap0;
        if constexpr (REUSE) {
          // One group = one box row (kz, ky) = the taps kx = 0, 1, 2: six MFMAs from four fragments.  Fragment m of the
          // row is requested two MFMAs ahead of its first use (m = 2, 3 under taps 0 and 1, the next row's m = 0, 1
          // under tap 2); per accumulator block the taps come in the plain stage's order with the plain stage's operands.
          constexpr int G = 3, NG = 9;
          static_assert(G == WG0 && KS == 1 && WKS == 1, "a weight group is one box row");
          auto rfrag = [&](int j, int m) {
            return *reinterpret_cast<const uint4*>(lh + rowaddr[0] + (((j / 3) * RBY + j % 3) * LDS_PITCH_BF16 + reuse_xslot(m)) * VS);
          };
          uint4 wset[2][G];
#pragma unroll
          for (int t = 0; t < G; ++t) wset[0][t] = wfirst[t][0];
          uint4 f[4], fn[2];
          f[0] = rfrag(0, 0);
          f[1] = rfrag(0, 1);
#pragma unroll
          for (int g = 0; g < NG; ++g) {
            if (g + 1 < NG) {
#pragma unroll
              for (int t = 0; t < G; ++t) wset[(g + 1) & 1][t] = wfrag27(c0, (g + 1) * G + t, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < G; ++t) {
              const bf16x8 bfr = __builtin_bit_cast(bf16x8, wset[g & 1][t]);
              if (t < 2) f[t + 2] = rfrag(g, t + 2);
              else if (g + 1 < NG) fn[0] = rfrag(g + 1, 0);
              acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f[t]), bfr, acc[0], 0, 0, 0);
              if (t == 2 && g + 1 < NG) fn[1] = rfrag(g + 1, 1);
              acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f[t + 1]), bfr, acc[1], 0, 0, 0);
              const bool rd0 = t < 2 || g + 1 < NG, rd1 = t == 2 && g + 1 < NG;
              if (rd0) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // one LDS read ...
              __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);               // ... then one MFMA
              if (rd1) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
              __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            }
            f[0] = fn[0];
            f[1] = fn[1];
            __builtin_amdgcn_sched_barrier(0);
          }
        } else if (nks == KS && ntap == 27) {
          // Full 27-tap stage: the weight fragments of G taps are fetched as a group while the previous group's
          // G*KS*MB MFMAs run - two register sets, straight-line code, scheduling barriers so the loads stay ahead
          // (the scheduler otherwise sinks each load next to its use and every tap exposes an L2 round trip:
          // measured 15-18k cycles per stage against 3.5k cycles of MFMA).
          constexpr int G = OCC > 2 ? 3 : (KS == 1 ? 9 : 5);
          constexpr int NG = (27 + G - 1) / G;
          static_assert(G == WG0 && KS == WKS, "first-group prefetch must match the group shape");
          // canonical stage (row loader): tap offsets are immediates, weight requests scalar-based (tap27_off, wfrag27);
          // otherwise both come from the tap tables
          auto stage27 = [&](auto fc) {
          constexpr bool CANON = decltype(fc)::value;
          uint4 wset[2][G][KS];
#pragma unroll
          for (int t = 0; t < G; ++t)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) wset[0][t][ks] = wfirst[t][ks];     // requested before the staging pass
          uint4 avc[MB];
          {
            const int ta0 = CANON ? 0 : ttoff[0] * VS;
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) avc[mb] = *reinterpret_cast<const uint4*>(lh + rowaddr[mb] + ta0);
          }
#pragma unroll
          for (int g = 0; g < NG; ++g) {
            if (g + 1 < NG) {
#pragma unroll
              for (int t = 0; t < G; ++t) {
                if ((g + 1) * G + t < 27) {
#pragma unroll
                  for (int ks = 0; ks < KS; ++ks)
                    wset[(g + 1) & 1][t][ks] = CANON ? wfrag27(c0, (g + 1) * G + t, ks) : wcol[tslab[(g + 1) * G + t] * slabsz8 + ks * np2];
                }
              }
            }
            if (g == NG - 2 && pipe && stage + 1 < ks1) issue(stage + 1);     // behind the stage's last weight request
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < G; ++t) {
              if (g * G + t < 27) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                  const bf16x8 bfr = __builtin_bit_cast(bf16x8, wset[g & 1][t][ks]);
                  // the activation fragments of the NEXT (tap, k-step) are read while this one's MFMAs run: left to
                  // itself the compiler emits read -> wait -> MFMA per fragment (one register set) and every MFMA
                  // exposes an LDS round trip (measured ~93 cycles per 32-cycle MFMA)
                  const int idx = g * G + t;
                  const bool more = !(idx == 26 && ks == KS - 1);
                  const int nidx = ks + 1 < KS ? idx : idx + 1, nks2 = ks + 1 < KS ? ks + 1 : 0;
                  uint4 avn[MB];
                  int tan = 0;
                  if (more) tan = (CANON ? tap27_off(nidx, RBY) : ttoff[nidx]) * VS + nks2 * 16;
#pragma unroll
                  for (int mb = 0; mb < MB; ++mb) {
                    if (more) avn[mb] = *reinterpret_cast<const uint4*>(lh + rowaddr[mb] + tan);
                    acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, avc[mb]), bfr, acc[mb], 0, 0, 0);
                  }
#pragma unroll
                  for (int mb = 0; mb < MB; ++mb) {
                    if (more) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);    // one LDS read ...
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);              // ... then one MFMA
                  }
                  if (more) {
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) avc[mb] = avn[mb];
                  }
                }
              }
            }
            __builtin_amdgcn_sched_barrier(0);
          }
          };
          if constexpr (CANON_CFG) {
            if (fast) stage27(std::true_type{});
            else stage27(std::false_type{});
          } else {
            stage27(std::false_type{});
          }
        } else if (nks == KS && ntap >= 4) {
          // A tap is only MB*KS MFMAs of 32 cycles: far less than an L2 round trip, so the weight fragments run
          // through a ring of D taps in flight.  The body is branch-free (a load behind a branch is waited for on
          // the spot): the tap count is padded to a multiple of D, a padded tap multiplies by a zero fragment and
          // re-reads a valid LDS / weight address.
          constexpr int D = 4;
          uint4 ring[D][KS];
#pragma unroll
          for (int d = 0; d < D; ++d) {
            const uint4* wb = wcol + tslab[d] * slabsz8;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) ring[d][ks] = wb[ks * np2];
          }
          const int ntap_pad = (ntap + D - 1) / D * D;
          for (int tp0 = 0; tp0 < ntap_pad; tp0 += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
              const int tp = tp0 + d;
              const bool live = tp < ntap;
              bf16x8 bfrag[KS];
#pragma unroll
              for (int ks = 0; ks < KS; ++ks) {
                uint4 q = ring[d][ks];
                q.x = live ? q.x : 0u; q.y = live ? q.y : 0u; q.z = live ? q.z : 0u; q.w = live ? q.w : 0u;
                bfrag[ks] = __builtin_bit_cast(bf16x8, q);
              }
              const uint4* wb = wcol + tslab[min(tp + D, ntap - 1)] * slabsz8;
#pragma unroll
              for (int ks = 0; ks < KS; ++ks) ring[d][ks] = wb[ks * np2];
              const int ta = ttoff[min(tp, ntap - 1)] * VS;
#pragma unroll
              for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                  const uint4 av = *reinterpret_cast<const uint4*>(lh + rowaddr[mb] + ta + ks * 16);
                  acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), bfrag[ks], acc[mb], 0, 0, 0);
                }
              }
            }
          }
        } else {
          for (int tp = 0; tp < ntap; ++tp) {
            const uint4* wb = wcol + tslab[tp] * slabsz8;
            const int ta = ttoff[tp] * VS;
            for (int ks = 0; ks < nks; ++ks) {
              const bf16x8 bfrag = __builtin_bit_cast(bf16x8, wb[ks * np2]);
#pragma unroll
              for (int mb = 0; mb < MB; ++mb) {
                const uint4 av = *reinterpret_cast<const uint4*>(lh + rowaddr[mb] + ta + ks * 16);
                acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), bfrag, acc[mb], 0, 0, 0);
              }
            }
          }
        }
      } else if (pipe && stage + 1 < ks1) {
        // a wave without live columns (Np no multiple of 32 * NB) still stages its share of the next box: its prefetch
        // is due all the same, or the next stage commits the registers of this one
        issue(stage + 1);
      }
    } else {
    // ---------------- MFMA over taps x channel pairs ----------------
    if (colact) {
      constexpr int KK = KCI / 2;
      const int kreal = min(KCI, a.Ci - c0);
      const float* wcol = wpn + (long long)c0 * a.Np + colbase + r + (long long)h * a.Np;
      const long long slabsz = (long long)a.Kp * a.Np;
      const int np2 = 2 * a.Np;
      const int ntap = ci.ntaps;
      const int* tslab = a.slab + ci.tap0;
      const int* ttoff = a.toff + ci.tap0;
      if (kreal == KCI) {
        // full stage: branch-free body, weight fragments one tap ahead
        float bcur[KK], bnxt[KK];
        {
          const float* wb = wcol + tslab[0] * slabsz;
#pragma unroll
          for (int kk = 0; kk < KK; ++kk) bcur[kk] = wb[kk * np2];
        }
        for (int tp = 0; tp < ntap; ++tp) {
          const int tn = min(tp + 1, ntap - 1);
          const float* wb = wcol + tslab[tn] * slabsz;
#pragma unroll
          for (int kk = 0; kk < KK; ++kk) bnxt[kk] = wb[kk * np2];
          const int ta = ttoff[tp] * VS;
#pragma unroll
          for (int kk = 0; kk < KK; ++kk) {
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
              const float av = lds[rowaddr[mb] + ta + 2 * kk];
              acc[mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bcur[kk], acc[mb], 0, 0, 0);
            }
          }
#pragma unroll
          for (int kk = 0; kk < KK; ++kk) bcur[kk] = bnxt[kk];
        }
      } else {
        // tail stage (Cin not a multiple of KCI): only the channel pairs that carry data
        const int kkn = (kreal + 1) >> 1;
        for (int tp = 0; tp < ntap; ++tp) {
          const float* wb = wcol + tslab[tp] * slabsz;
          const int ta = ttoff[tp] * VS;
          for (int kk = 0; kk < kkn; ++kk) {
            const float b = wb[kk * np2];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
              const float av = lds[rowaddr[mb] + ta + 2 * kk];
              acc[mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b, acc[mb], 0, 0, 0);
            }
          }
        }
      }
    }
    }
    __syncthreads();
  }

  // ---------------- epilogue ----------------
  const int col = colbase + r;
  const bool colok = colact && col < a.Co;
  float s_sum = 0.f, s_sq = 0.f;
  if (!REUSE && a.ksplit > 1) {
    if (colact) {
      float* wsb = a.ws + ((long long)lbz * gridDim.x + bx) * MT * a.Np + col;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
          const int v = (mg * MB + mb) * 32 + row;
          wsb[(long long)v * a.Np] = acc[mb][i];
        }
    }
    return;
  }
  if (REUSE || a.ovec) {
    // 16-byte stores through a wave-private LDS tile (the K loop ended with a barrier: the box image is dead)
    constexpr int ETF = (REUSE ? 2 : 1) * EPI_TILE_FLOATS;      // (reuse: both blocks of a wave are in the tile at once)
    float v_sum[4], v_sq[4];
    epilogue_vec16<TZ, TY, TX, MB, BF, ABF, REUSE>(a, biasn, ci, acc, lds + wave * ETF, lane, mg * MB, colbase, colact, n, gz0,
                                                   gy0, gx0, v_sum, v_sq);
    if (a.stats != nullptr) {
      float* red = lds + 4 * ETF;      // [4 waves][2][32], behind the four tiles
      if (lane < 8) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          red[(wave * 2 + 0) * 32 + lane * 4 + j] = v_sum[j];
          red[(wave * 2 + 1) * 32 + lane * 4 + j] = v_sq[j];
        }
      }
      __syncthreads();
      if (mg == 0 && h == 0 && colok) {
        float ts = 0.f, tq = 0.f;
#pragma unroll
        for (int g = 0; g < MG; ++g) {
          ts += red[((g * NB + cb) * 2 + 0) * 32 + r];
          tq += red[((g * NB + cb) * 2 + 1) * 32 + r];
        }
        const long long row = (long long)n * a.stats_rows_per_n + cidx * (a.tz * a.ty * a.tx) + tile_in_n;
        a.stats[(row * 2 + 0) * a.Co + col] = ts;
        a.stats[(row * 2 + 1) * a.Co + col] = tq;
      }
    }
    return;
  }
  float bias = 0.f, asc = 1.f, ash = 0.f;
  if (colok) {
    if (biasn) bias = biasn[col];
    if (a.add) nl_coeff(a.tadd, n, a.Co, col, asc, ash);
  }
  // Per 32-row block: addresses and masks of its 16 rows first, then ALL loads of the fused add / accumulate
  // (unconditional, from clamped addresses, under wave-uniform branches), then the arithmetic and the stores: a load
  // inside a per-element branch would be waited for on the spot, 16 exposed round trips per block.
  const int colc = min(col, a.Co - 1);
  const float* addb = a.add;
  float* outb = a.out;
  const long long abase = (long long)n * a.asn + colc, obase = (long long)n * a.osn + colc;
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {       // 8 rows at a time: keeps the kernel at two waves per SIMD
      int ooff[8], aoff[8];                      // element offsets inside batch item n (host checks < 2^31)
      bool ok[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = half * 8 + j;
        const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
        int zl, yl, xl;
        row_to_local<TZ, TY, TX, BF>((mg * MB + mb) * 32 + row, zl, yl, xl);
        const int gz = gz0 + zl, gy = gy0 + yl, gx = gx0 + xl;
        const int oz = gz * a.so + ci.oz, oy = gy * a.so + ci.oy, ox = gx * a.so + ci.ox;
        ok[j] = colok && gz < ci.Dg && gy < ci.Hg && gx < ci.Wg && oz < a.Do && oy < a.Ho && ox < a.Wo;
        const int cz = min(oz, a.Do - 1), cy = min(oy, a.Ho - 1), cx = min(ox, a.Wo - 1);
        ooff[j] = cz * (int)a.osd + cy * (int)a.osh + cx * (int)a.osw;
        aoff[j] = cz * (int)a.asd + cy * (int)a.ash + cx * (int)a.asw;
      }
      float addv[8], oldv[8];
      if (a.add) {
#pragma unroll
        for (int j = 0; j < 8; ++j) addv[j] = ld1_t<ABF>(addb, abase + aoff[j]);
      }
      if (a.accumulate) {
#pragma unroll
        for (int j = 0; j < 8; ++j) oldv[j] = ld1_t<ABF>(outb, obase + ooff[j]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = acc[mb][half * 8 + j] + bias;
        if (a.add) v += nl_apply(addv[j], asc, ash, a.tadd.relu);
        if (a.accumulate) v += oldv[j];
        if (ok[j]) {
          st1_t<ABF>(outb, obase + ooff[j], v);
          s_sum += v;
          s_sq += v * v;
        }
      }
    }
  }
  if (a.stats != nullptr) {
    // lanes l and l+32 hold the same column; waves of different m-groups too.
    s_sum += __shfl_xor(s_sum, 32, 64);
    s_sq += __shfl_xor(s_sq, 32, 64);
    float* red = lds;  // [4 waves][2][32]; safe: the K loop ended with a barrier
    if (h == 0) {
      red[(wave * 2 + 0) * 32 + r] = s_sum;
      red[(wave * 2 + 1) * 32 + r] = s_sq;
    }
    __syncthreads();
    if (mg == 0 && h == 0 && colok) {
      float ts = 0.f, tq = 0.f;
#pragma unroll
      for (int g = 0; g < MG; ++g) {
        ts += red[((g * NB + cb) * 2 + 0) * 32 + r];
        tq += red[((g * NB + cb) * 2 + 1) * 32 + r];
      }
      const long long row = (long long)n * a.stats_rows_per_n + cidx * (a.tz * a.ty * a.tx) + tile_in_n;
      a.stats[(row * 2 + 0) * a.Co + col] = ts;
      a.stats[(row * 2 + 1) * a.Co + col] = tq;
    }
  }
