// Body of chan_mfma_kernel and chan_mfma_lean_kernel (conv_direct.hip): the text is included into both; `LEAN` (a constexpr
// bool of the including kernel) switches the lean stage and epilogue in.  With LEAN = false every site below is what
// chan_mfma_kernel was before the split.
//
// LEAN (MMTTA_OPT_THIN_LEAN bit 0; host: chan_lean_applicable): y and the fused add are bf16-stored with 16-byte rows,
// N == 32 * NB exactly, no accumulate.  The accumulator layout is "lanes along N" (lane = channel), which made the store of
// a bf16 row a cross-lane exchange through LDS per value (ds_bpermute) and a 4-byte store from half the lanes, each under
// three predicates.  Here the values of a wave (32 voxels x N channels) go through a wave-private LDS tile instead:
//   * a pair of accumulators (voxels m, m + 1 of one channel) is rounded to one bf16x2 dword, exchanged with the
//     neighbouring channel's lane by a DPP move (quad_perm [1,0,3,2], a plain VALU op) and recombined by one v_perm_b32:
//     the even lane ends up with voxel m, the odd lane with voxel m + 1, channels (r & ~1, r | 1) - one ds_write_b32 per
//     pair from EVERY lane, no predicate;
//   * the tile comes back as 16-byte items, 8 channels of one voxel per lane: 2 * NB global_store_dwordx4 per lane;
//   * the fused add is loaded the same way (16-byte items, all issued before the first use), parked in the tile and read
//     per value as ds_read_u16, so that val = acc + bias + NL(add) and the per-lane statistics sums keep their order;
//   * a workgroup-uniform test picks the interior form: no spatial mask on the sums or the stores.
// Tile layout (dwords): voxel (yl, xl) of the z-slice sits at ((xl & 3) + 4 yl) * RD + (xl >> 2) * HP, RD = 16 NB dwords of
// channels; HP pads the xl >= 4 half so that the 64 lanes of one ds_write_b32 (2 voxels x 2 halves x 16 dwords) fall on
// 64 distinct banks.
  constexpr int TZ = 4, TY = 4, TX = 8;
  constexpr int BZ = (TZ - 1) * S + 3, BY = (TY - 1) * S + 3, BX = (TX - 1) * S + 3, BOX = BZ * BY * BX;
  __shared__ uint2 box[BOX];                       // 4 bf16 channels per voxel
  __shared__ float red[2][4][32 * NB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, r = lane & 31;
  int t = blockIdx.x;
  const int tile_in_n = t % a.tiles_per_n;
  const int txi = t % a.tx; t /= a.tx;
  const int tyi = t % a.ty; t /= a.ty;
  const int tzi = t % a.tz;
  const int n = t / a.tz;
  a.w = pset_packed(a.ps, a.w, n); a.bias = pset_bias(a.ps, a.bias, n);      // this batch item's parameter set
  const int oz0 = tzi * TZ, oy0 = tyi * TY, ox0 = txi * TX;
  const int iz0 = oz0 * S - 1, iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
  const int N = a.out.c;
  // ---- LEAN: the 16-byte items of this lane (store and fused add): item c = lane + 64 j is channels 8 * (c % CPV) ... + 7 of
  // voxel c / CPV of the wave's z-slice
  constexpr int LRD = 16 * NB, LHP = 16 * LRD + (NB == 1 ? 32 : 16), LWT = 2 * 16 * LRD + (NB == 1 ? 32 : 16);
  constexpr int LNJ = LEAN ? 2 * NB : 1;
  constexpr bool EARLY_ADD = NB == 1;              // NB = 2 sits at 152 registers: its add items are loaded in the epilogue
  unsigned lgo[LNJ], lao[LNJ], ltl[LNJ], lok = 0u;
  uint4 addq[LNJ];
  bool interior = false;
  if constexpr (LEAN) {
    constexpr int CPV = 4 * NB;
    const int oz = oz0 + wave;
    interior = oz0 + TZ <= a.out.d && oy0 + TY <= a.out.h && ox0 + TX <= a.out.w;
#pragma unroll
    for (int j = 0; j < LNJ; ++j) {
      const int c = lane + 64 * j;
      const int v = c / CPV, part = c % CPV;
      const int yl = v >> 3, xl = v & 7;
      const int oy = oy0 + yl, ox = ox0 + xl;
      lok |= ((oz < a.out.d && oy < a.out.h && ox < a.out.w) ? 1u : 0u) << j;
      lgo[j] = (unsigned)oy * (unsigned)a.out.sh + (unsigned)ox * (unsigned)a.out.sw + (unsigned)(part * 8);
      lao[j] = (unsigned)oy * (unsigned)a.ash + (unsigned)ox * (unsigned)a.asw + (unsigned)(part * 8);
      ltl[j] = (unsigned)(((xl & 3) + 4 * yl) * LRD + (xl >> 2) * LHP + part * 4);
      addq[j] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
  auto load_add = [&]() {
    if constexpr (LEAN) {
      if (a.add != nullptr) {
        const unsigned short* ap = reinterpret_cast<const unsigned short*>(a.add) + ((long long)n * a.asn + (long long)(oz0 + wave) * a.asd);
#pragma unroll
        for (int j = 0; j < LNJ; ++j)
          if (interior || ((lok >> j) & 1u)) addq[j] = *reinterpret_cast<const uint4*>(ap + lao[j]);
      }
    }
  };
  if constexpr (LEAN && EARLY_ADD) load_add();
  {  // ---- stage the halo box: all loads (clamped) first, then transform / zero-fill / round to bf16.
     // A thread keeps one box column bx and walks box rows (bz, by): the x clamp and mask are computed once, a row costs one
     // small decode, offsets are 32-bit elements from the batch item (host-checked), validity travels as a bit mask.
    constexpr int RPP = 256 / BX, NROW = BZ * BY, NQ = (NROW + RPP - 1) / RPP;
    float sc[4] = {1.f, 1.f, 1.f, 1.f}, sh[4] = {0.f, 0.f, 0.f, 0.f};
    if (HAS_T) nl_coeff_vec<4>(a.tin, n, KI, 0, sc, sh);
    const float* inb = XBF ? reinterpret_cast<const float*>(reinterpret_cast<const unsigned short*>(a.in.p) + (long long)n * a.in.sn)
                           : a.in.p + (long long)n * a.in.sn;
    const int bx = tid % BX, r0 = tid / BX;
    const int ix = ix0 + bx;
    const bool xok = (unsigned)ix < (unsigned)a.in.w && r0 < RPP;
    const unsigned xoff = (unsigned)min(max(ix, 0), a.in.w - 1) * (unsigned)a.in.sw;
    const unsigned sd = (unsigned)a.in.sd, shh = (unsigned)a.in.sh;
    float4 raw[NQ];
    uint2 rawh[NQ];
    unsigned okm = 0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int row = min(r0 + q * RPP, NROW - 1);
      const int by = row % BY, bz = row / BY;
      const int iz = iz0 + bz, iy = iy0 + by;
      const bool ok = xok && (unsigned)iz < (unsigned)a.in.d && (unsigned)iy < (unsigned)a.in.h;
      okm |= (ok ? 1u : 0u) << q;
      const unsigned off = (unsigned)min(max(iz, 0), a.in.d - 1) * sd + (unsigned)min(max(iy, 0), a.in.h - 1) * shh + xoff;
      if constexpr (XBF) rawh[q] = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(inb) + off);
      else raw[q] = *reinterpret_cast<const float4*>(inb + off);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int row = r0 + q * RPP;
      if (r0 < RPP && row < NROW) {
        const bool ok = (okm >> q) & 1u;
        if constexpr (XBF && !HAS_T && KI == 4) {           // already what the image holds: mask and store
          const unsigned m = ok ? 0xffffffffu : 0u;
          box[row * BX + bx] = make_uint2(rawh[q].x & m, rawh[q].y & m);
          continue;
        }
        if constexpr (LEAN && XBF && !HAS_T) {
          // KI < 4 the same way: unpack, select and round return the stored bits of channels < KI and +0 behind them, which
          // is a mask.  (The lanes behind KI are masked, not trusted: a pad lane need not hold zeros.)
          const unsigned mx = ok ? (KI >= 2 ? 0xffffffffu : 0xffffu) : 0u;
          const unsigned my = ok ? (KI >= 4 ? 0xffffffffu : KI == 3 ? 0xffffu : 0u) : 0u;
          box[row * BX + bx] = make_uint2(rawh[q].x & mx, rawh[q].y & my);
          continue;
        }
        if constexpr (XBF)
          raw[q] = make_float4(bf16_bits_to_f32(rawh[q].x & 0xffffu), __uint_as_float(rawh[q].x & 0xffff0000u),
                               bf16_bits_to_f32(rawh[q].y & 0xffffu), __uint_as_float(rawh[q].y & 0xffff0000u));
        float r4[4] = {raw[q].x, raw[q].y, raw[q].z, raw[q].w};
        if (KI == 1) r4[0] = a.koff == 0 ? raw[q].x : a.koff == 1 ? raw[q].y : a.koff == 2 ? raw[q].z : raw[q].w;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          v[k] = (ok && k < KI) ? (HAS_T ? nl_apply(r4[k], sc[k], sh[k], a.tin.relu) : r4[k]) : 0.f;
        uint2 pk;
        pk.x = __builtin_bit_cast(unsigned int, __builtin_convertvector((float2_t){v[0], v[1]}, bf16x2_t));
        pk.y = __builtin_bit_cast(unsigned int, __builtin_convertvector((float2_t){v[2], v[3]}, bf16x2_t));
        box[row * BX + bx] = pk;
      }
    }
  }
  // ---- B fragments: k = s*16 + h*8 + e  <->  tap = s*4 + h*2 + (e >> 2), channel = e & 3; column = nb*32 + r: the
  // fragment-ordered bf16 image behind the fp32 tap image of this batch item's packed weights (chan_frag_bytes, written by
  // the pack kernels): one 16-byte load per fragment and lane, issued before the box is staged
  uint4 wfrag[7][NB];
  {
    const uint4* fr = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(a.w) + (size_t)27 * a.Kp * a.Np * 4) + lane;
#pragma unroll
    for (int s2 = 0; s2 < 7; ++s2)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) wfrag[s2][nb] = fr[(s2 * NB + nb) * 64];
  }
  float bias[NB], asc[NB], ash[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int col = min(nb * 32 + r, N - 1);
    bias[nb] = a.bias ? a.bias[col] : 0.f;
    asc[nb] = 1.f; ash[nb] = 0.f;
    if (a.add) nl_coeff(a.tadd, n, N, col, asc[nb], ash[nb]);
  }
  __syncthreads();
  // ---- A fragments: MFMA row m = r  <->  voxel (zl = wave, yl = m / 8, xl = m % 8)
  ufloat16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;
  {
    const int xl = r % TX, yl = r / TX;
    const uint2* bp = box + ((wave * S) * BY + yl * S) * BX + xl * S;
    uint2 av[7][2];
#pragma unroll
    for (int s2 = 0; s2 < 7; ++s2)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int tap = min(s2 * 4 + h * 2 + j, 26);           // tap 27: any valid address, its weights are zero
        const int dz = tap / 9, dy = (tap / 3) % 3, dx = tap % 3;
        av[s2][j] = bp[(dz * BY + dy) * BX + dx];
      }
#pragma unroll
    for (int s2 = 0; s2 < 7; ++s2) {
      const uint4 a4 = make_uint4(av[s2][0].x, av[s2][0].y, av[s2][1].x, av[s2][1].y);
      const ubf16x8 af = __builtin_bit_cast(ubf16x8, a4);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, __builtin_bit_cast(ubf16x8, wfrag[s2][nb]), acc[nb], 0, 0, 0);
    }
  }
  // ---- epilogue: accumulator i of lane (h, r) = voxel m = (i & 3) + 8 * (i >> 2) + 4 * h, channel nb*32 + r
  float ssum[NB], ssq[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) { ssum[nb] = 0.f; ssq[nb] = 0.f; }
  // voxel m of accumulator i: row oy0 + (i >> 2), column ox0 + (i & 3) + 4 * h; the z-slice (wave) is uniform.  Offsets are
  // 32-bit elements from the slice (host-checked): four row terms plus four column terms, one add per store.
  const int oz = oz0 + wave;
  const bool zok = oz < a.out.d;
  if constexpr (LEAN) {
    __shared__ uint4 otile[4 * LWT / 4];           // one tile per wave; never shared between waves: no workgroup barrier
    unsigned int* const tw = reinterpret_cast<unsigned int*>(otile) + wave * LWT;
    if constexpr (!EARLY_ADD) load_add();
    unsigned okrow = 0, okcol = 0;                 // border tiles: the spatial mask of the sums, per row and per column
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      okrow |= (zok && oy0 + j < a.out.h ? 1u : 0u) << j;
      okcol |= (ox0 + j + 4 * h < a.out.w ? 1u : 0u) << j;
    }
    if (a.add != nullptr) {
      // the add items of the wave -> tile -> the accumulator layout: value (i, nb) of lane (h, r) is halfword r & 1 of
      // dword nb * 16 + (r >> 1) of its voxel's row.  (An item outside the tensor is zeros; its values are never used.)
#pragma unroll
      for (int j = 0; j < LNJ; ++j) *reinterpret_cast<uint4*>(tw + ltl[j]) = addq[j];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const unsigned short* th = reinterpret_cast<const unsigned short*>(tw) + 2 * (h * LHP + (r >> 1)) + (r & 1);
#pragma unroll
      for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          const float av = bf16_bits_to_f32(th[2 * (((i & 3) + 4 * (i >> 2)) * LRD + nb * 16)]);
          acc[nb][i] = (acc[nb][i] + bias[nb]) + nl_apply(av, asc[nb], ash[nb], a.tadd.relu);
        }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb][i] = acc[nb][i] + bias[nb];
    }
    // statistics: per lane over i = 0 ... 15 in order, as the plain epilogue sums them.  Its `ssq += val * val` is left to
    // hipcc's contraction, which in the bf16-row epilogue of every chan_mfma_kernel instantiation fuses every square (in the
    // fp32-row epilogue none); left to itself here it fused some and multiplied the others in pairs.  The rows are equal
    // bit for bit only with the same roundings, so the fused form is spelled out and implicit contraction is off
    // (tests/test_hip_thin_lean.py compares the two kernels).
    {
#pragma clang fp contract(off)
      auto square = [&](int i, int nb) {
#pragma clang fp contract(off)
        const float val = acc[nb][i];
        ssum[nb] += val;
        ssq[nb] = fmaf(val, val, ssq[nb]);
      };
      if (interior) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) square(i, nb);
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const bool vok = ((okrow >> (i >> 2)) & (okcol >> (i & 3)) & 1u) != 0;
#pragma unroll
          for (int nb = 0; nb < NB; ++nb)
            if (vok) square(i, nb);
        }
      }
    }
    {  // values -> tile: (voxel m, m + 1) x (channel r, r ^ 1) between a lane and its neighbour
      const unsigned sel = (r & 1) ? 0x03020706u : 0x05040100u;      // odd lane: (neighbour.hi, own.hi); even: (own.lo, neighbour.lo)
      unsigned int* const tp = tw + h * LHP + (r & 1) * LRD + (r >> 1);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");          // (the add values are read: the tile is free)
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int i = 0; i < 16; i += 2)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          const unsigned own = f32x2_to_bf16x2(acc[nb][i], acc[nb][i + 1]);
          const unsigned nei = (unsigned)__builtin_amdgcn_update_dpp(0, (int)own, 0xb1, 0xf, 0xf, true);      // lane ^ 1
          tp[((i & 3) + 4 * (i >> 2)) * LRD + nb * 16] = __builtin_amdgcn_perm(nei, own, sel);
        }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    unsigned short* const outh = reinterpret_cast<unsigned short*>(a.out.p) + ((long long)n * a.out.sn + (long long)oz * a.out.sd);
    uint4 oq[LNJ];
#pragma unroll
    for (int j = 0; j < LNJ; ++j) oq[j] = *reinterpret_cast<const uint4*>(tw + ltl[j]);
    if (interior) {
#pragma unroll
      for (int j = 0; j < LNJ; ++j) *reinterpret_cast<uint4*>(outh + lgo[j]) = oq[j];
    } else {
#pragma unroll
      for (int j = 0; j < LNJ; ++j)
        if ((lok >> j) & 1u) *reinterpret_cast<uint4*>(outh + lgo[j]) = oq[j];
    }
  } else {
  unsigned oyo[4], oxo[4], ayo[4], axo[4];
  unsigned okrow = 0, okcol = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int oy = oy0 + j, ox = ox0 + j + 4 * h;
    okrow |= (zok && oy < a.out.h ? 1u : 0u) << j;
    okcol |= (ox < a.out.w ? 1u : 0u) << j;
    oyo[j] = (unsigned)oy * (unsigned)a.out.sh; oxo[j] = (unsigned)ox * (unsigned)a.out.sw;
    ayo[j] = (unsigned)oy * (unsigned)a.ash; axo[j] = (unsigned)ox * (unsigned)a.asw;
  }
  const long long obase = (long long)n * a.out.sn + (long long)oz * a.out.sd;
  const long long abase = (long long)n * a.asn + (long long)oz * a.asd;
  MMTTA_BF_DISPATCH(a.out.bf, OBF, {
    float* const outp = OBF ? reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(a.out.p) + obase) : a.out.p + obase;
    const float* const addp = a.add == nullptr ? nullptr
                              : (OBF ? reinterpret_cast<const float*>(reinterpret_cast<const unsigned short*>(a.add) + abase) : a.add + abase);
_Pragma("unroll")
    for (int i = 0; i < 16; ++i) {
      const bool vok = ((okrow >> (i >> 2)) & (okcol >> (i & 3)) & 1u) != 0;
      const unsigned ooff = oyo[i >> 2] + oxo[i & 3];
      const unsigned aoff = ayo[i >> 2] + axo[i & 3];
_Pragma("unroll")
      for (int nb = 0; nb < NB; ++nb) {
        const int col = nb * 32 + r;
        const bool live = vok && col < N;
        float val = acc[nb][i] + bias[nb];
        // fused add / accumulate operands share the output's storage type (host-checked)
        if (a.add) val += nl_apply(live ? ld1_t<OBF>(addp, aoff + col) : 0.f, asc[nb], ash[nb], a.tadd.relu);
        if (a.accumulate && live) val += ld1_t<OBF>(outp, ooff + col);
        if constexpr (OBF) {
          // bf16 rows: neighbouring channel lanes pair up, the even one stores both as one dword (a 2-byte store per
          // lane is a partial-dword write: ~12x the time per byte of a full store)
          const float other = __shfl_xor(val, 1, 64);
          if (live && !(r & 1)) {
            if (col + 1 < N) reinterpret_cast<unsigned int*>(reinterpret_cast<unsigned short*>(outp) + ooff + col)[0] = f32x2_to_bf16x2(val, other);
            else st1_t<true>(outp, ooff + col, val);
          }
        } else {
          if (live) outp[ooff + col] = val;
        }
        if (live) { ssum[nb] += val; ssq[nb] += val * val; }
      }
    }
  });
  }
  if (a.stats != nullptr) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const float s0 = ssum[nb] + __shfl_xor(ssum[nb], 32, 64), s1 = ssq[nb] + __shfl_xor(ssq[nb], 32, 64);
      if (h == 0) { red[0][wave][nb * 32 + r] = s0; red[1][wave][nb * 32 + r] = s1; }
    }
    __syncthreads();
    if (tid < 32 * NB && tid < N) {
      const float s0 = (red[0][0][tid] + red[0][1][tid]) + (red[0][2][tid] + red[0][3][tid]);
      const float s1 = (red[1][0][tid] + red[1][1][tid]) + (red[1][2][tid] + red[1][3][tid]);
      const long long row = (long long)n * a.tiles_per_n + tile_in_n;
      a.stats[(row * 2 + 0) * N + tid] = s0;
      a.stats[(row * 2 + 1) * N + tid] = s1;
    }
  }
