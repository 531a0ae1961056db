// The body of igemm_cls8_kernel, igemm_cls8_raw_kernel, igemm_cls8_pipe_kernel and igemm_cls8_lean_kernel (conv_igemm.hip): included
// inside each kernel, which names KCI, ABF, RAW, PIPE and LEAN as compile-time constants and has the kernel argument `GArgs a`.  One text and no
// function in between, so that igemm_cls8_kernel compiles to exactly what it was before the other kernels existed
// (conv_igemm_body.h does the same).
// No include guard on purpose: it is included once per kernel.
  constexpr int TZ = 4, TY = 4, TX = 8, VS = KCI + 8, LP = LDS_PITCH_BF16, KS = KCI / 16, KC8 = KCI / 8;
  constexpr int BZ = TZ + 1, BY = TY + 1, BX = TX + 1;
  constexpr int BOX_HW = BZ * BY * LP * VS;                 // halfwords of the box image
  constexpr int WIMG = 27 * KC8 * 32;                       // uint4 entries of the stage's weight image
  extern __shared__ float lds[];
  unsigned short* lh = reinterpret_cast<unsigned short*>(lds);
  uint4* wimg = reinterpret_cast<uint4*>(lh + (BOX_HW + 7) / 8 * 8);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, r = lane & 31;
  int t = blockIdx.x;
  const int tile_in_n = t % (a.tz * a.ty * a.tx);
  const int txi = t % a.tx; t /= a.tx;
  const int tyi = t % a.ty; t /= a.ty;
  const int tzi = t % a.tz;
  const int n = t / a.tz;
  const float* biasn = pset_bias(a.ps, a.bias, n);
  const int gz0 = tzi * TZ, gy0 = tyi * TY, gx0 = txi * TX;
  const int colbase = blockIdx.y * 32;
  const bool colact = colbase < a.Np;

  int zl, yl, xl;
  row_to_local<TZ, TY, TX, true>(wave * 32 + r, zl, yl, xl);
  const unsigned short* arow = lh + ((zl * BY + yl) * LP + xl) * VS + 8 * h;
  const uint4* brow = wimg + h * 32 + r;

  f32x16 acc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[c][i] = 0.f;

  const uint4* wq = reinterpret_cast<const uint4*>(pset_packed(a.ps, a.wp, n));
  const long long slabsz8 = (long long)(a.Kp / 8) * a.Np;
  const unsigned isd = (unsigned)a.isd, ish = (unsigned)a.ish, isw = (unsigned)a.isw;
  const int cmax = ABF ? ((a.Ci - 1) & ~7) : ((a.Ci - 1) & ~3);
  constexpr int AIT = (BZ * BY * BX * KC8 + 255) / 256;      // box items per thread
  constexpr int BIT = (WIMG + 255) / 256;                    // weight entries per thread
  const float relu_lo = act_lo(a.tin.relu);

  // ---- PIPE (igemm_cls8_pipe_kernel; raw staging only): two weight images behind the box, image ks & 1 read by stage ks.
  // The image of stage ks + 1 comes by direct global-to-LDS loads issued behind the barrier that opens stage ks's MFMA
  // phase - no register holds it - and the box items of stage ks + 1 are requested there too and committed behind the
  // barrier that closes stage ks (the single box image is free then).  The plain barriers wait for every outstanding load,
  // so the closing barrier of stage ks retires the image stage ks + 1 reads one barrier later, and the last stage issues
  // nothing: the epilogue finds LDS quiet.  Entry i = tid + 256 j of an image is tap i / 64 = 4 j + wave, lane = (k8l, col):
  // a wave's 64 entries are 1 KiB in lane order, which is what one such load writes; at j = BIT - 1 waves 0-2 have work.
  // What does not depend on the stage is worked out once: the lane's 32-bit weight offset (the tap and the stage move a
  // wave-uniform base), its box offsets, LDS addresses and halo bits.  No ordinary load's result may be used between the
  // issue and the closing barrier (hipcc would wait for every load in flight there, the image included), a spill reload
  // counts, and the operand reads of the MFMA phase are typed loads (cls8_lds_q) for the same reason.
  static_assert(!PIPE || (RAW && ABF && KC8 * 32 == 64 && WIMG % 64 == 0), "the pipelined form: raw staging of 16-channel stages");
  unsigned wlane = 0u;      // the lane's byte offset inside a tap's two rows of the packed image
  unsigned poff[AIT], phalo = 0u;
  auto pipe_cv8 = [&](int j) { return (min(tid + 256 * j, BZ * BY * BX * KC8 - 1) % KC8) * 8; };      // item j's chunk in the stage
  int plds[AIT];
  Oct8<ABF> pav[AIT];
  if constexpr (PIPE) {
    wlane = (unsigned)((lane >> 5) * a.Np + colbase + (lane & 31)) * 16u;
#pragma unroll
    for (int j = 0; j < AIT; ++j) {
      const int i = min(tid + 256 * j, BZ * BY * BX * KC8 - 1);
      const int cv = i % KC8, bv = i / KC8;
      const int bz = bv / (BY * BX), brem = bv - bz * (BY * BX), by = brem / BX, bx = brem - by * BX;
      const int iz = gz0 + bz, iy = gy0 + by, ix = gx0 + bx;
      phalo |= ((iz < a.Di && iy < a.Hi && ix < a.Wi) ? 1u : 0u) << j;
      poff[j] = __umul24((unsigned)min(iz, a.Di - 1), isd) + __umul24((unsigned)min(iy, a.Hi - 1), ish) +
                __umul24((unsigned)min(ix, a.Wi - 1), isw) + cv * 8;
      plds[j] = ((bz * BY + by) * LP + bx) * VS + cv * 8;
    }
  }
  auto pipe_issue = [&](int ks) {      // the weight image and the box items of stage ks
    if constexpr (PIPE) {
    const char* src = reinterpret_cast<const char*>(wq + (long long)ks * KC8 * a.Np);      // wave-uniform; the lane adds 32 bits
    uint4* dst = wimg + (ks & 1) * WIMG + 64 * wave;
#pragma unroll
    for (int j = 0; j < BIT; ++j)
      if (j < BIT - 1 || 256 * j + 64 * wave < WIMG)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (long long)(4 * j + wave) * slabsz8 * 16 + wlane),
                                         (__attribute__((address_space(3))) void*)(dst + 256 * j), 16, 0, 0);
    const int c0 = ks * KCI;
    const float* sb = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.in) + ((long long)n * a.isn + c0) * 2);
#pragma unroll
    for (int j = 0; j < AIT; ++j) {
      const int over = max(c0 + pipe_cv8(j) - cmax, 0);      // a chunk past Ci re-reads the last valid one; the mask blanks it
      pav[j] = oct8_ld<ABF>(sb, poff[j] - over, 0u);
    }
    }
  };
  auto pipe_commit = [&](int ks) {     // the box items of stage ks, as loaded, under halo and chunk mask
    if constexpr (PIPE) {
#pragma unroll
    for (int j = 0; j < AIT; ++j) {
      const unsigned okm = (((phalo >> j) & 1u) && ks * KCI + pipe_cv8(j) < a.Ci) ? 0xffffffffu : 0u;
      uint4 pk = pav[j].q;
      pk.x &= okm; pk.y &= okm; pk.z &= okm; pk.w &= okm;
      if (tid + 256 * j < BZ * BY * BX * KC8) *reinterpret_cast<uint4*>(lh + plds[j]) = pk;
    }
    }
  };
  if constexpr (PIPE) {
    __builtin_assume(a.nstages > 0);      // (K >= 1: no path around the loop; with one the epilogue spills one register more)
    pipe_issue(0);
  }

  for (int ks = 0; ks < a.nstages; ++ks) {
    const uint4* const bst = PIPE ? brow + (ks & 1) * WIMG : brow;      // the stage's weight image
    if constexpr (PIPE) {
      pipe_commit(ks);
    } else {
    const int c0 = ks * KCI;
    const float* sb = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.in) + ((long long)n * a.isn + c0) * (ABF ? 2 : 4));
    // ---- requests first: weights of the stage, norm-on-load coefficients, box items (one round trip for all of them)
    uint4 wv[BIT];
#pragma unroll
    for (int j = 0; j < BIT; ++j) {
      const int i = min(tid + 256 * j, WIMG - 1);
      const int tap = i / (KC8 * 32), rem = i - tap * (KC8 * 32), k8l = rem >> 5, col = rem & 31;
      wv[j] = wq[tap * slabsz8 + (long long)(c0 / 8 + k8l) * a.Np + colbase + col];
    }
    Oct8<ABF> av[AIT];
    unsigned aok = 0u;
    int alds[AIT];
#pragma unroll
    for (int j = 0; j < AIT; ++j) {
      const int i = min(tid + 256 * j, BZ * BY * BX * KC8 - 1);
      const int cv = i % KC8, bv = i / KC8;
      const int bz = bv / (BY * BX), brem = bv - bz * (BY * BX), by = brem / BX, bx = brem - by * BX;
      const int iz = gz0 + bz, iy = gy0 + by, ix = gx0 + bx;
      bool ok = iz < a.Di && iy < a.Hi && ix < a.Wi;
      // RAW: no zero coefficients blank the chunks past Ci of a partial last stage (the re-read last valid chunk): the mask does
      if constexpr (RAW) ok = ok && c0 + cv * 8 < a.Ci;
      aok |= (ok ? 1u : 0u) << j;
      const unsigned off = __umul24((unsigned)min(iz, a.Di - 1), isd) + __umul24((unsigned)min(iy, a.Hi - 1), ish) +
                           __umul24((unsigned)min(ix, a.Wi - 1), isw) + cv * 8;
      const int over = max(c0 + cv * 8 - cmax, 0), over_hi = max(c0 + cv * 8 + 4 - cmax, 0);
      av[j] = oct8_ld<ABF>(sb, off - over, off + 4 - over_hi);
      alds[j] = ((bz * BY + by) * LP + bx) * VS + cv * 8;
    }
    float sc[AIT][8], sh[AIT][8];
    if constexpr (!RAW) {
#pragma unroll
    for (int j = 0; j < AIT; ++j) {
      const int i = min(tid + 256 * j, BZ * BY * BX * KC8 - 1);
      nl_coeff_vec<8>(a.tin, n, a.Ci, c0 + (i % KC8) * 8, sc[j], sh[j]);
    }
    }
    // ---- commit
#pragma unroll
    for (int j = 0; j < BIT; ++j)
      if (tid + 256 * j < WIMG) wimg[tid + 256 * j] = wv[j];
#pragma unroll
    for (int j = 0; j < AIT; ++j) {
      const unsigned okm = ((aok >> j) & 1u) ? 0xffffffffu : 0u;
      uint4 pk;
      if constexpr (RAW) {      // the item as loaded, under its mask
        pk = av[j].q;
        pk.x &= okm; pk.y &= okm; pk.z &= okm; pk.w &= okm;
      } else {
      float v[8];
      oct8_f8(av[j], v);
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = act_max(fmaf(v[q], sc[j][q], sh[j][q]), relu_lo);
      pk.x = pack_bf16x2(v[0], v[1]) & okm; pk.y = pack_bf16x2(v[2], v[3]) & okm;
      pk.z = pack_bf16x2(v[4], v[5]) & okm; pk.w = pack_bf16x2(v[6], v[7]) & okm;
      }
      if (tid + 256 * j < BZ * BY * BX * KC8) *reinterpret_cast<uint4*>(lh + alds[j]) = pk;
    }
    }
    __syncthreads();
    if constexpr (PIPE) {
      if (ks + 1 < a.nstages) pipe_issue(ks + 1);
    }
    // ---- MFMAs: 8 activation fragments per k step (one per tap offset), then the 27 (class, tap) products; weight
    // fragment f is read LA products ahead through a ring (a fence per MFMA keeps the reads where they are written)
    if (colact) {
#pragma unroll
      for (int k16 = 0; k16 < KS; ++k16) {
        uint4 af[8];
#pragma unroll
        for (int d = 0; d < 8; ++d)
          af[d] = cls8_lds_q<PIPE>(arow + ((((d >> 2) & 1) * BY + ((d >> 1) & 1)) * LP + (d & 1)) * VS + k16 * 16);
        constexpr int LA = 3;
        uint4 bring[LA + 1];
        static_for<0, LA>([&](auto fc) {
          constexpr int f = decltype(fc)::value;
          bring[f] = cls8_lds_q<PIPE>(bst + (cls_tap(f).slab * KC8 + k16 * 2) * 32);
        });
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, 27>([&](auto fc) {
          constexpr int f = decltype(fc)::value;
          constexpr ClsTap ct = cls_tap(f);
          if constexpr (f + LA < 27) bring[(f + LA) % (LA + 1)] = cls8_lds_q<PIPE>(bst + (cls_tap(f + LA).slab * KC8 + k16 * 2) * 32);
          acc[ct.cls] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[ct.d]),
                                                                __builtin_bit_cast(bf16x8, bring[f % (LA + 1)]), acc[ct.cls], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        });
      }
    }
    __syncthreads();
  }
  // ---- epilogue: every class's 32 x 32 block through this wave's LDS transposition tile (the box image is dead)
  float tsum[4] = {0.f, 0.f, 0.f, 0.f}, tsq[4] = {0.f, 0.f, 0.f, 0.f};
  // LEAN (igemm_cls8_lean_kernel): one workgroup-uniform test per tile.  The tile's 8 x 8 x 16 output block lies wholly inside
  // the tensor when the class of odd parity on every axis - the shortest: it ends one voxel early at an odd extent - has its
  // last row inside, 2 (g0 + T - 1) + 1 < extent; that is also g0 + T <= Dg of every class.  Such a tile takes
  // epilogue_cls8_lean, every other one the eight calls below.
  bool lean_tile = false;
  if constexpr (LEAN) lean_tile = 2 * (gz0 + TZ) <= a.Do && 2 * (gy0 + TY) <= a.Ho && 2 * (gx0 + TX) <= a.Wo;
  if (lean_tile) {
    if constexpr (LEAN)
      epilogue_cls8_lean<ABF>(a, biasn, acc, lds + wave * EPI_TILE_FLOATS, lane, wave, colbase, colact, n, gz0, gy0, gx0, tsum, tsq);
  } else {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float v_sum[4], v_sq[4];
    epilogue_vec16<TZ, TY, TX, 1, true, ABF>(a, biasn, a.cls[c], *reinterpret_cast<f32x16(*)[1]>(&acc[c]), lds + wave * EPI_TILE_FLOATS,
                                             lane, wave, colbase, colact, n, gz0, gy0, gx0, v_sum, v_sq);
#pragma unroll
    for (int j = 0; j < 4; ++j) { tsum[j] += v_sum[j]; tsq[j] += v_sq[j]; }
  }
  }
  if (a.stats != nullptr) {
    float* red = lds + 4 * EPI_TILE_FLOATS;      // [4 waves][2][32], behind the four tiles
    if (lane < 8) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        red[(wave * 2 + 0) * 32 + lane * 4 + j] = tsum[j];
        red[(wave * 2 + 1) * 32 + lane * 4 + j] = tsq[j];
      }
    }
    __syncthreads();
    const int col = colbase + tid;
    if (tid < 32 && col < a.Co) {
      float ts = 0.f, tq = 0.f;
#pragma unroll
      for (int g = 0; g < 4; ++g) { ts += red[(g * 2 + 0) * 32 + tid]; tq += red[(g * 2 + 1) * 32 + tid]; }
      const long long row = (long long)n * a.stats_rows_per_n + tile_in_n;
      a.stats[(row * 2 + 0) * a.Co + col] = ts;
      a.stats[(row * 2 + 1) * a.Co + col] = tq;
    }
  }
