// The body of conv3_mfma4_kernel and conv3_mfma4_loss_kernel (conv_direct.hip): included inside each kernel, which names
// HAS_T, TZ and GBF as compile-time constants and has the kernel argument `DArgs a`.  One text and no function in between, so
// that conv3_mfma4_kernel compiles to exactly what it was before its twin existed (conv_igemm_body.h and
// conv_wgrad_tr_body.h do the same).  No include guard on purpose.
// MMTTA_HEAD_LOSS_BODY (defined around the twin's include; GBF = false there): the epilogue stores no output.  The value it
// would have stored is the logit of (voxel, region jc); the lane takes its Bernoulli entropy terms (voxel_loss.h), the
// voxel's h is summed over the regions in order across the four lanes of the voxel and enters a double accumulator once,
// and g / count goes to `hl.dz` (HeadLoss: the kernel's second argument) as loss_vec_kernel would have stored it.
  // 8 x 8 x 64 tile: the halo box is 1.6x the tile.  The box rows are padded to 68 voxels so that a staging item is a run
  // of 4 voxels along x (one decode, one row address, four 16-byte loads): phase timing of the first version showed 26 of
  // its 44 us in per-voxel index / address arithmetic and in 108 scalar weight loads per lane, not in loads or MFMAs.
  constexpr int TY = 8, TX = 64, BZ = TZ + 2, BY = TY + 2, BX = 68, RUNS = BX / 4, NRUN = BZ * BY * RUNS;
  __shared__ uint2 box[BZ * BY * BX];
  __shared__ uint2 wtab[27 * 4];                // [tap][column] x 4 k values (bf16)
  __shared__ float red[32];
  const int n = blockIdx.y;
  a.w = pset_packed(a.ps, a.w, n); a.bias = pset_bias(a.ps, a.bias, n);      // this batch item's parameter set
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int txn = (a.out.w + TX - 1) / TX, tyn = (a.out.h + TY - 1) / TY;
  int t = blockIdx.x;
  const int txi = t % txn; t /= txn;
  const int tyi = t % tyn;
  const int tzi = t / tyn;
  const int oz0 = tzi * TZ, oy0 = tyi * TY, ox0 = txi * TX;
  // ---- B operand table: column j of tap tp = the 4 k values w[tp][k][j] (fp32 image [tap][K][4], mirrored for the gradient)
  if (tid < 27 * 4) {
    const int tp = tid >> 2, j = tid & 3;
    const float* wt = a.w + (a.transposed ? 26 - tp : tp) * a.K * 4;
    float wk[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) wk[k] = (k < a.K && j < a.N) ? wt[k * 4 + j] : 0.f;
    wtab[tid] = make_uint2(f32x2_to_bf16x2(wk[0], wk[1]), f32x2_to_bf16x2(wk[2], wk[3]));
  }
  {  // ---- stage the halo box: runs of 4 voxels, two runs (8 loads) in flight per thread
    constexpr int NIT = (NRUN + 255) / 256, RND = NIT;      // every load of the box in flight at once (RND = 2: two dependent round trips)
    float sc[4] = {1.f, 1.f, 1.f, 1.f}, sh[4] = {0.f, 0.f, 0.f, 0.f};
    if (HAS_T) nl_coeff_vec<4>(a.tin, n, a.K, 0, sc, sh);          // channels >= K: scale = shift = 0
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k >= a.K) { sc[k] = 0.f; sh[k] = 0.f; }                   // pad lanes of the voxel row may hold anything
    const float relu_lo = act_lo(HAS_T ? a.tin.relu : MMTTA_ACT_ID);
    const float* inb = GBF ? reinterpret_cast<const float*>(reinterpret_cast<const unsigned short*>(a.in.p) + (long long)n * a.in.sn)
                           : a.in.p + (long long)n * a.in.sn;
    const unsigned isw = (unsigned)a.in.sw;
#pragma unroll 1
    for (int j0 = 0; j0 < NIT; j0 += RND) {
      float4 raw[RND][4];
      unsigned okm = 0u;
#pragma unroll
      for (int j = 0; j < RND; ++j) {
        const int v = min(tid + 256 * (j0 + j), NRUN - 1);
        const int bz = v / (BY * RUNS), rem = v - bz * (BY * RUNS), by = rem / RUNS, run = rem - by * RUNS;
        const int iz = oz0 - 1 + bz, iy = oy0 - 1 + by, ix = ox0 - 1 + 4 * run;
        const bool rok = (unsigned)iz < (unsigned)a.in.d && (unsigned)iy < (unsigned)a.in.h;
        const long long rowo = (long long)min(max(iz, 0), a.in.d - 1) * a.in.sd + (long long)min(max(iy, 0), a.in.h - 1) * a.in.sh;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          okm |= ((rok && (unsigned)(ix + q) < (unsigned)a.in.w) ? 1u : 0u) << (4 * j + q);
          const long long eo = rowo + (unsigned)min(max(ix + q, 0), a.in.w - 1) * isw;
          if constexpr (GBF) {          // the four bf16 channels travel in two dwords of the raw register
            const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(inb) + eo);
            raw[j][q].x = __uint_as_float(u.x); raw[j][q].y = __uint_as_float(u.y);
          } else {
            raw[j][q] = *reinterpret_cast<const float4*>(inb + eo);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < RND; ++j) {
        uint2 pk[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if constexpr (GBF) {
            const unsigned ux = __float_as_uint(raw[j][q].x), uy = __float_as_uint(raw[j][q].y);
            raw[j][q] = make_float4(bf16_bits_to_f32(ux & 0xffffu), __uint_as_float(ux & 0xffff0000u),
                                    bf16_bits_to_f32(uy & 0xffffu), __uint_as_float(uy & 0xffff0000u));
          }
          const float xs[4] = {raw[j][q].x, raw[j][q].y, raw[j][q].z, raw[j][q].w};
          float v4[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) v4[k] = act_max(fmaf(xs[k], sc[k], sh[k]), relu_lo);
          const unsigned m = ((okm >> (4 * j + q)) & 1u) ? 0xffffffffu : 0u;
          pk[q].x = f32x2_to_bf16x2(v4[0], v4[1]) & m; pk[q].y = f32x2_to_bf16x2(v4[2], v4[3]) & m;
        }
        if (tid + 256 * (j0 + j) < NRUN) {
          // run v = voxels 4 v .. 4 v + 3 of its box row.  The first 64 voxels of a row are stored PERMUTED, voxel xi at slot
          // (xi % 16) * 4 + xi / 16: the A operand of lane (blk, arow) is voxel 16 arow + blk (+ tap), and in plain order
          // arow 0 / 2 and 1 / 3 met in the same banks (SQ_LDS_BANK_CONFLICT: 42 % of the launch's cycles per CU);
          // permuted, the 64 lanes of a tap read 64 consecutive slots
          const int v = tid + 256 * (j0 + j), brow = v / RUNS, run = v - brow * RUNS;
          uint2* drow = box + brow * BX;
#pragma unroll
          for (int q = 0; q < 4; ++q) drow[run < 16 ? 16 * (run & 3) + 4 * q + (run >> 2) : 64 + q] = pk[q];
        }
      }
    }
  }
  const int jc = lane & 3, blk = lane >> 2;
  float bias = 0.f, asc = 1.f, ash = 0.f;
  if (jc < a.N) {
    if (a.bias) bias = a.bias[jc];
    if (a.add) nl_coeff(a.tadd, n, a.N, jc, asc, ash);
  }
  __syncthreads();
  cs4 wb[27];
#pragma unroll
  for (int tp = 0; tp < 27; ++tp) wb[tp] = __builtin_bit_cast(cs4, wtab[tp * 4 + jc]);
  float ssum = 0.f, ssq = 0.f;
  const int arow = lane & 3;                    // A: this lane supplies row `arow` of block `blk`: voxel x = 16 arow + blk
  const int jl = min(jc, a.N - 1);
  // element offsets of this lane's four output voxels inside a row (x = ox0 + 16 r + blk), and whether they exist
  unsigned xoff_o[4], xoff_a[4];
  unsigned xok = 0u;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ox = ox0 + 16 * r + blk;
    xok |= (ox < a.out.w ? 1u : 0u) << r;
    xoff_o[r] = (unsigned)min(ox, a.out.w - 1) * (unsigned)a.out.sw;
    xoff_a[r] = (unsigned)min(ox, a.out.w - 1) * (unsigned)a.asw;
  }
#ifdef MMTTA_HEAD_LOSS_BODY
  double lacc = 0.0;                            // this lane's share of the item's entropy sum (the lanes jc == 0 add)
  // batch item n of the gradient: dense voxel rows of 4 lanes (host: loss_vec), elements 2 or 4 bytes wide
  float* const dzn = hl.dbf ? reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(hl.dz) + (long long)n * hl.dsn)
                            : hl.dz + (long long)n * hl.dsn;
#endif
  // the fused-add / accumulate operands of trip rp + 1 are requested before the MFMAs of trip rp: behind the MFMA loop
  // every trip waited a full memory latency for them (both 3 -> 3 launches of a step carry the residual add)
  float addn[2][4], oldn[2][4];
  auto fetch = [&](int rp) {
    const int r0 = rp * 8 + wave * 2;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int oz = min(oz0 + (r0 + q) / TY, a.out.d - 1), oy = min(oy0 + (r0 + q) % TY, a.out.h - 1);
#pragma unroll
      for (int r = 0; r < 4; ++r) { addn[q][r] = 0.f; oldn[q][r] = 0.f; }
      if (a.add) {
        const long long ao = (long long)n * a.asn + (long long)oz * a.asd + (long long)oy * a.ash;
#pragma unroll
        for (int r = 0; r < 4; ++r) addn[q][r] = ld1_t<GBF>(a.add, ao + xoff_a[r] + jl);
      }
      if (a.accumulate) {
        const long long oo = (long long)n * a.out.sn + (long long)oz * a.out.sd + (long long)oy * a.out.sh;
#pragma unroll
        for (int r = 0; r < 4; ++r) oldn[q][r] = ld1_t<GBF>(a.out.p, oo + xoff_o[r] + jl);
      }
    }
  };
  fetch(0);
#pragma unroll 1
  for (int rp = 0; rp < TZ * TY / 8; ++rp) {    // two rows of the tile per wave and trip (independent accumulator chains)
    const int r0 = rp * 8 + wave * 2;
    float addc[2][4], oldc[2][4];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) { addc[q][r] = addn[q][r]; oldc[q][r] = oldn[q][r]; }
    if (rp + 1 < TZ * TY / 8) fetch(rp + 1);
    cf4v acc[2];
    const uint2* ab[2][3];                        // per x tap: the lane's slot of voxel 16 arow + blk + dx in the permuted row
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int zl = (r0 + q) / TY, yl = (r0 + q) % TY;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int xi = 16 * arow + blk + dx;
        ab[q][dx] = box + (zl * BY + yl) * BX + (xi < 64 ? ((xi & 15) << 2) | (xi >> 4) : xi);
      }
      acc[q] = cf4v{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int tp = 0; tp < 27; ++tp) {
      const int toff = ((tp / 9) * BY + (tp / 3) % 3) * BX;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const uint2 av = ab[q][tp % 3][toff];
        acc[q] = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(__builtin_bit_cast(cs4, av), wb[tp], acc[q], 0, 0, 0);
      }
    }
    // ---- epilogue: register r of lane (blk, jc) = output voxel x = 16 r + blk, channel jc
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int oz = oz0 + (r0 + q) / TY, oy = oy0 + (r0 + q) % TY;
      const bool rowok = oz < a.out.d && oy < a.out.h;
      const long long orowo = (long long)n * a.out.sn + (long long)min(oz, a.out.d - 1) * a.out.sd + (long long)min(oy, a.out.h - 1) * a.out.sh;
      float* orow = a.out.p + orowo;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[q][r] + bias;
        if (a.add) v += nl_apply(addc[q][r], asc, ash, a.tadd.relu);
        if (a.accumulate) v += oldc[q][r];
#ifdef MMTTA_HEAD_LOSS_BODY
        {
          float hc, gc;
          bernoulli_entropy_terms(v, hc, gc);
          // the voxel's four lanes are a quad: its h values travel by DPP quad_perm (vector ALU, no trip through LDS)
          const int hb = __builtin_bit_cast(int, hc);
          const float h0 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, hb, 0x00, 0xf, 0xf, true));
          const float h1 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, hb, 0x55, 0xf, 0xf, true));
          const float h2 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, hb, 0xaa, 0xf, 0xf, true));
          const float h3 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, hb, 0xff, 0xf, 0xf, true));
          float h = 0.f;                         // regions 0 .. N - 1 in order, as loss_vec_kernel sums them
          h += h0;
          if (a.N > 1) h += h1;
          if (a.N > 2) h += h2;
          if (a.N > 3) h += h3;
          const float gs = jc < a.N ? gc * hl.inv_count : 0.f;      // the pad lanes of the row are stored as zeros
          const float other = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, gs), 0xb1, 0xf, 0xf, true));      // lane ^ 1
          if (rowok && ((xok >> r) & 1u)) {
            const unsigned go = (((unsigned)oz * (unsigned)a.out.h + (unsigned)oy) * (unsigned)a.out.w + (unsigned)(ox0 + 16 * r + blk)) * 4u + jc;
            if (hl.dbf) {
              if (!(jc & 1)) *reinterpret_cast<unsigned int*>(reinterpret_cast<unsigned short*>(dzn) + go) = f32x2_to_bf16x2(gs, other);
            } else {
              dzn[go] = gs;
            }
            if (jc == 0) lacc += (double)h;
          }
          continue;
        }
#endif
        if constexpr (GBF) {
          // 8-byte voxels: channel lanes pair up, the even one stores both as one dword (a 2-byte store per lane is a partial
          // dword write); channels >= N are stored as zeros (the rows own their pad)
          v = jc < a.N ? v : 0.f;
          const float other = __shfl_xor(v, 1, 64);
          if (rowok && ((xok >> r) & 1u)) {
            if (!(jc & 1))
              *reinterpret_cast<unsigned int*>(reinterpret_cast<unsigned short*>(a.out.p) + orowo + xoff_o[r] + jc) = f32x2_to_bf16x2(v, other);
            if (jc < a.N) { ssum += v; ssq += v * v; }
          }
          continue;
        }
        if (rowok && ((xok >> r) & 1u)) {
          if (jc < a.N) {
            orow[xoff_o[r] + jc] = v;
            ssum += v; ssq += v * v;
          } else if (a.out_vec4) {
            orow[xoff_o[r] + jc] = 0.f;          // the view owns its pad lanes: keep them zero
          }
        }
      }
    }
  }
#ifdef MMTTA_HEAD_LOSS_BODY
  {  // one fp64 partial per workgroup, partial[item][workgroup]: mean_finish_kernel sums the item's row
    lacc = wave_sum_d(lacc);
    if (lane == 0) {                             // (red is float storage: a double travels as its two halves)
      const unsigned long long bits = __builtin_bit_cast(unsigned long long, lacc);
      red[2 * wave] = __uint_as_float((unsigned)bits); red[2 * wave + 1] = __uint_as_float((unsigned)(bits >> 32));
    }
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
#pragma unroll
      for (int w = 0; w < 4; ++w)
        t += __builtin_bit_cast(double, (unsigned long long)__float_as_uint(red[2 * w]) | ((unsigned long long)__float_as_uint(red[2 * w + 1]) << 32));
      hl.partial[(long long)n * gridDim.x + blockIdx.x] = t;
    }
    return;                                      // no statistics rows: the head has no norm (host: stats == nullptr)
  }
#endif
  if (a.stats != nullptr) {   // lanes with the same l & 3 hold the same channel
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) { ssum += __shfl_xor(ssum, o, 64); ssq += __shfl_xor(ssq, o, 64); }
    if (lane < 4) { red[(0 * 4 + wave) * 4 + lane] = ssum; red[(1 * 4 + wave) * 4 + lane] = ssq; }
    __syncthreads();
    if (tid < a.N) {
      const float s2 = red[0 * 4 + tid] + red[1 * 4 + tid] + red[2 * 4 + tid] + red[3 * 4 + tid];
      const float q2 = red[16 + 0 * 4 + tid] + red[16 + 1 * 4 + tid] + red[16 + 2 * 4 + tid] + red[16 + 3 * 4 + tid];
      const long long rrow = (long long)n * a.blocks_per_n + blockIdx.x;
      a.stats[(rrow * 2 + 0) * a.N + tid] = s2;
      a.stats[(rrow * 2 + 1) * a.N + tid] = q2;
    }
  }
