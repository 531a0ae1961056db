// Body of upconv8_kernel and upconv8_lean_kernel (conv_direct.hip): the text is included into both; `LEAN` (a constexpr bool
// of the including kernel) switches two sites.  With LEAN = false this is upconv8_kernel as it was before the split.
// LEAN (MMTTA_OPT_THIN_LEAN bit 1; host: direct_upconv8_lean; INBF && !HAS_T only):
//   * the stage copies each loaded 16-byte item to LDS under its in-bounds mask.  Unpacking a bf16 item to eight floats and
//     rounding them back returns the stored bits (the chain applies no transform here), so the box image is the same;
//   * a tile that lies wholly inside the output skips the three bounds tests per fine voxel.
  constexpr int TZ = 4, TY = 4, TX = 8, BZ = TZ + 1, BY = TY + 1, BX = TX + 1;
  constexpr int VS = K + 8;                           // halfwords per staged voxel: 16 lanes of a ds_read_b128 -> 16 distinct slots
  constexpr int KS = K / 16, KC8 = K / 8;
  constexpr int BOXV = BZ * BY * BX;
  constexpr int NIT = (BOXV * KC8 + 255) / 256;       // 8-channel items per thread
  constexpr int SLAB_Z = 8 * 72 + 16, SLAB = 2 * SLAB_Z;   // floats of one wave's output slab (padded: conflict-free writes)
  constexpr int BOX_HW = (BOXV * VS + 7) / 8 * 8;
  extern __shared__ float lds[];
  unsigned short* lh = reinterpret_cast<unsigned short*>(lds);                 // box image, later the four output slabs
  uint4* wl = reinterpret_cast<uint4*>(lh + (BOX_HW > SLAB * 4 * 2 ? BOX_HW : SLAB * 4 * 2));   // W': 8 * KS * 64 fragments
  float* red = reinterpret_cast<float*>(wl + 8 * KS * 64);                     // 32 floats
  const int n = blockIdx.y;
  a.w = pset_packed(a.ps, a.w, n); a.bias = pset_bias(a.ps, a.bias, n);        // this batch item's parameter set
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, r = lane & 31;
  {  // W' of this batch item's set: behind the fp32 tap image [27][K][4]
    const uint4* src = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(a.w) + (size_t)27 * K * 16);
    for (int i = tid; i < 8 * KS * 64; i += 256) wl[i] = src[i];
  }
  // a thread's items i = tid + 256 j all carry the same channel octet (256 % KC8 == 0): one coefficient set per thread
  static_assert(256 % KC8 == 0, "items of a thread must share their channel octet");
  float sc[8], sh[8];
  if (HAS_T) nl_coeff_vec<8>(a.tin, n, K, (tid % KC8) * 8, sc, sh);
  const float relu_lo = act_lo(HAS_T ? a.tin.relu : MMTTA_ACT_ID);
  const float* inb = item_base<INBF>(a.in.p, n, a.in.sn);
  const unsigned isd = (unsigned)a.in.sd, ish = (unsigned)a.in.sh, isw = (unsigned)a.in.sw;
  long long tfirst, tlast;
  unit_range(tiles_per_n, xcd_contiguous_id(blockIdx.x, gridDim.x), gridDim.x, tfirst, tlast);
  // staging roles: a thread's box items are the same for every tile (decoded once); the loads of tile t + 1 are issued
  // right after tile t's image is complete and land under its MFMAs and epilogue (each tile used to start with a full
  // memory latency, two workgroups per CU to hide it)
  int pos[NIT];                                       // box voxel of item j: bz << 16 | by << 8 | bx
  const int cv = tid % KC8;
#pragma unroll
  for (int j = 0; j < NIT; ++j) {
    const int bv = min(tid + 256 * j, BOXV * KC8 - 1) / KC8;
    const int bz = bv / (BY * BX), brem = bv - bz * (BY * BX), by = brem / BX, bx = brem - by * BX;
    pos[j] = (bz << 16) | (by << 8) | bx;
  }
  Oct8<INBF> raw[NIT];
  unsigned okm = 0u;
  auto issue = [&](long long tile) {
    int t = (int)tile;
    const int txi = t % tx; t /= tx;
    const int tyi = t % ty;
    const int tzi = t / ty;
    const int gz0 = tzi * TZ, gy0 = tyi * TY, gx0 = txi * TX;
    okm = 0u;
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      const int iz = gz0 + (pos[j] >> 16), iy = gy0 + ((pos[j] >> 8) & 255), ix = gx0 + (pos[j] & 255);
      okm |= ((iz < a.in.d && iy < a.in.h && ix < a.in.w) ? 1u : 0u) << j;
      const unsigned off = (unsigned)min(iz, a.in.d - 1) * isd + (unsigned)min(iy, a.in.h - 1) * ish + (unsigned)min(ix, a.in.w - 1) * isw + cv * 8;
      raw[j] = oct8_ld<INBF>(inb, off, off + 4);
    }
  };
  if (tfirst < tlast) issue(tfirst);
  for (long long tile = tfirst; tile < tlast; ++tile) {
    int t = (int)tile;
    const int txi = t % tx; t /= tx;
    const int tyi = t % ty;
    const int tzi = t / ty;
    const int gz0 = tzi * TZ, gy0 = tyi * TY, gx0 = txi * TX;
    // ---- the halo box of this tile (requested one tile ago): transform / mask / pack
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      if constexpr (LEAN) {
        const unsigned m = ((okm >> j) & 1u) ? 0xffffffffu : 0u;
        if (tid + 256 * j < BOXV * KC8)
          *reinterpret_cast<uint4*>(lh + ((((pos[j] >> 16) * BY + ((pos[j] >> 8) & 255)) * BX + (pos[j] & 255)) * VS + cv * 8)) =
              make_uint4(raw[j].q.x & m, raw[j].q.y & m, raw[j].q.z & m, raw[j].q.w & m);
        continue;
      }
      float v[8];
      oct8_f8(raw[j], v);
      if (HAS_T) {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = act_max(fmaf(v[q], sc[q], sh[q]), relu_lo);
      }
      const unsigned m = ((okm >> j) & 1u) ? 0xffffffffu : 0u;
      uint4 pk;
      pk.x = f32x2_to_bf16x2(v[0], v[1]) & m; pk.y = f32x2_to_bf16x2(v[2], v[3]) & m;
      pk.z = f32x2_to_bf16x2(v[4], v[5]) & m; pk.w = f32x2_to_bf16x2(v[6], v[7]) & m;
      if (tid + 256 * j < BOXV * KC8)
        *reinterpret_cast<uint4*>(lh + ((((pos[j] >> 16) * BY + ((pos[j] >> 8) & 255)) * BX + (pos[j] & 255)) * VS + cv * 8)) = pk;
    }
    __syncthreads();
    if (tile + 1 < tlast) issue(tile + 1);
    // ---- 8 offsets x KS k-steps: one 32 x 32 block per wave (rows = the 4 x 8 coarse voxels of z-slice `wave`)
    ufloat16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    {
      const unsigned short* arow = lh + ((wave * BY + (r >> 3)) * BX + (r & 7)) * VS + 8 * h;
      const uint4* brow = wl + lane;
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        const unsigned short* ad = arow + ((((d >> 2) & 1) * BY + ((d >> 1) & 1)) * BX + (d & 1)) * VS;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const uint4 af = *reinterpret_cast<const uint4*>(ad + ks * 16);
          const uint4 bf = brow[(d * KS + ks) * 64];
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(ubf16x8, af), __builtin_bit_cast(ubf16x8, bf), acc, 0, 0, 0);
        }
      }
    }
    __syncthreads();                                   // the box image is dead: its space becomes the output slabs
    // ---- pixel shuffle through LDS.  Accumulator i of lane (h, r): coarse (y, x) = (i >> 2, (i & 3) + 4 h), column r =
    // (pz, py, px, co).  Slab address = pz * SLAB_Z + (2 y + py) * 72 + (2 x + px) * 4 + co: for one i the 64 lanes fall on
    // banks co + 4 px + 8 py + 16 pz + 32 h - all distinct.
    float* slab = lds + wave * SLAB;
    {
      const int pz = r >> 4, py = (r >> 3) & 1, px = (r >> 2) & 1, co = r & 3;
      float* sp = slab + pz * SLAB_Z + py * 72 + (px + 8 * h) * 4 + co;
#pragma unroll
      for (int i = 0; i < 16; ++i) sp[(i >> 2) * 144 + (i & 3) * 8] = acc[i];
    }
    __syncthreads();
    float ssum[NO], ssq[NO];
#pragma unroll
    for (int c = 0; c < NO; ++c) { ssum[c] = 0.f; ssq[c] = 0.f; }
    // (LEAN) the tile's 8 x 8 x 16 fine voxels all lie inside the output: workgroup-uniform
    const bool interior = LEAN && 2 * (gz0 + TZ) <= a.out.d && 2 * (gy0 + TY) <= a.out.h && 2 * (gx0 + TX) <= a.out.w;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int v = lane + 64 * q;                     // fine voxel of the slab: (fz, fy, fx) = (v >> 7, (v >> 4) & 7, v & 15)
      const int fz = v >> 7, fy = (v >> 4) & 7, fx = v & 15;
      const float4 o4 = *reinterpret_cast<const float4*>(slab + fz * SLAB_Z + fy * 72 + fx * 4);
      const int oz = 2 * (gz0 + wave) + fz, oy = 2 * gy0 + fy, ox = 2 * gx0 + fx;
      if ((LEAN && interior) || (oz < a.out.d && oy < a.out.h && ox < a.out.w)) {
        const float vals[4] = {o4.x, o4.y, o4.z, o4.w};
        direct_epilogue<NO>(a, n, oz, oy, ox, vals, ssum, ssq);
      }
    }
    // ---- statistics row of this tile (the following norm): lanes -> waves -> one row
    if (a.stats != nullptr) {
#pragma unroll
      for (int c = 0; c < NO; ++c) {
        const float s = wave_sum(ssum[c]), q2 = wave_sum(ssq[c]);
        if (lane == 0) { red[(0 * 4 + wave) * 4 + c] = s; red[(1 * 4 + wave) * 4 + c] = q2; }
      }
    }
    __syncthreads();                                   // slabs read, partial sums visible: the next tile may stage
    if (a.stats != nullptr && tid < NO) {
      const float s = red[0 * 4 + tid] + red[1 * 4 + tid] + red[2 * 4 + tid] + red[3 * 4 + tid];
      const float q2 = red[16 + 0 * 4 + tid] + red[16 + 1 * 4 + tid] + red[16 + 2 * 4 + tid] + red[16 + 3 * 4 + tid];
      const long long rrow = (long long)n * tiles_per_n + tile;
      a.stats[(rrow * 2 + 0) * a.N + tid] = s;
      a.stats[(rrow * 2 + 1) * a.N + tid] = q2;
    }
  }
