// Intensity-augmented views of the staged input (gfx950): the per-(volume, channel) range of a staged volume and the pass
// that writes the V views of every volume - each mirrored AND put through its own pointwise intensity transform (gamma,
// scale, shift, Gaussian noise; MONAI's RandAdjustContrast / RandScaleIntensity / RandShiftIntensity / RandGaussianNoise
// with fixed draws).  Both are single-pass HBM-bound streams over 4-channel voxel rows.  See include/mmtta.h for the
// contract of the entry points.
#include "common.h"

// every product and sum of this file is rounded on its own: x * a, then + b, must not contract into an fma (see the note
// in eata.hip - the __f*_rn helpers carry their own contraction setting, plain operators under this pragma do not fuse)
#pragma clang fp contract(off)

namespace mmtta {

constexpr int AUG_MAX_BLOCKS = 2048;       // block partials per volume (the entropy objective's figure)
constexpr int AUG_MAX_V = 8;
constexpr int AUG_TURN = 16;               // bit 4 of a view's code: H and W transposed before the mirrors (memo.hip's MEMO_TURN)
constexpr int AUG_MAX_GRID_Y = 65535;      // gridDim.y carries the volume
constexpr int AUG_ROW = 4;                 // channels of a voxel row: one 16-byte (fp32) or 8-byte (bf16) access

struct AugViews {
  int v;
  int axes[AUG_MAX_V];
};

// the four channel values of a voxel row and their bits (fp32: the word; bf16: the 16 bits in the low half)
template <bool BF> struct AugRow;
template <> struct AugRow<false> {
  typedef uint4 raw_t;
  static __device__ __forceinline__ void unpack(const raw_t& r, float (&f)[4], unsigned (&b)[4]) {
    b[0] = r.x; b[1] = r.y; b[2] = r.z; b[3] = r.w;
#pragma unroll
    for (int c = 0; c < 4; ++c) f[c] = __uint_as_float(b[c]);
  }
  static __device__ __forceinline__ unsigned bits(float v) { return __float_as_uint(v); }
  static __device__ __forceinline__ raw_t pack(const unsigned (&b)[4]) { return make_uint4(b[0], b[1], b[2], b[3]); }
};
template <> struct AugRow<true> {
  typedef uint2 raw_t;
  static __device__ __forceinline__ void unpack(const raw_t& r, float (&f)[4], unsigned (&b)[4]) {
    b[0] = r.x & 0xffffu; b[1] = r.x >> 16; b[2] = r.y & 0xffffu; b[3] = r.y >> 16;
#pragma unroll
    for (int c = 0; c < 4; ++c) f[c] = bf16_bits_to_f32(b[c]);
  }
  static __device__ __forceinline__ unsigned bits(float v) { return f32_to_bf16_bits(v); }      // round to nearest even, once
  static __device__ __forceinline__ raw_t pack(const unsigned (&b)[4]) { return make_uint2(b[0] | (b[1] << 16), b[2] | (b[3] << 16)); }
};

// ------------------------------------------------------------------ range
// min / max of every channel over the voxels of volume blockIdx.y: a thread owns whole voxel rows (one 16- / 8-byte load),
// the pad lanes (c >= C) never enter.  Block partials [volume][block][4][2], then one workgroup per volume: min and max are
// exact in any order, the order is fixed all the same.
template <bool BF>
__global__ __launch_bounds__(256) void intensity_range_kernel(const typename AugRow<BF>::raw_t* __restrict__ x, long long xsn,
                                                              unsigned dhw, float* __restrict__ partial) {
  __shared__ float sh[4][AUG_ROW][2];
  x += (long long)blockIdx.y * xsn;
  float lo[4], hi[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) { lo[c] = __builtin_inff(); hi[c] = -__builtin_inff(); }
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < dhw; i += gridDim.x * 256u) {
    float f[4];
    unsigned b[4];
    AugRow<BF>::unpack(x[i], f, b);
#pragma unroll
    for (int c = 0; c < 4; ++c) { lo[c] = fminf(lo[c], f[c]); hi[c] = fmaxf(hi[c], f[c]); }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo[c] = fminf(lo[c], __shfl_xor(lo[c], o, 64));
      hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o, 64));
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) { sh[wave][c][0] = lo[c]; sh[wave][c][1] = hi[c]; }
  }
  __syncthreads();
  if (threadIdx.x < AUG_ROW * 2) {
    const int c = threadIdx.x >> 1, k = threadIdx.x & 1;
    float v = sh[0][c][k];
    for (int w = 1; w < 4; ++w) v = k ? fmaxf(v, sh[w][c][k]) : fminf(v, sh[w][c][k]);
    partial[((long long)blockIdx.y * gridDim.x + blockIdx.x) * (AUG_ROW * 2) + threadIdx.x] = v;
  }
}

__global__ __launch_bounds__(64) void intensity_range_finish_kernel(const float* __restrict__ partial, int nblocks, int C,
                                                                    float* __restrict__ range) {
  partial += (long long)blockIdx.x * nblocks * (AUG_ROW * 2);      // one workgroup per volume
  float lo[4], hi[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) { lo[c] = __builtin_inff(); hi[c] = -__builtin_inff(); }
  for (int i = threadIdx.x; i < nblocks; i += 64) {
    const float4 a = *reinterpret_cast<const float4*>(partial + (long long)i * 8);
    const float4 b = *reinterpret_cast<const float4*>(partial + (long long)i * 8 + 4);
    lo[0] = fminf(lo[0], a.x); hi[0] = fmaxf(hi[0], a.y); lo[1] = fminf(lo[1], a.z); hi[1] = fmaxf(hi[1], a.w);
    lo[2] = fminf(lo[2], b.x); hi[2] = fmaxf(hi[2], b.y); lo[3] = fminf(lo[3], b.z); hi[3] = fmaxf(hi[3], b.w);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo[c] = fminf(lo[c], __shfl_xor(lo[c], o, 64));
      hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o, 64));
    }
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) {
        range[((long long)blockIdx.x * C + c) * 2] = lo[c];
        range[((long long)blockIdx.x * C + c) * 2 + 1] = hi[c];
      }
  }
}

// ------------------------------------------------------------------ views
// Philox4x32-10 (Salmon et al., SC 2011), written out as in cotta.hip: the same generator, another fourth counter word.
__device__ __forceinline__ uint4 aug_philox4x32_10(uint4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}
// Box-Muller on two words: R = sqrt(-2 ln(((wa >> 8) + 1) 2^-24)), theta = 2 pi (wb >> 8) 2^-24 -> (R cos theta, R sin theta).
// The uniforms are exact in fp32; logf / sqrtf are the library's (the hardware log2 loses R next to u = 1) and the angle
// goes in half-turns, 2 f, to sincospif, whose argument reduction is exact.
__device__ __forceinline__ void aug_normal_pair(unsigned wa, unsigned wb, float& n0, float& n1) {
  const float u = (float)((wa >> 8) + 1u) * 5.9604644775390625e-8f;
  const float f2 = (float)(wb >> 8) * 1.1920928955078125e-7f;
  const float r = sqrtf(-2.f * logf(u));
  float s, c;
  sincospif(f2, &s, &c);
  n0 = r * c;
  n1 = r * s;
}

// flags of a view: bit c = channel c is transformed, bit 4 + c = with gamma, bit 8 + c = with noise
constexpr unsigned AUG_ANY = 0xfu, AUG_GAMMA = 0xf0u, AUG_NOISE = 0xf00u;

// y[g * V + v] = view v of x[g]: a thread owns a voxel row of the volume's frame, loads it once and writes it V times at
// the mirrored coordinates (inside a row of W the order of voxels reverses, the 64 rows of a wavefront still cover one
// contiguous segment of every view).  The table rows of the volume's views, made identity for constant channels and pad
// lanes, and the ranges sit in LDS; what a view needs (nothing / arithmetic / gamma / noise) is one flag word per view, read
// through readfirstlane: every branch below is on a wavefront-uniform value and holds no global load.
// TR (a view of the call has bit 4: H and W transposed before the mirrors, H == W): frame voxel (z, y, x) goes to
// (fd(z), fh(x), fw(y)) of such a view - stores W rows apart, uncoalesced, once per volume.  The noise counter stays the
// voxel's index in the volume's own frame: a transposed view draws the field a mirror view would at the same frame voxel.
template <bool BF, bool TR>
__global__ __launch_bounds__(256) void augment_views_kernel(const typename AugRow<BF>::raw_t* __restrict__ x,
                                                            typename AugRow<BF>::raw_t* __restrict__ y, long long xsn,
                                                            long long ysn, int C, unsigned D, unsigned H, unsigned W, AugViews mv,
                                                            const float* __restrict__ table, const float* __restrict__ range,
                                                            const int* __restrict__ ordinals, unsigned k0, unsigned k1) {
  typedef typename AugRow<BF>::raw_t raw_t;
  __shared__ float tab[AUG_MAX_V][AUG_ROW][4];      // g, a, b, sigma
  __shared__ float rng[AUG_ROW][2];                 // lo, hi - lo
  __shared__ unsigned flags[AUG_MAX_V];
  const int V = mv.v, g = blockIdx.y;
  if (threadIdx.x < AUG_MAX_V * AUG_ROW) {
    const int v = threadIdx.x >> 2, c = threadIdx.x & 3;
    const bool live = v < V && c < C;
    // (clamped indices: the loads are unconditional, the selects follow)
    const long long row = ((long long)g * V + (live ? v : 0)) * C + (live ? c : 0);
    const float4 p = *reinterpret_cast<const float4*>(table + row * 4);
    const float lo = range[((long long)g * C + (live ? c : 0)) * 2], hi = range[((long long)g * C + (live ? c : 0)) * 2 + 1];
    const bool on = live && v > 0 && hi > lo && !(p.x == 1.f && p.y == 1.f && p.z == 0.f && p.w == 0.f);
    tab[v][c][0] = on ? p.x : 1.f; tab[v][c][1] = on ? p.y : 1.f; tab[v][c][2] = on ? p.z : 0.f; tab[v][c][3] = on ? p.w : 0.f;
    if (v == 0) { rng[c][0] = lo; rng[c][1] = hi - lo; }
  }
  __syncthreads();
  if (threadIdx.x < AUG_MAX_V) {
    unsigned f = 0;
#pragma unroll
    for (int c = 0; c < AUG_ROW; ++c) {
      const float pg = tab[threadIdx.x][c][0], pa = tab[threadIdx.x][c][1], pb = tab[threadIdx.x][c][2], ps = tab[threadIdx.x][c][3];
      if (!(pg == 1.f && pa == 1.f && pb == 0.f && ps == 0.f)) f |= 1u << c;
      if (pg != 1.f) f |= 16u << c;
      if (ps > 0.f) f |= 256u << c;
    }
    flags[threadIdx.x] = f;
  }
  __syncthreads();
  const unsigned ord = (unsigned)ordinals[g];
  const unsigned dhw = D * H * W;
  const raw_t* xb = x + (long long)g * xsn;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < dhw; i += gridDim.x * 256u) {
    const unsigned t = i / W, px = i - t * W, pz = t / H, py = t - pz * H;
    const raw_t raw = xb[i];
    float f[4];
    unsigned b[4];
    AugRow<BF>::unpack(raw, f, b);
    for (int v = 0; v < V; ++v) {
      const int m = mv.axes[v];
      const unsigned qx = (TR && (m & AUG_TURN)) ? py : px, qy = (TR && (m & AUG_TURN)) ? px : py;
      const unsigned xx = (m & 1) ? W - 1 - qx : qx, yy = (m & 2) ? H - 1 - qy : qy, zz = (m & 4) ? D - 1 - pz : pz;
      raw_t* yb = y + ((long long)g * V + v) * ysn;
      const unsigned o = (zz * H + yy) * W + xx;
      const unsigned fl = __builtin_amdgcn_readfirstlane(flags[v]);
      if ((fl & AUG_ANY) == 0u) {
        yb[o] = raw;          // an identity view moves the row's bits
        continue;
      }
      float nz[4] = {0.f, 0.f, 0.f, 0.f};
      if (fl & AUG_NOISE) {
        const uint4 w4 = aug_philox4x32_10(make_uint4(i, (unsigned)v, ord, 1u), k0, k1);      // (quad 0 << 8) | v
        aug_normal_pair(w4.x, w4.y, nz[0], nz[1]);
        if (C > 2) aug_normal_pair(w4.z, w4.w, nz[2], nz[3]);
      }
      unsigned ob[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        ob[c] = b[c];
        if (fl & (1u << c)) {
          float val = f[c];
          if (fl & (16u << c)) {
            // ((x - lo) / (hi - lo))^g (hi - lo) + lo; t in [0, 1]: t = 0 gives log2 = -inf and exp2 = 0
            const float lo = rng[c][0], w = rng[c][1];
            const float tt = (val - lo) / w;
            const float pw = __builtin_amdgcn_exp2f(tab[v][c][0] * __builtin_amdgcn_logf(tt));
            val = pw * w;
            val = val + lo;
          }
          val = val * tab[v][c][1];
          val = val + tab[v][c][2];
          if (fl & (256u << c)) {
            const float sn = tab[v][c][3] * nz[c];
            val = val + sn;
          }
          ob[c] = AugRow<BF>::bits(val);
        }
      }
      yb[o] = AugRow<BF>::pack(ob);
    }
  }
}

static int aug_blocks(const mmtta_tensor* x) {
  const long long total = (long long)x->d * x->h * x->w;
  long long b = (total + 255) / 256;
  if (b < 1) b = 1;
  if (b > AUG_MAX_BLOCKS) b = AUG_MAX_BLOCKS;
  return (int)b;
}

// dense channels-last 4-channel voxel rows, aligned to a row; every voxel index of an item fits 31 bits
static int aug_layout_check(const char* what, const mmtta_tensor* t) {
  MMTTA_CHECK(t->dtype == MMTTA_F32 || t->dtype == MMTTA_BF16, MMTTA_ERR_UNSUPPORTED, "%s: fp32 or bf16 rows", what);
  MMTTA_CHECK(t->n > 0 && t->c > 0 && t->d > 0 && t->h > 0 && t->w > 0, MMTTA_ERR_INVALID, "%s: empty tensor", what);
  MMTTA_CHECK(t->c <= AUG_ROW && t->sc == 1 && t->sw == AUG_ROW && t->sh == (int64_t)t->w * AUG_ROW &&
                  t->sd == (int64_t)t->h * t->sh && t->sn % AUG_ROW == 0 && t->sn >= (int64_t)t->d * t->sd,
              MMTTA_ERR_UNSUPPORTED, "%s: dense channels-last voxel rows of 4 channels (<= 4 channels)", what);
  const uintptr_t row = t->dtype == MMTTA_BF16 ? 8 : 16;
  MMTTA_CHECK(((uintptr_t)t->ptr) % row == 0, MMTTA_ERR_UNSUPPORTED, "%s: misaligned tensor", what);
  MMTTA_CHECK((long long)t->d * t->h * t->w * AUG_ROW < (1ll << 31), MMTTA_ERR_UNSUPPORTED, "%s: an item of 2^31 elements or more", what);
  return MMTTA_OK;
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int64_t mmtta_intensity_range_partials(const mmtta_tensor* x) {
  if (x == nullptr || x->n < 1 || x->d < 1 || x->h < 1 || x->w < 1) {
    set_error("intensity range partials: null or empty tensor");
    return -1;
  }
  return (int64_t)aug_blocks(x) * x->n * (AUG_ROW * 2);
}

extern "C" int mmtta_intensity_range(const mmtta_tensor* x, float* partial, float* range, void* stream) {
  MMTTA_CHECK(x && partial && range && x->ptr, MMTTA_ERR_INVALID, "intensity range: null argument");
  int st = aug_layout_check("intensity range", x);
  if (st) return st;
  MMTTA_CHECK(x->n <= AUG_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "intensity range: more than %d volumes in one call", AUG_MAX_GRID_Y);
  MMTTA_CHECK(((uintptr_t)partial) % 16 == 0, MMTTA_ERR_UNSUPPORTED, "intensity range: `partial` must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int blocks = aug_blocks(x);
  const unsigned dhw = (unsigned)((long long)x->d * x->h * x->w);
  const dim3 grid(blocks, x->n);
  if (is_bf16(x))
    hipLaunchKernelGGL(intensity_range_kernel<true>, grid, dim3(256), 0, s, (const uint2*)x->ptr, (long long)(x->sn / AUG_ROW), dhw, partial);
  else
    hipLaunchKernelGGL(intensity_range_kernel<false>, grid, dim3(256), 0, s, (const uint4*)x->ptr, (long long)(x->sn / AUG_ROW), dhw, partial);
  st = launch_status("intensity range");
  if (st) return st;
  hipLaunchKernelGGL(intensity_range_finish_kernel, dim3(x->n), dim3(64), 0, s, (const float*)partial, blocks, (int)x->c, range);
  return launch_status("intensity range finish");
}

extern "C" int mmtta_augment_views(const mmtta_tensor* x, const mmtta_tensor* y, int views, const int32_t* view_axes,
                                   const float* table_host, const float* table, const float* range, uint64_t seed,
                                   const int32_t* ordinals, void* stream) {
  MMTTA_CHECK(x && y && x->ptr && y->ptr && table_host && table && range && ordinals, MMTTA_ERR_INVALID, "augment views: null argument");
  MMTTA_CHECK(views == 1 || views == 2 || views == 4 || views == 8, MMTTA_ERR_INVALID, "augment views: views = %d (1, 2, 4 or 8)", views);
  MMTTA_CHECK(view_axes != nullptr, MMTTA_ERR_INVALID, "augment views: null argument (view_axes)");
  MMTTA_CHECK(view_axes[0] == 0, MMTTA_ERR_INVALID, "augment views: view_axes[0] = %d, view 0 is the unmirrored volume", view_axes[0]);
  AugViews mv;
  mv.v = views;
  for (int v = 0; v < AUG_MAX_V; ++v) {
    mv.axes[v] = v < views ? view_axes[v] : 0;
    MMTTA_CHECK((mv.axes[v] & ~(7 | AUG_TURN)) == 0, MMTTA_ERR_INVALID,
                "augment views: view_axes[%d] = %d (bit 0 = W, 1 = H, 2 = D mirrored, bit 4 = H and W transposed first)", v, mv.axes[v]);
  }
  bool turned = false;
  for (int v = 0; v < views; ++v)
    if (mv.axes[v] & AUG_TURN) {
      turned = true;
      MMTTA_CHECK(y->h == y->w, MMTTA_ERR_INVALID,
                  "augment views: view_axes[%d] = %d transposes H and W, which needs h == w: h = %d, w = %d", v, mv.axes[v], y->h, y->w);
    }
  MMTTA_CHECK(y->n >= views && y->n % views == 0, MMTTA_ERR_INVALID, "augment views: batch %d is no multiple of views %d", y->n, views);
  MMTTA_CHECK(y->n == x->n * views && x->c == y->c && x->d == y->d && x->h == y->h && x->w == y->w && x->dtype == y->dtype,
              MMTTA_ERR_INVALID, "augment views: shape mismatch");
  int st = aug_layout_check("augment views", x);
  if (st) return st;
  st = aug_layout_check("augment views", y);
  if (st) return st;
  MMTTA_CHECK(y->c == AUG_ROW || (y->flags & MMTTA_TENSOR_OWNS_PAD), MMTTA_ERR_UNSUPPORTED, "augment views: `y` must own the pad lanes of its rows");
  MMTTA_CHECK(x->n <= AUG_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "augment views: more than %d volumes in one call", AUG_MAX_GRID_Y);
  MMTTA_CHECK(((uintptr_t)table) % 16 == 0, MMTTA_ERR_UNSUPPORTED, "augment views: `table` must be 16-byte aligned");
  for (int g = 0; g < x->n; ++g)
    for (int c = 0; c < x->c; ++c) {
      const float* p = table_host + (((long long)g * views) * x->c + c) * 4;
      MMTTA_CHECK(p[0] == 1.f && p[1] == 1.f && p[2] == 0.f && p[3] == 0.f, MMTTA_ERR_INVALID,
                  "augment views: view 0 of volume %d, channel %d has the row (%g, %g, %g, %g): view 0 is the volume itself, "
                  "(1, 1, 0, 0)", g, c, (double)p[0], (double)p[1], (double)p[2], (double)p[3]);
    }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(aug_blocks(x), x->n);
  const unsigned k0 = (unsigned)(seed & 0xffffffffu), k1 = (unsigned)(seed >> 32);
  const long long xsn = x->sn / AUG_ROW, ysn = y->sn / AUG_ROW;
#define AUG_VIEWS(BF, TR, RAW)                                                                                                  \
  hipLaunchKernelGGL((augment_views_kernel<BF, TR>), grid, dim3(256), 0, s, (const RAW*)x->ptr, (RAW*)y->ptr, xsn, ysn, (int)x->c, \
                     (unsigned)x->d, (unsigned)x->h, (unsigned)x->w, mv, table, range, (const int*)ordinals, k0, k1)
  if (!turned) {
    if (is_bf16(x)) AUG_VIEWS(true, false, uint2);
    else AUG_VIEWS(false, false, uint4);
  } else {
    if (is_bf16(x)) AUG_VIEWS(true, true, uint2);
    else AUG_VIEWS(false, true, uint4);
  }
#undef AUG_VIEWS
  return launch_status("augment views");
}
