// Sliding-window adaptation and inference (window_tta) on gfx950: the crop of the staged volume into its windows, the entropy
// of all windows with every voxel of the volume counted once (shared among the windows that see it), and the blend of the
// windows' logits back onto the volume.  See include/mmtta.h for the contract of the four entry points.
//
// Batch layout everywhere: [G * W_n, rd, rh, rw, C], item g * W_n + w = window w of volume g; w = (kd * ch + kh) * cw + kw over
// the per-axis start lists (W fastest), origin o_w = (start_d[kd], start_h[kh], start_w[kw]) - negative on a padded axis.  The
// weight of window w at its voxel (i, j, k) is a = (A_d[kd][i] * A_h[kh][j]) * A_w[kw][k] in fp32, in that order everywhere;
// the tables A (host-built, fp32 [count][roi] per axis, D then H then W in one buffer) carry 0 outside the volume.
#include <cstring>

#include "voxel_loss.h"

namespace mmtta {

constexpr int WIN_MAX_WINDOWS = 32;      // windows of one volume (and so of one axis)
constexpr int WIN_MAX_ROI = 512;         // roi extent per axis: a window's three table rows sit in 6 KB of LDS

struct WinGrid {
  int count[3];       // starts per axis (D, H, W)
  int roi[3];
  int extent[3];      // the volume's
  int windows;        // count[0] * count[1] * count[2]
};

// ------------------------------------------------------------------ the windows of the staged input
// y[g * W_n + w] = x[g] cropped at origin o_w; a voxel outside the volume takes `pad` in the real channels.  The pad lanes
// that y owns take +0.  Kept values keep their bits.  Fast path: a thread owns a voxel row of 4 lanes - one 16-byte (fp32:
// Q = uint4) or 8-byte (bf16: Q = uint2) load and store; `padq` is the padded row, `laneq` the mask of the real channels.
// gridDim.y = item.
__device__ __forceinline__ uint4 win_and(uint4 a, uint4 b) { return make_uint4(a.x & b.x, a.y & b.y, a.z & b.z, a.w & b.w); }
__device__ __forceinline__ uint2 win_and(uint2 a, uint2 b) { return make_uint2(a.x & b.x, a.y & b.y); }

template <class Q>
__global__ __launch_bounds__(256) void window_views_vec_kernel(const Q* __restrict__ x, Q* __restrict__ y, long long xsn,
                                                               long long ysn, const int* __restrict__ origins, WinGrid g,
                                                               Q padq, Q laneq) {
  const int item = blockIdx.y, vol = item / g.windows, win = item - vol * g.windows;
  const int oz = origins[win * 3], oy = origins[win * 3 + 1], ox = origins[win * 3 + 2];
  const Q* xb = x + (long long)vol * xsn;
  Q* yb = y + (long long)item * ysn;
  const unsigned rh = g.roi[1], rw = g.roi[2], total = (unsigned)g.roi[0] * rh * rw;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned t = i / rw, xx = i - t * rw, zz = t / rh, yy = t - zz * rh;
    const int sz = (int)zz + oz, sy = (int)yy + oy, sx = (int)xx + ox;
    const bool in = sz >= 0 && sz < g.extent[0] && sy >= 0 && sy < g.extent[1] && sx >= 0 && sx < g.extent[2];
    Q q = padq;
    if (in) q = win_and(xb[((long long)sz * g.extent[1] + sy) * g.extent[2] + sx], laneq);
    yb[i] = q;
  }
}
// Generic path: any strides, any channel count; a thread owns one lane of a voxel row of `y` (lanes = the row width where
// `y` owns its pad, else its channels).  T: the element as bits.
template <class T>
__global__ __launch_bounds__(256) void window_views_kernel(TV x, TV y, unsigned lanes, const int* __restrict__ origins, WinGrid g,
                                                           T padbits) {
  const int item = blockIdx.y, vol = item / g.windows, win = item - vol * g.windows;
  const int oz = origins[win * 3], oy = origins[win * 3 + 1], ox = origins[win * 3 + 2];
  const unsigned C = x.c, rh = g.roi[1], rw = g.roi[2];
  const unsigned total = (unsigned)g.roi[0] * rh * rw * lanes;
  const T* xb = reinterpret_cast<const T*>(x.p) + (long long)vol * x.sn;
  T* yb = reinterpret_cast<T*>(y.p) + (long long)item * y.sn;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned vox = i / lanes, c = i - vox * lanes;
    const unsigned t = vox / rw, xx = vox - t * rw, zz = t / rh, yy = t - zz * rh;
    const int sz = (int)zz + oz, sy = (int)yy + oy, sx = (int)xx + ox;
    const bool in = sz >= 0 && sz < g.extent[0] && sy >= 0 && sy < g.extent[1] && sx >= 0 && sx < g.extent[2];
    T val = (T)0;
    if (c < C) val = in ? xb[vox_addr(x, 0, sz, sy, sx) + (long long)c * x.sc] : padbits;
    yb[vox_addr(y, 0, zz, yy, xx) + (long long)c * (c < C ? y.sc : 1)] = val;
  }
}

// ------------------------------------------------------------------ the objective: a policy of the plain walk
// The weight a of the item's window rides where a second operand would: the row / at / vox accessors return it for the voxel,
// and the arithmetic is the entropy objective's own times a.  item() puts the window's three table rows into LDS once per
// workgroup.  A voxel with a == 0 (outside the volume) stores a gradient of +0 whatever its logits are.
struct WindowEntropy {
  const float* tables;      // device: A_d | A_h | A_w
  WinGrid g;
  const float *ad, *ah, *aw;      // LDS rows of this workgroup's window

  __device__ __forceinline__ void item(int n, long long) {
    __shared__ float rows[3 * WIN_MAX_ROI];
    const int win = n % g.windows;
    const int kw = win % g.count[2], t = win / g.count[2], kh = t % g.count[1], kd = t / g.count[1];
    const float* gd = tables + (long long)kd * g.roi[0];
    const float* gh = tables + (long long)g.count[0] * g.roi[0] + (long long)kh * g.roi[1];
    const float* gw = tables + (long long)g.count[0] * g.roi[0] + (long long)g.count[1] * g.roi[1] + (long long)kw * g.roi[2];
    for (int i = threadIdx.x; i < g.roi[0]; i += blockDim.x) rows[i] = gd[i];
    for (int i = threadIdx.x; i < g.roi[1]; i += blockDim.x) rows[WIN_MAX_ROI + i] = gh[i];
    for (int i = threadIdx.x; i < g.roi[2]; i += blockDim.x) rows[2 * WIN_MAX_ROI + i] = gw[i];
    __syncthreads();
    ad = rows; ah = rows + WIN_MAX_ROI; aw = rows + 2 * WIN_MAX_ROI;
  }
  __device__ __forceinline__ float weight(int z, int y, int x) const { return (ad[z] * ah[y]) * aw[x]; }
  template <class I> __device__ __forceinline__ float4 row(I v) const {
    const unsigned u = (unsigned)v, rw = g.roi[2], rh = g.roi[1];
    const unsigned t = u / rw, x = u - t * rw, z = t / rh, y = t - z * rh;
    const float a = weight(z, y, x);
    return make_float4(a, a, a, a);
  }
  __device__ __forceinline__ float at(const VoxPos& p, int) const { return weight(p.z, p.y, p.x); }
  __device__ __forceinline__ float vox(const VoxPos& p) const { return weight(p.z, p.y, p.x); }

  __device__ __forceinline__ void fast(float z, float a, float& h, float& g_) const {
    float hh, gg;
    bernoulli_entropy_terms(z, hh, gg);
    h = a > 0.f ? hh * a : 0.f;
    g_ = a > 0.f ? gg * a : 0.f;
  }
  __device__ __forceinline__ void generic(float z, float a, float& h, float& g_) const {
    const BernoulliLibm b = bernoulli_entropy_libm(z);
    h = a > 0.f ? b.h * a : 0.f;
    g_ = a > 0.f ? b.g * a : 0.f;
  }
  // The shifted form Hs = log se - sum p (z - max) (voxel_loss.h), not the entropy objective's lse - sum p z: that one carries
  // the rounding of lse times (1 + the mean logit) - 5e-6 at |z| = 10, which is 2e-5 of the largest gradient two classes can
  // have (0.224) - and the shifted form is exact to fp32 rounding at any magnitude.
  template <class F>
  __device__ __forceinline__ float categorical(const float* zp, float a, int R, F&& put) const {
    CategoricalVoxel v;
    categorical_entropy<true>(zp, R, v);
#pragma unroll
    for (int r = 0; r < LOSS_MAX_R; ++r)
      if (r < R) put(r, a > 0.f ? categorical_entropy_grad<true>(v, r) * a : 0.f);
    return a > 0.f ? v.Hs * a : 0.f;
  }
};

// loss[g] = inv_count * the block partials of the volume's W_n items, item by item in ascending order: one wave per volume,
// lane l owns blocks l, l + 64, ... of every item, then the wave shuffle.
__global__ __launch_bounds__(64) void window_finish_kernel(const double* partial, int nblocks, int windows, double inv_count,
                                                           float* loss) {
  partial += (long long)blockIdx.x * windows * nblocks;
  double s = 0.0;
  for (int w = 0; w < windows; ++w)
    for (int i = threadIdx.x; i < nblocks; i += 64) s += partial[(long long)w * nblocks + i];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) loss[blockIdx.x] = (float)(s * inv_count);
}

// ------------------------------------------------------------------ the blend: a gather
// A thread owns an output voxel (VEC: its dense row of <= 4 logits; else one (voxel, region) element, any strides).  Per
// axis it walks the start list and keeps the starts that cover its coordinate; the windows that meet at the voxel are the
// product of the three kept lists, visited in ascending window order, out = fma(a_w, z_w, out) from 0.  The start lists
// sit in LDS; the tables are read through the cache (a few KB, every workgroup reads the same).
template <bool VEC>
__global__ __launch_bounds__(256) void window_blend_kernel(TV z, TV out, const int* __restrict__ origins,
                                                           const float* __restrict__ tables, WinGrid g) {
  __shared__ int starts[3][WIN_MAX_WINDOWS];
  const int cd = g.count[0], ch = g.count[1], cw = g.count[2];
  if (threadIdx.x < WIN_MAX_WINDOWS) {
    const int k = threadIdx.x;
    if (k < cd) starts[0][k] = origins[(long long)k * ch * cw * 3];
    if (k < ch) starts[1][k] = origins[(long long)k * cw * 3 + 1];
    if (k < cw) starts[2][k] = origins[(long long)k * 3 + 2];
  }
  __syncthreads();
  const int vol = blockIdx.y;
  const float* td = tables;
  const float* th = td + (long long)cd * g.roi[0];
  const float* tw = th + (long long)ch * g.roi[1];
  const unsigned R = VEC ? 1u : (unsigned)z.c;
  const unsigned H = g.extent[1], W = g.extent[2];
  const unsigned total = (unsigned)g.extent[0] * H * W * R;
  const float* zb = z.p + (long long)vol * g.windows * z.sn;
  float* ob = out.p + (long long)vol * out.sn;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned vox = i / R, c = i - vox * R;
    const unsigned t = vox / W, px = vox - t * W, pz = t / H, py = t - pz * H;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int kd = 0; kd < cd; ++kd) {
      const int iz = (int)pz - starts[0][kd];
      if (iz < 0 || iz >= g.roi[0]) continue;
      const float wd = td[kd * g.roi[0] + iz];
      for (int kh = 0; kh < ch; ++kh) {
        const int iy = (int)py - starts[1][kh];
        if (iy < 0 || iy >= g.roi[1]) continue;
        const float wdh = wd * th[kh * g.roi[1] + iy];
        for (int kw = 0; kw < cw; ++kw) {
          const int ix = (int)px - starts[2][kw];
          if (ix < 0 || ix >= g.roi[2]) continue;
          const float a = wdh * tw[kw * g.roi[2] + ix];
          const int win = (kd * ch + kh) * cw + kw;
          const float* zp = zb + vox_addr(z, win, iz, iy, ix);
          if (VEC) {
            const float4 q = *reinterpret_cast<const float4*>(zp);
            acc.x = fmaf(a, q.x, acc.x); acc.y = fmaf(a, q.y, acc.y);
            acc.z = fmaf(a, q.z, acc.z); acc.w = fmaf(a, q.w, acc.w);
          } else {
            acc.x = fmaf(a, zp[c], acc.x);
          }
        }
      }
    }
    float* op = ob + vox_addr(out, 0, pz, py, px);
    if (VEC) {
      // the lanes past the channels held the windows' pad lanes: the output's pad takes +0
      if (z.c < 4) acc.w = 0.f;
      if (z.c < 3) acc.z = 0.f;
      if (z.c < 2) acc.y = 0.f;
      *reinterpret_cast<float4*>(op) = acc;
    } else {
      op[c] = acc.x;
    }
  }
}

// ------------------------------------------------------------------ host: the grid's checks
inline int win_grid(const char* what, const mmtta_window_grid* w, const mmtta_tensor* item, WinGrid& g) {
  MMTTA_CHECK(w != nullptr, MMTTA_ERR_INVALID, "%s: null window grid", what);
  long long windows = 1;
  for (int a = 0; a < 3; ++a) {
    g.count[a] = w->count[a];
    g.extent[a] = w->extent[a];
    MMTTA_CHECK(g.count[a] >= 1 && g.count[a] <= WIN_MAX_WINDOWS && g.extent[a] >= 1, MMTTA_ERR_INVALID,
                "%s: axis %d has %d starts over an extent of %d (1 .. %d starts, extent >= 1)", what, a, g.count[a], g.extent[a],
                WIN_MAX_WINDOWS);
    windows *= g.count[a];
  }
  g.roi[0] = item->d; g.roi[1] = item->h; g.roi[2] = item->w;
  MMTTA_CHECK(windows <= WIN_MAX_WINDOWS, MMTTA_ERR_INVALID, "%s: %lld windows per volume (1 .. %d)", what, windows, WIN_MAX_WINDOWS);
  MMTTA_CHECK(item->n >= windows && item->n % windows == 0, MMTTA_ERR_INVALID, "%s: batch %d is no multiple of the %lld windows",
              what, item->n, windows);
  MMTTA_CHECK((long long)g.extent[0] * g.extent[1] * g.extent[2] < (1ll << 29), MMTTA_ERR_UNSUPPORTED,
              "%s: a volume of 2^29 voxels or more", what);
  g.windows = (int)windows;
  return MMTTA_OK;
}

}  // namespace mmtta

using namespace mmtta;

static unsigned short win_bf16_bits(float v) {
  uint32_t u;
  std::memcpy(&u, &v, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);      // NaN stays a NaN
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);                    // round to nearest even
}

extern "C" int mmtta_window_views(const mmtta_tensor* x, const mmtta_tensor* y, const mmtta_window_grid* windows,
                                  const int32_t* origins_host, const int32_t* origins, float pad_value, void* stream) {
  MMTTA_CHECK(x && y && origins_host && origins && x->ptr && y->ptr, MMTTA_ERR_INVALID, "window views: null argument");
  WinGrid g;
  int st = win_grid("window views", windows, y, g);
  if (st) return st;
  MMTTA_CHECK(x->n >= 1 && y->n == (int64_t)x->n * g.windows && x->c == y->c && x->dtype == y->dtype, MMTTA_ERR_INVALID,
              "window views: shape mismatch");
  MMTTA_CHECK(x->d == g.extent[0] && x->h == g.extent[1] && x->w == g.extent[2], MMTTA_ERR_INVALID,
              "window views: the grid's extents are not those of `x`");
  MMTTA_CHECK(x->dtype == MMTTA_F32 || x->dtype == MMTTA_BF16, MMTTA_ERR_UNSUPPORTED, "window views: fp32 or bf16 rows");
  MMTTA_CHECK(x->c >= 1, MMTTA_ERR_INVALID, "window views: no channels");
  MMTTA_CHECK(is_cl(x) && is_cl(y), MMTTA_ERR_UNSUPPORTED, "window views: channels-last only");
  MMTTA_CHECK(!loss_overlap(x, y), MMTTA_ERR_INVALID, "window views: `y` overlaps `x`");
  MMTTA_CHECK(loss_small_item(x) && loss_small_item(y), MMTTA_ERR_UNSUPPORTED, "window views: an item of 2^31 elements or more");
  MMTTA_CHECK(y->n <= LOSS_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "window views: more than %d items in one call", LOSS_MAX_GRID_Y);
  // every window meets the volume: an origin further out than one roi would be a window of pad alone
  for (int w = 0; w < g.windows; ++w)
    for (int a = 0; a < 3; ++a) {
      const int o = origins_host[w * 3 + a];
      MMTTA_CHECK(o > -g.roi[a] && o < g.extent[a], MMTTA_ERR_INVALID, "window views: origin %d of window %d on axis %d misses the volume (extent %d, roi %d)",
                  o, w, a, g.extent[a], g.roi[a]);
    }
  hipStream_t s = (hipStream_t)stream;
  const long long nvox = (long long)g.roi[0] * g.roi[1] * g.roi[2];
  const bool owns = (y->flags & MMTTA_TENSOR_OWNS_PAD) != 0 && y->sc == 1 && y->sw >= y->c;
  const bool vec = x->c <= 4 && loss_dense4(x) && loss_dense4(y) && (owns || y->c == 4);
  if (vec) {
    long long b = (nvox + 255) / 256;
    if (b > 4096) b = 4096;
    const dim3 grid((unsigned)b, y->n);
    if (x->dtype == MMTTA_BF16) {
      const unsigned p = win_bf16_bits(pad_value);
      const unsigned lane[4] = {x->c > 0 ? 0xffffu : 0u, x->c > 1 ? 0xffffu : 0u, x->c > 2 ? 0xffffu : 0u, x->c > 3 ? 0xffffu : 0u};
      const uint2 laneq = make_uint2(lane[0] | (lane[1] << 16), lane[2] | (lane[3] << 16));
      const uint2 padq = make_uint2((p | (p << 16)) & laneq.x, (p | (p << 16)) & laneq.y);
      hipLaunchKernelGGL(window_views_vec_kernel<uint2>, grid, dim3(256), 0, s, (const uint2*)x->ptr, (uint2*)y->ptr,
                         (long long)(x->sn / 4), (long long)(y->sn / 4), (const int*)origins, g, padq, laneq);
    } else {
      uint32_t p;
      std::memcpy(&p, &pad_value, 4);
      const uint4 laneq = make_uint4(x->c > 0 ? ~0u : 0u, x->c > 1 ? ~0u : 0u, x->c > 2 ? ~0u : 0u, x->c > 3 ? ~0u : 0u);
      const uint4 padq = make_uint4(p & laneq.x, p & laneq.y, p & laneq.z, p & laneq.w);
      hipLaunchKernelGGL(window_views_vec_kernel<uint4>, grid, dim3(256), 0, s, (const uint4*)x->ptr, (uint4*)y->ptr,
                         (long long)(x->sn / 4), (long long)(y->sn / 4), (const int*)origins, g, padq, laneq);
    }
    return launch_status("window views");
  }
  const long long lanes = owns ? y->sw : y->c;
  MMTTA_CHECK(nvox * lanes < (1ll << 31), MMTTA_ERR_UNSUPPORTED, "window views: an item of 2^31 elements or more");
  long long b = (nvox * lanes + 255) / 256;
  if (b > 4096) b = 4096;
  const dim3 grid((unsigned)b, y->n);
  if (x->dtype == MMTTA_BF16) {
    hipLaunchKernelGGL(window_views_kernel<unsigned short>, grid, dim3(256), 0, s, tv(x), tv(y), (unsigned)lanes, (const int*)origins, g,
                       win_bf16_bits(pad_value));
  } else {
    uint32_t p;
    std::memcpy(&p, &pad_value, 4);
    hipLaunchKernelGGL(window_views_kernel<unsigned>, grid, dim3(256), 0, s, tv(x), tv(y), (unsigned)lanes, (const int*)origins, g, (unsigned)p);
  }
  return launch_status("window views generic");
}

extern "C" int64_t mmtta_window_partials(const mmtta_tensor* logits) {
  if (logits == nullptr || logits->n < 1 || logits->c < 1 || logits->d < 1 || logits->h < 1 || logits->w < 1) return -1;
  return (int64_t)loss_blocks(logits) * logits->n;
}

extern "C" int mmtta_window_entropy_items(const mmtta_tensor* logits, int softmax, const mmtta_window_grid* windows,
                                          const float* tables, const mmtta_tensor* dlogits, double* partial, float* loss,
                                          void* stream) {
  MMTTA_CHECK(logits && dlogits && tables && partial && loss && logits->ptr && dlogits->ptr, MMTTA_ERR_INVALID,
              "window entropy: null argument");
  WinGrid g;
  int st = win_grid("window entropy", windows, logits, g);
  if (st) return st;
  MMTTA_CHECK(same_shape(logits, dlogits), MMTTA_ERR_INVALID, "window entropy: shape mismatch");
  MMTTA_CHECK(g.roi[0] <= WIN_MAX_ROI && g.roi[1] <= WIN_MAX_ROI && g.roi[2] <= WIN_MAX_ROI, MMTTA_ERR_UNSUPPORTED,
              "window entropy: a roi extent above %d", WIN_MAX_ROI);
  MMTTA_CHECK(logits->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "window entropy: `logits` must be fp32-stored");
  MMTTA_CHECK(is_cl(logits) && is_cl(dlogits), MMTTA_ERR_UNSUPPORTED, "window entropy: channels-last only");
  MMTTA_CHECK(loss_small_item(logits) && loss_small_item(dlogits), MMTTA_ERR_UNSUPPORTED, "window entropy: an item of 2^31 elements or more");
  MMTTA_CHECK(!loss_overlap(logits, dlogits), MMTTA_ERR_INVALID, "window entropy: `dlogits` overlaps `logits`");
  MMTTA_CHECK(logits->n <= LOSS_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "window entropy: more than %d items in one call", LOSS_MAX_GRID_Y);
  const bool vec = !softmax && loss_vec(logits, dlogits);
  const LossNames nm{"window entropy", "window entropy", "window entropy"};
  st = loss_head_check(nm, logits, dlogits, softmax, vec);
  if (st) return st;
  // roi = the volume on every axis: by the grid's construction one window with a == 1 - the entropy objective itself, handed
  // to its own kernels (the tables are not read), as mmtta_memo_loss_items hands over a single view
  if (g.windows == 1 && g.extent[0] == g.roi[0] && g.extent[1] == g.roi[1] && g.extent[2] == g.roi[2])
    return mmtta_entropy_loss_items(logits, softmax, dlogits, partial, loss, stream);
  hipStream_t s = (hipStream_t)stream;
  // the launch geometry and block partials of ONE item, repeated along gridDim.y; the scale is the volume's: every voxel of
  // the unpadded volume counts once
  const int items = logits->n, blocks = loss_blocks(logits);
  const double nvol = (double)g.extent[0] * g.extent[1] * g.extent[2];
  const double cnt = softmax ? nvol : nvol * logits->c;
  const float inv = (float)(1.0 / cnt);
  WindowEntropy p;
  p.tables = tables;
  p.g = g;
  p.ad = p.ah = p.aw = nullptr;
  const dim3 grid(blocks, items);
  typedef unsigned I;
  if (softmax)
    hipLaunchKernelGGL((loss_voxel_kernel<WindowEntropy, I>), grid, dim3(256), 0, s, tv(logits), tv(dlogits), partial, inv, 1, p);
  else if (vec && is_bf16(dlogits))
    hipLaunchKernelGGL((loss_vec_kernel<WindowEntropy, I, true>), grid, dim3(256), 0, s, tv(logits), tv(dlogits), partial, inv, 1, p);
  else if (vec)
    hipLaunchKernelGGL((loss_vec_kernel<WindowEntropy, I, false>), grid, dim3(256), 0, s, tv(logits), tv(dlogits), partial, inv, 1, p);
  else
    hipLaunchKernelGGL((loss_region_kernel<WindowEntropy, I>), grid, dim3(256), 0, s, tv(logits), tv(dlogits), partial, inv, 1, p);
  st = loss_status(nm, softmax ? "categorical" : "bernoulli");
  if (st) return st;
  hipLaunchKernelGGL(window_finish_kernel, dim3(items / g.windows), dim3(64), 0, s, (const double*)partial, blocks, g.windows,
                     1.0 / cnt, loss);
  return loss_status(nm, "finish");
}

extern "C" int mmtta_window_blend(const mmtta_tensor* logits, const mmtta_tensor* out, const mmtta_window_grid* windows,
                                  const int32_t* origins, const float* tables, void* stream) {
  MMTTA_CHECK(logits && out && origins && tables && logits->ptr && out->ptr, MMTTA_ERR_INVALID, "window blend: null argument");
  WinGrid g;
  int st = win_grid("window blend", windows, logits, g);
  if (st) return st;
  MMTTA_CHECK(out->n >= 1 && logits->n == (int64_t)out->n * g.windows && logits->c == out->c, MMTTA_ERR_INVALID,
              "window blend: shape mismatch");
  MMTTA_CHECK(out->d == g.extent[0] && out->h == g.extent[1] && out->w == g.extent[2], MMTTA_ERR_INVALID,
              "window blend: the grid's extents are not those of `out`");
  MMTTA_CHECK(logits->dtype == MMTTA_F32 && out->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "window blend: fp32-stored logits only");
  MMTTA_CHECK(is_cl(logits) && is_cl(out), MMTTA_ERR_UNSUPPORTED, "window blend: channels-last only");
  MMTTA_CHECK(loss_small_item(logits) && loss_small_item(out), MMTTA_ERR_UNSUPPORTED, "window blend: an item of 2^31 elements or more");
  MMTTA_CHECK(!loss_overlap(logits, out), MMTTA_ERR_INVALID, "window blend: `out` overlaps `logits`");
  MMTTA_CHECK(out->n <= LOSS_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "window blend: more than %d volumes in one call", LOSS_MAX_GRID_Y);
  hipStream_t s = (hipStream_t)stream;
  const long long nvox = (long long)g.extent[0] * g.extent[1] * g.extent[2];
  const bool owns = (out->flags & MMTTA_TENSOR_OWNS_PAD) != 0;
  const bool vec = logits->c <= 4 && loss_dense16(logits) && loss_dense16(out) && (owns || out->c == 4);
  if (vec) {
    long long b = (nvox + 255) / 256;
    if (b > 4096) b = 4096;
    hipLaunchKernelGGL(window_blend_kernel<true>, dim3((unsigned)b, out->n), dim3(256), 0, s, tv(logits), tv(out), (const int*)origins,
                       tables, g);
    return launch_status("window blend");
  }
  MMTTA_CHECK(nvox * logits->c < (1ll << 31), MMTTA_ERR_UNSUPPORTED, "window blend: a volume of 2^31 elements or more");
  long long b = (nvox * logits->c + 255) / 256;
  if (b > 4096) b = 4096;
  hipLaunchKernelGGL(window_blend_kernel<false>, dim3((unsigned)b, out->n), dim3(256), 0, s, tv(logits), tv(out), (const int*)origins,
                     tables, g);
  return launch_status("window blend generic");
}
