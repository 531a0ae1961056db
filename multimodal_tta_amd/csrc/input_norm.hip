// Input-normaliser adaptation on gfx950 (Karani et al., MedIA 2021, "Test-time adaptable neural networks for robust medical
// image segmentation": the network stays as it is, a shallow per-volume intensity map in front of it adapts).  Per volume
// and modality theta = (s, b, g):  x' = exp(s) u + b,  u = x  or  ((x - lo) / (hi - lo))^exp(g) (hi - lo) + lo.
// Two entry points: the streaming pass that writes x' from the raw staged volume, and the REDUCED input gradient of the
// first level - dL/dx' of its one or two strided 3x3x3 convolutions, gathered per input voxel from the output gradients the
// backward has left in memory, multiplied by dx'/dtheta and summed over the volume, without dX ever reaching memory - with
// the Adam step and the clamp of theta in its finish.  See include/mmtta.h for the contract of the entry points.
#include "input_gather.h"

// x * exp(s), then + b, round on their own as torch's do; the gather spells its fused multiply-adds out (see eata.hip)
#pragma clang fp contract(off)

namespace mmtta {

constexpr int IN_SUMS = 12;                // per channel: sum dx, sum dx u, sum dx t^gamma ln t
constexpr float IN_LN2 = 0.693147180559945309f;

// what a channel's map needs, per (volume, channel): filled by the first four threads of a workgroup
struct InChan {
  float lo, w, gam, es, b;
  int on, pw;          // on: the channel is transformed at all; pw: with the power
};

__device__ __forceinline__ InChan in_channel(const float* __restrict__ theta, const float* __restrict__ range, int n, int C, int c,
                                             unsigned keep, int gamma) {
  InChan k;
  const bool live = c < C && ((keep >> c) & 1u);
  const int cc = c < C ? c : 0;            // (clamped index: the loads are unconditional, the selects follow)
  const float4 th = *reinterpret_cast<const float4*>(theta + ((long long)n * C + cc) * 4);
  const float lo = range[((long long)n * C + cc) * 2], hi = range[((long long)n * C + cc) * 2 + 1];
  k.lo = lo;
  k.w = hi - lo;
  k.on = live && !(th.x == 0.f && th.y == 0.f && th.z == 0.f);
  k.pw = k.on && gamma && th.z != 0.f && hi > lo;
  k.es = expf(th.x);
  k.b = th.y;
  k.gam = expf(th.z);
  return k;
}

// u of one value; with the power as mmtta_augment_views computes it: t in [0, 1], t = 0 gives log2 = -inf and exp2 = 0
__device__ __forceinline__ float in_power(float x, float lo, float w, float gam, float& pw, float& l2) {
  const float t = (x - lo) / w;
  l2 = __builtin_amdgcn_logf(t);
  pw = __builtin_amdgcn_exp2f(gam * l2);
  const float v = pw * w;
  return v + lo;
}

__device__ __forceinline__ float in_map(float x, const InChan& k) {
  float u = x;
  if (k.pw) {
    float pw, l2;
    u = in_power(x, k.lo, k.w, k.gam, pw, l2);
  }
  const float v = u * k.es;
  return v + k.b;
}

// ------------------------------------------------------------------ the map
// y[n, v, c] = x' from the raw fp32 rows: one 16-byte load per voxel; fp32 out one 16-byte store per voxel, bf16 out one
// 16-byte store per PAIR of voxels (the pairs start where the item's rows are 16-byte aligned: `lead` = 1 shifts them by
// one voxel, and the voxel without a partner at either end takes an 8-byte store).  A channel that is not transformed -
// theta all zero, absent, a pad lane - moves its bits (fp32) or is rounded once (bf16).
template <bool BF>
__global__ __launch_bounds__(256) void input_norm_apply_kernel(const uint4* __restrict__ x, void* __restrict__ y, long long xsn,
                                                               long long ysn, unsigned dhw, int C, unsigned keep, int gamma,
                                                               const float* __restrict__ theta, const float* __restrict__ range) {
  __shared__ InChan ch[IN_ROW];
  const int n = blockIdx.y;
  if (threadIdx.x < IN_ROW) ch[threadIdx.x] = in_channel(theta, range, n, C, threadIdx.x, keep, gamma);
  __syncthreads();
  InChan k[IN_ROW];
#pragma unroll
  for (int c = 0; c < IN_ROW; ++c) k[c] = ch[c];
  in_stream_rows<BF>(x + (long long)n * xsn, y, n, ysn, dhw, [&](const uint4& r, unsigned, unsigned (&o)[4]) {
    o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
#pragma unroll
    for (int c = 0; c < IN_ROW; ++c)
      if (k[c].on) o[c] = __float_as_uint(in_map(__uint_as_float(o[c]), k[c]));
  });
}

// ------------------------------------------------------------------ the reduced gradient
struct InGradArgs {
  InGather g;
  int gamma;
  const float* theta;
  const float* range;
  double* partial;       // [N][tiles][IN_SUMS]
};

// A workgroup owns a tile of IN_TZ x IN_TY x IN_TX input voxels of volume blockIdx.y and gathers dX' of its threads' 8 voxels
// each (in_gather: fp32 registers, a fixed order); times the three derivatives it goes into fp64 sums per thread, those over
// the wavefront and the workgroup in a fixed order, and the workgroup writes its IN_SUMS partials.
template <bool BF>
__global__ __launch_bounds__(256) void input_norm_grad_kernel(InGradArgs ga) {
  extern __shared__ float4 in_w[];                       // [27][c0]: the branch in hand
  __shared__ float4 dys[2][IN_POS];
  __shared__ InChan ch[IN_ROW];
  __shared__ double red[4][IN_SUMS];
  const InGather& a = ga.g;
  const int n = blockIdx.y, tid = threadIdx.x;
  if (tid < IN_ROW) ch[tid] = in_channel(ga.theta, ga.range, n, a.C, tid, a.keep, ga.gamma);
  const InTile t(a);
  float acc[8][4];
  in_gather<BF>(a, t, n, in_w, dys, acc);

  InChan k[IN_ROW];
#pragma unroll
  for (int c = 0; c < IN_ROW; ++c) k[c] = ch[c];
  const uint4* xb = a.x + (long long)n * a.xsn;
  double s[IN_SUMS];
#pragma unroll
  for (int j = 0; j < IN_SUMS; ++j) s[j] = 0.0;
  static_for<0, 8>([&](auto cls_) {
    constexpr int cls = decltype(cls_)::value;
    int iz, iy, ix;
    const bool in = in_voxel<cls>(a, t, iz, iy, ix);
    const uint4 raw = xb[in ? ((unsigned)iz * a.H + (unsigned)iy) * a.W + (unsigned)ix : 0u];
    const float xv[4] = {__uint_as_float(raw.x), __uint_as_float(raw.y), __uint_as_float(raw.z), __uint_as_float(raw.w)};
#pragma unroll
    for (int c = 0; c < IN_ROW; ++c) {
      const float dx = in ? acc[cls][c] : 0.f;
      float u = xv[c], q = 0.f;
      if (ga.gamma && k[c].w > 0.f) {       // (wavefront-uniform)
        float pw, l2;
        const float up = in_power(xv[c], k[c].lo, k[c].w, k[c].gam, pw, l2);
        if (k[c].pw) u = up;
        const float lt = l2 * IN_LN2;
        q = l2 > -__builtin_inff() ? pw * lt : 0.f;
      }
      const float e1 = dx * u, e2 = dx * q;
      s[c * 3] += (double)dx;
      s[c * 3 + 1] += in ? (double)e1 : 0.0;
      s[c * 3 + 2] += in ? (double)e2 : 0.0;
    }
  });
#pragma unroll
  for (int j = 0; j < IN_SUMS; ++j) s[j] = wave_sum_d(s[j]);
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < IN_SUMS; ++j) red[wave][j] = s[j];
  }
  __syncthreads();
  if (tid < IN_SUMS)
    ga.partial[((long long)n * gridDim.x + blockIdx.x) * IN_SUMS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

struct InStep {
  double lr, bound[3];
  float* m;
  float* v;
  int* step;
};

// One wavefront per volume: the workgroups' partials summed in a fixed order, G[n][c] = (dL/ds, dL/db, dL/dg, 0), then - with
// lr > 0 - torch.optim.Adam's step (default betas and eps, no decay; fp64 arithmetic on fp32 state; the call that finds
// step[n] == 0 starts from zero moments) and the clamp of theta to its box.  An absent channel has G = 0 and keeps theta.
__global__ __launch_bounds__(64) void input_norm_finish_kernel(const double* __restrict__ partial, int nblocks, int C, unsigned keep,
                                                              int gamma, float* __restrict__ theta, const float* __restrict__ range,
                                                              float* __restrict__ grad, InStep st) {
  const int n = blockIdx.x, lane = threadIdx.x;
  partial += (long long)n * nblocks * IN_SUMS;
  double s[IN_SUMS];
#pragma unroll
  for (int j = 0; j < IN_SUMS; ++j) s[j] = 0.0;
  for (int i = lane; i < nblocks; i += 64) {
#pragma unroll
    for (int j = 0; j < IN_SUMS; ++j) s[j] += partial[(long long)i * IN_SUMS + j];
  }
#pragma unroll
  for (int j = 0; j < IN_SUMS; ++j) s[j] = wave_sum_d(s[j]);
  const int t0 = st.lr > 0.0 ? st.step[n] : 0;
  if (lane < C) {
    const int c = lane;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int j = 0; j < IN_ROW; ++j)
      if (j == c) { s0 = s[j * 3]; s1 = s[j * 3 + 1]; s2 = s[j * 3 + 2]; }
    const long long row = ((long long)n * C + c) * 4;
    const float4 th = *reinterpret_cast<const float4*>(theta + row);
    const float lo = range[((long long)n * C + c) * 2], hi = range[((long long)n * C + c) * 2 + 1];
    const bool present = (keep >> c) & 1u;
    const double es = exp((double)th.x), w = (double)hi - (double)lo;
    float g[3];
    g[0] = present ? (float)(es * s1) : 0.f;
    g[1] = present ? (float)s0 : 0.f;
    g[2] = (present && gamma && hi > lo) ? (float)(es * w * exp((double)th.z) * s2) : 0.f;
    *reinterpret_cast<float4*>(grad + row) = make_float4(g[0], g[1], g[2], 0.f);
    if (st.lr > 0.0 && present) {
      float p[3] = {th.x, th.y, th.z};
      const int nk = gamma ? 3 : 2;
      for (int j = 0; j < nk; ++j) p[j] = in_adam(p[j], g[j], t0, st.lr, st.bound[j], st.m + row + j, st.v + row + j);
      *reinterpret_cast<float4*>(theta + row) = make_float4(p[0], p[1], p[2], 0.f);
    }
  }
  if (lane == 0 && st.lr > 0.0) st.step[n] = t0 + 1;
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int mmtta_input_norm_apply(const mmtta_tensor* x, const mmtta_tensor* y, const float* theta, const float* range,
                                      uint32_t keep_mask, int gamma, void* stream) {
  int st = in_apply_check("input norm apply", x, y);
  if (st) return st;
  MMTTA_CHECK(theta != nullptr, MMTTA_ERR_INVALID, "input norm apply: null `theta`");
  MMTTA_CHECK(range != nullptr, MMTTA_ERR_INVALID, "input norm apply: null `range`");
  MMTTA_CHECK(((uintptr_t)theta) % 16 == 0, MMTTA_ERR_UNSUPPORTED, "input norm apply: `theta` must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const unsigned dhw = (unsigned)((long long)x->d * x->h * x->w);
  long long blocks = ((long long)dhw + 255) / 256;
  if (blocks > IN_MAX_BLOCKS) blocks = IN_MAX_BLOCKS;
  const dim3 grid((unsigned)blocks, x->n);
  if (is_bf16(y))
    hipLaunchKernelGGL(input_norm_apply_kernel<true>, grid, dim3(256), 0, s, (const uint4*)x->ptr, y->ptr, (long long)(x->sn / IN_ROW),
                       (long long)y->sn, dhw, (int)x->c, keep_mask, gamma, theta, range);
  else
    hipLaunchKernelGGL(input_norm_apply_kernel<false>, grid, dim3(256), 0, s, (const uint4*)x->ptr, y->ptr, (long long)(x->sn / IN_ROW),
                       (long long)y->sn, dhw, (int)x->c, keep_mask, gamma, theta, range);
  return launch_status("input norm apply");
}

extern "C" int64_t mmtta_input_norm_grad_partials(const mmtta_tensor* x) {
  if (x == nullptr || x->n < 1 || x->d < 1 || x->h < 1 || x->w < 1) {
    set_error("input norm grad partials: null or empty tensor");
    return -1;
  }
  int ty, tx;
  return in_tiles(x, ty, tx) * x->n * IN_SUMS;
}

extern "C" int mmtta_input_norm_grad(const mmtta_tensor* x, const mmtta_input_norm_branch* branches, int n_branches, float* theta,
                                     const float* range, uint32_t keep_mask, int gamma, double* partial, float* grad,
                                     float* exp_avg, float* exp_avg_sq, int32_t* step, double lr, double bound_log_scale,
                                     double bound_shift, double bound_log_gamma, void* stream) {
  MMTTA_CHECK(x && x->ptr, MMTTA_ERR_INVALID, "input norm grad: null `x`");
  MMTTA_CHECK(branches != nullptr, MMTTA_ERR_INVALID, "input norm grad: null `branches`");
  MMTTA_CHECK(n_branches == 1 || n_branches == 2, MMTTA_ERR_INVALID, "input norm grad: n_branches = %d (1 or 2)", n_branches);
  MMTTA_CHECK(theta != nullptr, MMTTA_ERR_INVALID, "input norm grad: null `theta`");
  MMTTA_CHECK(range != nullptr, MMTTA_ERR_INVALID, "input norm grad: null `range`");
  MMTTA_CHECK(partial != nullptr, MMTTA_ERR_INVALID, "input norm grad: null `partial`");
  MMTTA_CHECK(grad != nullptr, MMTTA_ERR_INVALID, "input norm grad: null `grad`");
  MMTTA_CHECK(__builtin_isfinite(lr) && lr >= 0.0, MMTTA_ERR_INVALID, "input norm grad: lr must be finite and >= 0, got %g", lr);
  if (lr > 0.0) {
    MMTTA_CHECK(exp_avg && exp_avg_sq && step, MMTTA_ERR_INVALID, "input norm grad: null `exp_avg`, `exp_avg_sq` or `step` with lr > 0");
    MMTTA_CHECK(__builtin_isfinite(bound_log_scale) && bound_log_scale > 0.0 && __builtin_isfinite(bound_shift) && bound_shift > 0.0 &&
                    __builtin_isfinite(bound_log_gamma) && bound_log_gamma > 0.0,
                MMTTA_ERR_INVALID, "input norm grad: the bounds must be finite and > 0, got (%g, %g, %g)", bound_log_scale, bound_shift,
                bound_log_gamma);
  }
  MMTTA_CHECK(is_f32(x), MMTTA_ERR_UNSUPPORTED, "input norm grad: `x` must be fp32-stored (the raw volume)");
  int st = in_rows_check("input norm grad", "x", x);
  if (st) return st;
  MMTTA_CHECK(((uintptr_t)theta) % 16 == 0 && ((uintptr_t)grad) % 16 == 0, MMTTA_ERR_UNSUPPORTED,
              "input norm grad: `theta` and `grad` must be 16-byte aligned");
  MMTTA_CHECK(((uintptr_t)partial) % 8 == 0, MMTTA_ERR_UNSUPPORTED, "input norm grad: `partial` must be 8-byte aligned");
  InGradArgs a;
  long long tiles;
  st = in_gather_fill("input norm grad", x, branches, n_branches, keep_mask, a.g, tiles);
  if (st) return st;
  a.gamma = gamma ? 1 : 0;
  a.theta = theta; a.range = range; a.partial = partial;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)tiles, x->n);
  const size_t lds = (size_t)27 * a.g.c0 * sizeof(float4);
  if (is_bf16(branches[0].dy)) hipLaunchKernelGGL(input_norm_grad_kernel<true>, grid, dim3(256), lds, s, a);
  else hipLaunchKernelGGL(input_norm_grad_kernel<false>, grid, dim3(256), lds, s, a);
  st = launch_status("input norm grad");
  if (st) return st;
  InStep os;
  os.lr = lr; os.bound[0] = bound_log_scale; os.bound[1] = bound_shift; os.bound[2] = bound_log_gamma;
  os.m = exp_avg; os.v = exp_avg_sq; os.step = step;
  hipLaunchKernelGGL(input_norm_finish_kernel, dim3(x->n), dim3(64), 0, s, (const double*)partial, (int)tiles, (int)x->c, keep_mask,
                     a.gamma, theta, range, grad, os);
  return launch_status("input norm grad finish");
}
