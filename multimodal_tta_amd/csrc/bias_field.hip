// Bias-field adaptation on gfx950: the receive-coil intensity non-uniformity of an MRI volume is a smooth multiplicative
// field per sequence, and this input map learns one per volume and modality while the network may stay frozen.
//     F_c(z, y, x) = sum_k theta_ck phi_k(z, y, x),   x'_c = (x_c - a_c) exp(F_c) + a_c
// phi_k = P_a(t_z) P_b(t_y) P_c(t_x): Legendre polynomials of the normalised voxel-centre coordinates up to total degree
// `order` <= 3, from three host-built tables; a_c the intensity the field leaves fixed (the channel's minimum, or 0).
// Two entry points, the twins of input_norm.hip's: the streaming pass that writes x' from the raw staged volume, and the
// REDUCED input gradient of the first level - dL/dx' gathered per input voxel (input_gather.h, the one copy of that gather),
// multiplied by dx'/dtheta_k and summed over the volume, K numbers per modality - with the Adam step and the clamp of theta
// in its finish.  See include/mmtta.h for the contract of the entry points.
#include "input_gather.h"

// the arithmetic of the map is specified rounding by rounding (include/mmtta.h): nothing contracts
#pragma clang fp contract(off)

namespace mmtta {

constexpr int BF_MAX_ORDER = 3;
constexpr int BF_TERMS = 20;               // coefficients of a theta / grad row, whatever the order
constexpr int BF_MAX_EXTENT = 512;         // per axis: the tables of a workgroup fit 24 KB of LDS
constexpr int BF_MAX_BLOCKS = 1024;        // workgroups per volume of the streaming pass (each stages the tables once)
constexpr int BF_FINISH_PARTS = 12;        // the finish adds the tile partials up in this many interleaved parts
// the terms (a, b, c) by (a + b + c, a, b, c) ascending: the first (order + 1)(order + 2)(order + 3) / 6 are an order's
constexpr int BF_TA[BF_TERMS] = {0, 0, 0, 1, 0, 0, 0, 1, 1, 2, 0, 0, 0, 0, 1, 1, 1, 2, 2, 3};
constexpr int BF_TB[BF_TERMS] = {0, 0, 1, 0, 0, 1, 2, 0, 1, 0, 0, 1, 2, 3, 0, 1, 2, 0, 1, 0};
constexpr int BF_TC[BF_TERMS] = {0, 1, 0, 0, 2, 1, 0, 1, 0, 0, 3, 2, 1, 0, 2, 1, 0, 1, 0, 0};
__host__ __device__ constexpr int bf_terms(int order) { return (order + 1) * (order + 2) * (order + 3) / 6; }

struct BfTables {        // T[a][i] = P_a(t_i), fp32 [4][extent] per axis
  const float* d;
  const float* h;
  const float* w;
};

// the same table as 2-bit fields of one word per axis, for a loop whose k is a run-time value
constexpr unsigned long long bf_pack(const int (&t)[BF_TERMS]) {
  unsigned long long v = 0;
  for (int k = 0; k < BF_TERMS; ++k) v |= (unsigned long long)t[k] << (2 * k);
  return v;
}
constexpr unsigned long long BF_PA = bf_pack(BF_TA), BF_PB = bf_pack(BF_TB), BF_PC = bf_pack(BF_TC);

// phi_k of a voxel from its three table values: two products, rounded in this order
__device__ __forceinline__ float bf_phi(float z, float y, float x) {
  const float zy = z * y;
  return zy * x;
}
// v[i] of a register array for a wavefront-uniform run-time i (selects: the array stays in registers)
__device__ __forceinline__ float bf_sel(const float (&v)[4], int i) { return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3])); }

// F of the four channels at one voxel: phi_k = (T_d[a][z] T_h[b][y]) T_w[c][x] rounded in that order, F = fmaf(theta_k, phi_k, F)
// from 0 in ascending k.  pz / py / px: the voxel's (P_0 .. P_3) per axis; th[k] = theta_k of the four channels.
template <int ORDER>
__device__ __forceinline__ void bf_field(const float (&pz)[4], const float (&py)[4], const float (&px)[4], const float4* th, float (&F)[4]) {
  F[0] = 0.f; F[1] = 0.f; F[2] = 0.f; F[3] = 0.f;
  static_for<0, bf_terms(ORDER)>([&](auto k_) {
    constexpr int k = decltype(k_)::value, a = BF_TA[k], b = BF_TB[k], c = BF_TC[k];
    const float phi = bf_phi(pz[a], py[b], px[c]);
    const float4 t = th[k];
    F[0] = fmaf(t.x, phi, F[0]); F[1] = fmaf(t.y, phi, F[1]); F[2] = fmaf(t.z, phi, F[2]); F[3] = fmaf(t.w, phi, F[3]);
  });
}

// theta of volume n as [k][channel] (pad lanes 0) and the anchors a_c, by the first threads of a workgroup
__device__ __forceinline__ void bf_stage_theta(const float* __restrict__ theta, const float* __restrict__ range, int n, int C, int K, int anchor,
                                               float4* ths, float* anc) {
  const int tid = threadIdx.x;
  if (tid < K * IN_ROW) {
    const int k = tid >> 2, c = tid & 3;
    reinterpret_cast<float*>(ths)[tid] = c < C ? theta[((long long)n * C + c) * BF_TERMS + k] : 0.f;
  }
  if (tid < IN_ROW) anc[tid] = (anchor == MMTTA_BIAS_ANCHOR_MIN && tid < C) ? range[((long long)n * C + tid) * 2] : 0.f;
}

// ------------------------------------------------------------------ the map
// y[n, v, c] = x' from the raw fp32 rows (in_stream_rows: one 16-byte load per voxel, 16-byte stores).  The three tables go
// to LDS once per workgroup as one float4 (P_0 .. P_3) per coordinate, theta to registers.  A channel that is not
// transformed - its K coefficients all zero, absent, a pad lane - moves its bits (fp32) or is rounded once (bf16).
template <bool BF, int ORDER>
__global__ __launch_bounds__(256) void bias_field_apply_kernel(const uint4* __restrict__ x, void* __restrict__ y, long long xsn,
                                                               long long ysn, unsigned dhw, int D, int H, int W, int C, unsigned keep,
                                                               int anchor, const float* __restrict__ theta,
                                                               const float* __restrict__ range, BfTables tb) {
  constexpr int K = bf_terms(ORDER);
  extern __shared__ float4 tab[];          // [D + H + W]
  __shared__ float4 ths[K];
  __shared__ float anc[IN_ROW];
  const int n = blockIdx.y, tid = threadIdx.x;
  for (int i = tid; i < D + H + W; i += 256) {
    const float* src = i < D ? tb.d : (i < D + H ? tb.h : tb.w);
    const int len = i < D ? D : (i < D + H ? H : W), j = i < D ? i : (i < D + H ? i - D : i - D - H);
    tab[i] = make_float4(src[j], src[len + j], src[2 * len + j], src[3 * len + j]);
  }
  bf_stage_theta(theta, range, n, C, K, anchor, ths, anc);
  __syncthreads();
  float4 th[K];
  bool on[IN_ROW] = {false, false, false, false};
#pragma unroll
  for (int k = 0; k < K; ++k) {
    th[k] = ths[k];
    on[0] = on[0] || th[k].x != 0.f; on[1] = on[1] || th[k].y != 0.f; on[2] = on[2] || th[k].z != 0.f; on[3] = on[3] || th[k].w != 0.f;
  }
  float a[IN_ROW];
#pragma unroll
  for (int c = 0; c < IN_ROW; ++c) {
    on[c] = on[c] && c < C && ((keep >> c) & 1u);
    a[c] = anc[c];
  }
  const bool any = on[0] || on[1] || on[2] || on[3];
  const unsigned hw = (unsigned)H * (unsigned)W;
  in_stream_rows<BF>(x + (long long)n * xsn, y, n, ysn, dhw, [&](const uint4& r, unsigned i, unsigned (&o)[4]) {
    o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
    if (!any) return;                      // (workgroup-uniform)
    const unsigned iz = i / hw, rem = i - iz * hw, iy = rem / (unsigned)W, ix = rem - iy * (unsigned)W;
    const float4 tz = tab[iz], ty = tab[D + iy], tx = tab[D + H + ix];
    const float pz[4] = {tz.x, tz.y, tz.z, tz.w}, py[4] = {ty.x, ty.y, ty.z, ty.w}, px[4] = {tx.x, tx.y, tx.z, tx.w};
    float F[4];
    bf_field<ORDER>(pz, py, px, th, F);
#pragma unroll
    for (int c = 0; c < IN_ROW; ++c)
      if (on[c]) {
        const float d = __uint_as_float(o[c]) - a[c];
        const float v = d * expf(F[c]);
        o[c] = __float_as_uint(v + a[c]);
      }
  });
}

// ------------------------------------------------------------------ the reduced gradient
struct BfGradArgs {
  InGather g;
  int anchor;
  const float* theta;
  const float* range;
  BfTables tb;
  double* partial;       // [N][tiles][K][4 channels]
};

// A workgroup owns a tile of IN_TZ x IN_TY x IN_TX input voxels of volume blockIdx.y and gathers dX' of its threads' 8 voxels
// each (in_gather).  Behind the finished gather: e = dX' ((x - a) exp(F)) per voxel and channel, F recomputed as the map
// computes it (bf_field's arithmetic, term by term over the 8 voxels), in place of dX'; then term by term e phi_k in fp32 into
// four fp64 sums per thread, those over the wavefront and the workgroup in a fixed order.  A thread's 8 voxels share two
// coordinates per axis: 24 table values in registers.
template <bool BF, int ORDER>
__global__ __launch_bounds__(256) void bias_field_grad_kernel(BfGradArgs ga) {
  constexpr int K = bf_terms(ORDER);
  extern __shared__ float4 in_w[];                       // [27][c0]: the branch in hand
  __shared__ float4 dys[2][IN_POS];
  __shared__ float4 ths[K];
  __shared__ float anc[IN_ROW];
  __shared__ double red[4][K * IN_ROW];
  const InGather& a = ga.g;
  const int n = blockIdx.y, tid = threadIdx.x;
  bf_stage_theta(ga.theta, ga.range, n, a.C, K, ga.anchor, ths, anc);
  const InTile t(a);
  float acc[8][4];
  in_gather<BF>(a, t, n, in_w, dys, acc);

  float pz[2][4], py[2][4], px[2][4];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    // (a coordinate past the volume reads the last one's row: its voxels contribute 0)
    const int iz = min(t.bz * IN_TZ + 2 * t.lz + p, a.D - 1), iy = min(t.by * IN_TY + 2 * t.ly + p, a.H - 1);
    const int ix = min(t.bx * IN_TX + 2 * t.lx + p, a.W - 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pz[p][j] = ga.tb.d[j * a.D + iz];
      py[p][j] = ga.tb.h[j * a.H + iy];
      px[p][j] = ga.tb.w[j * a.W + ix];
    }
  }
  // the terms one at a time (k a run-time value: what is live is bounded by one term's, not by K terms'): the phi_k of the
  // thread's 8 voxels from one selected table value per axis and coordinate
  auto phis = [&](int k, float (&phi)[8]) {
    const int ka = (int)(BF_PA >> (2 * k)) & 3, kb = (int)(BF_PB >> (2 * k)) & 3, kc = (int)(BF_PC >> (2 * k)) & 3;
    const float z[2] = {bf_sel(pz[0], ka), bf_sel(pz[1], ka)}, y[2] = {bf_sel(py[0], kb), bf_sel(py[1], kb)};
    const float x[2] = {bf_sel(px[0], kc), bf_sel(px[1], kc)};
#pragma unroll
    for (int cls = 0; cls < 8; ++cls) phi[cls] = bf_phi(z[cls >> 2], y[(cls >> 1) & 1], x[cls & 1]);
  };
  // (up to 4 terms the loop is unrolled and the selects fold away)
  auto for_terms = [&](auto&& body) {
    if constexpr (ORDER <= 1) {
      static_for<0, K>([&](auto k_) { body((int)decltype(k_)::value); });
    } else {
#pragma unroll 1
      for (int k = 0; k < K; ++k) body(k);
    }
  };
  float F[8][4];
#pragma unroll
  for (int v = 0; v < 8; ++v) { F[v][0] = 0.f; F[v][1] = 0.f; F[v][2] = 0.f; F[v][3] = 0.f; }
  for_terms([&](int k) {
    float phi[8];
    phis(k, phi);
    const float4 th = ths[k];
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      F[v][0] = fmaf(th.x, phi[v], F[v][0]); F[v][1] = fmaf(th.y, phi[v], F[v][1]);
      F[v][2] = fmaf(th.z, phi[v], F[v][2]); F[v][3] = fmaf(th.w, phi[v], F[v][3]);
    }
  });
  const uint4* xb = a.x + (long long)n * a.xsn;
  static_for<0, 8>([&](auto cls_) {
    constexpr int cls = decltype(cls_)::value;
    int iz, iy, ix;
    const bool in = in_voxel<cls>(a, t, iz, iy, ix);
    const uint4 raw = xb[in ? ((unsigned)iz * a.H + (unsigned)iy) * a.W + (unsigned)ix : 0u];
    const float xv[4] = {__uint_as_float(raw.x), __uint_as_float(raw.y), __uint_as_float(raw.z), __uint_as_float(raw.w)};
#pragma unroll
    for (int c = 0; c < IN_ROW; ++c) {
      const float d = xv[c] - anc[c];
      const float de = d * expf(F[cls][c]);
      const float e = acc[cls][c] * de;
      acc[cls][c] = in ? e : 0.f;
    }
  });
  const int lane = tid & 63, wave = tid >> 6;
  for_terms([&](int k) {
    float phi[8];
    phis(k, phi);
    double s[IN_ROW] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int v = 0; v < 8; ++v) {
#pragma unroll
      for (int c = 0; c < IN_ROW; ++c) {
        const float ep = acc[v][c] * phi[v];
        s[c] += (double)ep;
      }
    }
#pragma unroll
    for (int c = 0; c < IN_ROW; ++c) {
      s[c] = wave_sum_d(s[c]);
      if (lane == 0) red[wave][k * IN_ROW + c] = s[c];
    }
  });
  __syncthreads();
  if (tid < K * IN_ROW)
    ga.partial[((long long)n * gridDim.x + blockIdx.x) * (K * IN_ROW) + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

struct BfStep {
  double lr, bound_gain, bound_field, l2;
  float* m;
  float* v;
  int* step;
};

// One workgroup per volume: thread (part, j) adds up every BF_FINISH_PARTS-th tile's partial j, the parts are added in a fixed
// order, G[n][c][k] = dL/dtheta_ck + 2 l2 theta_ck (k >= 1: the gain is not penalised) goes to the 20-float row of `grad`
// (the terms past the order's are 0); then - with lr > 0 - in_adam's step and the clamp, theta_c0 to +- bound_gain and every
// other coefficient to +- bound_field.  An absent channel has G = 0 and keeps theta.
__global__ __launch_bounds__(BF_FINISH_PARTS* BF_TERMS* IN_ROW) void bias_field_finish_kernel(const double* __restrict__ partial, int nblocks,
                                                                                             int C, int K, unsigned keep,
                                                                                             float* __restrict__ theta,
                                                                                             float* __restrict__ grad, BfStep st) {
  constexpr int ROW = BF_TERMS * IN_ROW;
  __shared__ double part[BF_FINISH_PARTS][ROW];
  const int n = blockIdx.x, tid = threadIdx.x, j = tid % ROW, q = tid / ROW, nk = K * IN_ROW;
  double s = 0.0;
  if (j < nk) {
#pragma unroll 8          // (eight loads in flight; the additions keep their order)
    for (int i = q; i < nblocks; i += BF_FINISH_PARTS) s += partial[((long long)n * nblocks + i) * nk + j];
  }
  part[q][j] = s;
  const int t0 = st.lr > 0.0 ? st.step[n] : 0;
  __syncthreads();
  const int k = tid >> 2, c = tid & 3;
  if (tid < ROW && c < C) {
    const long long at = ((long long)n * C + c) * BF_TERMS + k;
    if (k < K) {
      const bool present = (keep >> c) & 1u;
      const float th = theta[at];
      double total = part[0][tid];
#pragma unroll
      for (int r = 1; r < BF_FINISH_PARTS; ++r) total += part[r][tid];
      if (k >= 1) total += 2.0 * st.l2 * (double)th;
      const float g = present ? (float)total : 0.f;
      grad[at] = g;
      if (st.lr > 0.0 && present) theta[at] = in_adam(th, g, t0, st.lr, k == 0 ? st.bound_gain : st.bound_field, st.m + at, st.v + at);
    } else {
      grad[at] = 0.f;
    }
  }
  if (tid == 0 && st.lr > 0.0) st.step[n] = t0 + 1;
}

// what both entry points check of the field's description; nothing touches the device
static int bf_field_check(const char* what, const mmtta_tensor* x, const float* theta, const float* range, const float* tables_d,
                          const float* tables_h, const float* tables_w, int order, int anchor) {
  MMTTA_CHECK(theta != nullptr, MMTTA_ERR_INVALID, "%s: null `theta`", what);
  MMTTA_CHECK(range != nullptr, MMTTA_ERR_INVALID, "%s: null `range`", what);
  MMTTA_CHECK(tables_d != nullptr, MMTTA_ERR_INVALID, "%s: null `tables_d`", what);
  MMTTA_CHECK(tables_h != nullptr, MMTTA_ERR_INVALID, "%s: null `tables_h`", what);
  MMTTA_CHECK(tables_w != nullptr, MMTTA_ERR_INVALID, "%s: null `tables_w`", what);
  MMTTA_CHECK(order >= 0, MMTTA_ERR_INVALID, "%s: order = %d (0 .. %d)", what, order, BF_MAX_ORDER);
  MMTTA_CHECK(order <= BF_MAX_ORDER, MMTTA_ERR_UNSUPPORTED, "%s: order = %d: the basis stops at total degree %d", what, order,
              BF_MAX_ORDER);
  MMTTA_CHECK(anchor == MMTTA_BIAS_ANCHOR_MIN || anchor == MMTTA_BIAS_ANCHOR_ZERO, MMTTA_ERR_INVALID,
              "%s: anchor = %d (MMTTA_BIAS_ANCHOR_MIN or _ZERO)", what, anchor);
  MMTTA_CHECK(x->d <= BF_MAX_EXTENT && x->h <= BF_MAX_EXTENT && x->w <= BF_MAX_EXTENT, MMTTA_ERR_UNSUPPORTED,
              "%s: extent [%d, %d, %d] of `x`: at most %d voxels per axis", what, x->d, x->h, x->w, BF_MAX_EXTENT);
  MMTTA_CHECK(((uintptr_t)theta) % 16 == 0, MMTTA_ERR_UNSUPPORTED, "%s: `theta` must be 16-byte aligned", what);
  MMTTA_CHECK(((uintptr_t)tables_d) % 4 == 0 && ((uintptr_t)tables_h) % 4 == 0 && ((uintptr_t)tables_w) % 4 == 0 &&
                  ((uintptr_t)range) % 4 == 0,
              MMTTA_ERR_UNSUPPORTED, "%s: misaligned `range` or `tables`", what);
  return MMTTA_OK;
}

// f(bf16, order) as compile-time constants, for the run-time pair
template <class F>
static void bf_dispatch(bool bf16, int order, F&& f) {
  auto with_order = [&](auto bf_) {
    switch (order) {
      case 0: f(bf_, std::integral_constant<int, 0>{}); break;
      case 1: f(bf_, std::integral_constant<int, 1>{}); break;
      case 2: f(bf_, std::integral_constant<int, 2>{}); break;
      default: f(bf_, std::integral_constant<int, 3>{}); break;
    }
  };
  if (bf16) with_order(std::integral_constant<bool, true>{});
  else with_order(std::integral_constant<bool, false>{});
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int mmtta_bias_field_apply(const mmtta_tensor* x, const mmtta_tensor* y, const float* theta, const float* range,
                                      const float* tables_d, const float* tables_h, const float* tables_w, int order, int anchor,
                                      uint32_t keep_mask, void* stream) {
  int st = in_apply_check("bias field apply", x, y);
  if (st) return st;
  st = bf_field_check("bias field apply", x, theta, range, tables_d, tables_h, tables_w, order, anchor);
  if (st) return st;
  hipStream_t s = (hipStream_t)stream;
  const unsigned dhw = (unsigned)((long long)x->d * x->h * x->w);
  long long blocks = ((long long)dhw + 255) / 256;
  if (blocks > BF_MAX_BLOCKS) blocks = BF_MAX_BLOCKS;
  const dim3 grid((unsigned)blocks, x->n);
  const size_t lds = (size_t)(x->d + x->h + x->w) * sizeof(float4);
  const BfTables tb = {tables_d, tables_h, tables_w};
  bf_dispatch(is_bf16(y), order, [&](auto bf_, auto o_) {
    hipLaunchKernelGGL((bias_field_apply_kernel<decltype(bf_)::value, decltype(o_)::value>), grid, dim3(256), lds, s, (const uint4*)x->ptr,
                       y->ptr, (long long)(x->sn / IN_ROW), (long long)y->sn, dhw, (int)x->d, (int)x->h, (int)x->w, (int)x->c, keep_mask,
                       anchor, theta, range, tb);
  });
  return launch_status("bias field apply");
}

extern "C" int64_t mmtta_bias_field_grad_partials(const mmtta_tensor* x, int order) {
  if (x == nullptr || x->n < 1 || x->d < 1 || x->h < 1 || x->w < 1) {
    set_error("bias field grad partials: null or empty tensor");
    return -1;
  }
  if (order < 0 || order > BF_MAX_ORDER) {
    set_error("bias field grad partials: order = %d (0 .. %d)", order, BF_MAX_ORDER);
    return -1;
  }
  int ty, tx;
  return in_tiles(x, ty, tx) * x->n * (bf_terms(order) * IN_ROW);
}

extern "C" int mmtta_bias_field_grad(const mmtta_tensor* x, const mmtta_input_norm_branch* branches, int n_branches, float* theta,
                                     const float* range, const float* tables_d, const float* tables_h, const float* tables_w, int order,
                                     int anchor, uint32_t keep_mask, double* partial, float* grad, float* exp_avg, float* exp_avg_sq,
                                     int32_t* step, double lr, double bound_gain, double bound_field, double l2, void* stream) {
  MMTTA_CHECK(x && x->ptr, MMTTA_ERR_INVALID, "bias field grad: null `x`");
  MMTTA_CHECK(branches != nullptr, MMTTA_ERR_INVALID, "bias field grad: null `branches`");
  MMTTA_CHECK(n_branches == 1 || n_branches == 2, MMTTA_ERR_INVALID, "bias field grad: n_branches = %d (1 or 2)", n_branches);
  MMTTA_CHECK(partial != nullptr, MMTTA_ERR_INVALID, "bias field grad: null `partial`");
  MMTTA_CHECK(grad != nullptr, MMTTA_ERR_INVALID, "bias field grad: null `grad`");
  MMTTA_CHECK(__builtin_isfinite(lr) && lr >= 0.0, MMTTA_ERR_INVALID, "bias field grad: lr must be finite and >= 0, got %g", lr);
  MMTTA_CHECK(__builtin_isfinite(l2) && l2 >= 0.0, MMTTA_ERR_INVALID, "bias field grad: l2 must be finite and >= 0, got %g", l2);
  if (lr > 0.0) {
    MMTTA_CHECK(exp_avg && exp_avg_sq && step, MMTTA_ERR_INVALID, "bias field grad: null `exp_avg`, `exp_avg_sq` or `step` with lr > 0");
    MMTTA_CHECK(__builtin_isfinite(bound_gain) && bound_gain > 0.0 && __builtin_isfinite(bound_field) && bound_field > 0.0,
                MMTTA_ERR_INVALID, "bias field grad: the bounds must be finite and > 0, got (%g, %g)", bound_gain, bound_field);
  }
  MMTTA_CHECK(is_f32(x), MMTTA_ERR_UNSUPPORTED, "bias field grad: `x` must be fp32-stored (the raw volume)");
  int st = in_rows_check("bias field grad", "x", x);
  if (st) return st;
  st = bf_field_check("bias field grad", x, theta, range, tables_d, tables_h, tables_w, order, anchor);
  if (st) return st;
  MMTTA_CHECK(((uintptr_t)grad) % 16 == 0, MMTTA_ERR_UNSUPPORTED, "bias field grad: `grad` must be 16-byte aligned");
  MMTTA_CHECK(((uintptr_t)partial) % 8 == 0, MMTTA_ERR_UNSUPPORTED, "bias field grad: `partial` must be 8-byte aligned");
  BfGradArgs a;
  long long tiles;
  st = in_gather_fill("bias field grad", x, branches, n_branches, keep_mask, a.g, tiles);
  if (st) return st;
  a.anchor = anchor; a.theta = theta; a.range = range; a.partial = partial;
  a.tb.d = tables_d; a.tb.h = tables_h; a.tb.w = tables_w;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)tiles, x->n);
  const size_t lds = (size_t)27 * a.g.c0 * sizeof(float4);
  bf_dispatch(is_bf16(branches[0].dy), order, [&](auto bf_, auto o_) {
    hipLaunchKernelGGL((bias_field_grad_kernel<decltype(bf_)::value, decltype(o_)::value>), grid, dim3(256), lds, s, a);
  });
  st = launch_status("bias field grad");
  if (st) return st;
  BfStep os;
  os.lr = lr; os.bound_gain = bound_gain; os.bound_field = bound_field; os.l2 = l2;
  os.m = exp_avg; os.v = exp_avg_sq; os.step = step;
  hipLaunchKernelGGL(bias_field_finish_kernel, dim3(x->n), dim3(BF_FINISH_PARTS * BF_TERMS * IN_ROW), 0, s, (const double*)partial, (int)tiles,
                     (int)x->c, bf_terms(order), keep_mask, theta, grad, os);
  return launch_status("bias field grad finish");
}
