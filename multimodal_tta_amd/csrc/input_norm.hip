// Input-normaliser adaptation on gfx950 (Karani et al., MedIA 2021, "Test-time adaptable neural networks for robust medical
// image segmentation": the network stays as it is, a shallow per-volume intensity map in front of it adapts).  Per volume
// and modality theta = (s, b, g):  x' = exp(s) u + b,  u = x  or  ((x - lo) / (hi - lo))^exp(g) (hi - lo) + lo.
// Two entry points: the streaming pass that writes x' from the raw staged volume, and the REDUCED input gradient of the
// first level - dL/dx' of its one or two strided 3x3x3 convolutions, gathered per input voxel from the output gradients the
// backward has left in memory, multiplied by dx'/dtheta and summed over the volume, without dX ever reaching memory - with
// the Adam step and the clamp of theta in its finish.  See include/mmtta.h for the contract of the entry points.
#include "common.h"

// x * exp(s), then + b, round on their own as torch's do; the gather spells its fused multiply-adds out (see eata.hip)
#pragma clang fp contract(off)

namespace mmtta {

constexpr int IN_ROW = 4;                  // channels of an input voxel row: one 16-byte (fp32) or 8-byte (bf16) access
constexpr int IN_MAX_BLOCKS = 2048;        // workgroups per volume of the streaming pass
constexpr int IN_MAX_GRID_Y = 65535;       // gridDim.y carries the volume
constexpr int IN_MAX_C0 = 64;              // output channels of the first level's convolutions
constexpr int IN_TZ = 4, IN_TY = 8, IN_TX = 64;      // input voxels of a workgroup's tile: 8 parity classes x 256 threads
constexpr int IN_PZ = IN_TZ / 2 + 1, IN_PY = IN_TY / 2 + 1, IN_PX = IN_TX / 2 + 1;      // output positions behind a tile
constexpr int IN_POS = IN_PZ * IN_PY * IN_PX;
constexpr int IN_OC = 8;                   // output channels of a staged dy chunk
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
  const uint4* xb = x + (long long)n * xsn;
  auto row = [&](const uint4& r, unsigned (&o)[4]) {
    o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
#pragma unroll
    for (int c = 0; c < IN_ROW; ++c)
      if (k[c].on) o[c] = __float_as_uint(in_map(__uint_as_float(o[c]), k[c]));
  };
  if constexpr (!BF) {
    uint4* yb = reinterpret_cast<uint4*>(y) + (long long)n * (ysn / IN_ROW);
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < dhw; i += gridDim.x * 256u) {
      unsigned o[4];
      row(xb[i], o);
      yb[i] = make_uint4(o[0], o[1], o[2], o[3]);
    }
  } else {
    char* yb = reinterpret_cast<char*>(y) + (long long)n * ysn * 2;
    const unsigned lead = (unsigned)((reinterpret_cast<uintptr_t>(yb) >> 3) & 1u);
    const unsigned pairs = (dhw + lead + 1u) / 2u;
    for (unsigned j = blockIdx.x * 256u + threadIdx.x; j < pairs; j += gridDim.x * 256u) {
      const long long v0 = 2ll * j - lead, v1 = v0 + 1;
      const bool h0 = v0 >= 0, h1 = v1 < (long long)dhw;
      unsigned o0[4] = {0u, 0u, 0u, 0u}, o1[4] = {0u, 0u, 0u, 0u};
      if (h0) row(xb[v0], o0);
      if (h1) row(xb[v1], o1);
      const uint2 a = make_uint2(f32x2_to_bf16x2(__uint_as_float(o0[0]), __uint_as_float(o0[1])),
                                 f32x2_to_bf16x2(__uint_as_float(o0[2]), __uint_as_float(o0[3])));
      const uint2 b = make_uint2(f32x2_to_bf16x2(__uint_as_float(o1[0]), __uint_as_float(o1[1])),
                                 f32x2_to_bf16x2(__uint_as_float(o1[2]), __uint_as_float(o1[3])));
      if (h0 && h1) *reinterpret_cast<uint4*>(yb + v0 * 8) = make_uint4(a.x, a.y, b.x, b.y);
      else if (h0) *reinterpret_cast<uint2*>(yb + v0 * 8) = a;
      else if (h1) *reinterpret_cast<uint2*>(yb + v1 * 8) = b;
    }
  }
}

// ------------------------------------------------------------------ the reduced gradient
struct InBranch {
  const float* dy;       // [N, Do, Ho, Wo, c0], fp32 or bf16 elements
  long long sn;          // strides in ELEMENTS (a channel slice of a wider tensor keeps the wide row stride)
  unsigned sd, sh, sw;
  const float* w;        // fp32 [c0, C, 27], set 0
  long long wset;        // elements between the sets of consecutive items (0: one set)
};
struct InGradArgs {
  const uint4* x;
  long long xsn;         // rows between items
  int C, D, H, W, Do, Ho, Wo, c0, nbr, gamma;
  unsigned keep;
  int tiles_y, tiles_x;
  InBranch br[2];
  const float* theta;
  const float* range;
  double* partial;       // [N][tiles][IN_SUMS]
};

// A workgroup owns a tile of IN_TZ x IN_TY x IN_TX input voxels of volume blockIdx.y: 8 parity classes with one voxel per
// thread each.  Stride 2, pad 1: an even coordinate i meets tap 1 at output i / 2, an odd one taps 0 and 2 at outputs
// (i + 1) / 2 and (i - 1) / 2, so the tile needs the IN_PZ x IN_PY x IN_PX output positions behind it and all threads of a
// class see the same taps.  Per branch the weights go to LDS as [tap][o][4 channels] (absent channels and pad lanes zero:
// read at wavefront-uniform addresses), and per chunk of IN_OC output channels the dy values of those positions as
// [half][position][4] fp32 (coalesced rows in, zeros outside the output; neighbouring lanes read neighbouring 16 bytes).
// dX' of the 8 voxels stays in registers (fp32, a fixed order); times the three derivatives it goes into fp64 sums per
// thread, those over the wavefront and the workgroup in a fixed order, and the workgroup writes its IN_SUMS partials.
template <bool BF>
__global__ __launch_bounds__(256) void input_norm_grad_kernel(InGradArgs a) {
  extern __shared__ float4 in_w[];                       // [27][c0]: the branch in hand
  __shared__ float4 dys[2][IN_POS];
  __shared__ InChan ch[IN_ROW];
  __shared__ double red[4][IN_SUMS];
  const int n = blockIdx.y, tid = threadIdx.x;
  const int c0 = a.c0, C = a.C;
  if (tid < IN_ROW) ch[tid] = in_channel(a.theta, a.range, n, C, tid, a.keep, a.gamma);
  const int bx = blockIdx.x % a.tiles_x, by = (blockIdx.x / a.tiles_x) % a.tiles_y, bz = blockIdx.x / (a.tiles_x * a.tiles_y);
  const int lx = tid & 31, ly = (tid >> 5) & 3, lz = tid >> 7;
  const int oz0 = bz * (IN_TZ / 2), oy0 = by * (IN_TY / 2), ox0 = bx * (IN_TX / 2);
  const int p0 = (lz * IN_PY + ly) * IN_PX + lx;
  float acc[8][4];
#pragma unroll
  for (int v = 0; v < 8; ++v) { acc[v][0] = 0.f; acc[v][1] = 0.f; acc[v][2] = 0.f; acc[v][3] = 0.f; }

  for (int r = 0; r < a.nbr; ++r) {
    const InBranch& b = a.br[r];
    const float* wsrc = b.w + (long long)n * b.wset;
    const float* db = item_base<BF>(b.dy, n, b.sn);
    __syncthreads();                                     // (the previous branch's weights are no longer read)
    for (int i = tid; i < 27 * c0; i += 256) {
      const int t = i / c0, o = i - t * c0;
      float wv[4];
#pragma unroll
      for (int c = 0; c < IN_ROW; ++c) {
        const float v = wsrc[(o * C + (c < C ? c : 0)) * 27 + t];
        wv[c] = (c < C && ((a.keep >> c) & 1u)) ? v : 0.f;
      }
      in_w[i] = make_float4(wv[0], wv[1], wv[2], wv[3]);
    }
    for (int oc = 0; oc < c0; oc += IN_OC) {
      const bool two = oc + 4 < c0;                      // (c0 is a multiple of 4: the chunk's second half may not exist)
      __syncthreads();                                   // (the previous chunk's tile is no longer read; the weights are in)
      for (int p = tid; p < IN_POS; p += 256) {
        const int qx = p % IN_PX, t = p / IN_PX, qy = t % IN_PY, qz = t / IN_PY;
        const int oz = oz0 + qz, oy = oy0 + qy, ox = ox0 + qx;
        float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0;
        if (oz < a.Do && oy < a.Ho && ox < a.Wo) {
          const unsigned off = (unsigned)oz * b.sd + (unsigned)oy * b.sh + (unsigned)ox * b.sw + (unsigned)oc;
          g0 = ld4_t<BF>(db, (long long)off);
          if (two) g1 = ld4_t<BF>(db, (long long)(off + 4u));
        }
        dys[0][p] = g0;
        dys[1][p] = g1;
      }
      __syncthreads();
      const float4* wc = in_w + oc;
      static_for<0, 8>([&](auto cls_) {
        constexpr int cls = decltype(cls_)::value, pz = cls >> 2, py = (cls >> 1) & 1, px = cls & 1;
        static_for<0, pz + 1>([&](auto jz_) {
          constexpr int jz = decltype(jz_)::value, tz = pz ? 2 * jz : 1, dz = (pz && jz == 0) ? 1 : 0;
          static_for<0, py + 1>([&](auto jy_) {
            constexpr int jy = decltype(jy_)::value, ty = py ? 2 * jy : 1, dy = (py && jy == 0) ? 1 : 0;
            static_for<0, px + 1>([&](auto jx_) {
              constexpr int jx = decltype(jx_)::value, tx = px ? 2 * jx : 1, dx = (px && jx == 0) ? 1 : 0;
              constexpr int tap = (tz * 3 + ty) * 3 + tx, dp = (dz * IN_PY + dy) * IN_PX + dx;
              const float4* wl = wc + tap * c0;
              const float4 g0 = dys[0][p0 + dp];
              const float4 w0 = wl[0], w1 = wl[1], w2 = wl[2], w3 = wl[3];
              float* q = acc[cls];
              q[0] = fmaf(g0.x, w0.x, q[0]); q[1] = fmaf(g0.x, w0.y, q[1]); q[2] = fmaf(g0.x, w0.z, q[2]); q[3] = fmaf(g0.x, w0.w, q[3]);
              q[0] = fmaf(g0.y, w1.x, q[0]); q[1] = fmaf(g0.y, w1.y, q[1]); q[2] = fmaf(g0.y, w1.z, q[2]); q[3] = fmaf(g0.y, w1.w, q[3]);
              q[0] = fmaf(g0.z, w2.x, q[0]); q[1] = fmaf(g0.z, w2.y, q[1]); q[2] = fmaf(g0.z, w2.z, q[2]); q[3] = fmaf(g0.z, w2.w, q[3]);
              q[0] = fmaf(g0.w, w3.x, q[0]); q[1] = fmaf(g0.w, w3.y, q[1]); q[2] = fmaf(g0.w, w3.z, q[2]); q[3] = fmaf(g0.w, w3.w, q[3]);
              if (two) {
                const float4 g1 = dys[1][p0 + dp];
                const float4 w4 = wl[4], w5 = wl[5], w6 = wl[6], w7 = wl[7];
                q[0] = fmaf(g1.x, w4.x, q[0]); q[1] = fmaf(g1.x, w4.y, q[1]); q[2] = fmaf(g1.x, w4.z, q[2]); q[3] = fmaf(g1.x, w4.w, q[3]);
                q[0] = fmaf(g1.y, w5.x, q[0]); q[1] = fmaf(g1.y, w5.y, q[1]); q[2] = fmaf(g1.y, w5.z, q[2]); q[3] = fmaf(g1.y, w5.w, q[3]);
                q[0] = fmaf(g1.z, w6.x, q[0]); q[1] = fmaf(g1.z, w6.y, q[1]); q[2] = fmaf(g1.z, w6.z, q[2]); q[3] = fmaf(g1.z, w6.w, q[3]);
                q[0] = fmaf(g1.w, w7.x, q[0]); q[1] = fmaf(g1.w, w7.y, q[1]); q[2] = fmaf(g1.w, w7.z, q[2]); q[3] = fmaf(g1.w, w7.w, q[3]);
              }
            });
          });
        });
      });
    }
  }

  InChan k[IN_ROW];
#pragma unroll
  for (int c = 0; c < IN_ROW; ++c) k[c] = ch[c];
  const uint4* xb = a.x + (long long)n * a.xsn;
  double s[IN_SUMS];
#pragma unroll
  for (int j = 0; j < IN_SUMS; ++j) s[j] = 0.0;
  static_for<0, 8>([&](auto cls_) {
    constexpr int cls = decltype(cls_)::value, pz = cls >> 2, py = (cls >> 1) & 1, px = cls & 1;
    const int iz = bz * IN_TZ + 2 * lz + pz, iy = by * IN_TY + 2 * ly + py, ix = bx * IN_TX + 2 * lx + px;
    const bool in = iz < a.D && iy < a.H && ix < a.W;      // (a voxel past the volume saw zeros or its neighbours' outputs: dropped)
    const uint4 raw = xb[in ? ((unsigned)iz * a.H + (unsigned)iy) * a.W + (unsigned)ix : 0u];
    const float xv[4] = {__uint_as_float(raw.x), __uint_as_float(raw.y), __uint_as_float(raw.z), __uint_as_float(raw.w)};
#pragma unroll
    for (int c = 0; c < IN_ROW; ++c) {
      const float dx = in ? acc[cls][c] : 0.f;
      float u = xv[c], q = 0.f;
      if (a.gamma && k[c].w > 0.f) {       // (wavefront-uniform)
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
    a.partial[((long long)n * gridDim.x + blockIdx.x) * IN_SUMS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
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
      const double t = (double)(t0 + 1);
      const double b1 = 0.9, b2 = 0.999, eps = 1e-8;
      const double step_size = st.lr / (1.0 - pow(b1, t)), bc2_sqrt = sqrt(1.0 - pow(b2, t));
      float p[3] = {th.x, th.y, th.z};
      const int nk = gamma ? 3 : 2;
      for (int j = 0; j < nk; ++j) {
        const double gi = (double)g[j];
        const double m0 = t0 == 0 ? 0.0 : (double)st.m[row + j], v0 = t0 == 0 ? 0.0 : (double)st.v[row + j];
        const double m1 = b1 * m0 + (1.0 - b1) * gi, v1 = b2 * v0 + (1.0 - b2) * gi * gi;
        double q = (double)p[j] - step_size * (m1 / (sqrt(v1) / bc2_sqrt + eps));
        q = fmin(fmax(q, -st.bound[j]), st.bound[j]);
        st.m[row + j] = (float)m1;
        st.v[row + j] = (float)v1;
        p[j] = (float)q;
      }
      *reinterpret_cast<float4*>(theta + row) = make_float4(p[0], p[1], p[2], 0.f);
    }
  }
  if (lane == 0 && st.lr > 0.0) st.step[n] = t0 + 1;
}

// dense channels-last voxel rows of 4 lanes (<= 4 channels), aligned to a row; every row index of an item fits 31 bits
static int in_rows_check(const char* what, const char* name, const mmtta_tensor* t) {
  MMTTA_CHECK(t->n > 0 && t->c > 0 && t->d > 0 && t->h > 0 && t->w > 0, MMTTA_ERR_INVALID, "%s: empty `%s`", what, name);
  MMTTA_CHECK(t->c <= IN_ROW, MMTTA_ERR_UNSUPPORTED, "%s: `%s` has %d channels, more than %d", what, name, t->c, IN_ROW);
  MMTTA_CHECK(t->sc == 1 && t->sw == IN_ROW && t->sh == (int64_t)t->w * IN_ROW && t->sd == (int64_t)t->h * t->sh &&
                  t->sn % IN_ROW == 0 && t->sn >= (int64_t)t->d * t->sd,
              MMTTA_ERR_UNSUPPORTED, "%s: `%s` must be dense channels-last voxel rows of 4 lanes", what, name);
  MMTTA_CHECK(((uintptr_t)t->ptr) % (t->dtype == MMTTA_BF16 ? 8 : 16) == 0, MMTTA_ERR_UNSUPPORTED, "%s: misaligned `%s`", what, name);
  MMTTA_CHECK((long long)t->d * t->h * t->w * IN_ROW < (1ll << 31), MMTTA_ERR_UNSUPPORTED, "%s: an item of 2^31 elements or more", what);
  MMTTA_CHECK(t->n <= IN_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "%s: more than %d volumes in one call", what, IN_MAX_GRID_Y);
  return MMTTA_OK;
}

static long long in_tiles(const mmtta_tensor* x, int& ty, int& tx) {
  const long long tz = (x->d + IN_TZ - 1) / IN_TZ;
  ty = (x->h + IN_TY - 1) / IN_TY;
  tx = (x->w + IN_TX - 1) / IN_TX;
  return tz * ty * tx;
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int mmtta_input_norm_apply(const mmtta_tensor* x, const mmtta_tensor* y, const float* theta, const float* range,
                                      uint32_t keep_mask, int gamma, void* stream) {
  MMTTA_CHECK(x && x->ptr, MMTTA_ERR_INVALID, "input norm apply: null `x`");
  MMTTA_CHECK(y && y->ptr, MMTTA_ERR_INVALID, "input norm apply: null `y`");
  MMTTA_CHECK(theta != nullptr, MMTTA_ERR_INVALID, "input norm apply: null `theta`");
  MMTTA_CHECK(range != nullptr, MMTTA_ERR_INVALID, "input norm apply: null `range`");
  MMTTA_CHECK(same_shape(x, y), MMTTA_ERR_INVALID, "input norm apply: shape mismatch between `x` and `y`");
  MMTTA_CHECK(x->ptr != y->ptr, MMTTA_ERR_INVALID, "input norm apply: `y` must not be `x` (the raw volume is kept)");
  MMTTA_CHECK(is_f32(x), MMTTA_ERR_UNSUPPORTED, "input norm apply: `x` must be fp32-stored (the raw volume)");
  MMTTA_CHECK(is_f32(y) || is_bf16(y), MMTTA_ERR_UNSUPPORTED, "input norm apply: `y` must be fp32 or bf16");
  int st = in_rows_check("input norm apply", "x", x);
  if (st) return st;
  st = in_rows_check("input norm apply", "y", y);
  if (st) return st;
  MMTTA_CHECK(y->c == IN_ROW || (y->flags & MMTTA_TENSOR_OWNS_PAD), MMTTA_ERR_UNSUPPORTED,
              "input norm apply: `y` must own the pad lanes of its rows");
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
  const int Do = (x->d + 1) / 2, Ho = (x->h + 1) / 2, Wo = (x->w + 1) / 2;
  for (int r = 0; r < n_branches; ++r) {
    const mmtta_input_norm_branch& b = branches[r];
    MMTTA_CHECK(b.dy && b.dy->ptr, MMTTA_ERR_INVALID, "input norm grad: null `dy` of branch %d", r);
    MMTTA_CHECK(b.weight != nullptr, MMTTA_ERR_INVALID, "input norm grad: null `weight` of branch %d", r);
    MMTTA_CHECK(b.ksize == 3 && b.stride == 2, MMTTA_ERR_UNSUPPORTED,
                "input norm grad: branch %d is a convolution k = %d, stride %d; the kernel gathers k = 3, stride 2, pad 1", r, b.ksize, b.stride);
    const mmtta_tensor* d = b.dy;
    MMTTA_CHECK(d->n == x->n && d->d == Do && d->h == Ho && d->w == Wo, MMTTA_ERR_INVALID,
                "input norm grad: shape mismatch: `dy` of branch %d is [%d, %d, %d, %d], the input's outputs are [%d, %d, %d, %d]", r,
                d->n, d->d, d->h, d->w, x->n, Do, Ho, Wo);
    MMTTA_CHECK(d->c >= 4 && d->c % 4 == 0 && d->c <= IN_MAX_C0, MMTTA_ERR_UNSUPPORTED,
                "input norm grad: branch %d has %d output channels (a multiple of 4 up to %d)", r, d->c, IN_MAX_C0);
    MMTTA_CHECK(d->c == branches[0].dy->c, MMTTA_ERR_INVALID, "input norm grad: the branches differ in output channels (%d, %d)",
                branches[0].dy->c, d->c);
    MMTTA_CHECK(is_f32(d) || is_bf16(d), MMTTA_ERR_UNSUPPORTED, "input norm grad: `dy` must be fp32 or bf16");
    MMTTA_CHECK(d->dtype == branches[0].dy->dtype, MMTTA_ERR_INVALID, "input norm grad: storage mismatch between the branches' `dy`");
    MMTTA_CHECK(d->sc == 1, MMTTA_ERR_UNSUPPORTED, "input norm grad: `dy` must be channels-last");
    MMTTA_CHECK(quad_aligned(d, quad_bytes(d)) && d->sw >= d->c && d->sh > 0 && d->sd > 0, MMTTA_ERR_UNSUPPORTED,
                "input norm grad: misaligned `dy` of branch %d", r);
    MMTTA_CHECK(item_fits_31(d, d->c), MMTTA_ERR_UNSUPPORTED, "input norm grad: an item of 2^31 elements or more");
    MMTTA_CHECK(b.set_stride >= 0, MMTTA_ERR_INVALID, "input norm grad: negative set stride of branch %d", r);
    a.br[r].dy = (const float*)d->ptr;
    a.br[r].sn = d->sn; a.br[r].sd = (unsigned)d->sd; a.br[r].sh = (unsigned)d->sh; a.br[r].sw = (unsigned)d->sw;
    a.br[r].w = b.weight; a.br[r].wset = b.set_stride;
  }
  if (n_branches == 1) a.br[1] = a.br[0];
  a.x = (const uint4*)x->ptr;
  a.xsn = x->sn / IN_ROW;
  a.C = x->c; a.D = x->d; a.H = x->h; a.W = x->w; a.Do = Do; a.Ho = Ho; a.Wo = Wo;
  a.c0 = branches[0].dy->c; a.nbr = n_branches; a.gamma = gamma ? 1 : 0; a.keep = keep_mask;
  const long long tiles = in_tiles(x, a.tiles_y, a.tiles_x);
  MMTTA_CHECK(tiles < (1ll << 31), MMTTA_ERR_UNSUPPORTED, "input norm grad: 2^31 tiles or more");
  a.theta = theta; a.range = range; a.partial = partial;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)tiles, x->n);
  const size_t lds = (size_t)27 * a.c0 * sizeof(float4);
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
