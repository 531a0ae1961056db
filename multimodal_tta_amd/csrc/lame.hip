// LAME (Boudiaf et al., CVPR 2022, "Parameter-free Online Test-time Adaptation") on gfx950: Laplacian-regularised voxel
// posteriors as a 3-D stencil over the logits.  The weights are left alone; T synchronous iterations
//   l_i <- l0_i + weight * sum_j w_ij y(l_j),   y = tanh(l / 2) (sigmoid head) or softmax(l) (softmax head),
// over the 6 / 18 / 26 spatial neighbours j of voxel i, w_ij = exp(-|x_i - x_j|^2 / (2 sigma^2)) / n on the staged input.
// One launch per iteration, ping-pong between `work` and `out`.  See include/mmtta.h for the contract.
#include "common.h"

namespace mmtta {

constexpr int LAME_MAX_R = 16;            // regions / input channels of the generic path
constexpr int LAME_MAX_GRID_Y = 65535;    // gridDim.y carries the item
// The tile of the fast path: 4 x 8 x 32 output voxels per 256-thread workgroup (a thread owns one (y, x) column of 4), staged
// with a one-voxel halo as 6 x 10 x 34 rows of 16 bytes: 32,640 B of y and as many of x - two workgroups of the affinity
// form per CU (one stages while the other computes), four of the sigma = 0 form.  32 voxels along W make every staging
// and store access of a wave a run of 16-byte rows; a lane group of ds_read_b128 reads 16 consecutive rows (no conflicts).
constexpr int LAME_TD = 4, LAME_TH = 8, LAME_TW = 32;
constexpr int LAME_HD = LAME_TD + 2, LAME_HH = LAME_TH + 2, LAME_HW = LAME_TW + 2;
constexpr int LAME_HALO = LAME_HD * LAME_HH * LAME_HW;
constexpr float LAME_LOG2E = 1.4426950408889634f;

// tanh(l / 2) = sign(l) (1 - e) / (1 + e), e = exp(-|l|): no cancellation but the harmless one at l -> 0
__device__ __forceinline__ float lame_tanh_half(float l) {
  const float e = __builtin_amdgcn_exp2f(-fabsf(l) * LAME_LOG2E);
  return copysignf((1.f - e) / (1.f + e), l);
}

// y of one voxel row of <= 4 regions (lanes >= R come out 0, whatever the pad holds)
template <bool SOFTMAX>
__device__ __forceinline__ float4 lame_y4(float4 l, int R) {
  if (!SOFTMAX)
    return make_float4(lame_tanh_half(l.x), R > 1 ? lame_tanh_half(l.y) : 0.f, R > 2 ? lame_tanh_half(l.z) : 0.f,
                       R > 3 ? lame_tanh_half(l.w) : 0.f);
  float m = l.x;
  if (R > 1) m = fmaxf(m, l.y);
  if (R > 2) m = fmaxf(m, l.z);
  if (R > 3) m = fmaxf(m, l.w);
  const float ex = __builtin_amdgcn_exp2f((l.x - m) * LAME_LOG2E);
  const float ey = R > 1 ? __builtin_amdgcn_exp2f((l.y - m) * LAME_LOG2E) : 0.f;
  const float ez = R > 2 ? __builtin_amdgcn_exp2f((l.z - m) * LAME_LOG2E) : 0.f;
  const float ew = R > 3 ? __builtin_amdgcn_exp2f((l.w - m) * LAME_LOG2E) : 0.f;
  const float s = (ex + ey) + (ez + ew);
  return make_float4(ex / s, ey / s, ez / s, ew / s);
}

// hard prediction changed?  sigmoid head: per region 1[l >= 0]; softmax head: the FIRST arg max of the voxel
template <bool SOFTMAX>
__device__ __forceinline__ int lame_flips(const float* a, const float* b, int R) {
  if (!SOFTMAX) {
    int c = 0;
#pragma unroll
    for (int r = 0; r < LAME_MAX_R; ++r)
      if (r < R) c += ((a[r] >= 0.f) != (b[r] >= 0.f)) ? 1 : 0;
    return c;
  }
  int ia = 0, ib = 0;
  float ma = a[0], mb = b[0];
#pragma unroll
  for (int r = 1; r < LAME_MAX_R; ++r)
    if (r < R) {
      if (a[r] > ma) { ma = a[r]; ia = r; }
      if (b[r] > mb) { mb = b[r]; ib = r; }
    }
  return ia != ib ? 1 : 0;
}

// integer block sum + ONE atomic per workgroup: integer addition commutes, so the count is the same in every run
__device__ __forceinline__ void lame_add_flipped(int cnt, long long* flipped, int* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = sh[0] + sh[1] + sh[2] + sh[3];
    if (total > 0) atomicAdd(reinterpret_cast<unsigned long long*>(flipped) + blockIdx.y, (unsigned long long)total);
  }
}

struct LameArgs {
  const float* l0;       // the model's logits: never written
  const float* cur;      // l(t)
  float* dst;            // l(t+1)
  const float* x;        // staged input (fp32 or bf16 elements), null when sigma == 0
  long long l0sn, csn, dsn, xsn;    // item strides in elements
  int D, H, W, R;
  unsigned mask;         // present channels, already cut to the C channels of x
  int maxl1;             // |d|_1 <= 1 / 2 / 3 for connectivity 6 / 18 / 26
  float scale, negk;     // weight / n;  -log2(e) / (2 sigma^2)
  int full_rows;         // dst rows are stored as one 16-byte access (R == 4 or the view owns its pad: pad lanes get 0)
  int tiles_x, tiles_y;
  long long* flipped;    // the last launch only
};

// ------------------------------------------------------------------ tiled fast path: R <= 4, C <= 4, 16-byte logit rows
template <bool AFF, bool SOFTMAX, bool XBF>
__global__ __launch_bounds__(256) void lame_tiled_kernel(LameArgs a) {
  __shared__ float4 ys[LAME_HALO];
  __shared__ float4 xs[AFF ? LAME_HALO : 1];
  __shared__ int shc[4];
  const int D = a.D, H = a.H, W = a.W, R = a.R;
  unsigned t = blockIdx.x;
  const int bx = (int)(t % (unsigned)a.tiles_x);
  t /= (unsigned)a.tiles_x;
  const int by = (int)(t % (unsigned)a.tiles_y), bz = (int)(t / (unsigned)a.tiles_y);
  const int x0 = bx * LAME_TW, y0 = by * LAME_TH, z0 = bz * LAME_TD;
  const float* cur = a.cur + (long long)blockIdx.y * a.csn;
  const float* l0 = a.l0 + (long long)blockIdx.y * a.l0sn;
  float* dst = a.dst + (long long)blockIdx.y * a.dsn;
  const float* xb = AFF ? item_base<XBF>(a.x, blockIdx.y, a.xsn) : nullptr;

  // stage y(l(t)) and x with the halo; a voxel outside the volume is y = 0 (it adds nothing whatever its weight), x = 0
  for (int h = threadIdx.x; h < LAME_HALO; h += 256) {
    const int hx = h % LAME_HW, hr = h / LAME_HW;
    const int hy = hr % LAME_HH, hz = hr / LAME_HH;
    const int gx = x0 - 1 + hx, gy = y0 - 1 + hy, gz = z0 - 1 + hz;
    float4 y = make_float4(0.f, 0.f, 0.f, 0.f), xv = y;
    if ((unsigned)gx < (unsigned)W && (unsigned)gy < (unsigned)H && (unsigned)gz < (unsigned)D) {
      const unsigned v = ((unsigned)gz * H + gy) * W + gx;      // * 4 < 2^31: checked on the host
      y = lame_y4<SOFTMAX>(*reinterpret_cast<const float4*>(cur + v * 4u), R);
      if (AFF) {
        const float4 q = ld4_t<XBF>(xb, v * 4u);
        xv = make_float4((a.mask & 1u) ? q.x : 0.f, (a.mask & 2u) ? q.y : 0.f, (a.mask & 4u) ? q.z : 0.f,
                         (a.mask & 8u) ? q.w : 0.f);      // absent channels and pad lanes: no difference
      }
    }
    ys[h] = y;
    if (AFF) xs[h] = xv;
  }
  __syncthreads();

  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int gx = x0 + tx, gy = y0 + ty;
  int cnt = 0;
  if (gx < W && gy < H) {
    for (int tz = 0; tz < LAME_TD; ++tz) {
      const int gz = z0 + tz;
      if (gz >= D) break;
      const int c = ((tz + 1) * LAME_HH + ty + 1) * LAME_HW + tx + 1;
      float4 xi = make_float4(0.f, 0.f, 0.f, 0.f);
      if (AFF) xi = xs[c];
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const int l1 = (dz != 0) + (dy != 0) + (dx != 0);
            if (l1 == 0 || l1 > a.maxl1) continue;      // (wave-uniform)
            const int j = c + (dz * LAME_HH + dy) * LAME_HW + dx;
            const float4 yj = ys[j];
            float w = 1.f;
            if (AFF) {
              const float4 xj = xs[j];
              const float ex = xi.x - xj.x, ey = xi.y - xj.y, ez = xi.z - xj.z, ew = xi.w - xj.w;
              const float d2 = fmaf(ew, ew, fmaf(ez, ez, fmaf(ey, ey, ex * ex)));
              w = __builtin_amdgcn_exp2f(d2 * a.negk);
            }
            acc.x = fmaf(w, yj.x, acc.x);
            acc.y = fmaf(w, yj.y, acc.y);
            acc.z = fmaf(w, yj.z, acc.z);
            acc.w = fmaf(w, yj.w, acc.w);
          }
      const unsigned v = ((unsigned)gz * H + gy) * W + gx;
      const float4 b = *reinterpret_cast<const float4*>(l0 + v * 4u);
      const float o[4] = {fmaf(a.scale, acc.x, b.x), fmaf(a.scale, acc.y, b.y), fmaf(a.scale, acc.z, b.z),
                          fmaf(a.scale, acc.w, b.w)};
      if (a.full_rows) {
        *reinterpret_cast<float4*>(dst + v * 4u) = make_float4(o[0], R > 1 ? o[1] : 0.f, R > 2 ? o[2] : 0.f, R > 3 ? o[3] : 0.f);
      } else {
        dst[v * 4u] = o[0];
        if (R > 1) dst[v * 4u + 1] = o[1];
        if (R > 2) dst[v * 4u + 2] = o[2];
      }
      if (a.flipped != nullptr) {
        const float bb[4] = {b.x, b.y, b.z, b.w};
        if (!SOFTMAX) {
          for (int r = 0; r < 4; ++r)
            if (r < R) cnt += ((o[r] >= 0.f) != (bb[r] >= 0.f)) ? 1 : 0;
        } else {
          int ia = 0, ib = 0;
          float ma = o[0], mb = bb[0];
#pragma unroll
          for (int r = 1; r < 4; ++r)
            if (r < R) {
              if (o[r] > ma) { ma = o[r]; ia = r; }
              if (bb[r] > mb) { mb = bb[r]; ib = r; }
            }
          cnt += ia != ib ? 1 : 0;
        }
      }
    }
  }
  if (a.flipped != nullptr) lame_add_flipped(cnt, a.flipped, shc);
}

// ------------------------------------------------------------------ generic path: R <= 16, C <= 16, any channels-last rows
// One thread per voxel; the neighbours' y is recomputed from l(t) in global memory (the rows come from L2).
__global__ __launch_bounds__(256) void lame_generic_kernel(TV l0, TV cur, TV dst, TV x, int aff, int softmax, unsigned mask,
                                                           int maxl1, float scale, float negk, long long* flipped) {
  __shared__ int shc[4];
  const int D = l0.d, H = l0.h, W = l0.w, R = l0.c, C = aff ? x.c : 0;
  const unsigned total = (unsigned)D * H * W;      // < 2^31: checked on the host
  const unsigned v = blockIdx.x * 256u + threadIdx.x;
  const float* l0p = l0.p + (long long)blockIdx.y * l0.sn;
  const float* curp = cur.p + (long long)blockIdx.y * cur.sn;
  float* dstp = dst.p + (long long)blockIdx.y * dst.sn;
  const long long xitem = aff ? (long long)blockIdx.y * x.sn : 0;
  int cnt = 0;
  if (v < total) {
    const int gx = (int)(v % (unsigned)W), rr = (int)(v / (unsigned)W);
    const int gy = rr % H, gz = rr / H;
    float xi[LAME_MAX_R], acc[LAME_MAX_R];
#pragma unroll
    for (int c = 0; c < LAME_MAX_R; ++c) {
      acc[c] = 0.f;
      xi[c] = 0.f;
      if (c < C && ((mask >> c) & 1u)) xi[c] = ld1_any(x.p, xitem + gz * x.sd + gy * x.sh + gx * x.sw + c, x.bf);
    }
    for (int o = 0; o < 27; ++o) {
      const int dz = o / 9 - 1, dy = (o / 3) % 3 - 1, dx = o % 3 - 1;
      const int l1 = (dz != 0) + (dy != 0) + (dx != 0);
      if (l1 == 0 || l1 > maxl1) continue;
      const int nz = gz + dz, ny = gy + dy, nx = gx + dx;
      if ((unsigned)nz >= (unsigned)D || (unsigned)ny >= (unsigned)H || (unsigned)nx >= (unsigned)W) continue;
      float w = 1.f;
      if (aff) {
        const long long xo = xitem + nz * x.sd + ny * x.sh + nx * x.sw;
        float d2 = 0.f;
#pragma unroll
        for (int c = 0; c < LAME_MAX_R; ++c)
          if (c < C && ((mask >> c) & 1u)) {
            const float e = xi[c] - ld1_any(x.p, xo + c, x.bf);
            d2 = fmaf(e, e, d2);
          }
        w = __builtin_amdgcn_exp2f(d2 * negk);
      }
      const float* lp = curp + nz * cur.sd + ny * cur.sh + nx * cur.sw;
      float l[LAME_MAX_R];
      float m = -INFINITY;
#pragma unroll
      for (int r = 0; r < LAME_MAX_R; ++r)
        if (r < R) {
          l[r] = lp[r];
          m = fmaxf(m, l[r]);
        }
      if (softmax) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < LAME_MAX_R; ++r)
          if (r < R) {
            l[r] = __builtin_amdgcn_exp2f((l[r] - m) * LAME_LOG2E);
            s += l[r];
          }
        const float ws = w / s;
#pragma unroll
        for (int r = 0; r < LAME_MAX_R; ++r)
          if (r < R) acc[r] = fmaf(ws, l[r], acc[r]);
      } else {
#pragma unroll
        for (int r = 0; r < LAME_MAX_R; ++r)
          if (r < R) acc[r] = fmaf(w, lame_tanh_half(l[r]), acc[r]);
      }
    }
    const float* bp = l0p + gz * l0.sd + gy * l0.sh + gx * l0.sw;
    float* op = dstp + gz * dst.sd + gy * dst.sh + gx * dst.sw;
    float b[LAME_MAX_R], out[LAME_MAX_R];
#pragma unroll
    for (int r = 0; r < LAME_MAX_R; ++r) {
      b[r] = out[r] = 0.f;
      if (r < R) {
        b[r] = bp[r];
        out[r] = fmaf(scale, acc[r], b[r]);
        op[r] = out[r];      // pad lanes are left as they are
      }
    }
    if (flipped != nullptr) cnt = softmax ? lame_flips<true>(out, b, R) : lame_flips<false>(out, b, R);
  }
  if (flipped != nullptr) lame_add_flipped(cnt, flipped, shc);
}

// 16-byte voxel rows with nothing between them: what the tiled kernel addresses with one 32-bit voxel index
static bool lame_dense4(const mmtta_tensor* t, int esz) {
  return t->sc == 1 && t->sw == 4 && t->sh == (int64_t)t->w * 4 && t->sd == (int64_t)t->h * t->sh && t->sn % 4 == 0 &&
         ((uintptr_t)t->ptr) % (4 * esz) == 0;
}

static bool lame_overlap(const mmtta_tensor* a, const mmtta_tensor* b) {
  auto span = [](const mmtta_tensor* t, uintptr_t& lo, uintptr_t& hi) {
    const long long esz = t->dtype == MMTTA_BF16 ? 2 : 4;
    const long long last = (long long)(t->n - 1) * t->sn + (long long)(t->d - 1) * t->sd + (long long)(t->h - 1) * t->sh +
                           (long long)(t->w - 1) * t->sw + t->c;
    lo = (uintptr_t)t->ptr;
    hi = lo + (uintptr_t)(last * esz);
  };
  uintptr_t alo, ahi, blo, bhi;
  span(a, alo, ahi);
  span(b, blo, bhi);
  return !(ahi <= blo || bhi <= alo);
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int mmtta_lame_refine(const mmtta_tensor* logits0, const mmtta_tensor* x, uint32_t channel_mask, int softmax,
                                 int connectivity, float weight, float sigma, int iterations, const mmtta_tensor* work,
                                 const mmtta_tensor* out, int64_t* flipped, void* stream) {
  MMTTA_CHECK(logits0 && logits0->ptr, MMTTA_ERR_INVALID, "lame refine: null `logits0`");
  MMTTA_CHECK(work && work->ptr, MMTTA_ERR_INVALID, "lame refine: null `work`");
  MMTTA_CHECK(out && out->ptr, MMTTA_ERR_INVALID, "lame refine: null `out`");
  MMTTA_CHECK(flipped != nullptr, MMTTA_ERR_INVALID, "lame refine: null `flipped`");
  MMTTA_CHECK(connectivity == 6 || connectivity == 18 || connectivity == 26, MMTTA_ERR_INVALID,
              "lame refine: connectivity must be 6, 18 or 26, got %d", connectivity);
  MMTTA_CHECK(iterations >= 1 && iterations <= 64, MMTTA_ERR_INVALID, "lame refine: iterations must be 1 .. 64, got %d",
              iterations);
  MMTTA_CHECK(__builtin_isfinite(weight) && weight > 0.f && weight <= 16.f, MMTTA_ERR_INVALID,
              "lame refine: weight must be finite and in (0, 16], got %g", (double)weight);
  MMTTA_CHECK(__builtin_isfinite(sigma) && sigma >= 0.f, MMTTA_ERR_INVALID,
              "lame refine: sigma must be finite and >= 0, got %g", (double)sigma);
  const bool aff = sigma > 0.f;
  MMTTA_CHECK(!aff || (x && x->ptr), MMTTA_ERR_INVALID, "lame refine: null `x` with sigma > 0");
  MMTTA_CHECK(logits0->n >= 1 && logits0->c >= 1 && logits0->d >= 1 && logits0->h >= 1 && logits0->w >= 1, MMTTA_ERR_INVALID,
              "lame refine: empty `logits0`");
  MMTTA_CHECK(same_shape(logits0, work) && same_shape(logits0, out), MMTTA_ERR_INVALID,
              "lame refine: shape mismatch between `logits0`, `work` and `out`");
  MMTTA_CHECK(logits0->sw == work->sw && logits0->sw == out->sw, MMTTA_ERR_INVALID,
              "lame refine: row width mismatch between `logits0`, `work` and `out`");
  MMTTA_CHECK(!aff || (x->n == logits0->n && x->d == logits0->d && x->h == logits0->h && x->w == logits0->w && x->c >= 1),
              MMTTA_ERR_INVALID, "lame refine: shape mismatch between `x` and `logits0`");
  MMTTA_CHECK(logits0->c <= LAME_MAX_R, MMTTA_ERR_UNSUPPORTED, "lame refine: more than %d regions", LAME_MAX_R);
  MMTTA_CHECK(!aff || x->c <= LAME_MAX_R, MMTTA_ERR_UNSUPPORTED, "lame refine: more than %d input channels", LAME_MAX_R);
  const uint32_t mask = aff ? (channel_mask & ((1u << x->c) - 1u)) : 0u;
  MMTTA_CHECK(!aff || mask != 0u, MMTTA_ERR_INVALID,
              "lame refine: channel_mask 0x%x names none of the %d channels of `x` (sigma > 0)", channel_mask, aff ? x->c : 0);
  MMTTA_CHECK(is_f32(logits0) && is_f32(work) && is_f32(out), MMTTA_ERR_UNSUPPORTED,
              "lame refine: `logits0`, `work` and `out` must be fp32-stored");
  MMTTA_CHECK(!aff || x->dtype == MMTTA_F32 || x->dtype == MMTTA_BF16, MMTTA_ERR_UNSUPPORTED, "lame refine: `x` must be fp32 or bf16");
  auto cl = [](const mmtta_tensor* t) { return t->sc == 1 && t->sw >= t->c && t->sh >= 0 && t->sd >= 0 && t->sn >= 0; };
  MMTTA_CHECK(cl(logits0) && cl(work) && cl(out) && (!aff || cl(x)), MMTTA_ERR_UNSUPPORTED, "lame refine: channels-last only");
  MMTTA_CHECK(!lame_overlap(logits0, work) && !lame_overlap(logits0, out) && !lame_overlap(work, out), MMTTA_ERR_INVALID,
              "lame refine: `logits0`, `work` and `out` must be three distinct buffers (aliased)");
  MMTTA_CHECK(!aff || (!lame_overlap(x, work) && !lame_overlap(x, out)), MMTTA_ERR_INVALID,
              "lame refine: `x` is aliased by `work` or `out`");
  // the kernels index the voxels and the elements of one item with 32-bit arithmetic
  auto small = [](const mmtta_tensor* t) {
    const long long ld = t->sw > 4 ? t->sw : 4;
    return (long long)t->d * t->h * t->w * ld < (1ll << 31) && item_fits_31(t, ld);
  };
  MMTTA_CHECK(small(logits0) && small(work) && small(out) && (!aff || small(x)), MMTTA_ERR_UNSUPPORTED,
              "lame refine: an item of 2^31 elements or more");
  MMTTA_CHECK(logits0->n <= LAME_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "lame refine: more than %d items in one call", LAME_MAX_GRID_Y);

  hipStream_t s = (hipStream_t)stream;
  const int items = logits0->n, R = logits0->c;
  const int maxl1 = connectivity == 6 ? 1 : (connectivity == 18 ? 2 : 3);
  const float scale = (float)((double)weight / (double)connectivity);
  const float negk = aff ? (float)(-1.4426950408889634 / (2.0 * (double)sigma * (double)sigma)) : 0.f;
  const bool tiled = g_lame_tiled != 0 && R <= 4 && lame_dense4(logits0, 4) && lame_dense4(work, 4) && lame_dense4(out, 4) &&
                     (!aff || (x->c <= 4 && lame_dense4(x, x->dtype == MMTTA_BF16 ? 2 : 4)));
  if (hipMemsetAsync(flipped, 0, sizeof(int64_t) * (size_t)items, s) != hipSuccess) return launch_status("lame refine clear");
  for (int t = 1; t <= iterations; ++t) {
    // the result of iteration T lands in `out`: iteration t writes `out` when T - t is even, `work` otherwise
    const mmtta_tensor* dst = (iterations - t) % 2 == 0 ? out : work;
    const mmtta_tensor* src = t == 1 ? logits0 : (dst == out ? work : out);
    long long* fl = t == iterations ? (long long*)flipped : nullptr;
    if (tiled) {
      LameArgs a;
      a.l0 = (const float*)logits0->ptr; a.cur = (const float*)src->ptr; a.dst = (float*)dst->ptr;
      a.x = aff ? (const float*)x->ptr : nullptr;
      a.l0sn = logits0->sn; a.csn = src->sn; a.dsn = dst->sn; a.xsn = aff ? x->sn : 0;
      a.D = logits0->d; a.H = logits0->h; a.W = logits0->w; a.R = R;
      a.mask = mask; a.maxl1 = maxl1; a.scale = scale; a.negk = negk;
      a.full_rows = (R == 4 || (dst->flags & MMTTA_TENSOR_OWNS_PAD)) ? 1 : 0;
      a.tiles_x = (a.W + LAME_TW - 1) / LAME_TW; a.tiles_y = (a.H + LAME_TH - 1) / LAME_TH;
      a.flipped = fl;
      const long long tiles = (long long)a.tiles_x * a.tiles_y * ((a.D + LAME_TD - 1) / LAME_TD);      // < 2^31 / 4
      const dim3 launch((unsigned)tiles, items);
      const bool xbf = aff && x->dtype == MMTTA_BF16;
#define LAME_TILED(AFF, SM, XBF) hipLaunchKernelGGL((lame_tiled_kernel<AFF, SM, XBF>), launch, dim3(256), 0, s, a)
      if (!aff) { if (softmax) LAME_TILED(false, true, false); else LAME_TILED(false, false, false); }
      else if (xbf) { if (softmax) LAME_TILED(true, true, true); else LAME_TILED(true, false, true); }
      else { if (softmax) LAME_TILED(true, true, false); else LAME_TILED(true, false, false); }
#undef LAME_TILED
    } else {
      const unsigned blocks = (unsigned)(((long long)logits0->d * logits0->h * logits0->w + 255) / 256);
      hipLaunchKernelGGL(lame_generic_kernel, dim3(blocks, items), dim3(256), 0, s, tv(logits0), tv(src), tv(dst),
                         aff ? tv(x) : tv(logits0), aff ? 1 : 0, softmax ? 1 : 0, mask, maxl1, scale, negk, fl);
    }
    const int st = launch_status("lame refine");
    if (st) return st;
  }
  return MMTTA_OK;
}
