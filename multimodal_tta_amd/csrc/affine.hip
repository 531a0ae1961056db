// Affine (rotate / scale / shift) teacher views (gfx950): the trilinear resample that stages them and the ensemble that
// brings every view's prediction back into the volume's frame.  See include/mmtta.h for the contract of the two entry
// points.  The teacher's predictions take no gradient, so both directions are GATHERS: a thread owns an output voxel and
// reads the 8 corners around its image; there is no adjoint, no scatter and there are no atomics.
//
// One definition of "trilinear" serves both kernels.  A matrix is 12 fp32 numbers, row-major 3 x 4, and maps the voxel
// (d, h, w) a thread owns to the continuous coordinate it samples, axis k in this order (three fmaf, innermost first):
//     p_k = fmaf(m[4k], d, fmaf(m[4k + 1], h, fmaf(m[4k + 2], w, m[4k + 3])))
// Per axis, with f = floor(p_k) and t = p_k - f, corner f weighs 1 - t and corner f + 1 weighs t; a corner outside
// [0, extent) weighs 0, as does every corner of an axis with p_k outside (-1, extent) (or not finite).  The value is the
// sum over the 8 corners, in the order (d, h, w) = 000, 001, .. 111, of fmaf((w_d * w_h) * w_w, corner value, sum); a corner
// of weight 0 is not read.  This is torch.nn.functional.grid_sample(mode = "bilinear", padding_mode = "zeros",
// align_corners = True) on 5-D input up to rounding.  An identity matrix gives weight 1 to one corner: the value itself;
// an integer translation likewise (p_k = d + t_k is exact).
//
// Neighbouring threads share corners, so the gathers hit in cache; there is no LDS tile (profiles/affine_kernels.md has
// the decision and the figures it rests on).
#include "voxel_loss.h"

namespace mmtta {

constexpr int AFF_MAX_V = 8;
constexpr int AFF_TURN = 16;                    // bit 4 of a coded view: H and W transposed before the mirrors (memo.hip)
constexpr float AFF_TINY = 1.17549435e-38f;     // smallest normal fp32
constexpr float AFF_LOGIT_MAX = 87.3365f;       // -ln(AFF_TINY): as far as the fp32 sigmoid inverts

struct AffCodes {
  int v, first, count;
  int axes[AFF_MAX_V];
};

// one axis of the footprint: the two corners (clamped into the tensor) and their hat weights (0 where outside)
struct AffAxis {
  unsigned lo, hi;
  float wlo, whi;
};
__device__ __forceinline__ AffAxis aff_axis(float p, int E) {
  AffAxis a;
  const bool in = p > -1.f && p < (float)E;      // false for inf and NaN too
  const float pc = in ? p : 0.f;
  const float f = floorf(pc);
  const float t = pc - f;
  const int i = (int)f;                           // -1 .. E - 1
  a.wlo = (in && i >= 0) ? 1.f - t : 0.f;
  a.whi = (in && i + 1 < E) ? t : 0.f;
  a.lo = (unsigned)max(i, 0);
  a.hi = (unsigned)min(i + 1, E - 1);
  return a;
}
struct AffFoot {
  AffAxis d, h, w;
};
struct AffMat {
  float m[12];
};
__device__ __forceinline__ AffMat aff_load(const float* __restrict__ p) {
  AffMat a;
#pragma unroll
  for (int i = 0; i < 12; ++i) a.m[i] = p[i];
  return a;
}
__device__ __forceinline__ AffFoot aff_foot(const AffMat& a, unsigned z, unsigned y, unsigned x, int D, int H, int W) {
  const float fd = (float)z, fh = (float)y, fw = (float)x;
  AffFoot f;
  f.d = aff_axis(fmaf(a.m[0], fd, fmaf(a.m[1], fh, fmaf(a.m[2], fw, a.m[3]))), D);
  f.h = aff_axis(fmaf(a.m[4], fd, fmaf(a.m[5], fh, fmaf(a.m[6], fw, a.m[7]))), H);
  f.w = aff_axis(fmaf(a.m[8], fd, fmaf(a.m[9], fh, fmaf(a.m[10], fw, a.m[11]))), W);
  return f;
}
// corner k (bit 2 = d, bit 1 = h, bit 0 = w) of a footprint: its weight and coordinates
__device__ __forceinline__ float aff_corner(const AffFoot& f, int k, unsigned& zz, unsigned& yy, unsigned& xx) {
  zz = (k & 4) ? f.d.hi : f.d.lo;
  yy = (k & 2) ? f.h.hi : f.h.lo;
  xx = (k & 1) ? f.w.hi : f.w.lo;
  return (((k & 4) ? f.d.whi : f.d.wlo) * ((k & 2) ? f.h.whi : f.h.wlo)) * ((k & 1) ? f.w.whi : f.w.wlo);
}

// coordinates of linear voxel i of the frame (32-bit: the host checks loss_small_item)
__device__ __forceinline__ void aff_vox(unsigned i, unsigned H, unsigned W, unsigned& z, unsigned& y, unsigned& x) {
  const unsigned t = i / W;
  x = i - t * W;
  z = t / H;
  y = t - z * H;
}
// the image of frame voxel (z, y, x) in a coded view (mmtta_memo_ensemble's meaning of the code; bit 4 needs H == W)
__device__ __forceinline__ void aff_coded(int m, unsigned z, unsigned y, unsigned x, unsigned D, unsigned H, unsigned W,
                                          unsigned& zz, unsigned& yy, unsigned& xx) {
  const unsigned a = (m & AFF_TURN) ? x : y, b = (m & AFF_TURN) ? y : x;
  zz = (m & 4) ? D - 1 - z : z;
  yy = (m & 2) ? H - 1 - a : a;
  xx = (m & 1) ? W - 1 - b : b;
}

__device__ __forceinline__ float aff_ln(float x) { return __builtin_amdgcn_logf(x) * 0.6931471805599453f; }   // x normal
// log P - log Q of two non-negative sums over one denominator, held inside +-87.3365
__device__ __forceinline__ float aff_logit(float P, float Q) {
  const float t = aff_ln(fmaxf(P, AFF_TINY)) - aff_ln(fmaxf(Q, AFF_TINY));
  return fminf(fmaxf(t, -AFF_LOGIT_MAX), AFF_LOGIT_MAX);
}

// ------------------------------------------------------------------ staging: y item = trilinear resample of x[g]
// A thread owns L lanes of one output voxel row (L = 4: the whole 16- / 8-byte row of a 4-lane tensor, or a quad of a wider
// one; L = 1: rows no vector access fits): 8 gathers of L lanes, fp32 arithmetic, one store.  Lanes >= C take 0.
// gridDim.y = affine item (g, j).
template <int L, bool BF>
__global__ __launch_bounds__(256) void affine_views_kernel(const float* __restrict__ x, float* __restrict__ y, long long xsn,
                                                           long long ysn, unsigned upr, int C, int D, int H, int W, int views,
                                                           int first, int count, const float* __restrict__ mats) {
  const int g = blockIdx.y / count, j = blockIdx.y - g * count;
  const AffMat a = aff_load(mats + (long long)blockIdx.y * 12);
  const long long xb = (long long)g * xsn, yb = ((long long)g * views + first + j) * ysn;      // element offsets
  const unsigned total = (unsigned)D * H * W * upr;
  const unsigned row = upr * L;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned vox = i / upr, u = i - vox * upr;
    unsigned z, yv, xv;
    aff_vox(vox, H, W, z, yv, xv);
    const AffFoot f = aff_foot(a, z, yv, xv, D, H, W);
    float acc[L];
#pragma unroll
    for (int l = 0; l < L; ++l) acc[l] = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      unsigned zz, yy, xx;
      const float wgt = aff_corner(f, k, zz, yy, xx);
      if (wgt != 0.f) {
        const long long src = xb + (long long)(((zz * H + yy) * W + xx) * row + u * L);
        if constexpr (L == 4) {
          const float4 t = ld4_any(x, src, BF);
          acc[0] = fmaf(wgt, t.x, acc[0]);
          acc[1] = fmaf(wgt, t.y, acc[1]);
          acc[2] = fmaf(wgt, t.z, acc[2]);
          acc[3] = fmaf(wgt, t.w, acc[3]);
        } else {
          acc[0] = fmaf(wgt, ld1_any(x, src, BF), acc[0]);
        }
      }
    }
#pragma unroll
    for (int l = 0; l < L; ++l)
      if ((int)(u * L) + l >= C) acc[l] = 0.f;
    const long long dst = yb + (long long)(vox * row + u * L);
    if constexpr (L == 4) st4_any(y, dst, make_float4(acc[0], acc[1], acc[2], acc[3]), BF);
    else st1_any(y, dst, acc[0], BF);
  }
}

// ------------------------------------------------------------------ ensemble, Bernoulli head
// Fast path: <= 4 regions in dense 16-byte rows, `out` owning its pad lanes (they take 0).  A thread owns a frame voxel:
// one 16-byte load per coded view, up to 8 per affine view, one 16-byte store.  gridDim.y = volume.
__global__ __launch_bounds__(256) void affine_ensemble_vec_kernel(const float* __restrict__ z, float* __restrict__ out, long long zsn,
                                                                  long long osn, int C, int D, int H, int W, AffCodes cd,
                                                                  const float* __restrict__ inv) {
  const long long item0 = (long long)blockIdx.y * cd.v;
  const unsigned total = (unsigned)D * H * W;
  float* ob = out + (long long)blockIdx.y * osn;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    unsigned zf, yf, xf;
    aff_vox(i, H, W, zf, yf, xf);
    float P[4] = {0.f, 0.f, 0.f, 0.f}, Q[4] = {0.f, 0.f, 0.f, 0.f};
    auto add = [&](const float* zb, unsigned zz, unsigned yy, unsigned xx, float wgt) {
      const float4 t4 = *reinterpret_cast<const float4*>(zb + ((zz * H + yy) * W + xx) * 4u);
      const float ts[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) {
          const SigmoidPair s = sigmoid_pair(ts[c], exp_neg_abs(ts[c]));
          P[c] = fmaf(wgt, s.p, P[c]);
          Q[c] = fmaf(wgt, s.q, Q[c]);
        }
    };
#pragma unroll
    for (int v = 0; v < AFF_MAX_V; ++v)
      if (v < cd.first) {
        unsigned zz, yy, xx;
        aff_coded(cd.axes[v], zf, yf, xf, D, H, W, zz, yy, xx);
        add(z + (item0 + v) * zsn, zz, yy, xx, 1.f);
      }
    for (int j = 0; j < cd.count; ++j) {
      const AffMat a = aff_load(inv + ((long long)blockIdx.y * cd.count + j) * 12);
      const AffFoot f = aff_foot(a, zf, yf, xf, D, H, W);
      const float* zb = z + (item0 + cd.first + j) * zsn;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        unsigned zz, yy, xx;
        const float wgt = aff_corner(f, k, zz, yy, xx);
        if (wgt != 0.f) add(zb, zz, yy, xx, wgt);
      }
    }
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) o[c] = aff_logit(P[c], Q[c]);
    *reinterpret_cast<float4*>(ob + i * 4u) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// Generic path: any R, any strides; a thread owns a (voxel, region) pair.
__global__ __launch_bounds__(256) void affine_ensemble_bernoulli_kernel(TV z, TV out, AffCodes cd, const float* __restrict__ inv) {
  const long long item0 = (long long)blockIdx.y * cd.v;
  const int C = z.c, D = z.d, H = z.h, W = z.w;
  const unsigned total = (unsigned)D * H * W * C;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned vox = i / C, c = i - vox * C;
    unsigned zf, yf, xf;
    aff_vox(vox, H, W, zf, yf, xf);
    float P = 0.f, Q = 0.f;
    auto add = [&](long long item, unsigned zz, unsigned yy, unsigned xx, float wgt) {
      const float t = z.p[vox_addr(z, (int)item, (int)zz, (int)yy, (int)xx) + c];
      const SigmoidPair s = sigmoid_pair(t, exp_neg_abs(t));
      P = fmaf(wgt, s.p, P);
      Q = fmaf(wgt, s.q, Q);
    };
#pragma unroll
    for (int v = 0; v < AFF_MAX_V; ++v)
      if (v < cd.first) {
        unsigned zz, yy, xx;
        aff_coded(cd.axes[v], zf, yf, xf, D, H, W, zz, yy, xx);
        add(item0 + v, zz, yy, xx, 1.f);
      }
    for (int j = 0; j < cd.count; ++j) {
      const AffMat a = aff_load(inv + ((long long)blockIdx.y * cd.count + j) * 12);
      const AffFoot f = aff_foot(a, zf, yf, xf, D, H, W);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        unsigned zz, yy, xx;
        const float wgt = aff_corner(f, k, zz, yy, xx);
        if (wgt != 0.f) add(item0 + cd.first + j, zz, yy, xx, wgt);
      }
    }
    out.p[vox_addr(out, (int)blockIdx.y, (int)zf, (int)yf, (int)xf) + c] = aff_logit(P, Q);
  }
}

// ------------------------------------------------------------------ ensemble, categorical head (<= LOSS_MAX_R classes)
// A thread owns a frame voxel; P_r sums weight x softmax row over the coded views (weight 1) and the inside corners of the
// affine views, Wt the weights: out_r = log(P_r / Wt) >= -3e38.
__global__ __launch_bounds__(256) void affine_ensemble_categorical_kernel(TV z, TV out, AffCodes cd, const float* __restrict__ inv) {
  const long long item0 = (long long)blockIdx.y * cd.v;
  const int R = z.c, D = z.d, H = z.h, W = z.w;
  const unsigned total = (unsigned)D * H * W;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    unsigned zf, yf, xf;
    aff_vox(i, H, W, zf, yf, xf);
    float P[LOSS_MAX_R];
#pragma unroll
    for (int r = 0; r < LOSS_MAX_R; ++r) P[r] = 0.f;
    float Wt = 0.f;
    auto add = [&](long long item, unsigned zz, unsigned yy, unsigned xx, float wgt) {
      CategoricalVoxel cv;
      categorical_load(z.p + vox_addr(z, (int)item, (int)zz, (int)yy, (int)xx), R, cv);
      const float sc = wgt / cv.se;            // se >= 1
#pragma unroll
      for (int r = 0; r < LOSS_MAX_R; ++r)
        if (r < R) P[r] = fmaf(sc, expf(cv.t[r] - cv.m), P[r]);
      Wt += wgt;
    };
#pragma unroll 1
    for (int v = 0; v < cd.first; ++v) {
      unsigned zz, yy, xx;
      aff_coded(cd.axes[v], zf, yf, xf, D, H, W, zz, yy, xx);
      add(item0 + v, zz, yy, xx, 1.f);
    }
#pragma unroll 1
    for (int j = 0; j < cd.count; ++j) {
      const AffMat a = aff_load(inv + ((long long)blockIdx.y * cd.count + j) * 12);
      const AffFoot f = aff_foot(a, zf, yf, xf, D, H, W);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        unsigned zz, yy, xx;
        const float wgt = aff_corner(f, k, zz, yy, xx);
        if (wgt != 0.f) add(item0 + cd.first + j, zz, yy, xx, wgt);
      }
    }
    float* op = out.p + vox_addr(out, (int)blockIdx.y, (int)zf, (int)yf, (int)xf);
    const float iw = 1.f / Wt;                  // Wt >= first >= 1
#pragma unroll
    for (int r = 0; r < LOSS_MAX_R; ++r)
      if (r < R) op[r] = fmaxf(logf(P[r] * iw), -3e38f);
  }
}

// the argument rules both entry points share: the view counts, the extents and the matrices' pointers ...
static int affine_counts_check(const char* what, int views, int first, int count, int n, const float* host, const float* dev,
                               int d, int h, int w) {
  MMTTA_CHECK(views >= 2 && views <= AFF_MAX_V, MMTTA_ERR_INVALID, "%s: views = %d (2 .. 8)", what, views);
  MMTTA_CHECK(count >= 1 && first >= 1 && first + count == views, MMTTA_ERR_INVALID,
              "%s: first = %d, count = %d: expected first >= 1, count >= 1 and first + count == views = %d", what, first, count, views);
  MMTTA_CHECK(n >= views && n % views == 0, MMTTA_ERR_INVALID, "%s: batch %d is no multiple of views %d", what, n, views);
  MMTTA_CHECK(d >= 2 && h >= 2 && w >= 2, MMTTA_ERR_INVALID, "%s: extents d = %d, h = %d, w = %d: every extent must be >= 2", what, d, h, w);
  MMTTA_CHECK(host != nullptr && dev != nullptr, MMTTA_ERR_INVALID, "%s: null argument (matrices)", what);
  return MMTTA_OK;
}
// ... and the host copy [volumes, count, 12] of the matrices, read once the shapes agree
static int affine_finite_check(const char* what, const float* host, int volumes, int first, int count) {
  for (long long i = 0; i < (long long)volumes * count * 12; ++i)
    MMTTA_CHECK(__builtin_isfinite(host[i]), MMTTA_ERR_INVALID, "%s: matrix entry %lld (volume %lld, view %lld) is not finite", what,
                i, i / (12 * count), first + (i / 12) % count);
  return MMTTA_OK;
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int mmtta_affine_views(const mmtta_tensor* x, const mmtta_tensor* y, int views, int first, int count,
                                  const float* matrices_host, const float* matrices, void* stream) {
  MMTTA_CHECK(x && y && x->ptr && y->ptr, MMTTA_ERR_INVALID, "affine views: null argument");
  int st = affine_counts_check("affine views", views, first, count, y->n, matrices_host, matrices, x->d, x->h, x->w);
  if (st) return st;
  MMTTA_CHECK((int64_t)y->n == (int64_t)x->n * views && x->c == y->c && x->d == y->d && x->h == y->h && x->w == y->w &&
                  x->dtype == y->dtype, MMTTA_ERR_INVALID, "affine views: shape mismatch");
  st = affine_finite_check("affine views", matrices_host, x->n, first, count);
  if (st) return st;
  MMTTA_CHECK(x->dtype == MMTTA_F32 || x->dtype == MMTTA_BF16, MMTTA_ERR_UNSUPPORTED, "affine views: fp32 or bf16 rows");
  auto dense = [](const mmtta_tensor* t) {
    return t->sc == 1 && t->sw >= t->c && t->sh == (int64_t)t->w * t->sw && t->sd == (int64_t)t->h * t->sh;
  };
  MMTTA_CHECK(dense(x) && dense(y) && x->sw == y->sw, MMTTA_ERR_UNSUPPORTED, "affine views: dense channels-last rows of one width");
  MMTTA_CHECK(y->sw == y->c || (y->flags & MMTTA_TENSOR_OWNS_PAD), MMTTA_ERR_UNSUPPORTED, "affine views: `y` must own the pad lanes of its rows");
  MMTTA_CHECK(loss_small_item(x), MMTTA_ERR_UNSUPPORTED, "affine views: an item of 2^31 elements or more");
  MMTTA_CHECK((int64_t)x->n * count <= LOSS_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "affine views: more than %d output items in one call", LOSS_MAX_GRID_Y);
  const bool bf = x->dtype == MMTTA_BF16;
  const long long esz = bf ? 2 : 4;
  const uintptr_t both = (uintptr_t)x->ptr | (uintptr_t)y->ptr | (uintptr_t)(x->sn * esz) | (uintptr_t)(y->sn * esz);
  MMTTA_CHECK(both % esz == 0, MMTTA_ERR_UNSUPPORTED, "affine views: misaligned tensor");
  const bool quad = x->sw % 4 == 0 && both % (4 * esz) == 0;
  const int L = quad ? 4 : 1;
  const unsigned upr = (unsigned)(x->sw / L);
  const long long units = (long long)x->d * x->h * x->w * upr;
  long long b = (units + 255) / 256;
  if (b > 4096) b = 4096;
  const dim3 grid((unsigned)b, (unsigned)(x->n * count));
  hipStream_t s = (hipStream_t)stream;
#define AFF_VIEWS(LL, BB)                                                                                                       \
  hipLaunchKernelGGL((affine_views_kernel<LL, BB>), grid, dim3(256), 0, s, (const float*)x->ptr, (float*)y->ptr, (long long)x->sn, \
                     (long long)y->sn, upr, (int)x->c, (int)x->d, (int)x->h, (int)x->w, views, first, count, matrices)
  if (quad && bf) AFF_VIEWS(4, true);
  else if (quad) AFF_VIEWS(4, false);
  else if (bf) AFF_VIEWS(1, true);
  else AFF_VIEWS(1, false);
#undef AFF_VIEWS
  return launch_status("affine views");
}

extern "C" int mmtta_affine_ensemble(const mmtta_tensor* logits, int softmax, int views, const int32_t* view_axes, int first,
                                     int count, const float* inv_host, const float* inv, const mmtta_tensor* out, void* stream) {
  MMTTA_CHECK(logits && out && logits->ptr && out->ptr, MMTTA_ERR_INVALID, "affine ensemble: null argument");
  MMTTA_CHECK(view_axes != nullptr, MMTTA_ERR_INVALID, "affine ensemble: null argument (view_axes)");
  int st = affine_counts_check("affine ensemble", views, first, count, logits->n, inv_host, inv, logits->d, logits->h, logits->w);
  if (st) return st;
  AffCodes cd;
  cd.v = views; cd.first = first; cd.count = count;
  MMTTA_CHECK(view_axes[0] == 0, MMTTA_ERR_INVALID, "affine ensemble: view_axes[0] = %d, view 0 is the unmirrored volume", view_axes[0]);
  for (int v = 0; v < AFF_MAX_V; ++v) {
    cd.axes[v] = v < views ? view_axes[v] : 0;
    if (v < first) {
      MMTTA_CHECK((cd.axes[v] & ~(7 | AFF_TURN)) == 0, MMTTA_ERR_INVALID,
                  "affine ensemble: view_axes[%d] = %d (bit 0 = W, 1 = H, 2 = D mirrored, bit 4 = H and W transposed first)", v, cd.axes[v]);
      MMTTA_CHECK(!(cd.axes[v] & AFF_TURN) || logits->h == logits->w, MMTTA_ERR_INVALID,
                  "affine ensemble: view_axes[%d] = %d transposes H and W, which needs h == w: h = %d, w = %d", v, cd.axes[v],
                  logits->h, logits->w);
    } else {
      MMTTA_CHECK(cd.axes[v] == 0, MMTTA_ERR_INVALID, "affine ensemble: view_axes[%d] = %d on an affine view (views >= first = %d carry code 0)",
                  v, cd.axes[v], first);
    }
  }
  MMTTA_CHECK((int64_t)logits->n == (int64_t)out->n * views && logits->c == out->c && logits->d == out->d && logits->h == out->h &&
                  logits->w == out->w, MMTTA_ERR_INVALID, "affine ensemble: shape mismatch");
  st = affine_finite_check("affine ensemble", inv_host, out->n, first, count);
  if (st) return st;
  MMTTA_CHECK(logits->dtype == MMTTA_F32 && out->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "affine ensemble: fp32-stored tensors only");
  MMTTA_CHECK(is_cl(logits) && is_cl(out), MMTTA_ERR_UNSUPPORTED, "affine ensemble: channels-last only");
  MMTTA_CHECK(loss_small_item(logits) && loss_small_item(out), MMTTA_ERR_UNSUPPORTED, "affine ensemble: an item of 2^31 elements or more");
  MMTTA_CHECK(!softmax || logits->c <= LOSS_MAX_R, MMTTA_ERR_UNSUPPORTED, "affine ensemble softmax: more than %d classes", LOSS_MAX_R);
  MMTTA_CHECK(out->n <= LOSS_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "affine ensemble: more than %d volumes in one call", LOSS_MAX_GRID_Y);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(loss_blocks(logits), out->n);
  if (softmax) {
    hipLaunchKernelGGL(affine_ensemble_categorical_kernel, grid, dim3(256), 0, s, tv(logits), tv(out), cd, inv);
  } else if (logits->c <= 4 && loss_dense16(logits) && loss_dense16(out) && ((out->flags & MMTTA_TENSOR_OWNS_PAD) || out->c == 4)) {
    hipLaunchKernelGGL(affine_ensemble_vec_kernel, grid, dim3(256), 0, s, (const float*)logits->ptr, (float*)out->ptr,
                       (long long)logits->sn, (long long)out->sn, (int)logits->c, (int)logits->d, (int)logits->h, (int)logits->w, cd, inv);
  } else {
    hipLaunchKernelGGL(affine_ensemble_bernoulli_kernel, grid, dim3(256), 0, s, tv(logits), tv(out), cd, inv);
  }
  return launch_status("affine ensemble");
}
