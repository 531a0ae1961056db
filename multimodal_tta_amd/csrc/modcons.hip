// Modality-consistency objective (in the family of MM-TTA, Shin et al., CVPR 2022) over the modality-subset views of a
// volume (gfx950): the staging of the views, and the entropy of the full view plus the KL of the full view's prediction to
// every subset view's, with the gradient for every view.  See include/mmtta.h for the contract of the three entry points.
//
// Batch layout everywhere: [G * V, D, H, W, R], item g * V + v = view v of volume g; view 0 sees every present modality,
// view v >= 1 a subset of them (the other channels are +0).  The views share the voxel grid: a thread owns a voxel (or a
// (voxel, region) pair) of ALL V views, reads every logit once and writes every gradient once.
#include "voxel_loss.h"

namespace mmtta {

constexpr int MODCONS_MAX_V = 8;
constexpr float MODCONS_PLAIN_BELOW = 16.f;      // categorical head: where view 0's entropy leaves the entropy objective's form

struct ModViews {
  int v;
  unsigned keep[MODCONS_MAX_V];
};

// the scales of one call: ce = w_e / n, cc = lambda / ((V - 1) n), n = the elements of one volume
struct ModconsScale {
  float ce, cc;
  int detach;
};

// ------------------------------------------------------------------ the modality-subset views of the staged input
// y[g * V + v] = x[g] with channel c kept iff bit c of keep[v]; a dropped channel and the pad lanes take +0 - a select on
// the bits, never x * 0: NaN, infinities and -0 of a dropped channel do not reach the view.  Kept values keep their bits.
// Fast path: a thread owns a voxel row of 4 lanes - one 16-byte (fp32: Q = uint4) or 8-byte (bf16: Q = uint2) load, V
// stores.  gridDim.y = volume.
__device__ __forceinline__ uint4 modview_select(uint4 q, unsigned keep) {
  return make_uint4((keep & 1u) ? q.x : 0u, (keep & 2u) ? q.y : 0u, (keep & 4u) ? q.z : 0u, (keep & 8u) ? q.w : 0u);
}
__device__ __forceinline__ uint2 modview_select(uint2 q, unsigned keep) {
  const unsigned lo = ((keep & 1u) ? 0x0000ffffu : 0u) | ((keep & 2u) ? 0xffff0000u : 0u);
  const unsigned hi = ((keep & 4u) ? 0x0000ffffu : 0u) | ((keep & 8u) ? 0xffff0000u : 0u);
  return make_uint2(q.x & lo, q.y & hi);
}
template <class Q>
__global__ __launch_bounds__(256) void modality_views_vec_kernel(const Q* __restrict__ x, Q* __restrict__ y, long long xsn,
                                                                 long long ysn, unsigned dhw, ModViews mv) {
  const Q* xb = x + (long long)blockIdx.y * xsn;
  Q* yb = y + (long long)blockIdx.y * mv.v * ysn;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < dhw; i += gridDim.x * 256u) {
    const Q q = xb[i];
#pragma unroll
    for (int v = 0; v < MODCONS_MAX_V; ++v)
      if (v < mv.v) yb[(long long)v * ysn + i] = modview_select(q, mv.keep[v]);
  }
}
// Generic path: any strides, any channel count up to 32; a thread owns one lane of a voxel row of `y` (lanes = the row
// width where `y` owns its pad, else its channels) and writes it in all V views.  T: the element as bits.
template <class T>
__global__ __launch_bounds__(256) void modality_views_kernel(TV x, TV y, unsigned lanes, ModViews mv) {
  const unsigned C = x.c, D = x.d, H = x.h, W = x.w;
  const unsigned total = D * H * W * lanes;
  const T* xb = reinterpret_cast<const T*>(x.p) + (long long)blockIdx.y * x.sn;
  T* yb = reinterpret_cast<T*>(y.p) + (long long)blockIdx.y * mv.v * y.sn;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned vox = i / lanes, c = i - vox * lanes;
    const unsigned t = vox / W, xx = vox - t * W, zz = t / H, yy = t - zz * H;
    const T val = c < C ? xb[vox_addr(x, 0, zz, yy, xx) + (long long)c * x.sc] : (T)0;
    const long long a = vox_addr(y, 0, zz, yy, xx) + (long long)c * (c < C ? y.sc : 1);
#pragma unroll
    for (int v = 0; v < MODCONS_MAX_V; ++v)
      if (v < mv.v) yb[(long long)v * y.sn + a] = (c < C && ((mv.keep[v] >> c) & 1u)) ? val : (T)0;
  }
}

// ------------------------------------------------------------------ the objective, Bernoulli head
// One (voxel, region) of view 0: what the entropy term and every KL against it need.
struct ModconsTeacher {
  float a;          // the logit
  float p;          // sigmoid(a)
  float er;         // sigmoid(-|a|): the small one of (p, 1 - p)
  float pq;         // p (1 - p)
  float l1p;        // log1p(exp(-|a|))
  float h, gh;      // H(p) and dH/da: the bits of the entropy objective's own path (fast, or LIBM on the generic path)
  bool pos;         // a >= 0
};
template <bool LIBM>
__device__ __forceinline__ ModconsTeacher modcons_teacher(float a) {
  ModconsTeacher t;
  t.a = a;
  const float e = exp_neg_abs(a);
  const SigmoidPair s = sigmoid_pair(a, e);
  t.p = s.p;
  t.er = s.er;
  t.pq = s.er * s.r;
  t.l1p = log1p_unit(e);
  if (LIBM) {
    const BernoulliLibm b = bernoulli_entropy_libm(a);
    t.h = b.h; t.gh = b.g;
  } else {
    bernoulli_entropy_terms(a, t.h, t.gh);
  }
  t.pos = a >= 0.f;
  return t;
}
// KL(sigmoid(a) || sigmoid(b)) = sigmoid(a) (a - b) + softplus(b) - softplus(a) with the terms of the size of the logits
// taken out: sigmoid(a) = [a >= 0] -+ er and softplus(x) = max(x, 0) + log1p(exp(-|x|)), and [a >= 0] (a - b) + max(b, 0) -
// max(a, 0) is |b| where the signs differ and 0 where they agree - exactly.  What is left is of the size of the smaller
// probabilities, so a confident pair keeps its relative accuracy; equal bits give exactly 0; the result is held at 0 from
// below (the rounding of a pair that agrees to 1e-7).  dp = sigmoid(b) - sigmoid(a), from the small sides where the signs
// agree.  Finite for every finite pair whose difference is finite.
__device__ __forceinline__ void modcons_student(const ModconsTeacher& t, float b, float& kl, float& dp, bool& differs) {
  const float e = exp_neg_abs(b);
  const SigmoidPair s = sigmoid_pair(b, e);
  const float l1p = log1p_unit(e);
  const bool pos = b >= 0.f;
  differs = pos != t.pos;
  const float lin = differs ? fabsf(b) : 0.f;
  const float small = t.pos ? -t.er : t.er;          // sigmoid(a) - [a >= 0]
  kl = fmaxf(lin + ((l1p - t.l1p) + small * (t.a - b)), 0.f);
  dp = differs ? s.p - t.p : (pos ? t.er - s.er : s.er - t.er);
}

// Block partials of one volume: rows [entropy | KL of view 1 .. V-1 | disagreement of view 1 .. V-1] x gridDim.x, summed
// in a fixed order (wave shuffle, then the four waves in order).  V is a constant of the fast path's instantiations.
__device__ __forceinline__ void modcons_store_partials(int V, double acc_h, const double (&acc_k)[MODCONS_MAX_V - 1],
                                                       const int (&dis)[MODCONS_MAX_V - 1], double* partial, double* sh) {
  double t = block_sum_d(acc_h, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
#pragma unroll
  for (int v = 1; v < MODCONS_MAX_V; ++v) {
    if (v < V) {
      __syncthreads();
      t = block_sum_d(acc_k[v - 1], sh);
      if (threadIdx.x == 0) partial[(long long)v * gridDim.x + blockIdx.x] = t;
      __syncthreads();
      t = block_sum_d((double)dis[v - 1], sh);
      if (threadIdx.x == 0) partial[(long long)(V - 1 + v) * gridDim.x + blockIdx.x] = t;
    }
  }
}

// Fast path: <= 4 regions in dense 16-byte voxel rows.  A thread owns a voxel: V 16-byte loads, then view by view the four
// KL terms and one 16- / 8-byte gradient store (the gradient tensor owns its pad lane); view 0's row goes last, once the
// teacher's share of every KL is known.  At most 8 x 4 logits and the 4 teacher records are live.  gridDim.y = volume; the
// block partials and the scales of a volume are those of a call on that volume alone.
template <int V, bool OBF>
__global__ __launch_bounds__(256) void modcons_bernoulli_vec_kernel(const float* __restrict__ z, float* __restrict__ dz,
                                                                    long long zsn, long long dzsn, int C, unsigned dhw,
                                                                    double* partial, ModconsScale sc) {
  __shared__ double sh[4];
  const long long item0 = (long long)blockIdx.y * V;
  partial += (long long)blockIdx.y * (2 * V - 1) * gridDim.x;
  double acc_h = 0.0;
  double acc_k[MODCONS_MAX_V - 1];
  int dis[MODCONS_MAX_V - 1];
#pragma unroll
  for (int v = 0; v < MODCONS_MAX_V - 1; ++v) { acc_k[v] = 0.0; dis[v] = 0; }
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < dhw; i += gridDim.x * 256u) {
    const unsigned off = i * 4u;
    float4 t4[V];
#pragma unroll
    for (int v = 0; v < V; ++v) t4[v] = *reinterpret_cast<const float4*>(z + (item0 + v) * zsn + off);
    const float a4[4] = {t4[0].x, t4[0].y, t4[0].z, t4[0].w};
    ModconsTeacher te[4];
    float g0[4] = {0.f, 0.f, 0.f, 0.f};
    float h = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < C) {
        te[c] = modcons_teacher<false>(a4[c]);
        h += te[c].h;
      }
    }
    acc_h += (double)h;
#pragma unroll
    for (int v = 1; v < V; ++v) {
      const float b4[4] = {t4[v].x, t4[v].y, t4[v].z, t4[v].w};
      float g[4] = {0.f, 0.f, 0.f, 0.f};
      float k = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c < C) {
          float kl, dp;
          bool differs;
          modcons_student(te[c], b4[c], kl, dp, differs);
          k += kl;
          g[c] = sc.cc * dp;
          g0[c] += te[c].a - b4[c];
          dis[v - 1] += differs ? 1 : 0;
        }
      }
      acc_k[v - 1] += (double)k;
      st4_any(grad_item<OBF>(dz, item0 + v, dzsn), off, make_float4(g[0], g[1], g[2], g[3]), OBF);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) g0[c] = fmaf(sc.ce, te[c].gh, sc.detach ? 0.f : sc.cc * (te[c].pq * g0[c]));
    st4_any(grad_item<OBF>(dz, item0, dzsn), off, make_float4(g0[0], g0[1], g0[2], g0[3]), OBF);
  }
  modcons_store_partials(V, acc_h, acc_k, dis, partial, sh);
}

// Generic path: any R, any strides, fp32 gradients; a thread owns a (voxel, region) pair of all V views.
__global__ __launch_bounds__(256) void modcons_bernoulli_kernel(TV z, TV dz, int V, double* partial, ModconsScale sc) {
  __shared__ double sh[4];
  const long long item0 = (long long)blockIdx.y * V;
  partial += (long long)blockIdx.y * (2 * V - 1) * gridDim.x;
  const unsigned C = z.c, D = z.d, H = z.h, W = z.w;
  const unsigned total = D * H * W * C;
  double acc_h = 0.0;
  double acc_k[MODCONS_MAX_V - 1];
  int dis[MODCONS_MAX_V - 1];
#pragma unroll
  for (int v = 0; v < MODCONS_MAX_V - 1; ++v) { acc_k[v] = 0.0; dis[v] = 0; }
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned vox = i / C, c = i - vox * C;
    const unsigned t = vox / W, xx = vox - t * W, zz = t / H, yy = t - zz * H;
    const long long za = vox_addr(z, 0, zz, yy, xx) + c, ga = vox_addr(dz, 0, zz, yy, xx) + c;
    const ModconsTeacher te = modcons_teacher<true>(z.p[item0 * z.sn + za]);
    acc_h += (double)te.h;
    float g0 = 0.f;
#pragma unroll
    for (int v = 1; v < MODCONS_MAX_V; ++v) {
      if (v < V) {
        const float b = z.p[(item0 + v) * z.sn + za];
        float kl, dp;
        bool differs;
        modcons_student(te, b, kl, dp, differs);
        acc_k[v - 1] += (double)kl;
        dis[v - 1] += differs ? 1 : 0;
        g0 += te.a - b;
        dz.p[(item0 + v) * dz.sn + ga] = sc.cc * dp;
      }
    }
    dz.p[item0 * dz.sn + ga] = fmaf(sc.ce, te.gh, sc.detach ? 0.f : sc.cc * (te.pq * g0));
  }
  modcons_store_partials(V, acc_h, acc_k, dis, partial, sh);
}

// ------------------------------------------------------------------ the objective, categorical head
// A thread owns a voxel of up to LOSS_MAX_R classes.  View 0's row gives the entropy term, its log softmax
// l0 = (t - max) - log(sum) and p0 = exp(l0).  The entropy term is the entropy objective's own form and bits, H = lse - sum p z,
// while the largest logit stays below MODCONS_PLAIN_BELOW: that form carries the rounding of lse (1e-6 at |z| = 9, the 1e-5 of
// the gradient's maximum the objective is held to), which doubles with every binade; from there on the shifted form
// Hs = log se - sum p (z - max) takes over, exact to fp32 rounding at any magnitude (voxel_loss.h).  Then view by view the row's
// log softmax lv in the same form, KL = sum_k p0_k (l0_k - lv_k) (equal bits: exactly 0; held at 0 from below), the
// gradient (pv - p0) stored at once, and - unless detached - the teacher's share p0_k [(l0_k - lv_k) - KL] added up for
// view 0's row, which goes last.  hard = the first arg max.
__global__ __launch_bounds__(256) void modcons_categorical_kernel(TV z, TV dz, int V, double* partial, ModconsScale sc) {
  __shared__ double sh[4];
  const int R = z.c;
  const long long item0 = (long long)blockIdx.y * V;
  partial += (long long)blockIdx.y * (2 * V - 1) * gridDim.x;
  const unsigned D = z.d, H = z.h, W = z.w;
  const unsigned total = D * H * W;
  double acc_h = 0.0;
  double acc_k[MODCONS_MAX_V - 1];
  int dis[MODCONS_MAX_V - 1];
#pragma unroll
  for (int v = 0; v < MODCONS_MAX_V - 1; ++v) { acc_k[v] = 0.0; dis[v] = 0; }
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned t = i / W, xx = i - t * W, zz = t / H, yy = t - zz * H;
    const long long za = vox_addr(z, 0, zz, yy, xx), ga = vox_addr(dz, 0, zz, yy, xx);
    CategoricalVoxel v0;
    categorical_entropy<true>(z.p + item0 * z.sn + za, R, v0);
    const bool plain = fabsf(v0.m) < MODCONS_PLAIN_BELOW;
    acc_h += (double)(plain ? v0.H : v0.Hs);
    const int arg0 = categorical_argmax(v0, R);
    const float lg0 = v0.lgs;                // log(se), se >= 1: the maximum contributes exp(0)
    float l0[LOSS_MAX_R], p0[LOSS_MAX_R], g0[LOSS_MAX_R];
#pragma unroll
    for (int r = 0; r < LOSS_MAX_R; ++r)
      if (r < R) {
        l0[r] = fmaxf((v0.t[r] - v0.m) - lg0, -3e38f);
        p0[r] = expf(l0[r]);
        g0[r] = 0.f;
      }
    for (int v = 1; v < V; ++v) {
      CategoricalVoxel vv;
      categorical_load(z.p + (item0 + v) * z.sn + za, R, vv);
      const float lg = logf(vv.se);
      float d[LOSS_MAX_R];
      float kl = 0.f;
      float* gp = dz.p + (item0 + v) * dz.sn + ga;
#pragma unroll
      for (int r = 0; r < LOSS_MAX_R; ++r)
        if (r < R) {
          const float lv = fmaxf((vv.t[r] - vv.m) - lg, -3e38f);
          d[r] = l0[r] - lv;
          kl = fmaf(p0[r], d[r], kl);
          gp[r] = sc.cc * (expf(lv) - p0[r]);
        }
#pragma unroll
      for (int r = 0; r < LOSS_MAX_R; ++r)
        if (r < R) g0[r] = fmaf(p0[r], d[r] - kl, g0[r]);
      const double kd = (double)fmaxf(kl, 0.f);
      const int differs = categorical_argmax(vv, R) != arg0 ? 1 : 0;
      // (the view index is not a compile-time constant here: the accumulators are picked by a uniform select)
#pragma unroll
      for (int u = 0; u < MODCONS_MAX_V - 1; ++u)
        if (u == v - 1) { acc_k[u] += kd; dis[u] += differs; }
    }
    float* gp = dz.p + item0 * dz.sn + ga;
#pragma unroll
    for (int r = 0; r < LOSS_MAX_R; ++r)
      if (r < R) {
        const float gh = plain ? categorical_entropy_grad<false>(v0, r) : categorical_entropy_grad<true>(v0, r);
        gp[r] = fmaf(sc.ce, gh, sc.detach ? 0.f : sc.cc * g0[r]);
      }
  }
  modcons_store_partials(V, acc_h, acc_k, dis, partial, sh);
}

// One workgroup per volume: the rows of its block partials in a fixed order, then
// entropy = H, view_kl[v - 1] = K_v, consistency = mean_v K_v, loss = w_e H + lambda C, disagree[v - 1] = the count.
// 1024 threads: a row of 2048 partials is two loads per thread (64 threads take 32 dependent trips per row, 42 us for the 9
// rows of V = 5); a row's sum is the wave shuffle, then the 16 waves in order.
constexpr int MODCONS_FINISH_THREADS = 1024;
__global__ __launch_bounds__(MODCONS_FINISH_THREADS) void modcons_finish_kernel(const double* partial, int nblocks, int V,
                                                                                double inv_count, double we, double lambda,
                                                                                float* loss, float* entropy, float* consistency,
                                                                                float* view_kl, long long* disagree) {
  __shared__ double sh[2 * MODCONS_MAX_V - 1][MODCONS_FINISH_THREADS / 64];
  partial += (long long)blockIdx.x * (2 * V - 1) * nblocks;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < 2 * MODCONS_MAX_V - 1; ++r) {
    if (r < 2 * V - 1) {
      double s = 0.0;
      for (int i = threadIdx.x; i < nblocks; i += MODCONS_FINISH_THREADS) s += partial[(long long)r * nblocks + i];
      s = wave_sum_d(s);
      if (lane == 0) sh[r][wave] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  auto row = [&](int r) {
    double t = 0.0;
    for (int w = 0; w < MODCONS_FINISH_THREADS / 64; ++w) t += sh[r][w];
    return t;
  };
  const double h = row(0) * inv_count;
  double csum = 0.0;
  for (int v = 1; v < V; ++v) {
    const double k = row(v) * inv_count;
    csum += k;
    view_kl[(long long)blockIdx.x * (V - 1) + v - 1] = (float)k;
    disagree[(long long)blockIdx.x * (V - 1) + v - 1] = (long long)row(V - 1 + v);
  }
  const double c = csum / (double)(V - 1);
  entropy[blockIdx.x] = (float)h;
  consistency[blockIdx.x] = (float)c;
  loss[blockIdx.x] = (float)(we * h + lambda * c);
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int mmtta_modality_views(const mmtta_tensor* x, const mmtta_tensor* y, int views, const uint32_t* keep_masks,
                                    void* stream) {
  MMTTA_CHECK(x && y && keep_masks && x->ptr && y->ptr, MMTTA_ERR_INVALID, "modality views: null argument");
  MMTTA_CHECK(views >= 1 && views <= MODCONS_MAX_V, MMTTA_ERR_INVALID, "modality views: views = %d (1 .. %d)", views, MODCONS_MAX_V);
  MMTTA_CHECK(x->n >= 1 && y->n == (int64_t)x->n * views && x->c == y->c && x->d == y->d && x->h == y->h && x->w == y->w &&
                  x->dtype == y->dtype, MMTTA_ERR_INVALID, "modality views: shape mismatch");
  MMTTA_CHECK(x->dtype == MMTTA_F32 || x->dtype == MMTTA_BF16, MMTTA_ERR_UNSUPPORTED, "modality views: fp32 or bf16 rows");
  MMTTA_CHECK(x->c >= 1 && x->c <= 32, MMTTA_ERR_UNSUPPORTED, "modality views: %d channels (1 .. 32: a keep mask is 32 bits)", x->c);
  ModViews mv;
  mv.v = views;
  const uint32_t all = x->c == 32 ? 0xffffffffu : ((1u << x->c) - 1u);
  for (int v = 0; v < MODCONS_MAX_V; ++v) {
    mv.keep[v] = v < views ? keep_masks[v] : 0u;
    MMTTA_CHECK((mv.keep[v] & ~all) == 0, MMTTA_ERR_INVALID, "modality views: keep_masks[%d] = 0x%x names a channel outside the %d channels",
                v, mv.keep[v], x->c);
  }
  MMTTA_CHECK(is_cl(x) && is_cl(y), MMTTA_ERR_UNSUPPORTED, "modality views: channels-last only");
  MMTTA_CHECK(!loss_overlap(x, y), MMTTA_ERR_INVALID, "modality views: `y` overlaps `x`");
  MMTTA_CHECK(loss_small_item(x) && loss_small_item(y), MMTTA_ERR_UNSUPPORTED, "modality views: an item of 2^31 elements or more");
  MMTTA_CHECK(x->n <= LOSS_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "modality views: more than %d volumes in one call", LOSS_MAX_GRID_Y);
  hipStream_t s = (hipStream_t)stream;
  const long long nvox = (long long)x->d * x->h * x->w;
  const bool owns = (y->flags & MMTTA_TENSOR_OWNS_PAD) != 0 && y->sc == 1 && y->sw >= y->c;
  const bool vec = x->c <= 4 && loss_dense4(x) && loss_dense4(y) && (owns || y->c == 4);
  if (vec) {
    long long b = (nvox + 255) / 256;
    if (b > 4096) b = 4096;
    const dim3 grid((unsigned)b, x->n);
    if (x->dtype == MMTTA_BF16)
      hipLaunchKernelGGL(modality_views_vec_kernel<uint2>, grid, dim3(256), 0, s, (const uint2*)x->ptr, (uint2*)y->ptr,
                         (long long)(x->sn / 4), (long long)(y->sn / 4), (unsigned)nvox, mv);
    else
      hipLaunchKernelGGL(modality_views_vec_kernel<uint4>, grid, dim3(256), 0, s, (const uint4*)x->ptr, (uint4*)y->ptr,
                         (long long)(x->sn / 4), (long long)(y->sn / 4), (unsigned)nvox, mv);
    return launch_status("modality views");
  }
  const long long lanes = owns ? y->sw : y->c;
  MMTTA_CHECK(nvox * lanes < (1ll << 31), MMTTA_ERR_UNSUPPORTED, "modality views: an item of 2^31 elements or more");
  long long b = (nvox * lanes + 255) / 256;
  if (b > 4096) b = 4096;
  const dim3 grid((unsigned)b, x->n);
  if (x->dtype == MMTTA_BF16)
    hipLaunchKernelGGL(modality_views_kernel<unsigned short>, grid, dim3(256), 0, s, tv(x), tv(y), (unsigned)lanes, mv);
  else
    hipLaunchKernelGGL(modality_views_kernel<unsigned>, grid, dim3(256), 0, s, tv(x), tv(y), (unsigned)lanes, mv);
  return launch_status("modality views generic");
}

extern "C" int64_t mmtta_modcons_partials(const mmtta_tensor* logits, int views) {
  if (logits == nullptr || views < 2 || views > MODCONS_MAX_V || logits->n < views || logits->n % views) return -1;
  if (logits->c < 1 || logits->d < 1 || logits->h < 1 || logits->w < 1) return -1;
  return (int64_t)(2 * views - 1) * loss_blocks(logits) * (logits->n / views);
}

extern "C" int mmtta_modcons_loss_items(const mmtta_tensor* logits, int softmax, int views, float weight, float entropy_weight,
                                        int detach, const mmtta_tensor* dlogits, double* partial, float* loss, float* entropy,
                                        float* consistency, float* view_kl, int64_t* disagree, void* stream) {
  MMTTA_CHECK(logits && dlogits && partial && loss && entropy && consistency && view_kl && disagree && logits->ptr && dlogits->ptr,
              MMTTA_ERR_INVALID, "modcons loss: null argument");
  MMTTA_CHECK(views >= 2 && views <= MODCONS_MAX_V, MMTTA_ERR_INVALID, "modcons loss: views = %d (2 .. %d)", views, MODCONS_MAX_V);
  MMTTA_CHECK(logits->n >= views && logits->n % views == 0, MMTTA_ERR_INVALID, "modcons loss: batch %d is no multiple of views %d",
              logits->n, views);
  MMTTA_CHECK(same_shape(logits, dlogits), MMTTA_ERR_INVALID, "modcons loss: shape mismatch");
  MMTTA_CHECK(weight >= 0.f && weight <= 3e38f && entropy_weight >= 0.f && entropy_weight <= 3e38f, MMTTA_ERR_INVALID,
              "modcons loss: weight = %g, entropy_weight = %g (finite, >= 0)", (double)weight, (double)entropy_weight);
  MMTTA_CHECK(logits->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "modcons loss: `logits` must be fp32-stored");
  MMTTA_CHECK(is_cl(logits) && is_cl(dlogits), MMTTA_ERR_UNSUPPORTED, "modcons loss: channels-last only");
  MMTTA_CHECK(loss_small_item(logits) && loss_small_item(dlogits), MMTTA_ERR_UNSUPPORTED, "modcons loss: an item of 2^31 elements or more");
  MMTTA_CHECK(!loss_overlap(logits, dlogits), MMTTA_ERR_INVALID, "modcons loss: `dlogits` overlaps `logits`");
  const int volumes = logits->n / views;
  MMTTA_CHECK(volumes <= LOSS_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "modcons loss: more than %d volumes in one call", LOSS_MAX_GRID_Y);
  const bool vec = !softmax && loss_vec(logits, dlogits);
  int st = loss_head_check({"modcons loss", "modcons loss", "modcons"}, logits, dlogits, softmax, vec);
  if (st) return st;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = loss_blocks(logits);
  const long long nvox = (long long)logits->d * logits->h * logits->w;
  const double cnt = softmax ? (double)nvox : (double)nvox * logits->c;
  ModconsScale sc;
  sc.ce = (float)((double)entropy_weight / cnt);
  sc.cc = (float)((double)weight / ((double)(views - 1) * cnt));
  sc.detach = detach ? 1 : 0;
  const dim3 grid(blocks, volumes);
  if (softmax) {
    hipLaunchKernelGGL(modcons_categorical_kernel, grid, dim3(256), 0, s, tv(logits), tv(dlogits), views, partial, sc);
    st = launch_status("modcons categorical");
  } else if (vec) {
    const float* zp = (const float*)logits->ptr;
    float* gp = (float*)dlogits->ptr;
#define MODCONS_VEC(VV)                                                                                                     \
  case VV:                                                                                                                  \
    if (is_bf16(dlogits))                                                                                                   \
      hipLaunchKernelGGL((modcons_bernoulli_vec_kernel<VV, true>), grid, dim3(256), 0, s, zp, gp, (long long)logits->sn,      \
                         (long long)dlogits->sn, (int)logits->c, (unsigned)nvox, partial, sc);                              \
    else                                                                                                                    \
      hipLaunchKernelGGL((modcons_bernoulli_vec_kernel<VV, false>), grid, dim3(256), 0, s, zp, gp, (long long)logits->sn,     \
                         (long long)dlogits->sn, (int)logits->c, (unsigned)nvox, partial, sc);                              \
    break
    switch (views) {
      MODCONS_VEC(2);
      MODCONS_VEC(3);
      MODCONS_VEC(4);
      MODCONS_VEC(5);
      MODCONS_VEC(6);
      MODCONS_VEC(7);
      default:
      MODCONS_VEC(8);
    }
#undef MODCONS_VEC
    st = launch_status("modcons bernoulli");
  } else {
    hipLaunchKernelGGL(modcons_bernoulli_kernel, grid, dim3(256), 0, s, tv(logits), tv(dlogits), views, partial, sc);
    st = launch_status("modcons bernoulli generic");
  }
  if (st) return st;
  hipLaunchKernelGGL(modcons_finish_kernel, dim3(volumes), dim3(MODCONS_FINISH_THREADS), 0, s, (const double*)partial, blocks, views, 1.0 / cnt,
                     (double)entropy_weight, (double)weight, loss, entropy, consistency, view_kl, (long long*)disagree);
  return launch_status("modcons finish");
}
