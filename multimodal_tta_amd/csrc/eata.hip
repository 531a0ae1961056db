// EATA (Niu et al., ICML 2022, "Efficient Test-Time Model Adaptation without Forgetting") on the flat arena (gfx950): the
// weighted reliable entropy with its gradient, the pseudo-label loss the Fisher estimate differentiates, the accumulation
// of squared gradients into the Fisher span and the pass that adds the Fisher-weighted pull towards the source weights to
// the gradient of every parameter set.  All are single-pass HBM-bound streams.  See include/mmtta.h for the contracts.
#include "voxel_loss.h"

namespace mmtta {

constexpr int FISHER_MAX_BLOCKS = 4096;    // workgroups per parameter set (optim_kernel's figure)
constexpr int PENALTY_BLOCKS = 1024;       // block partials per parameter set of the penalty pass

// ------------------------------------------------------------------ weighted reliable entropy
// The filtered walk of voxel_loss.h, hence the launch geometry, the mask layout and the partial layout of
// mmtta_entropy_filtered_items (loss_optim_metric.hip), over the same entropy definitions (bernoulli_entropy_terms,
// bernoulli_entropy_libm, categorical_entropy), so that keep = H < margin and the kept count are that entry point's.  What
// differs is the weight c = exp(margin - H) in (1, e^margin] on every kept element, a constant of the gradient: pass 1
// leaves the kept sum of c H, pass 2 writes dlogits = keep * c * dH/dz / kept[item].
struct WeightedEntropy : NoOperand {
  static constexpr int ROWS = 2;
  float margin;
  __device__ __forceinline__ bool allowed(long long) const { return true; }
  __device__ __forceinline__ KeptTerms fast(float z, float) const {
    float h, g;
    bernoulli_entropy_terms(z, h, g);
    const float wgt = exp_fast(margin - fminf(h, margin));      // 1 where the element is not kept: never large
    return {h, wgt * h, wgt * g, true};
  }
  __device__ __forceinline__ KeptTerms generic(float z, float) const {
    const BernoulliLibm b = bernoulli_entropy_libm(z);
    const float wgt = expf(margin - fminf(b.h, margin));
    return {b.h, wgt * b.h, wgt * b.g, true};
  }
  template <class F>
  __device__ __forceinline__ KeptTerms categorical(const float* zp, const float*, int R, F&& put) const {
    CategoricalVoxel v;
    categorical_entropy<true>(zp, R, v);
    const float wgt = expf(margin - fminf(v.Hs, margin));
#pragma unroll
    for (int r = 0; r < LOSS_MAX_R; ++r)
      if (r < R) put(r, wgt * categorical_entropy_grad<true>(v, r));
    return {v.H, wgt * v.Hs, 0.f, true};
  }
};

// ------------------------------------------------------------------ pseudo-label loss (the Fisher estimate's objective)
// Bernoulli heads: y = 1[z >= 0], h = BCE(z, y) = -log sigmoid(s) with s = y ? z : -z (= |z|), taken as
// min(s, 0) - log1p(exp(-|s|)): finite for every finite z.  g = sigmoid(z) - y = -+ e / (1 + e), e = exp(-|z|), formed
// without a subtraction.  Both Bernoulli walks use the fast primitives.
// Categorical head: y = one-hot of the FIRST arg max, h = lse(z) - max z = log sum exp(z - max), g = softmax(z) - y.
struct PseudoLabelLoss : NoOperand {
  __device__ __forceinline__ void fast(float z, float, float& h, float& g) const {
    const bool y = z >= 0.f;
    const float s = y ? z : -z;
    const float e = exp_neg_abs(s);
    h = -(fminf(s, 0.f) - log1p_unit(e));
    const float er = sigmoid_pair(s, e).er;
    g = y ? -er : er;
  }
  __device__ __forceinline__ void generic(float z, float o, float& h, float& g) const { fast(z, o, h, g); }
  template <class F>
  __device__ __forceinline__ float categorical(const float* zp, const float*, int R, F&& put) const {
    CategoricalVoxel v;
    categorical_load(zp, R, v);
    const int arg = categorical_argmax(v, R);
    const float inv = 1.f / v.se;          // se >= 1: the maximum contributes exp(0)
#pragma unroll
    for (int r = 0; r < LOSS_MAX_R; ++r)
      if (r < R) put(r, expf(v.t[r] - v.m) * inv - (r == arg ? 1.f : 0.f));
    return logf(v.se);
  }
};

// ------------------------------------------------------------------ Fisher span
// F_i <- F_i + g_{s,i}^2 for s = 0 .. sets-1 in that order: fp32, product and sum rounded separately (torch's F + g * g).  A
// thread owns 4 consecutive elements (16-byte accesses); the last elements of a ragged n go one by one.
__global__ __launch_bounds__(256) void fisher_accumulate_kernel(float* __restrict__ f, const float* __restrict__ g, long long n,
                                                                int sets, long long stride) {
#pragma clang fp contract(off)      // plain operators under this pragma: product and sum must not fuse into an fma (the __f*_rn helpers
                                    // are inlined with their own contraction setting, and do fuse)
  const long long nq = (n + 3) >> 2;
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
    const long long i = q << 2;
    if (i + 4 <= n) {
      float4 a = *reinterpret_cast<const float4*>(f + i);
      for (int s = 0; s < sets; ++s) {
        const float4 v = *reinterpret_cast<const float4*>(g + (long long)s * stride + i);
        a.x = a.x + (v.x * v.x);
        a.y = a.y + (v.y * v.y);
        a.z = a.z + (v.z * v.z);
        a.w = a.w + (v.w * v.w);
      }
      *reinterpret_cast<float4*>(f + i) = a;
    } else {
      for (long long j = i; j < n; ++j) {
        float a = f[j];
        for (int s = 0; s < sets; ++s) {
          const float v = g[(long long)s * stride + j];
          a = a + (v * v);
        }
        f[j] = a;
      }
    }
  }
}

// F_i <- F_i / count (IEEE fp32 division)
__global__ __launch_bounds__(256) void fisher_scale_kernel(float* __restrict__ f, long long n, float count) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    f[i] = __fdiv_rn(f[i], count);
}

// One pass per parameter set (blockIdx.y): g += 2 lambda F (w - source), fp64 block partials of F (w - source)^2.  F and
// source are shared by the sets, w and g are [set][stride].  16 B read, 4 B written per parameter and set.
__global__ __launch_bounds__(256) void fisher_penalty_kernel(const float* __restrict__ w, float* __restrict__ g,
                                                             const float* __restrict__ f, const float* __restrict__ src,
                                                             long long n, long long stride, float two_lambda,
                                                             double* partial) {
#pragma clang fp contract(off)      // separate roundings, as the header states them
  __shared__ double sh[4];
  w += (long long)blockIdx.y * stride;
  g += (long long)blockIdx.y * stride;
  const long long n4 = n >> 2;
  double acc = 0.0;
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < n4; q += (long long)gridDim.x * blockDim.x) {
    const long long i = q << 2;
    const float4 wq = *reinterpret_cast<const float4*>(w + i);
    const float4 sq = *reinterpret_cast<const float4*>(src + i);
    const float4 fq = *reinterpret_cast<const float4*>(f + i);
    float4 gq = *reinterpret_cast<const float4*>(g + i);
    const float dx = (wq.x - sq.x), dy = (wq.y - sq.y), dz = (wq.z - sq.z), dw = (wq.w - sq.w);
    const float px = (fq.x * dx), py = (fq.y * dy), pz = (fq.z * dz), pw = (fq.w * dw);
    gq.x = gq.x + (two_lambda * px);
    gq.y = gq.y + (two_lambda * py);
    gq.z = gq.z + (two_lambda * pz);
    gq.w = gq.w + (two_lambda * pw);
    *reinterpret_cast<float4*>(g + i) = gq;
    acc += (double)px * dx + (double)py * dy + (double)pz * dz + (double)pw * dw;
  }
  const double t = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

__global__ __launch_bounds__(64) void fisher_penalty_finish_kernel(const double* partial, int nblocks, double lambda,
                                                                   float* penalty) {
  partial += (long long)blockIdx.x * nblocks;      // one workgroup per parameter set
  double s = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 64) s += partial[i];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) penalty[blockIdx.x] = (float)(lambda * s);
}

static long long fisher_blocks(int64_t n, int cap) {
  long long b = ((n + 3) / 4 + 255) / 256;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return b;
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int64_t mmtta_entropy_weighted_partials(const mmtta_tensor* logits) {
  if (logits == nullptr || logits->n < 1) return -1;
  return 2 * (int64_t)loss_blocks(logits) * logits->n;
}

extern "C" int mmtta_entropy_weighted_items(const mmtta_tensor* logits, int softmax, float margin, uint8_t* keep_out,
                                            const mmtta_tensor* dlogits, double* partial, float* loss, int64_t* kept,
                                            void* stream) {
  MMTTA_CHECK(__builtin_isfinite(margin) && margin > 0.f, MMTTA_ERR_INVALID,
              "entropy weighted: margin must be finite and positive, got %g", (double)margin);
  MMTTA_CHECK(keep_out != nullptr, MMTTA_ERR_INVALID, "entropy weighted: null mask output");
  MMTTA_CHECK(logits && dlogits && partial && loss && kept && logits->ptr && dlogits->ptr, MMTTA_ERR_INVALID,
              "entropy weighted: null argument");
  MMTTA_CHECK(logits->n == dlogits->n && logits->c == dlogits->c && logits->d == dlogits->d && logits->h == dlogits->h &&
                  logits->w == dlogits->w && logits->n >= 1 && logits->c >= 1 && logits->d >= 1 && logits->h >= 1 &&
                  logits->w >= 1,
              MMTTA_ERR_INVALID, "entropy weighted: shape mismatch");
  MMTTA_CHECK(logits->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "entropy weighted: `logits` must be fp32-stored");
  MMTTA_CHECK(is_cl(logits) && is_cl(dlogits), MMTTA_ERR_UNSUPPORTED, "entropy weighted: channels-last only");
  MMTTA_CHECK(logits->n <= LOSS_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "entropy weighted: more than %d items in one call",
              LOSS_MAX_GRID_Y);
  return kept_launch<WeightedEntropy, long long>({"entropy weighted", "entropy weighted", "entropy weighted"}, logits, dlogits,
                                                 softmax, loss_vec(logits, dlogits), keep_out, partial, loss, (long long*)kept,
                                                 nullptr, WeightedEntropy{{}, margin}, (hipStream_t)stream);
}

extern "C" int64_t mmtta_pseudo_label_partials(const mmtta_tensor* logits) {
  if (logits == nullptr || logits->n < 1) return -1;
  return (int64_t)loss_blocks(logits) * logits->n;
}

extern "C" int mmtta_pseudo_label_loss_items(const mmtta_tensor* logits, int softmax, const mmtta_tensor* dlogits,
                                             double* partial, float* loss, void* stream) {
  MMTTA_CHECK(logits && dlogits && partial && loss && logits->ptr && dlogits->ptr, MMTTA_ERR_INVALID,
              "pseudo-label loss: null argument");
  MMTTA_CHECK(logits->n == dlogits->n && logits->c == dlogits->c && logits->d == dlogits->d && logits->h == dlogits->h &&
                  logits->w == dlogits->w,
              MMTTA_ERR_INVALID, "pseudo-label loss: shape mismatch");
  MMTTA_CHECK(logits->n >= 1, MMTTA_ERR_INVALID, "pseudo-label loss: empty batch");
  MMTTA_CHECK(logits->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "pseudo-label loss: `logits` must be fp32-stored");
  MMTTA_CHECK(is_cl(logits) && is_cl(dlogits), MMTTA_ERR_UNSUPPORTED, "pseudo-label loss: channels-last only");
  MMTTA_CHECK(loss_small_item(logits) && loss_small_item(dlogits), MMTTA_ERR_UNSUPPORTED,
              "pseudo-label loss: an item of 2^31 elements or more");
  MMTTA_CHECK(logits->n <= LOSS_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "pseudo-label loss: more than %d items in one call",
              LOSS_MAX_GRID_Y);
  return loss_launch<PseudoLabelLoss, unsigned>({"pseudo-label loss", "pseudo-label loss", "pseudo-label"}, logits, dlogits,
                                                softmax, loss_vec(logits, dlogits), 1, partial, loss, PseudoLabelLoss{},
                                                (hipStream_t)stream);
}

extern "C" int mmtta_fisher_accumulate_sets(float* fisher, const float* grads, int64_t n, int sets, int64_t set_stride,
                                            void* stream) {
  MMTTA_CHECK(fisher && grads, MMTTA_ERR_INVALID, "fisher accumulate: null argument");
  MMTTA_CHECK(n >= 0, MMTTA_ERR_INVALID, "fisher accumulate: n = %lld", (long long)n);
  MMTTA_CHECK(sets >= 1 && sets <= LOSS_MAX_GRID_Y, MMTTA_ERR_INVALID, "fisher accumulate: sets = %d (1 .. %d)", sets, LOSS_MAX_GRID_Y);
  MMTTA_CHECK(set_stride >= 0 && set_stride % 4 == 0 && (sets == 1 || set_stride >= n), MMTTA_ERR_INVALID,
              "fisher accumulate: %d sets with set_stride %lld (n = %lld; a multiple of 4, >= n)", sets, (long long)set_stride,
              (long long)n);
  MMTTA_CHECK(((uintptr_t)fisher | (uintptr_t)grads) % 16 == 0, MMTTA_ERR_UNSUPPORTED,
              "fisher accumulate: buffers must be 16-byte aligned");
  if (n == 0) return MMTTA_OK;
  hipLaunchKernelGGL(fisher_accumulate_kernel, dim3((unsigned)fisher_blocks(n, FISHER_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream,
                     fisher, grads, (long long)n, sets, (long long)set_stride);
  return launch_status("fisher accumulate");
}

extern "C" int mmtta_fisher_scale(float* fisher, int64_t n, float count, void* stream) {
  MMTTA_CHECK(fisher, MMTTA_ERR_INVALID, "fisher scale: null argument");
  MMTTA_CHECK(n >= 0, MMTTA_ERR_INVALID, "fisher scale: n = %lld", (long long)n);
  MMTTA_CHECK(__builtin_isfinite(count) && count >= 1.f, MMTTA_ERR_INVALID, "fisher scale: count = %g (a finite number >= 1)",
              (double)count);
  if (n == 0) return MMTTA_OK;
  long long b = (n + 255) / 256;
  if (b > FISHER_MAX_BLOCKS) b = FISHER_MAX_BLOCKS;
  hipLaunchKernelGGL(fisher_scale_kernel, dim3((unsigned)b), dim3(256), 0, (hipStream_t)stream, fisher, (long long)n, count);
  return launch_status("fisher scale");
}

extern "C" int64_t mmtta_fisher_penalty_partials(int64_t n, int sets) {
  if (n < 0 || sets < 1) return -1;
  return fisher_blocks(n, PENALTY_BLOCKS) * sets;
}

extern "C" int mmtta_fisher_penalty_sets(const float* w, float* g, const float* fisher, const float* source, int64_t n, int sets,
                                         int replicas, int64_t set_stride, float lambda, double* partial, float* penalty,
                                         void* stream) {
  MMTTA_CHECK(__builtin_isfinite(lambda) && lambda >= 0.f && __builtin_isfinite(2.f * lambda), MMTTA_ERR_INVALID,
              "fisher penalty: lambda must be finite and >= 0, got %g", (double)lambda);
  MMTTA_CHECK(w && g && fisher && source && partial && penalty, MMTTA_ERR_INVALID, "fisher penalty: null argument");
  MMTTA_CHECK(n >= 0 && n % 4 == 0 && set_stride >= 0 && set_stride % 4 == 0, MMTTA_ERR_INVALID,
              "fisher penalty: n = %lld and set_stride = %lld must be multiples of 4", (long long)n, (long long)set_stride);
  MMTTA_CHECK(sets >= 1 && sets <= replicas && sets <= LOSS_MAX_GRID_Y && n <= set_stride, MMTTA_ERR_INVALID,
              "fisher penalty: %d sets of %lld elements do not fit %d replicas of stride %lld", sets, (long long)n, replicas,
              (long long)set_stride);
  MMTTA_CHECK(((uintptr_t)w | (uintptr_t)g | (uintptr_t)fisher | (uintptr_t)source) % 16 == 0, MMTTA_ERR_UNSUPPORTED,
              "fisher penalty: buffers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int blocks = (int)fisher_blocks(n, PENALTY_BLOCKS);
  hipLaunchKernelGGL(fisher_penalty_kernel, dim3((unsigned)blocks, (unsigned)sets), dim3(256), 0, s, w, g, fisher, source,
                     (long long)n, (long long)set_stride, 2.f * lambda, partial);
  int st = launch_status("fisher penalty");
  if (st) return st;
  hipLaunchKernelGGL(fisher_penalty_finish_kernel, dim3(sets), dim3(64), 0, s, (const double*)partial, blocks, (double)lambda,
                     penalty);
  return launch_status("fisher penalty finish");
}
