// CoTTA (Wang et al., CVPR 2022, "Continual Test-Time Domain Adaptation") on the flat arena (gfx950): the consistency loss
// of the student against the teacher's soft target with its gradient, and the pass that follows the student's optimizer
// step - the teacher's exponential moving average and the stochastic restore of the student - over every parameter set.
// Both are single-pass HBM-bound streams.  See include/mmtta.h for the contract of the entry points.
#include "voxel_loss.h"

namespace mmtta {

constexpr float CONS_CLAMP = 87.33654f;    // -ln(smallest normal fp32): where mmtta_memo_ensemble holds its logit
constexpr int COTTA_MAX_BLOCKS = 4096;     // workgroups per parameter set (optim_kernel's figure)

// The plain walk of voxel_loss.h over the consistency arithmetic; the second operand is the teacher's target.
// Bernoulli heads: h = -q log sigmoid(z) - (1 - q) log sigmoid(-z), g = sigmoid(z) - q with q = sigmoid(t).  Both sigmoids
// are taken at the logit held inside +-CONS_CLAMP (the ensemble's own bound) by the same instructions (sigmoid_pair), so
// t == z gives g == 0 exactly; neither 1 - q nor 1 - sigmoid(z) is formed by subtraction.  The clamp is this objective's
// own: the entropy terms take their logit as it is.  log sigmoid(z) = min(z, 0) - log1p(exp(-|z|)) with the unclamped z
// in front: finite for every finite z.
// Categorical head: h = -sum_r exp(t_r) log softmax(z)_r, g_r = softmax(z)_r - exp(t_r); t = log pbar as
// mmtta_memo_ensemble writes it (held at -3e38 from below, as that kernel holds its log softmax).  The log softmax is the
// ensemble's own form - (z - max) - log(sum) - so that a target made from the same logits gives g == 0 exactly.
struct ConsistencyLoss : SameVoxelOperand {
  __device__ __forceinline__ void fast(float z, float t, float& h, float& g) const {
    const float zc = fminf(fmaxf(z, -CONS_CLAMP), CONS_CLAMP), tc = fminf(fmaxf(t, -CONS_CLAMP), CONS_CLAMP);
    const SigmoidPair q = sigmoid_pair(tc, exp_neg_abs(tc));
    const float e = exp_neg_abs(zc);
    const float p = sigmoid_pair(zc, e).p;
    const float l1p = log1p_unit(e);
    const float lsp = fminf(z, 0.f) - l1p, lsn = fminf(-z, 0.f) - l1p;         // log sigmoid(z), log sigmoid(-z)
    h = -fmaf(q.p, lsp, q.q * lsn);
    g = p - q.p;
  }
  __device__ __forceinline__ void generic(float z, float t, float& h, float& g) const { fast(z, t, h, g); }
  template <class F>
  __device__ __forceinline__ float categorical(const float* zp, const float* tp, int R, F&& put) const {
    CategoricalVoxel v;
    categorical_load(zp, R, v);
    const float lg = logf(v.se);           // se >= 1: the maximum contributes exp(0)
    float h = 0.f;
#pragma unroll
    for (int r = 0; r < LOSS_MAX_R; ++r)
      if (r < R) {
        const float l = fmaxf((v.t[r] - v.m) - lg, -3e38f);
        const float q = expf(fmaxf(tp[r], -3e38f));
        h = fmaf(-q, l, h);
        put(r, expf(l) - q);
      }
    return h;
  }
};

// ------------------------------------------------------------------ teacher EMA + stochastic restore
// Philox4x32-10 (Salmon et al., SC 2011; the generator of Random123, curand and hiprand), written out.
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, unsigned k0, unsigned k1) {
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
__device__ __forceinline__ bool cotta_draw(unsigned word, float p) { return (float)(word >> 8) * 5.9604644775390625e-8f < p; }

// One pass over [sets][n]: w' <- a w' + b w (the student AFTER its optimizer step), then w_i <- w0_i where u_i < p.  A thread
// owns 4 consecutive elements - 16-byte accesses, 12 B read and 8 B written per parameter - and one Philox call, counter
// (i >> 2, *step, ordinal[set], 0), whose four words serve them.  The last elements of a ragged n go one by one.  The
// restored elements are counted per workgroup (int64 block partials) and summed per set by cotta_finish_kernel.
__global__ __launch_bounds__(256) void cotta_update_kernel(float* __restrict__ w, float* __restrict__ teacher,
                                                           const float* __restrict__ source, long long n, long long w_stride,
                                                           long long t_stride, float a, float b, float p, unsigned k0,
                                                           unsigned k1, const int* __restrict__ step,
                                                           const int* __restrict__ ordinals, long long* partial) {
  __shared__ int sh[4];
  w += (long long)blockIdx.y * w_stride;
  teacher += (long long)blockIdx.y * t_stride;
  const unsigned t = (unsigned)*step, ord = (unsigned)ordinals[blockIdx.y];
  const bool ema = !(a == 1.f && b == 0.f);      // alpha = 1: the teacher keeps its bits (-0 included) and is not written
  const bool draw = p > 0.f;
  const long long nq = (n + 3) >> 2;
  int count = 0;
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
    const long long i = q << 2;
    uint4 u = make_uint4(0u, 0u, 0u, 0u);
    if (draw) u = philox4x32_10(make_uint4((unsigned)q, t, ord, 0u), k0, k1);
    if (i + 4 <= n) {
      float4 wq = *reinterpret_cast<const float4*>(w + i);
      if (ema) {
        const float4 tq = *reinterpret_cast<const float4*>(teacher + i);
        *reinterpret_cast<float4*>(teacher + i) =
            make_float4(__fadd_rn(__fmul_rn(a, tq.x), __fmul_rn(b, wq.x)), __fadd_rn(__fmul_rn(a, tq.y), __fmul_rn(b, wq.y)),
                        __fadd_rn(__fmul_rn(a, tq.z), __fmul_rn(b, wq.z)), __fadd_rn(__fmul_rn(a, tq.w), __fmul_rn(b, wq.w)));
      }
      if (draw) {
        const bool r0 = cotta_draw(u.x, p), r1 = cotta_draw(u.y, p), r2 = cotta_draw(u.z, p), r3 = cotta_draw(u.w, p);
        if (r0 | r1 | r2 | r3) {
          const float4 sq = *reinterpret_cast<const float4*>(source + i);
          wq.x = r0 ? sq.x : wq.x; wq.y = r1 ? sq.y : wq.y; wq.z = r2 ? sq.z : wq.z; wq.w = r3 ? sq.w : wq.w;
          *reinterpret_cast<float4*>(w + i) = wq;
          count += (int)r0 + (int)r1 + (int)r2 + (int)r3;
        }
      }
    } else {
      const unsigned words[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        if (i + j < n) {
          const float wi = w[i + j];
          if (ema) teacher[i + j] = __fadd_rn(__fmul_rn(a, teacher[i + j]), __fmul_rn(b, wi));
          if (draw && cotta_draw(words[j], p)) { w[i + j] = source[i + j]; ++count; }
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = count;
  __syncthreads();
  if (threadIdx.x == 0) partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = (long long)sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(64) void cotta_finish_kernel(const long long* partial, int nblocks, long long* restored) {
  partial += (long long)blockIdx.x * nblocks;      // one workgroup per parameter set
  long long s = 0;
  for (int i = threadIdx.x; i < nblocks; i += 64) s += partial[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) restored[blockIdx.x] = s;
}

static long long cotta_blocks(int64_t n) {
  long long b = ((n + 3) / 4 + 255) / 256;
  if (b < 1) b = 1;
  if (b > COTTA_MAX_BLOCKS) b = COTTA_MAX_BLOCKS;
  return b;
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int64_t mmtta_consistency_partials(const mmtta_tensor* logits) {
  if (logits == nullptr || logits->n < 1) return -1;
  return (int64_t)loss_blocks(logits) * logits->n;
}

extern "C" int mmtta_consistency_loss_items(const mmtta_tensor* logits, const mmtta_tensor* target, int softmax,
                                            const mmtta_tensor* dlogits, double* partial, float* loss, void* stream) {
  MMTTA_CHECK(logits && target && dlogits && partial && loss && logits->ptr && target->ptr && dlogits->ptr, MMTTA_ERR_INVALID,
              "consistency loss: null argument");
  for (const mmtta_tensor* o : {target, dlogits})
    MMTTA_CHECK(logits->n == o->n && logits->c == o->c && logits->d == o->d && logits->h == o->h && logits->w == o->w,
                MMTTA_ERR_INVALID, "consistency loss: shape mismatch");
  MMTTA_CHECK(logits->n >= 1, MMTTA_ERR_INVALID, "consistency loss: empty batch");
  MMTTA_CHECK(logits->dtype == MMTTA_F32 && target->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED,
              "consistency loss: `logits` and `target` must be fp32-stored");
  MMTTA_CHECK(is_cl(logits) && is_cl(target) && is_cl(dlogits), MMTTA_ERR_UNSUPPORTED, "consistency loss: channels-last only");
  MMTTA_CHECK(loss_small_item(logits) && loss_small_item(target) && loss_small_item(dlogits), MMTTA_ERR_UNSUPPORTED,
              "consistency loss: an item of 2^31 elements or more");
  MMTTA_CHECK(logits->n <= LOSS_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "consistency loss: more than %d items in one call", LOSS_MAX_GRID_Y);
  ConsistencyLoss p;
  p.t = tv(target);
  return loss_launch<ConsistencyLoss, unsigned>({"consistency loss", "consistency loss", "consistency"}, logits, dlogits,
                                                softmax, loss_vec(logits, dlogits, target), 1, partial, loss, p,
                                                (hipStream_t)stream);
}

extern "C" int64_t mmtta_cotta_update_partials(int64_t n, int sets) {
  if (n < 0 || sets < 1) return -1;
  return (int64_t)cotta_blocks(n) * sets;
}

extern "C" int mmtta_cotta_update_sets(float* w, float* teacher, const float* source, int64_t n, int sets, int64_t w_stride,
                                       int64_t teacher_stride, double alpha, float restore_p, uint64_t seed,
                                       const int32_t* step, const int32_t* ordinals, int64_t* partial, int64_t* restored,
                                       void* stream) {
  MMTTA_CHECK(w && teacher && source && step && ordinals && partial && restored, MMTTA_ERR_INVALID, "cotta update: null argument");
  MMTTA_CHECK(n >= 0 && n <= (1ll << 34), MMTTA_ERR_INVALID, "cotta update: n = %lld (0 .. 2^34: the counter word is i >> 2)", (long long)n);
  MMTTA_CHECK(sets >= 1 && sets <= LOSS_MAX_GRID_Y, MMTTA_ERR_INVALID, "cotta update: sets = %d (1 .. %d)", sets, LOSS_MAX_GRID_Y);
  MMTTA_CHECK(w_stride % 4 == 0 && teacher_stride % 4 == 0 && (sets == 1 || (w_stride >= n && teacher_stride >= n)),
              MMTTA_ERR_INVALID, "cotta update: %d sets with strides %lld / %lld (n = %lld; multiples of 4, >= n)", sets,
              (long long)w_stride, (long long)teacher_stride, (long long)n);
  MMTTA_CHECK(alpha >= 0.0 && alpha <= 1.0, MMTTA_ERR_INVALID, "cotta update: alpha = %g (0 <= alpha <= 1)", alpha);
  MMTTA_CHECK(restore_p >= 0.f && restore_p < 1.f, MMTTA_ERR_INVALID, "cotta update: restore_p = %g (0 <= p < 1)", (double)restore_p);
  const bool al = ((uintptr_t)w | (uintptr_t)teacher | (uintptr_t)source) % 16 == 0;
  MMTTA_CHECK(al, MMTTA_ERR_UNSUPPORTED, "cotta update: buffers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int blocks = (int)cotta_blocks(n);
  const dim3 grid((unsigned)blocks, (unsigned)sets);
  hipLaunchKernelGGL(cotta_update_kernel, grid, dim3(256), 0, s, w, teacher, source, (long long)n, (long long)w_stride,
                     (long long)teacher_stride, (float)alpha, (float)(1.0 - alpha), restore_p, (unsigned)(seed & 0xffffffffu),
                     (unsigned)(seed >> 32), (const int*)step, (const int*)ordinals, (long long*)partial);
  int st = launch_status("cotta update");
  if (st) return st;
  hipLaunchKernelGGL(cotta_finish_kernel, dim3(sets), dim3(64), 0, s, (const long long*)partial, blocks, (long long*)restored);
  return launch_status("cotta finish");
}
