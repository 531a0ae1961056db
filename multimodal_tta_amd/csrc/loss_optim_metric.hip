// Entropy objective (+gradient), fused Adam over the flat parameter arena, and the
// sigmoid -> threshold -> Dice counting tail (gfx950).  All three are single-pass HBM-bound
// kernels; see include/mmtta.h for the reference lines each one stands in for.
#include "voxel_loss.h"

namespace mmtta {

// ------------------------------------------------------------------ entropy loss
// The plain walk of voxel_loss.h over the entropy arithmetic.  Its fast path ran at 100 - 120 % vector-ALU busy in libm's
// expf / log1pf / IEEE division with a double add per logit (profiles/r03d_sq_counters.md: 158 vector instructions per
// logit) - 203 us per group of 8 volumes at 128^3 against 85 us of HBM time, and vector issue is what the other lanes'
// kernels run short of.  Now per logit: v_exp_f32, v_rcp_f32, v_log_f32 and ~15 plain instructions
// (bernoulli_entropy_terms).  Against the libm form: loss within 1e-6 relative, gradient within 2e-6 of its maximum
// (tests/test_hip_pointwise.py::test_entropy_loss holds both to the torch reference at 2e-5).
struct EntropyLoss : NoOperand {
  __device__ __forceinline__ void fast(float z, float, float& h, float& g) const { bernoulli_entropy_terms(z, h, g); }
  __device__ __forceinline__ void generic(float z, float, float& h, float& g) const {
    const BernoulliLibm b = bernoulli_entropy_libm(z);
    h = b.h; g = b.g;
  }
  template <class F>
  __device__ __forceinline__ float categorical(const float* zp, const float*, int R, F&& put) const {
    CategoricalVoxel v;
    categorical_entropy<false>(zp, R, v);
#pragma unroll
    for (int r = 0; r < LOSS_MAX_R; ++r)
      if (r < R) put(r, categorical_entropy_grad<false>(v, r));
    return v.H;
  }
};

// ------------------------------------------------------------------ fused optimizers over the flat arena
// KIND 0: torch.optim.Adam (coupled L2), 1: torch.optim.AdamW (decoupled decay), 2: torch.optim.SGD (momentum, dampening,
// nesterov).  One thread owns 4 consecutive parameters (16-byte accesses; the arena keeps every parameter and both
// segment boundaries 16-byte aligned), the decay / no-decay split is the segment boundary n_decay
// (reference src/core/experiment_manager.py:199-237).
// OptimArgs / optim_update / optim_scalars: common.h

template <int KIND>
__global__ __launch_bounds__(256) void optim_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, long long n,
                                                    long long n_decay, OptimArgs a, const int* __restrict__ step,
                                                    long long set_stride) {
  __shared__ float s_step_size, s_bc2_sqrt;
  {  // replica blockIdx.y of the arena (a group of volumes, each with its own parameters and optimizer state)
    const long long o = (long long)blockIdx.y * set_stride;
    p += o; g += o; m += o;
    if (v != nullptr) v += o;
  }
  const int t0 = *step;
  if (threadIdx.x == 0) optim_scalars(KIND, a, t0, s_step_size, s_bc2_sqrt);
  __syncthreads();
  const float step_size = s_step_size, bc2_sqrt = s_bc2_sqrt;
  const bool first = t0 == 0;
  const bool wd_on = a.wd != 0.f;
  const long long n4 = n >> 2;
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < n4; q += (long long)gridDim.x * blockDim.x) {
    const long long i = q << 2;
    float4 pq = *reinterpret_cast<const float4*>(p + i);
    const float4 gq = *reinterpret_cast<const float4*>(g + i);
    // step 0 starts from zero moments whatever the buffers hold (torch creates them as zeros): the episodic reset need not
    // clear them, and the first step does not read them (8 of its 28 bytes per parameter)
    float4 mq = make_float4(0.f, 0.f, 0.f, 0.f), vq = mq;
    if (!first) {
      if (KIND != 2 || a.momentum != 0.f) mq = *reinterpret_cast<const float4*>(m + i);
      if (KIND != 2) vq = *reinterpret_cast<const float4*>(v + i);
    }
    const bool decay = wd_on && i < n_decay;          // n_decay is a multiple of 4
    optim_update<KIND>(pq.x, gq.x, mq.x, vq.x, decay, a, step_size, bc2_sqrt, first);
    optim_update<KIND>(pq.y, gq.y, mq.y, vq.y, decay, a, step_size, bc2_sqrt, first);
    optim_update<KIND>(pq.z, gq.z, mq.z, vq.z, decay, a, step_size, bc2_sqrt, first);
    optim_update<KIND>(pq.w, gq.w, mq.w, vq.w, decay, a, step_size, bc2_sqrt, first);
    *reinterpret_cast<float4*>(p + i) = pq;
    if (KIND != 2 || a.momentum != 0.f) *reinterpret_cast<float4*>(m + i) = mq;
    if (KIND != 2) *reinterpret_cast<float4*>(v + i) = vq;
  }
  // ragged tail (n not a multiple of 4: never the case for the arena, kept for arbitrary callers)
  const long long i = (n4 << 2) + blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i < n) {
    const bool has_m = KIND != 2 || a.momentum != 0.f;      // SGD without momentum keeps no buffer: `m` is neither read nor written
    float pi = p[i], mi = (has_m && !first) ? m[i] : 0.f, vi = (KIND != 2 && !first) ? v[i] : 0.f;
    optim_update<KIND>(pi, g[i], mi, vi, wd_on && i < n_decay, a, step_size, bc2_sqrt, first);
    p[i] = pi;
    if (has_m) m[i] = mi;
    if (KIND != 2) v[i] = vi;
  }
}

// optim_kernel over a table of segments of each replica (the parameters the fused weight updates of conv_wgrad.hip do not
// cover): seg[3 i .. 3 i + 2] = (start, length, decay), multiples of 4; a thread owns 4 consecutive parameters of the
// concatenation of the segments and finds its segment by binary search over their running starts (prefix[i]).
template <int KIND>
__global__ __launch_bounds__(256) void optim_segments_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                             float* __restrict__ m, float* __restrict__ v,
                                                             const long long* __restrict__ seg, const long long* __restrict__ prefix,
                                                             int count, long long total, OptimArgs a, const int* __restrict__ step,
                                                             long long set_stride) {
  __shared__ float s_step_size, s_bc2_sqrt;
  {
    const long long o = (long long)blockIdx.y * set_stride;
    p += o; g += o; m += o;
    if (v != nullptr) v += o;
  }
  const int t0 = *step;
  if (threadIdx.x == 0) optim_scalars(KIND, a, t0, s_step_size, s_bc2_sqrt);
  __syncthreads();
  const float step_size = s_step_size, bc2_sqrt = s_bc2_sqrt;
  const bool first = t0 == 0;
  const bool wd_on = a.wd != 0.f;
  const long long n4 = total >> 2;
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < n4; q += (long long)gridDim.x * blockDim.x) {
    const long long j = q << 2;
    int lo = 0, hi = count - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (prefix[mid] <= j) lo = mid; else hi = mid - 1;
    }
    const long long i = seg[3 * lo] + (j - prefix[lo]);
    float4 pq = *reinterpret_cast<const float4*>(p + i);
    const float4 gq = *reinterpret_cast<const float4*>(g + i);
    float4 mq = make_float4(0.f, 0.f, 0.f, 0.f), vq = mq;
    if (!first) {
      if (KIND != 2 || a.momentum != 0.f) mq = *reinterpret_cast<const float4*>(m + i);
      if (KIND != 2) vq = *reinterpret_cast<const float4*>(v + i);
    }
    const bool decay = wd_on && seg[3 * lo + 2] != 0;
    optim_update<KIND>(pq.x, gq.x, mq.x, vq.x, decay, a, step_size, bc2_sqrt, first);
    optim_update<KIND>(pq.y, gq.y, mq.y, vq.y, decay, a, step_size, bc2_sqrt, first);
    optim_update<KIND>(pq.z, gq.z, mq.z, vq.z, decay, a, step_size, bc2_sqrt, first);
    optim_update<KIND>(pq.w, gq.w, mq.w, vq.w, decay, a, step_size, bc2_sqrt, first);
    *reinterpret_cast<float4*>(p + i) = pq;
    if (KIND != 2 || a.momentum != 0.f) *reinterpret_cast<float4*>(m + i) = mq;
    if (KIND != 2) *reinterpret_cast<float4*>(v + i) = vq;
  }
}

__global__ void step_inc_kernel(int* step) { *step += 1; }

// ------------------------------------------------------------------ mask + Dice counts
__global__ __launch_bounds__(256) void dice_counts_kernel(TV z, TV lab, float thr, unsigned long long* counts,
                                                          unsigned char* mask, int blocks_per_n) {
  __shared__ unsigned int sh[3][256];
  const int R = z.c;
  int rp = 1;
  while (rp < R) rp <<= 1;        // R <= 256 enforced by the host
  const int nvl = 256 / rp;
  const int r = threadIdx.x % rp, vl = threadIdx.x / rp;
  const int n = blockIdx.x / blocks_per_n, bn = blockIdx.x % blocks_per_n;
  const long long dhw = (long long)z.d * z.h * z.w;
  unsigned int ci = 0, cp = 0, cg = 0;
  if (r < R) {
    for (long long v = (long long)bn * nvl + vl; v < dhw; v += (long long)blocks_per_n * nvl) {
      long long t = v;
      const int x = (int)(t % z.w); t /= z.w;
      const int y = (int)(t % z.h);
      const int zz = (int)(t / z.h);
      const float lg = z.p[n * z.sn + (long long)r * z.sc + zz * z.sd + y * z.sh + x * z.sw];
      const float prob = 1.f / (1.f + expf(-lg));
      const unsigned int pb = prob >= thr ? 1u : 0u;
      const float lv = lab.p[n * lab.sn + (long long)r * lab.sc + zz * lab.sd + y * lab.sh + x * lab.sw];
      const unsigned int gb = lv > 0.5f ? 1u : 0u;
      ci += pb & gb; cp += pb; cg += gb;
      if (mask) mask[((long long)n * R + r) * dhw + v] = (unsigned char)pb;
    }
  }
  sh[0][threadIdx.x] = ci; sh[1][threadIdx.x] = cp; sh[2][threadIdx.x] = cg;
  __syncthreads();
  if (vl == 0 && r < R) {
    unsigned long long ti = 0, tp = 0, tg = 0;
    for (int j = 0; j < nvl; ++j) { ti += sh[0][j * rp + r]; tp += sh[1][j * rp + r]; tg += sh[2][j * rp + r]; }
    unsigned long long* c = counts + ((long long)n * R + r) * 3;
    atomicAdd(c + 0, ti); atomicAdd(c + 1, tp); atomicAdd(c + 2, tg);
  }
}

// ------------------------------------------------------------------ DiceCE sums (evaluation report_loss)
// per (n,r): sum p*y, sum p (or p^2), sum y (or y^2), p = sigmoid(z); plus the CE numerator:
// R == 1: BCE-with-logits (pos_weight);  R > 1: soft-label softmax CE  -sum_r w_r y_r log_softmax(z)_r.
// Block partials [N][blocks_per_n][R*3 + 1] in the scratch buffer, summed in block order by dice_ce_finish_kernel:
// no atomics, the sums (and the gradient built from them) are bitwise reproducible.
constexpr int DCE_MAX_R = 8;
__global__ __launch_bounds__(256) void dice_ce_sums_kernel(TV z, TV lab, const float* weight, int squared, int softmax,
                                                           double* out, int blocks_per_n) {
  __shared__ double sh[4];
  const int R = z.c;
  const int n = blockIdx.x / blocks_per_n, bn = blockIdx.x % blocks_per_n;
  const long long dhw = (long long)z.d * z.h * z.w;
  double acc[DCE_MAX_R * 3 + 1];
#pragma unroll
  for (int i = 0; i < DCE_MAX_R * 3 + 1; ++i) acc[i] = 0.0;
  for (long long v = (long long)bn * 256 + threadIdx.x; v < dhw; v += (long long)blocks_per_n * 256) {
    long long t = v;
    const int x = (int)(t % z.w); t /= z.w;
    const int y = (int)(t % z.h);
    const int zz = (int)(t / z.h);
    float lg[DCE_MAX_R], yv[DCE_MAX_R];
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < DCE_MAX_R; ++r)
      if (r < R) {
        lg[r] = z.p[n * z.sn + (long long)r * z.sc + zz * z.sd + y * z.sh + x * z.sw];
        yv[r] = lab.p[n * lab.sn + (long long)r * lab.sc + zz * lab.sd + y * lab.sh + x * lab.sw];
        m = fmaxf(m, lg[r]);
      }
    float se = 0.f;
#pragma unroll
    for (int r = 0; r < DCE_MAX_R; ++r)
      if (r < R) se += expf(lg[r] - m);
    // lse rounds at ulp(m): fine for the CE term below (an absolute error of the size of z's own rounding), not for a
    // probability expf(z - lse), which would inherit it as a relative error (5e-4 at a saturated logit of 1e4)
    const float lse = m + logf(se);
#pragma unroll
    for (int r = 0; r < DCE_MAX_R; ++r)
      if (r < R) {
        const float e = expf(-fabsf(lg[r]));
        // Dice probability: sigmoid (multilabel heads) or softmax over the channels (softmax heads with more than one channel;
        // the form of dice_ce_grad_kernel)
        const float p = (softmax && R > 1) ? expf(lg[r] - m) / se : (lg[r] >= 0.f ? 1.f / (1.f + e) : e / (1.f + e));
        acc[r * 3 + 0] += (double)(p * yv[r]);
        acc[r * 3 + 1] += (double)(squared ? p * p : p);
        acc[r * 3 + 2] += (double)(squared ? yv[r] * yv[r] : yv[r]);
        if (R == 1) {
          const float pw = weight ? weight[0] : 1.f;
          const float softplus_neg = log1pf(e) + fmaxf(-lg[r], 0.f);
          acc[DCE_MAX_R * 3] += (double)((1.f - yv[r]) * lg[r] + (1.f + (pw - 1.f) * yv[r]) * softplus_neg);
        } else {
          const float wr = weight ? weight[r] : 1.f;
          acc[DCE_MAX_R * 3] += (double)(-wr * yv[r] * (lg[r] - lse));
        }
      }
  }
  for (int i = 0; i < DCE_MAX_R * 3 + 1; ++i) {
    const bool used = (i == DCE_MAX_R * 3) || (i / 3 < R);
    if (!used) continue;                       // uniform across the block
    const double t = block_sum_d(acc[i], sh);
    if (threadIdx.x == 0) {
      const int col = (i == DCE_MAX_R * 3) ? R * 3 : i;
      out[((long long)n * blocks_per_n + bn) * (R * 3 + 1) + col] = t;     // block partial: no atomics, fixed order later
    }
    __syncthreads();
  }
}

// out[n][col] = sum over the block partials of batch item n, in block order (deterministic)
__global__ __launch_bounds__(64) void dice_ce_finish_kernel(const double* part, int blocks_per_n, int cols, double* out) {
  const int n = blockIdx.x / cols, col = blockIdx.x % cols;
  double s = 0.0;
  for (int b = threadIdx.x; b < blocks_per_n; b += 64) s += part[((long long)n * blocks_per_n + b) * cols + col];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) out[(long long)n * cols + col] = s;
}

// Gradient of DiceCE (lambda_dice * Dice + lambda_ce * CE, reduction mean) with respect to the logits, from the
// per-(n,r) sums of dice_ce_sums_kernel (monai DiceCELoss as built at reference
// src/core/trainers/seg_trainer.py:59-79).  One thread per voxel, all R channels.
struct DceGradArgs {
  TV z, lab, dz;
  const float* weight;
  const double* sums;       // [N][R*3+1]
  int squared, jaccard, include_background, softmax;
  float lambda_dice, lambda_ce, smooth_nr, smooth_dr;
};

__global__ __launch_bounds__(256) void dice_ce_grad_kernel(DceGradArgs a) {
  const int R = a.z.c;
  const long long dhw = (long long)a.z.d * a.z.h * a.z.w;
  const long long total = (long long)a.z.n * dhw;
  const int r0 = (!a.include_background && R > 1) ? 1 : 0;
  const int Rd = R - r0;                                  // channels in the Dice mean
  const float dice_scale = a.lambda_dice / (float)((long long)a.z.n * Rd);
  const float ce_scale = a.lambda_ce / (float)((long long)a.z.n * dhw * (R == 1 ? 1 : 1));
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int n = (int)(i / dhw);
    long long t = i - (long long)n * dhw;
    const int x = (int)(t % a.z.w); t /= a.z.w;
    const int y = (int)(t % a.z.h);
    const int zz = (int)(t / a.z.h);
    float lg[DCE_MAX_R], yv[DCE_MAX_R], g[DCE_MAX_R];
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < DCE_MAX_R; ++r)
      if (r < R) {
        lg[r] = a.z.p[n * a.z.sn + (long long)r * a.z.sc + zz * a.z.sd + y * a.z.sh + x * a.z.sw];
        yv[r] = a.lab.p[n * a.lab.sn + (long long)r * a.lab.sc + zz * a.lab.sd + y * a.lab.sh + x * a.lab.sw];
        m = fmaxf(m, lg[r]);
      }
    float se = 0.f, S = 0.f;
#pragma unroll
    for (int r = 0; r < DCE_MAX_R; ++r)
      if (r < R) { se += expf(lg[r] - m); S += (a.weight ? a.weight[r] : 1.f) * yv[r]; }
    const bool smx = a.softmax && R > 1;
    // softmax heads: dDice/dz_k = p_k (dLdp_k - sum_r dLdp_r p_r) (the softmax Jacobian); first pass: dLdp_r and their p-weighted sum
    float dldp[DCE_MAX_R], dot = 0.f;
#pragma unroll
    for (int r = 0; r < DCE_MAX_R; ++r) dldp[r] = 0.f;
#pragma unroll
    for (int r = 0; r < DCE_MAX_R; ++r)
      if (r < R) {
        const float e = expf(-fabsf(lg[r]));
        const float p = smx ? expf(lg[r] - m) / se : (lg[r] >= 0.f ? 1.f / (1.f + e) : e / (1.f + e));
        float gd = 0.f;
        if (r >= r0) {
          const double* sm = a.sums + (long long)n * (R * 3 + 1) + r * 3;
          const float I = (float)sm[0], Q = (float)sm[1], G = (float)sm[2];
          const float A = 2.f * I + a.smooth_nr;
          float den = G + Q;
          float dden = a.squared ? 2.f * p : 1.f;            // d(sum p or p^2)/dp
          if (a.jaccard) { den = 2.f * (den - I); dden = 2.f * (dden - yv[r]); }
          const float Dn = den + a.smooth_dr;
          const float dfdp = -(2.f * yv[r] * Dn - A * dden) / (Dn * Dn);
          // class weights scale the Dice terms only when there is more than one Dice channel (monai)
          const float cw = (a.weight != nullptr && Rd != 1) ? a.weight[r] : 1.f;
          gd = dice_scale * cw * dfdp * (smx ? 1.f : p * (1.f - p));
        }
        if (smx) { dldp[r] = gd; dot += gd * p; continue; }
        float gc;
        if (R == 1) {
          const float pw = a.weight ? a.weight[0] : 1.f;
          gc = -pw * yv[r] * (1.f - p) + (1.f - yv[r]) * p;
        } else {
          const float sp = expf(lg[r] - m) / se;
          gc = sp * S - (a.weight ? a.weight[r] : 1.f) * yv[r];
        }
        g[r] = gd + ce_scale * gc;
        a.dz.p[n * a.dz.sn + (long long)r * a.dz.sc + zz * a.dz.sd + y * a.dz.sh + x * a.dz.sw] = g[r];
      }
    if (smx) {
#pragma unroll
      for (int r = 0; r < DCE_MAX_R; ++r)
        if (r < R) {
          const float sp = expf(lg[r] - m) / se;
          const float gc = sp * S - (a.weight ? a.weight[r] : 1.f) * yv[r];
          g[r] = sp * (dldp[r] - dot) + ce_scale * gc;
          a.dz.p[n * a.dz.sn + (long long)r * a.dz.sc + zz * a.dz.sd + y * a.dz.sh + x * a.dz.sw] = g[r];
        }
    }
  }
}

// ------------------------------------------------------------------ filtered entropy (SAR's reliable-entropy loss)
// The filtered walk of voxel_loss.h over the entropy arithmetic above: keep = H < margin, ANDed with an incoming mask.  With
// every element kept the block partials, the loss arithmetic and the gradient scale are those of mmtta_entropy_loss_items.
struct FilteredEntropy : NoOperand {
  static constexpr int ROWS = 2;
  float margin;
  const unsigned char* kin;      // the incoming mask in the layout of the outgoing one, or null
  __device__ __forceinline__ void item(int n, long long elems) { if (kin) kin += n * elems; }
  __device__ __forceinline__ bool allowed(long long i) const { return kin == nullptr || kin[i] != 0; }
  __device__ __forceinline__ KeptTerms fast(float z, float) const {
    KeptTerms e;
    bernoulli_entropy_terms(z, e.h, e.g);
    e.v = e.h; e.pass = true;
    return e;
  }
  __device__ __forceinline__ KeptTerms generic(float z, float) const {
    const BernoulliLibm b = bernoulli_entropy_libm(z);
    return {b.h, b.h, b.g, true};
  }
  template <class F>
  __device__ __forceinline__ KeptTerms categorical(const float* zp, const float*, int R, F&& put) const {
    CategoricalVoxel v;
    categorical_entropy<false>(zp, R, v);
#pragma unroll
    for (int r = 0; r < LOSS_MAX_R; ++r)
      if (r < R) put(r, categorical_entropy_grad<false>(v, r));
    return {v.H, v.H, 0.f, true};
  }
};

// ------------------------------------------------------------------ SAM ascent over arena replicas
// eps = rho * g / (||g||_2 + 1e-12) over [0, n) of each of the first `sets` replicas; w_saved = w, w += eps.  Stage 1: fp64
// block partials of g^2 per replica [set][SAM_BLOCKS]; stage 2: every workgroup sums its replica's partials in the same
// fixed order (deterministic, identical in every workgroup), then rewrites its slice.  The scale and the update are fp32 with
// separate roundings, as torch's p.add_(p.grad * scale) computes them.
constexpr int SAM_BLOCKS = 256;

__global__ __launch_bounds__(256) void sam_sumsq_kernel(const float* __restrict__ g, long long n, long long stride,
                                                        double* partial) {
  __shared__ double sh[4];
  g += (long long)blockIdx.y * stride;
  const long long n4 = n >> 2;
  double acc = 0.0;
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < n4; q += (long long)gridDim.x * blockDim.x) {
    const float4 v = *reinterpret_cast<const float4*>(g + (q << 2));
    acc += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
  }
  const double t = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void sam_ascent_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ saved, long long n, long long stride,
                                                         long long saved_stride, const double* partial, int nblocks,
                                                         float rho) {
  __shared__ float s_scale;
  const long long o = (long long)blockIdx.y * stride;
  p += o; g += o; saved += (long long)blockIdx.y * saved_stride;
  if (threadIdx.x < 64) {
    const double* pp = partial + (long long)blockIdx.y * nblocks;
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 64) s += pp[i];
    s = wave_sum_d(s);
    if (threadIdx.x == 0) s_scale = rho / ((float)sqrt(s) + 1e-12f);
  }
  __syncthreads();
  const float scale = s_scale;
  const long long n4 = n >> 2;
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < n4; q += (long long)gridDim.x * blockDim.x) {
    const long long i = q << 2;
    const float4 w = *reinterpret_cast<const float4*>(p + i);
    const float4 gq = *reinterpret_cast<const float4*>(g + i);
    *reinterpret_cast<float4*>(saved + i) = w;
    *reinterpret_cast<float4*>(p + i) = make_float4(__fadd_rn(w.x, __fmul_rn(gq.x, scale)), __fadd_rn(w.y, __fmul_rn(gq.y, scale)),
                                                    __fadd_rn(w.z, __fmul_rn(gq.z, scale)), __fadd_rn(w.w, __fmul_rn(gq.w, scale)));
  }
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int64_t mmtta_entropy_partials(const mmtta_tensor* logits) {
  if (logits == nullptr) return -1;
  return loss_blocks(logits, logits->n);
}

static int entropy_launch(const mmtta_tensor* logits, int softmax, const mmtta_tensor* dlogits, double* partial, float* loss,
                          int per_item, void* stream) {
  MMTTA_CHECK(logits == nullptr || logits->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "mmtta_entropy_loss: `logits` must be fp32-stored");
  MMTTA_CHECK(logits && dlogits && partial && loss && logits->ptr && dlogits->ptr, MMTTA_ERR_INVALID, "entropy: null argument");
  MMTTA_CHECK(logits->n == dlogits->n && logits->c == dlogits->c && logits->d == dlogits->d && logits->h == dlogits->h &&
                  logits->w == dlogits->w, MMTTA_ERR_INVALID, "entropy: shape mismatch");
  MMTTA_CHECK(is_cl(logits) && is_cl(dlogits), MMTTA_ERR_UNSUPPORTED, "entropy: channels-last only");
  return loss_launch<EntropyLoss, long long>({"mmtta_entropy_loss", "entropy", "entropy"}, logits, dlogits, softmax,
                                             loss_vec(logits, dlogits), per_item, partial, loss, EntropyLoss{},
                                             (hipStream_t)stream);
}

extern "C" int mmtta_entropy_loss(const mmtta_tensor* logits, int softmax, const mmtta_tensor* dlogits, double* partial,
                                  float* loss, void* stream) {
  return entropy_launch(logits, softmax, dlogits, partial, loss, 0, stream);
}

extern "C" int64_t mmtta_entropy_partials_items(const mmtta_tensor* logits) {
  if (logits == nullptr) return -1;
  return (int64_t)loss_blocks(logits) * logits->n;
}

extern "C" int mmtta_entropy_loss_items(const mmtta_tensor* logits, int softmax, const mmtta_tensor* dlogits, double* partial,
                                        float* loss, void* stream) {
  return entropy_launch(logits, softmax, dlogits, partial, loss, 1, stream);
}

static int optim_launch(int kind, float* p, const float* g, float* m, float* v, int64_t n, int64_t n_decay, const OptimArgs& a,
                        int32_t* step, hipStream_t s, int sets = 1, int64_t set_stride = 0) {
  MMTTA_CHECK(sets >= 1 && set_stride >= 0 && set_stride % 4 == 0 && (sets == 1 || set_stride >= n), MMTTA_ERR_INVALID,
              "optimizer: %d sets with stride %lld (n = %lld)", sets, (long long)set_stride, (long long)n);
  MMTTA_CHECK(p && g && m && step && n >= 0 && n_decay >= 0 && n_decay <= n, MMTTA_ERR_INVALID, "optimizer: bad argument");
  MMTTA_CHECK(kind == MMTTA_OPTIM_SGD || v != nullptr, MMTTA_ERR_INVALID, "optimizer: Adam/AdamW need the second-moment buffer");
  MMTTA_CHECK(kind >= MMTTA_OPTIM_ADAM && kind <= MMTTA_OPTIM_SGD, MMTTA_ERR_INVALID, "optimizer: kind %d", kind);
  if (n == 0) return MMTTA_OK;
  const bool al = ((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16 == 0 && n_decay % 4 == 0;
  MMTTA_CHECK(al, MMTTA_ERR_UNSUPPORTED, "optimizer: buffers must be 16-byte aligned and n_decay a multiple of 4");
  long long blocks = ((n + 3) / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  const dim3 grid((unsigned)blocks, (unsigned)sets), blk(256);
  const long long ss = (long long)set_stride;
  if (kind == MMTTA_OPTIM_ADAM)
    hipLaunchKernelGGL(optim_kernel<0>, grid, blk, 0, s, p, g, m, v, (long long)n, (long long)n_decay, a, step, ss);
  else if (kind == MMTTA_OPTIM_ADAMW)
    hipLaunchKernelGGL(optim_kernel<1>, grid, blk, 0, s, p, g, m, v, (long long)n, (long long)n_decay, a, step, ss);
  else
    hipLaunchKernelGGL(optim_kernel<2>, grid, blk, 0, s, p, g, m, v, (long long)n, (long long)n_decay, a, step, ss);
  int st = launch_status("optimizer");
  if (st) return st;
  hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, s, step);
  return launch_status("optimizer step counter");
}

extern "C" int mmtta_adam_step(float* p, const float* g, float* m, float* v, int64_t n, int64_t n_decay, float lr,
                               float beta1, float beta2, float eps, float weight_decay, int32_t* step, void* stream) {
  OptimArgs a{lr, beta1, beta2, eps, weight_decay, 0.f, 0.f, 0};
  return optim_launch(MMTTA_OPTIM_ADAM, p, g, m, v, n, n_decay, a, step, (hipStream_t)stream);
}

extern "C" int mmtta_optim_step(const mmtta_optim_desc* d, float* p, const float* g, float* m, float* v, int64_t n,
                                int64_t n_decay, int32_t* step, void* stream) {
  MMTTA_CHECK(d != nullptr, MMTTA_ERR_INVALID, "optimizer: null desc");
  OptimArgs a{d->lr, d->beta1, d->beta2, d->eps, d->weight_decay, d->momentum, d->dampening, d->nesterov};
  if (d->kind == MMTTA_OPTIM_SGD)
    MMTTA_CHECK(!(d->nesterov && (d->momentum <= 0.f || d->dampening != 0.f)), MMTTA_ERR_INVALID,
                "optimizer: nesterov needs momentum > 0 and zero dampening (torch.optim.SGD raises the same)");
  return optim_launch(d->kind, p, g, m, v, n, n_decay, a, step, (hipStream_t)stream);
}

extern "C" int mmtta_optim_step_sets(const mmtta_optim_desc* d, float* p, const float* g, float* m, float* v, int64_t n,
                                     int64_t n_decay, int sets, int64_t set_stride, int32_t* step, void* stream) {
  MMTTA_CHECK(d != nullptr, MMTTA_ERR_INVALID, "optimizer: null desc");
  OptimArgs a{d->lr, d->beta1, d->beta2, d->eps, d->weight_decay, d->momentum, d->dampening, d->nesterov};
  if (d->kind == MMTTA_OPTIM_SGD)
    MMTTA_CHECK(!(d->nesterov && (d->momentum <= 0.f || d->dampening != 0.f)), MMTTA_ERR_INVALID,
                "optimizer: nesterov needs momentum > 0 and zero dampening (torch.optim.SGD raises the same)");
  return optim_launch(d->kind, p, g, m, v, n, n_decay, a, step, (hipStream_t)stream, sets, set_stride);
}

extern "C" int mmtta_optim_step_segments(const mmtta_optim_desc* d, float* p, const float* g, float* m, float* v,
                                         const int64_t* segments, int count, int64_t total, int sets, int64_t set_stride,
                                         int32_t* step, void* stream) {
  MMTTA_CHECK(d != nullptr, MMTTA_ERR_INVALID, "optimizer: null desc");
  OptimArgs a{d->lr, d->beta1, d->beta2, d->eps, d->weight_decay, d->momentum, d->dampening, d->nesterov};
  const int kind = d->kind;
  if (kind == MMTTA_OPTIM_SGD)
    MMTTA_CHECK(!(d->nesterov && (d->momentum <= 0.f || d->dampening != 0.f)), MMTTA_ERR_INVALID,
                "optimizer: nesterov needs momentum > 0 and zero dampening (torch.optim.SGD raises the same)");
  MMTTA_CHECK(kind >= MMTTA_OPTIM_ADAM && kind <= MMTTA_OPTIM_SGD, MMTTA_ERR_INVALID, "optimizer: kind %d", kind);
  MMTTA_CHECK(p && g && m && step && (kind == MMTTA_OPTIM_SGD || v != nullptr), MMTTA_ERR_INVALID, "optimizer: bad argument");
  MMTTA_CHECK(sets >= 1 && set_stride >= 0 && set_stride % 4 == 0 && total >= 0 && total % 4 == 0 && count >= 0,
              MMTTA_ERR_INVALID, "optimizer segments: %d sets, stride %lld, %lld elements", sets, (long long)set_stride,
              (long long)total);
  const bool al = ((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16 == 0;
  MMTTA_CHECK(al, MMTTA_ERR_UNSUPPORTED, "optimizer: buffers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (total > 0) {
    MMTTA_CHECK(segments != nullptr && count > 0, MMTTA_ERR_INVALID, "optimizer segments: no table");
    // the table is [count][3] followed by the [count] running starts (mmtta.h: the caller builds both)
    const long long* seg = (const long long*)segments;
    const long long* prefix = seg + 3 * (long long)count;
    long long blocks = (total / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    const dim3 grid((unsigned)blocks, (unsigned)sets), blk(256);
    const long long ss = (long long)set_stride;
    if (kind == MMTTA_OPTIM_ADAM)
      hipLaunchKernelGGL(optim_segments_kernel<0>, grid, blk, 0, s, p, g, m, v, seg, prefix, count, (long long)total, a, step, ss);
    else if (kind == MMTTA_OPTIM_ADAMW)
      hipLaunchKernelGGL(optim_segments_kernel<1>, grid, blk, 0, s, p, g, m, v, seg, prefix, count, (long long)total, a, step, ss);
    else
      hipLaunchKernelGGL(optim_segments_kernel<2>, grid, blk, 0, s, p, g, m, v, seg, prefix, count, (long long)total, a, step, ss);
    int st = launch_status("optimizer segments");
    if (st) return st;
  }
  hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, s, step);
  return launch_status("optimizer step counter");
}

extern "C" int mmtta_mask_dice_counts(const mmtta_tensor* logits, const mmtta_tensor* label, float threshold, int64_t* counts,
                                      uint8_t* mask, void* stream) {
  MMTTA_CHECK(logits == nullptr || logits->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "mmtta_mask_dice_counts: `logits` must be fp32-stored");
  MMTTA_CHECK(label == nullptr || label->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "mmtta_mask_dice_counts: `label` must be fp32-stored");
  MMTTA_CHECK(logits && label && counts && logits->ptr && label->ptr, MMTTA_ERR_INVALID, "dice: null argument");
  MMTTA_CHECK(logits->n == label->n && logits->c == label->c && logits->d == label->d && logits->h == label->h &&
                  logits->w == label->w, MMTTA_ERR_INVALID, "dice: logits/label shape mismatch");
  MMTTA_CHECK(logits->c <= 256, MMTTA_ERR_UNSUPPORTED, "dice: more than 256 regions");
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)logits->n * logits->c * 3 * sizeof(int64_t), s);
  MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "dice: memset failed: %s", hipGetErrorString(e));
  const long long dhw = (long long)logits->d * logits->h * logits->w;
  int rp = 1;
  while (rp < logits->c) rp <<= 1;
  const int nvl = 256 / rp;
  long long bpn = (dhw + (long long)nvl * 16 - 1) / ((long long)nvl * 16);
  if (bpn < 1) bpn = 1;
  if (bpn > 1024) bpn = 1024;
  hipLaunchKernelGGL(dice_counts_kernel, dim3((unsigned)(bpn * logits->n)), dim3(256), 0, s, tv(logits), tv(label), threshold,
                     (unsigned long long*)counts, mask, (int)bpn);
  return launch_status("dice counts");
}

static long long dice_ce_blocks_per_n(const mmtta_tensor* logits) {
  const long long dhw = (long long)logits->d * logits->h * logits->w;
  long long bpn = (dhw + 256 * 4 - 1) / (256 * 4);
  if (bpn < 1) bpn = 1;
  if (bpn > 1024) bpn = 1024;
  return bpn;
}

extern "C" int64_t mmtta_dice_ce_scratch_bytes(const mmtta_tensor* logits) {
  if (logits == nullptr || logits->c < 1 || logits->c > DCE_MAX_R) return -1;
  return (int64_t)logits->n * dice_ce_blocks_per_n(logits) * (logits->c * 3 + 1) * (int64_t)sizeof(double);
}

extern "C" int mmtta_dice_ce_sums(const mmtta_tensor* logits, const mmtta_tensor* label, const float* weight,
                                  int squared_pred, int softmax, double* out, void* scratch, void* stream) {
  MMTTA_CHECK(logits == nullptr || logits->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "mmtta_dice_ce_sums: `logits` must be fp32-stored");
  MMTTA_CHECK(label == nullptr || label->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "mmtta_dice_ce_sums: `label` must be fp32-stored");
  MMTTA_CHECK(logits && label && out && scratch && logits->ptr && label->ptr, MMTTA_ERR_INVALID, "dice_ce: null argument");
  MMTTA_CHECK(logits->n == label->n && logits->c == label->c && logits->d == label->d && logits->h == label->h &&
                  logits->w == label->w, MMTTA_ERR_INVALID, "dice_ce: logits/label shape mismatch");
  MMTTA_CHECK(logits->c <= DCE_MAX_R, MMTTA_ERR_UNSUPPORTED, "dice_ce: more than %d regions", DCE_MAX_R);
  hipStream_t s = (hipStream_t)stream;
  const long long bpn = dice_ce_blocks_per_n(logits);
  const int cols = logits->c * 3 + 1;
  hipLaunchKernelGGL(dice_ce_sums_kernel, dim3((unsigned)(bpn * logits->n)), dim3(256), 0, s, tv(logits), tv(label), weight,
                     squared_pred, softmax, (double*)scratch, (int)bpn);
  int st = launch_status("dice_ce sums");
  if (st) return st;
  hipLaunchKernelGGL(dice_ce_finish_kernel, dim3(logits->n * cols), dim3(64), 0, s, (const double*)scratch, (int)bpn, cols, out);
  return launch_status("dice_ce finish");
}

extern "C" int mmtta_dice_ce_grad(const mmtta_tensor* logits, const mmtta_tensor* label, const float* weight, int squared_pred,
                                  int softmax, int jaccard, int include_background, float lambda_dice, float lambda_ce, float smooth_nr,
                                  float smooth_dr, const double* sums, const mmtta_tensor* dlogits, void* stream) {
  MMTTA_CHECK(logits == nullptr || logits->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "mmtta_dice_ce_grad: `logits` must be fp32-stored");
  MMTTA_CHECK(label == nullptr || label->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "mmtta_dice_ce_grad: `label` must be fp32-stored");
  MMTTA_CHECK(dlogits == nullptr || dlogits->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "mmtta_dice_ce_grad: `dlogits` must be fp32-stored");
  MMTTA_CHECK(logits && label && dlogits && sums && logits->ptr && label->ptr && dlogits->ptr, MMTTA_ERR_INVALID,
              "dice_ce grad: null argument");
  MMTTA_CHECK(logits->n == label->n && logits->c == label->c && logits->d == label->d && logits->h == label->h &&
                  logits->w == label->w && logits->n == dlogits->n && logits->c == dlogits->c && logits->d == dlogits->d &&
                  logits->h == dlogits->h && logits->w == dlogits->w, MMTTA_ERR_INVALID, "dice_ce grad: shape mismatch");
  MMTTA_CHECK(logits->c <= DCE_MAX_R, MMTTA_ERR_UNSUPPORTED, "dice_ce grad: more than %d regions", DCE_MAX_R);
  DceGradArgs a;
  a.z = tv(logits); a.lab = tv(label); a.dz = tv(dlogits); a.weight = weight; a.sums = sums;
  a.squared = squared_pred; a.jaccard = jaccard; a.include_background = include_background; a.softmax = softmax;
  a.lambda_dice = lambda_dice; a.lambda_ce = lambda_ce; a.smooth_nr = smooth_nr; a.smooth_dr = smooth_dr;
  const long long total = (long long)logits->n * logits->d * logits->h * logits->w;
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(dice_ce_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status("dice_ce grad");
}

extern "C" int64_t mmtta_entropy_filtered_partials(const mmtta_tensor* logits) {
  if (logits == nullptr) return -1;
  return 2 * (int64_t)loss_blocks(logits) * logits->n;
}

extern "C" int mmtta_entropy_filtered_items(const mmtta_tensor* logits, int softmax, float margin, const uint8_t* keep_in,
                                            uint8_t* keep_out, const mmtta_tensor* dlogits, double* partial, float* loss,
                                            int64_t* kept, void* stream) {
  MMTTA_CHECK(__builtin_isfinite(margin) && margin > 0.f, MMTTA_ERR_INVALID,
              "entropy filtered: margin must be finite and positive, got %g", (double)margin);
  MMTTA_CHECK(keep_out != nullptr, MMTTA_ERR_INVALID, "entropy filtered: null mask output");
  MMTTA_CHECK(logits && dlogits && partial && loss && kept && logits->ptr && dlogits->ptr, MMTTA_ERR_INVALID,
              "entropy filtered: null argument");
  MMTTA_CHECK(logits->n == dlogits->n && logits->c == dlogits->c && logits->d == dlogits->d && logits->h == dlogits->h &&
                  logits->w == dlogits->w && logits->n >= 1 && logits->c >= 1,
              MMTTA_ERR_INVALID, "entropy filtered: shape mismatch");
  MMTTA_CHECK(logits->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "entropy filtered: `logits` must be fp32-stored");
  MMTTA_CHECK(is_cl(logits) && is_cl(dlogits), MMTTA_ERR_UNSUPPORTED, "entropy filtered: channels-last only");
  return kept_launch<FilteredEntropy, long long>({"entropy filtered", "entropy filtered", "entropy filtered"}, logits, dlogits,
                                                 softmax, loss_vec(logits, dlogits), keep_out, partial, loss, (long long*)kept,
                                                 nullptr, FilteredEntropy{{}, margin, keep_in}, (hipStream_t)stream);
}

static long long sam_blocks(int64_t n) {
  long long b = ((n + 3) / 4 + 255) / 256;
  if (b < 1) b = 1;
  if (b > SAM_BLOCKS) b = SAM_BLOCKS;
  return b;
}

extern "C" int64_t mmtta_sam_ascent_partials(int64_t n, int sets) {
  if (n < 0 || sets < 1) return -1;
  return sam_blocks(n) * sets;
}

extern "C" int mmtta_sam_ascent_sets(float* p, const float* g, float* saved, int64_t saved_stride, double* partial, int64_t n,
                                     int sets, int replicas, int64_t set_stride, float rho, void* stream) {
  MMTTA_CHECK(__builtin_isfinite(rho) && rho >= 0.f, MMTTA_ERR_INVALID, "sam ascent: rho must be finite and >= 0, got %g",
              (double)rho);
  MMTTA_CHECK(p && g && saved && partial, MMTTA_ERR_INVALID, "sam ascent: null argument");
  MMTTA_CHECK(n >= 0 && n % 4 == 0 && set_stride >= 0 && set_stride % 4 == 0, MMTTA_ERR_INVALID,
              "sam ascent: n = %lld and set_stride = %lld must be multiples of 4", (long long)n, (long long)set_stride);
  MMTTA_CHECK(saved_stride >= n && saved_stride % 4 == 0, MMTTA_ERR_INVALID,
              "sam ascent: saved_stride = %lld must be a multiple of 4 and at least n = %lld", (long long)saved_stride,
              (long long)n);
  MMTTA_CHECK(sets >= 1 && sets <= replicas && n <= set_stride, MMTTA_ERR_INVALID,
              "sam ascent: %d sets of %lld elements do not fit %d replicas of stride %lld", sets, (long long)n, replicas,
              (long long)set_stride);
  MMTTA_CHECK(((uintptr_t)p | (uintptr_t)g | (uintptr_t)saved) % 16 == 0, MMTTA_ERR_INVALID,
              "sam ascent: buffers must be 16-byte aligned");
  if (n == 0) return MMTTA_OK;
  hipStream_t s = (hipStream_t)stream;
  const long long nb = sam_blocks(n);
  hipLaunchKernelGGL(sam_sumsq_kernel, dim3((unsigned)nb, (unsigned)sets), dim3(256), 0, s, g, (long long)n, (long long)set_stride,
                     partial);
  int st = launch_status("sam sum of squares");
  if (st) return st;
  long long ub = ((n + 3) / 4 + 255) / 256;
  if (ub > 4096) ub = 4096;
  hipLaunchKernelGGL(sam_ascent_kernel, dim3((unsigned)ub, (unsigned)sets), dim3(256), 0, s, p, g, saved, (long long)n,
                     (long long)set_stride, (long long)saved_stride, (const double*)partial, (int)nb, rho);
  return launch_status("sam ascent");
}
