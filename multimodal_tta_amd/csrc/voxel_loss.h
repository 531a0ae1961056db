// The per-voxel adaptation losses (entropy, filtered / weighted entropy, pseudo-label, consistency, DeYO; MEMO for the
// helpers): one copy of what their kernels share - the host-side geometry and predicates, the per-logit primitives, the
// grid-stride voxel walks with their block partials, the finish kernels and the launch ladders.  An objective supplies a
// small policy struct with its per-element arithmetic (and its second operand, if it has one); everything a policy or a
// primitive supplies is __forceinline__, so an instantiation compiles to the kernel one would write by hand.
#pragma once
#include "common.h"

namespace mmtta {

// ------------------------------------------------------------------ host: launch geometry and operand predicates
constexpr int LOSS_MAX_BLOCKS = 2048;      // block partials per item
constexpr int LOSS_MAX_R = 16;             // classes of the categorical paths
constexpr int LOSS_MAX_GRID_Y = 65535;     // gridDim.y carries the item

// Workgroups of one objective over `items` batch items of t's extents (1: the per-item entry points).  The figure counts
// (voxel, region) pairs for every head: the kernels that give a thread a whole voxel get up to c times the workgroups they
// have voxels for below the cap, and those write a zero partial.
inline int loss_blocks(const mmtta_tensor* t, long long items = 1) {
  const long long total = items * t->d * t->h * t->w * t->c;
  long long b = (total + 255) / 256;
  if (b < 1) b = 1;
  if (b > LOSS_MAX_BLOCKS) b = LOSS_MAX_BLOCKS;
  return (int)b;
}
// dense voxel order in 16-byte fp32 rows (or 8-byte bf16 rows) of 4 lanes
inline bool loss_dense16(const mmtta_tensor* t) {
  return t->sc == 1 && t->sw == 4 && t->sh == (int64_t)t->w * 4 && t->sd == (int64_t)t->h * t->sh && t->sn % 4 == 0 &&
         ((uintptr_t)t->ptr) % 16 == 0;
}
// 4-element voxel rows with nothing between them, fp32 or bf16: what a kernel addresses with one 32-bit voxel index
inline bool loss_dense4(const mmtta_tensor* t) {
  const int esz = t->dtype == MMTTA_BF16 ? 2 : 4;
  return t->sc == 1 && t->sw == 4 && t->sh == (int64_t)t->w * 4 && t->sd == (int64_t)t->h * t->sh && t->sn % 4 == 0 &&
         ((uintptr_t)t->ptr) % (4 * esz) == 0;
}
// the byte spans of two views meet
inline bool loss_overlap(const mmtta_tensor* a, const mmtta_tensor* b) {
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
// every offset inside one item fits 31 bits (the kernels that index voxels with 32-bit arithmetic)
inline bool loss_small_item(const mmtta_tensor* t) {
  const long long ld = t->sw > t->c ? t->sw : t->c;
  return t->d > 0 && t->h > 0 && t->w > 0 && t->c > 0 && (long long)t->d * t->h * t->w * (ld > 4 ? ld : 4) < (1ll << 31);
}
// The fast path applies: <= 4 regions, the logits, the gradient and a second operand (if any) in dense 16-byte voxel rows,
// and a gradient that owns its pad lane (a whole row is stored).
inline bool loss_vec(const mmtta_tensor* z, const mmtta_tensor* dz, const mmtta_tensor* other = nullptr) {
  return z->c <= 4 && loss_dense16(z) && (other == nullptr || loss_dense16(other)) && loss_dense16(dz) &&
         ((dz->flags & MMTTA_TENSOR_OWNS_PAD) || dz->c == 4);
}

// ------------------------------------------------------------------ device: block sums
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
  v = wave_sum_d(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sh[w];
  return t;  // valid on thread 0
}

// Pass 1 of a filtered objective: fp64 block partials partial[item][row][block] of the kept sum, of the kept count and
// (ROWS == 3) of the count that passed the entropy margin alone.
template <int ROWS>
__device__ __forceinline__ void fent_store_partials(double acc, int cnt, int cnt1, double* partial, double* sh) {
  const double s = block_sum_d(acc, sh);
  __syncthreads();
  const double c = block_sum_d((double)cnt, sh);
  double c1 = 0.0;
  if (ROWS == 3) {
    __syncthreads();
    c1 = block_sum_d((double)cnt1, sh);
  }
  if (threadIdx.x == 0) {
    double* p = partial + (long long)blockIdx.y * ROWS * gridDim.x;
    p[blockIdx.x] = s;
    p[gridDim.x + blockIdx.x] = c;
    if (ROWS == 3) p[2 * gridDim.x + blockIdx.x] = c1;
  }
}

__device__ __forceinline__ float fent_scale(const long long* kept) {
  const long long k = kept[blockIdx.y];
  return k > 0 ? (float)(1.0 / (double)k) : 0.f;
}

// ------------------------------------------------------------------ device: per-logit primitives
// The fast path per logit: v_exp_f32, v_rcp_f32, v_log_f32 and plain instructions.
__device__ __forceinline__ float exp_neg_abs(float t) { return __builtin_amdgcn_exp2f(-fabsf(t) * 1.4426950408889634f); }
__device__ __forceinline__ float exp_fast(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

// sigmoid(t) = p and sigmoid(-t) = q from e = exp(-|t|), neither formed by subtraction; r = sigmoid(|t|), er = 1 - r
struct SigmoidPair {
  float p, q, r, er;
};
__device__ __forceinline__ SigmoidPair sigmoid_pair(float t, float e) {
  SigmoidPair s;
  s.r = __builtin_amdgcn_rcpf(1.f + e);
  s.er = e * s.r;
  s.p = t >= 0.f ? s.r : s.er;
  s.q = t >= 0.f ? s.er : s.r;
  return s;
}
// log1p(e) of e = exp(-|t|) in (0, 1]: the 4-term series below 2^-6 (relative error < 2e-8) and log(1 + e) above (absolute
// rounding 6e-8 against a value >= 0.0155)
__device__ __forceinline__ float log1p_unit(float e) {
  const float series = e * fmaf(e, fmaf(e, fmaf(e, -0.25f, 0.33333334f), -0.5f), 1.f);
  const float lg = __builtin_amdgcn_logf(1.f + e) * 0.6931471805599453f;     // v_log_f32 is log2
  return e < 0.015625f ? series : lg;
}

// One (voxel, region) of the Bernoulli entropy on the fast path: h = H(sigmoid(t)), g = dH/dt.
__device__ __forceinline__ void bernoulli_entropy_terms(float t, float& h, float& g) {
  const float e = exp_neg_abs(t);
  const SigmoidPair s = sigmoid_pair(t, e);
  const float l1p = log1p_unit(e);      // ahead of the max: hipcc's register count of the entropy fast path follows this order
  h = fmaxf(t, 0.f) + l1p - t * s.p;
  g = -t * (s.er * s.r);           // sig (1 - sig) = sig(|t|) (1 - sig(|t|)) = r * (e r): even in t
}

// ... and on the generic path, in libm's expf / log1pf and IEEE division.  g is -t sig (1 - sig) with the subtraction, not
// the fast path's -t (e r r): the two forms round differently, and each path keeps its own.
struct BernoulliLibm {
  float e, sig, h, g;
};
__device__ __forceinline__ BernoulliLibm bernoulli_entropy_libm(float t) {
  BernoulliLibm b;
  b.e = expf(-fabsf(t));
  b.sig = t >= 0.f ? 1.f / (1.f + b.e) : b.e / (1.f + b.e);
  const float softplus = fmaxf(t, 0.f) + log1pf(b.e);
  b.h = softplus - t * b.sig;
  b.g = -t * b.sig * (1.f - b.sig);
  return b;
}

// A voxel's logits and its softmax entropy.  H = lse - sum p z is the form that decides keep = H < margin in every filtered
// objective.  SHIFTED adds Hs = log se - sum p u (u = z - max <= 0, log p = u - log se), the value that enters the loss, the
// weight and the gradient of the weighted objectives: lse and sum p z are both of the size of the largest logit, so their
// difference carries that logit's rounding (1e-6 at |z| = 9) - more than the 2e-5 of its maximum the gradient of a
// confident, kept voxel is held to.
struct CategoricalVoxel {
  float t[LOSS_MAX_R];
  float m, se, lse, H, lgs, Hs;
};
// t, m = max t and se = sum exp(t - m) >= 1 alone (what every categorical head starts from)
__device__ __forceinline__ void categorical_load(const float* zp, int R, CategoricalVoxel& v) {
  v.m = -INFINITY;
#pragma unroll
  for (int r = 0; r < LOSS_MAX_R; ++r)
    if (r < R) { v.t[r] = zp[r]; v.m = fmaxf(v.m, v.t[r]); }
  v.se = 0.f;
#pragma unroll
  for (int r = 0; r < LOSS_MAX_R; ++r)
    if (r < R) v.se += expf(v.t[r] - v.m);
}
template <bool SHIFTED>
__device__ __forceinline__ void categorical_entropy(const float* zp, int R, CategoricalVoxel& v) {
  categorical_load(zp, R, v);
  v.lse = v.m + logf(v.se);
  float pz = 0.f;
#pragma unroll
  for (int r = 0; r < LOSS_MAX_R; ++r)
    if (r < R) pz += expf(v.t[r] - v.lse) * v.t[r];
  v.H = v.lse - pz;
  if (SHIFTED) {
    v.lgs = logf(v.se);
    float pu = 0.f;
#pragma unroll
    for (int r = 0; r < LOSS_MAX_R; ++r)
      if (r < R) {
        const float u = v.t[r] - v.m;
        pu += expf(u - v.lgs) * u;
      }
    v.Hs = v.lgs - pu;
  }
}
// dH/dz_r (plain) or dHs/dz_r (SHIFTED) of that voxel
template <bool SHIFTED>
__device__ __forceinline__ float categorical_entropy_grad(const CategoricalVoxel& v, int r) {
  if (SHIFTED) {
    const float logp = (v.t[r] - v.m) - v.lgs;
    return -expf(logp) * (logp + v.Hs);
  }
  const float logp = v.t[r] - v.lse;
  return -expf(logp) * (logp + v.H);
}
// the FIRST arg max of the voxel's logits
__device__ __forceinline__ int categorical_argmax(const CategoricalVoxel& v, int R) {
  float m = -INFINITY;
  int arg = 0;
#pragma unroll
  for (int r = 0; r < LOSS_MAX_R; ++r)
    if (r < R) {
      arg = v.t[r] > m ? r : arg;
      m = fmaxf(m, v.t[r]);
    }
  return arg;
}

// ------------------------------------------------------------------ device: the voxel walk
// Coordinates of linear voxel v (n, z, y, x order) of a view; I is the index type of the walk: long long for the entropy
// family, unsigned behind loss_small_item for the rest.
struct VoxPos {
  int n, z, y, x;
};
template <class I>
__device__ __forceinline__ VoxPos vox_pos(const TV& t, I v) {
  VoxPos p;
  p.x = (int)(v % t.w); v /= t.w;
  p.y = (int)(v % t.h); v /= t.h;
  p.z = t.n == 1 ? (int)v : (int)(v % t.d);      // a walk inside one item: no third division (uniform branch)
  p.n = t.n == 1 ? 0 : (int)(v / t.d);
  return p;
}
__device__ __forceinline__ long long vox_addr(const TV& t, const VoxPos& p) { return vox_addr(t, p.n, p.z, p.y, p.x); }
// batch item n of a gradient tensor whose elements are 2 (OBF) or 4 bytes wide
template <bool OBF>
__device__ __forceinline__ float* grad_item(float* p, long long n, long long sn) {
  return OBF ? reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(p) + n * sn) : p + n * sn;
}

// The second operand of a policy: none, or a tensor of the logits' shape read at the same voxel (the consistency target).
// A policy with an operand runs per item only (item() has moved it to the item, the position's n is 0).
struct NoOperand {
  __device__ __forceinline__ void item(int, long long) {}
  template <class I> __device__ __forceinline__ float4 row(I) const { return make_float4(0.f, 0.f, 0.f, 0.f); }
  __device__ __forceinline__ float at(const VoxPos&, int) const { return 0.f; }
  __device__ __forceinline__ const float* vox(const VoxPos&) const { return nullptr; }
};
struct SameVoxelOperand {
  TV t;
  __device__ __forceinline__ void item(int n, long long) { t.p += (long long)n * t.sn; }
  template <class I> __device__ __forceinline__ float4 row(I v) const { return *reinterpret_cast<const float4*>(t.p + (long long)v * 4); }
  __device__ __forceinline__ float at(const VoxPos& p, int c) const { return t.p[vox_addr(t, p) + c]; }
  __device__ __forceinline__ const float* vox(const VoxPos& p) const { return t.p + vox_addr(t, p); }
};

// ---- the plain walk: loss = mean of h, dlogits = g / count.  A policy P gives, next to its operand (item / row / at / vox):
//   fast(z, o, h, g)                 one (voxel, region) of the fast path; o = the operand's value there
//   generic(z, o, h, g)              ... of the any-stride path
//   categorical(zp, op, R, put) -> h  one voxel of the categorical head; put(r, g_r) takes the gradient class by class
// The walk owns the item offset, the traversal, the stores, the fp64 block partial [item][block] and the 1 / count scale.
// per_item = 0 (mmtta_entropy_loss alone): one objective over the whole batch, gridDim.y = 1.
template <class P, bool OBF>
__device__ __forceinline__ void loss_item(TV& z, TV& dz, double*& partial, P& p) {
  z.p += (long long)blockIdx.y * z.sn;
  dz.p = grad_item<OBF>(dz.p, blockIdx.y, dz.sn);
  z.n = 1; dz.n = 1;
  partial += (long long)blockIdx.y * gridDim.x;
  p.item(blockIdx.y, 0);
}

// A thread owns a voxel of <= 4 regions in a dense 16-byte row: one 16-byte load per operand, one 16- / 8-byte store (the
// gradient tensor owns its pad lane), no index arithmetic; the voxel's terms are summed in fp32 and enter the double
// accumulator once.  OBF: the gradient is bf16-stored (its readers round it to bf16 while staging).
template <class P, class I, bool OBF>
__global__ __launch_bounds__(256) void loss_vec_kernel(TV z, TV dz, double* partial, float inv_count, int per_item, P p) {
  __shared__ double sh[4];
  if (per_item) loss_item<P, OBF>(z, dz, partial, p);
  const int C = z.c;
  const I dhw = (I)z.d * z.h * z.w;
  const I total = (I)z.n * dhw;
  double acc = 0.0;
  for (I i = blockIdx.x * (I)blockDim.x + threadIdx.x; i < total; i += (I)gridDim.x * blockDim.x) {
    // one volume per launch in the adaptation loop: no 64-bit division per voxel then (uniform branch)
    const I n = z.n == 1 ? 0 : i / dhw, v = i - n * dhw;
    const float4 t4 = *reinterpret_cast<const float4*>(z.p + n * z.sn + (long long)v * 4);
    const float4 o4 = p.row(v);
    const float ts[4] = {t4.x, t4.y, t4.z, t4.w}, os[4] = {o4.x, o4.y, o4.z, o4.w};
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    float h = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < C) {
        float hc, gc;
        p.fast(ts[c], os[c], hc, gc);
        h += hc;
        g[c] = gc * inv_count;
      }
    }
    acc += (double)h;
    st4_any(dz.p, n * dz.sn + (long long)v * 4, make_float4(g[0], g[1], g[2], g[3]), OBF);
  }
  const double t = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// A thread owns a (voxel, region) pair: any R, any strides, fp32 gradients.
template <class P, class I>
__global__ __launch_bounds__(256) void loss_region_kernel(TV z, TV dz, double* partial, float inv_count, int per_item, P p) {
  __shared__ double sh[4];
  if (per_item) loss_item<P, false>(z, dz, partial, p);
  const int C = z.c;
  const I total = (I)z.n * z.d * z.h * z.w * C;
  double acc = 0.0;
  for (I i = blockIdx.x * (I)blockDim.x + threadIdx.x; i < total; i += (I)gridDim.x * blockDim.x) {
    const I vox = i / C;
    const int c = (int)(i - vox * C);
    const VoxPos pos = vox_pos(z, vox);
    float h, g;
    p.generic(z.p[vox_addr(z, pos) + c], p.at(pos, c), h, g);
    acc += (double)h;
    dz.p[vox_addr(dz, pos) + c] = g * inv_count;
  }
  const double t = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// A thread owns a voxel of up to LOSS_MAX_R classes.
template <class P, class I>
__global__ __launch_bounds__(256) void loss_voxel_kernel(TV z, TV dz, double* partial, float inv_count, int per_item, P p) {
  __shared__ double sh[4];
  if (per_item) loss_item<P, false>(z, dz, partial, p);
  const int R = z.c;
  const I total = (I)z.n * z.d * z.h * z.w;
  double acc = 0.0;
  for (I i = blockIdx.x * (I)blockDim.x + threadIdx.x; i < total; i += (I)gridDim.x * blockDim.x) {
    const VoxPos pos = vox_pos(z, i);
    float* gp = dz.p + vox_addr(dz, pos);
    acc += (double)p.categorical(z.p + vox_addr(z, pos), p.vox(pos), R, [&](int r, float g) { gp[r] = g * inv_count; });
  }
  const double t = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// loss[item] = sum of the item's block partials * inv_count (static: one copy per translation unit that launches it)
static __global__ __launch_bounds__(64) void mean_finish_kernel(const double* partial, int nblocks, double inv_count, float* loss) {
  partial += (long long)blockIdx.x * nblocks;      // one workgroup per independent item (a single one otherwise)
  double s = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 64) s += partial[i];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) loss[blockIdx.x] = (float)(s * inv_count);
}

// ---- the filtered walk, per item (gridDim.y), in two passes over the same grid.  Pass 1 (kept == nullptr) writes
// keep = h < margin && pass && allowed as one byte per element (dense channels-last: (voxel, region) for the Bernoulli heads,
// voxel for the categorical one) and leaves the fp64 block partials of fent_store_partials<P::ROWS>; the finish kernel writes
// loss[item] and kept[item]; pass 2 writes dlogits = keep * g / kept[item], the count read on the device.  With every
// element kept and v = h the block partials, the loss arithmetic and the gradient scale are those of the plain walk.
// One element of a filtered objective, as the policy returns it:
struct KeptTerms {
  float h;        // the entropy that decides keep against the margin
  float v;        // what a kept element adds to the loss (weight included)
  float g;        // ... and its gradient before the 1 / kept scale (Bernoulli heads; the categorical one hands it to put)
  bool pass;      // the policy's second predicate (DeYO's PLPD threshold; true elsewhere)
};
// A policy P gives, next to its operand accessors: ROWS (2, or 3 with the count of h < margin alone), margin,
// allowed(i) (an incoming mask; true elsewhere), fast(z, o) / generic(z, o) / categorical(zp, op, R, put) -> KeptTerms.
template <class P, class I, bool OBF>
__global__ __launch_bounds__(256) void kept_vec_kernel(TV z, TV dz, unsigned char* kout, double* partial, const long long* kept, P p) {
  __shared__ double sh[4];
  const int C = z.c;
  const I total = (I)z.d * z.h * z.w;
  z.p += (long long)blockIdx.y * z.sn;
  kout += (long long)blockIdx.y * total * C;
  p.item(blockIdx.y, (long long)total * C);
  const bool grad = kept != nullptr;      // pass 2: kout is the mask pass 1 wrote
  if (grad) dz.p = grad_item<OBF>(dz.p, blockIdx.y, dz.sn);
  const float scale = grad ? fent_scale(kept) : 0.f;
  double acc = 0.0;
  int cnt = 0, cnt1 = 0;
  for (I v = blockIdx.x * (I)blockDim.x + threadIdx.x; v < total; v += (I)gridDim.x * blockDim.x) {
    const float4 t4 = *reinterpret_cast<const float4*>(z.p + (long long)v * 4);
    const float4 o4 = p.row(v);
    const float ts[4] = {t4.x, t4.y, t4.z, t4.w}, os[4] = {o4.x, o4.y, o4.z, o4.w};
    unsigned char km[4] = {0, 0, 0, 0};      // pass 2 reads the voxel's mask bytes before the per-region work, not inside it
    if (grad) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) km[c] = kout[(long long)v * C + c];
    }
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    float h = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < C) {
        const KeptTerms e = p.fast(ts[c], os[c]);
        if (grad) {
          g[c] = km[c] ? e.g * scale : 0.f;
        } else {
          const bool keep1 = e.h < p.margin;
          const bool keep = keep1 && e.pass && p.allowed((long long)v * C + c);
          km[c] = keep ? 1 : 0;
          cnt1 += keep1 ? 1 : 0;
          if (keep) { h += e.v; ++cnt; }
        }
      }
    }
    if (grad) {
      st4_any(dz.p, (long long)v * 4, make_float4(g[0], g[1], g[2], g[3]), OBF);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) kout[(long long)v * C + c] = km[c];
      acc += (double)h;
    }
  }
  if (!grad) fent_store_partials<P::ROWS>(acc, cnt, cnt1, partial, sh);
}

template <class P, class I>
__global__ __launch_bounds__(256) void kept_region_kernel(TV z, TV dz, unsigned char* kout, double* partial, const long long* kept, P p) {
  __shared__ double sh[4];
  const int C = z.c;
  const I total = (I)z.d * z.h * z.w * C;
  z.p += (long long)blockIdx.y * z.sn;
  z.n = 1;
  kout += (long long)blockIdx.y * total;
  p.item(blockIdx.y, (long long)total);
  const bool grad = kept != nullptr;
  if (grad) dz.p += (long long)blockIdx.y * dz.sn;
  const float scale = grad ? fent_scale(kept) : 0.f;
  double acc = 0.0;
  int cnt = 0, cnt1 = 0;
  for (I i = blockIdx.x * (I)blockDim.x + threadIdx.x; i < total; i += (I)gridDim.x * blockDim.x) {
    const I vox = i / C;
    const int c = (int)(i - vox * C);
    const VoxPos pos = vox_pos(z, vox);
    const KeptTerms e = p.generic(z.p[vox_addr(z, pos) + c], p.at(pos, c));
    if (grad) {
      dz.p[vox_addr(dz, pos) + c] = kout[i] ? e.g * scale : 0.f;
      continue;
    }
    const bool keep1 = e.h < p.margin;
    const bool keep = keep1 && e.pass && p.allowed((long long)i);
    kout[i] = keep ? 1 : 0;
    cnt1 += keep1 ? 1 : 0;
    if (keep) { acc += (double)e.v; ++cnt; }
  }
  if (!grad) fent_store_partials<P::ROWS>(acc, cnt, cnt1, partial, sh);
}

template <class P, class I>
__global__ __launch_bounds__(256) void kept_voxel_kernel(TV z, TV dz, unsigned char* kout, double* partial, const long long* kept, P p) {
  __shared__ double sh[4];
  const int R = z.c;
  const I total = (I)z.d * z.h * z.w;
  z.p += (long long)blockIdx.y * z.sn;
  z.n = 1;
  kout += (long long)blockIdx.y * total;
  p.item(blockIdx.y, (long long)total);
  const bool grad = kept != nullptr;
  if (grad) dz.p += (long long)blockIdx.y * dz.sn;
  const float scale = grad ? fent_scale(kept) : 0.f;
  double acc = 0.0;
  int cnt = 0, cnt1 = 0;
  for (I i = blockIdx.x * (I)blockDim.x + threadIdx.x; i < total; i += (I)gridDim.x * blockDim.x) {
    const VoxPos pos = vox_pos(z, i);
    if (grad) {
      float* gp = dz.p + vox_addr(dz, pos);
      const bool keep = kout[i] != 0;
      p.categorical(z.p + vox_addr(z, pos), p.vox(pos), R, [&](int r, float g) { gp[r] = keep ? g * scale : 0.f; });
      continue;
    }
    const KeptTerms e = p.categorical(z.p + vox_addr(z, pos), p.vox(pos), R, [](int, float) {});
    const bool keep1 = e.h < p.margin;
    const bool keep = keep1 && e.pass && p.allowed((long long)i);
    kout[i] = keep ? 1 : 0;
    cnt1 += keep1 ? 1 : 0;
    if (keep) { acc += (double)e.v; ++cnt; }
  }
  if (!grad) fent_store_partials<P::ROWS>(acc, cnt, cnt1, partial, sh);
}

// loss[item] = kept sum / kept count (NaN where nothing is kept), kept[item] and (ROWS == 3) kept1[item]
template <int ROWS>
__global__ __launch_bounds__(64) void kept_finish_kernel(const double* partial, int nblocks, float* loss, long long* kept, long long* kept1) {
  partial += (long long)blockIdx.x * ROWS * nblocks;      // one workgroup per item
  double s = 0.0, c = 0.0, c1 = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 64) {
    s += partial[i];
    c += partial[nblocks + i];
    if (ROWS == 3) c1 += partial[2 * nblocks + i];
  }
  s = wave_sum_d(s);
  c = wave_sum_d(c);
  if (ROWS == 3) c1 = wave_sum_d(c1);
  if (threadIdx.x == 0) {
    kept[blockIdx.x] = (long long)c;
    if (ROWS == 3) kept1[blockIdx.x] = (long long)c1;
    loss[blockIdx.x] = c > 0.0 ? (float)(s * (1.0 / c)) : __builtin_nanf("");
  }
}

// ------------------------------------------------------------------ host: the launch ladders
// How an entry point names itself: in the refusal of a bf16 gradient, in the checks of the categorical head, and in the
// status of its launches ("<status> bernoulli", "<status> categorical gradient", "<status> finish", ...).
struct LossNames {
  const char *bf16, *softmax, *status;
};
inline int loss_status(const LossNames& nm, const char* stage) {
  char what[96];
  snprintf(what, sizeof(what), "%s %s", nm.status, stage);
  return launch_status(what);
}
// The head's checks, shared by both ladders: bf16 gradients outside the fast path are refused.
inline int loss_head_check(const LossNames& nm, const mmtta_tensor* z, const mmtta_tensor* dz, int softmax, bool vec) {
  if (!softmax) {
    MMTTA_CHECK(is_f32(dz) || vec, MMTTA_ERR_UNSUPPORTED, "%s: a bf16-stored `dlogits` needs dense 4-channel voxel rows that own their pad", nm.bf16);
    return MMTTA_OK;
  }
  MMTTA_CHECK(z->c <= LOSS_MAX_R, MMTTA_ERR_UNSUPPORTED, "%s softmax: more than %d classes", nm.softmax, LOSS_MAX_R);
  MMTTA_CHECK(is_f32(dz), MMTTA_ERR_UNSUPPORTED, "%s softmax: `dlogits` must be fp32-stored", nm.softmax);
  return MMTTA_OK;
}

// The plain objective of policy P over index type I: the walk the head and the operands allow, then the finish kernel.
// per_item: every batch item is its own objective - the launch geometry, block partials and scale of ONE item, repeated
// along gridDim.y (bit-identical to N separate calls).
template <class P, class I>
inline int loss_launch(const LossNames& nm, const mmtta_tensor* z, const mmtta_tensor* dz, int softmax, bool vec, int per_item,
                       double* partial, float* loss, const P& p, hipStream_t s) {
  int st = loss_head_check(nm, z, dz, softmax, vec);
  if (st) return st;
  const int items = per_item ? z->n : 1;
  const int blocks = loss_blocks(z, per_item ? 1 : z->n);
  const long long nvox = (long long)(per_item ? 1 : z->n) * z->d * z->h * z->w;
  const double cnt = softmax ? (double)nvox : (double)nvox * z->c;
  const float inv = (float)(1.0 / cnt);
  const dim3 grid(blocks, items);
  if (softmax)
    hipLaunchKernelGGL((loss_voxel_kernel<P, I>), grid, dim3(256), 0, s, tv(z), tv(dz), partial, inv, per_item, p);
  else if (vec && is_bf16(dz))
    hipLaunchKernelGGL((loss_vec_kernel<P, I, true>), grid, dim3(256), 0, s, tv(z), tv(dz), partial, inv, per_item, p);
  else if (vec)
    hipLaunchKernelGGL((loss_vec_kernel<P, I, false>), grid, dim3(256), 0, s, tv(z), tv(dz), partial, inv, per_item, p);
  else
    hipLaunchKernelGGL((loss_region_kernel<P, I>), grid, dim3(256), 0, s, tv(z), tv(dz), partial, inv, per_item, p);
  st = loss_status(nm, softmax ? "categorical" : "bernoulli");
  if (st) return st;
  hipLaunchKernelGGL(mean_finish_kernel, dim3(items), dim3(64), 0, s, partial, blocks, 1.0 / cnt, loss);
  return loss_status(nm, "finish");
}

// The filtered objective of policy P: pass 1, the finish kernel, pass 2.  kept1 is read by P::ROWS == 3 alone.
template <class P, class I>
inline int kept_launch(const LossNames& nm, const mmtta_tensor* z, const mmtta_tensor* dz, int softmax, bool vec,
                       unsigned char* kout, double* partial, float* loss, long long* kept, long long* kept1, const P& p,
                       hipStream_t s) {
  int st = loss_head_check(nm, z, dz, softmax, vec);
  if (st) return st;
  const int items = z->n;
  const int blocks = loss_blocks(z);
  const dim3 grid(blocks, items);
  auto pass = [&](double* part, const long long* kk) {
    if (softmax)
      hipLaunchKernelGGL((kept_voxel_kernel<P, I>), grid, dim3(256), 0, s, tv(z), tv(dz), kout, part, kk, p);
    else if (vec && is_bf16(dz))
      hipLaunchKernelGGL((kept_vec_kernel<P, I, true>), grid, dim3(256), 0, s, tv(z), tv(dz), kout, part, kk, p);
    else if (vec)
      hipLaunchKernelGGL((kept_vec_kernel<P, I, false>), grid, dim3(256), 0, s, tv(z), tv(dz), kout, part, kk, p);
    else
      hipLaunchKernelGGL((kept_region_kernel<P, I>), grid, dim3(256), 0, s, tv(z), tv(dz), kout, part, kk, p);
  };
  pass(partial, nullptr);
  st = loss_status(nm, softmax ? "categorical" : "bernoulli");
  if (st) return st;
  hipLaunchKernelGGL(kept_finish_kernel<P::ROWS>, dim3(items), dim3(64), 0, s, (const double*)partial, blocks, loss, kept, kept1);
  st = loss_status(nm, "finish");
  if (st) return st;
  pass(nullptr, kept);
  return loss_status(nm, softmax ? "categorical gradient" : "bernoulli gradient");
}

}  // namespace mmtta
