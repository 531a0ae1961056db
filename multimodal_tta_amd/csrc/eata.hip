// EATA (Niu et al., ICML 2022, "Efficient Test-Time Model Adaptation without Forgetting") on the flat arena (gfx950): the
// weighted reliable entropy with its gradient, the pseudo-label loss the Fisher estimate differentiates, the accumulation
// of squared gradients into the Fisher span and the pass that adds the Fisher-weighted pull towards the source weights to
// the gradient of every parameter set.  All are single-pass HBM-bound streams.  See include/mmtta.h for the contracts.
#include "common.h"

namespace mmtta {

constexpr int EATA_MAX_BLOCKS = 2048;      // block partials per item (the entropy objective's figure)
constexpr int EATA_MAX_R = 16;             // classes of the categorical paths
constexpr int EATA_MAX_GRID_Y = 65535;     // gridDim.y carries the item / the parameter set
constexpr int FISHER_MAX_BLOCKS = 4096;    // workgroups per parameter set (optim_kernel's figure)
constexpr int PENALTY_BLOCKS = 1024;       // block partials per parameter set of the penalty pass

// ------------------------------------------------------------------ weighted reliable entropy
// The launch geometry, the mask layout and the partial layout of mmtta_entropy_filtered_items (loss_optim_metric.hip), and
// its entropy arithmetic: the fast path calls the same bernoulli_entropy_terms / fent_store_partials / fent_scale (common.h),
// the generic and categorical kernels restate that entry point's expressions in the same order, so that keep = H < margin
// and the kept count come out bit for bit as that entry point's.  What differs is the weight c = exp(margin - H) in
// (1, e^margin] on every kept element, a constant of the gradient: pass 1 leaves fp64 block partials of the kept sum of c H
// and of the kept count, pass 2 writes dlogits = keep * c * dH/dz / kept[item] with the count read on the device.

__global__ __launch_bounds__(256) void went_bernoulli_kernel(TV z, TV dz, float margin, unsigned char* kout, double* partial,
                                                             const long long* kept) {
  __shared__ double sh[4];
  const int C = z.c;
  const long long total = (long long)z.d * z.h * z.w * C;
  z.p += (long long)blockIdx.y * z.sn;
  kout += (long long)blockIdx.y * total;
  const bool grad = kept != nullptr;      // pass 2: kout is the mask pass 1 wrote
  if (grad) dz.p += (long long)blockIdx.y * dz.sn;
  const float scale = grad ? fent_scale(kept) : 0.f;
  double acc = 0.0;
  int cnt = 0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    long long v = i / C;
    const int x = (int)(v % z.w); v /= z.w;
    const int y = (int)(v % z.h); v /= z.h;
    const int zz = (int)v;
    const float t = z.p[zz * z.sd + y * z.sh + x * z.sw + c];
    const float e = expf(-fabsf(t));
    const float sig = t >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    const float softplus = fmaxf(t, 0.f) + log1pf(e);
    const float h = softplus - t * sig;
    const float wgt = expf(margin - fminf(h, margin));      // 1 where the element is not kept: never large
    if (grad) {
      dz.p[zz * dz.sd + y * dz.sh + x * dz.sw + c] = kout[i] ? wgt * (-t * sig * (1.f - sig)) * scale : 0.f;
      continue;
    }
    const bool keep = h < margin;
    kout[i] = keep ? 1 : 0;
    if (keep) { acc += (double)(wgt * h); ++cnt; }
  }
  if (!grad) fent_store_partials(acc, cnt, partial, sh);
}

// Fast path: <= 4 regions in dense 16-byte voxel rows; a thread owns a voxel.  OBF: bf16-stored gradient.  Pass 2 reads the
// voxel's <= 4 mask bytes before the per-region work, not inside it.
template <bool OBF>
__global__ __launch_bounds__(256) void went_bernoulli_vec_kernel(TV z, TV dz, float margin, unsigned char* kout,
                                                                 double* partial, const long long* kept) {
  __shared__ double sh[4];
  const int C = z.c;
  const long long total = (long long)z.d * z.h * z.w;
  z.p += (long long)blockIdx.y * z.sn;
  kout += (long long)blockIdx.y * total * C;
  const bool grad = kept != nullptr;
  if (grad)
    dz.p = OBF ? reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(dz.p) + (long long)blockIdx.y * dz.sn)
               : dz.p + (long long)blockIdx.y * dz.sn;
  const float scale = grad ? fent_scale(kept) : 0.f;
  double acc = 0.0;
  int cnt = 0;
  for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < total;
       v += (long long)gridDim.x * blockDim.x) {
    const float4 t4 = *reinterpret_cast<const float4*>(z.p + v * 4);
    const float ts[4] = {t4.x, t4.y, t4.z, t4.w};
    unsigned char km[4] = {0, 0, 0, 0};
    if (grad) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) km[c] = kout[v * C + c];
    }
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    float h = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < C) {
        float hc, gc;
        bernoulli_entropy_terms(ts[c], hc, gc);
        const float wgt = __builtin_amdgcn_exp2f((margin - fminf(hc, margin)) * 1.4426950408889634f);
        if (grad) {
          g[c] = km[c] ? wgt * gc * scale : 0.f;
        } else {
          const bool keep = hc < margin;
          km[c] = keep ? 1 : 0;
          if (keep) { h += wgt * hc; ++cnt; }
        }
      }
    }
    if (grad) {
      st4_any(dz.p, v * 4, make_float4(g[0], g[1], g[2], g[3]), OBF);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) kout[v * C + c] = km[c];
      acc += (double)h;
    }
  }
  if (!grad) fent_store_partials(acc, cnt, partial, sh);
}

__global__ __launch_bounds__(256) void went_categorical_kernel(TV z, TV dz, float margin, unsigned char* kout, double* partial,
                                                               const long long* kept) {
  __shared__ double sh[4];
  const int R = z.c;
  const long long total = (long long)z.d * z.h * z.w;
  z.p += (long long)blockIdx.y * z.sn;
  kout += (long long)blockIdx.y * total;
  const bool grad = kept != nullptr;
  if (grad) dz.p += (long long)blockIdx.y * dz.sn;
  const float scale = grad ? fent_scale(kept) : 0.f;
  double acc = 0.0;
  int cnt = 0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    long long v = i;
    const int x = (int)(v % z.w); v /= z.w;
    const int y = (int)(v % z.h); v /= z.h;
    const int zz = (int)v;
    const float* zp = z.p + zz * z.sd + y * z.sh + x * z.sw;
    float t[EATA_MAX_R];
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < EATA_MAX_R; ++r)
      if (r < R) { t[r] = zp[r]; m = fmaxf(m, t[r]); }
    float se = 0.f;
#pragma unroll
    for (int r = 0; r < EATA_MAX_R; ++r)
      if (r < R) se += expf(t[r] - m);
    const float lse = m + logf(se);
    float pz = 0.f;
#pragma unroll
    for (int r = 0; r < EATA_MAX_R; ++r)
      if (r < R) pz += expf(t[r] - lse) * t[r];
    const float H = lse - pz;              // the filtered kernel's H: it decides keep, bit for bit
    // The value that enters the loss, the weight and the gradient is H in the shifted form (u = z - max <= 0, log p =
    // u - log se, H = log se - sum p u): lse and sum p z above are both of the size of the largest logit, so their
    // difference carries that logit's rounding (1e-6 at |z| = 9) - more than the 2e-5 of its maximum the gradient of a
    // confident, kept voxel is held to.
    const float lgs = logf(se);
    float pu = 0.f;
#pragma unroll
    for (int r = 0; r < EATA_MAX_R; ++r)
      if (r < R) {
        const float u = t[r] - m;
        pu += expf(u - lgs) * u;
      }
    const float Hs = lgs - pu;
    const float wgt = expf(margin - fminf(Hs, margin));
    if (grad) {
      float* gp = dz.p + zz * dz.sd + y * dz.sh + x * dz.sw;
      const bool keep = kout[i] != 0;
#pragma unroll
      for (int r = 0; r < EATA_MAX_R; ++r)
        if (r < R) {
          const float logp = (t[r] - m) - lgs;
          gp[r] = keep ? wgt * (-expf(logp) * (logp + Hs)) * scale : 0.f;
        }
      continue;
    }
    const bool keep = H < margin;
    kout[i] = keep ? 1 : 0;
    if (keep) { acc += (double)(wgt * Hs); ++cnt; }
  }
  if (!grad) fent_store_partials(acc, cnt, partial, sh);
}

__global__ __launch_bounds__(64) void went_finish_kernel(const double* partial, int nblocks, float* loss, long long* kept) {
  partial += (long long)blockIdx.x * 2 * nblocks;      // one workgroup per item
  double s = 0.0, c = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 64) { s += partial[i]; c += partial[nblocks + i]; }
  s = wave_sum_d(s);
  c = wave_sum_d(c);
  if (threadIdx.x == 0) {
    kept[blockIdx.x] = (long long)c;
    loss[blockIdx.x] = c > 0.0 ? (float)(s * (1.0 / c)) : __builtin_nanf("");
  }
}

static int eata_blocks(const mmtta_tensor* z) {      // mmtta_entropy_filtered_partials' figure for ONE item
  const long long total = (long long)z->d * z->h * z->w * z->c;
  long long b = (total + 255) / 256;
  if (b < 1) b = 1;
  if (b > EATA_MAX_BLOCKS) b = EATA_MAX_BLOCKS;
  return (int)b;
}

static bool eata_dense16(const mmtta_tensor* t) {
  return t->sc == 1 && t->sw == 4 && t->sh == (int64_t)t->w * 4 && t->sd == (int64_t)t->h * t->sh && t->sn % 4 == 0 &&
         ((uintptr_t)t->ptr) % 16 == 0;
}

// ------------------------------------------------------------------ pseudo-label loss (the Fisher estimate's objective)
// Bernoulli heads: y = 1[z >= 0], h = BCE(z, y) = -log sigmoid(s) with s = y ? z : -z (= |z|), taken as
// min(s, 0) - log1p(exp(-|s|)): finite for every finite z.  g = sigmoid(z) - y = -+ e / (1 + e), e = exp(-|z|), formed
// without a subtraction.  v_exp_f32 / v_rcp_f32 / v_log_f32 and the 4-term series as the entropy fast path.
__device__ __forceinline__ void pseudo_bernoulli_terms(float z, float& h, float& g) {
  const bool y = z >= 0.f;
  const float s = y ? z : -z;
  const float e = __builtin_amdgcn_exp2f(-fabsf(s) * 1.4426950408889634f);
  const float r = __builtin_amdgcn_rcpf(1.f + e);
  const float series = e * fmaf(e, fmaf(e, fmaf(e, -0.25f, 0.33333334f), -0.5f), 1.f);
  const float lg = __builtin_amdgcn_logf(1.f + e) * 0.6931471805599453f;
  const float l1p = e < 0.015625f ? series : lg;
  h = -(fminf(s, 0.f) - l1p);
  const float er = e * r;
  g = y ? -er : er;
}

template <bool OBF>
__global__ __launch_bounds__(256) void pseudo_bernoulli_vec_kernel(const float* __restrict__ z, float* __restrict__ dz,
                                                                   long long zsn, long long dzsn, int C, unsigned dhw,
                                                                   double* partial, float inv_count) {
  __shared__ double sh[4];
  z += (long long)blockIdx.y * zsn;
  dz = OBF ? reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(dz) + (long long)blockIdx.y * dzsn)
           : dz + (long long)blockIdx.y * dzsn;
  partial += (long long)blockIdx.y * gridDim.x;
  double acc = 0.0;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < dhw; i += gridDim.x * 256u) {
    const float4 z4 = *reinterpret_cast<const float4*>(z + (long long)i * 4);
    const float zs[4] = {z4.x, z4.y, z4.z, z4.w};
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    float h = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < C) {
        float hc, gc;
        pseudo_bernoulli_terms(zs[c], hc, gc);
        h += hc;
        g[c] = gc * inv_count;
      }
    }
    acc += (double)h;
    st4_any(dz, (long long)i * 4, make_float4(g[0], g[1], g[2], g[3]), OBF);
  }
  const double s = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void pseudo_bernoulli_kernel(TV z, TV dz, double* partial, float inv_count) {
  __shared__ double sh[4];
  const int item = blockIdx.y;
  partial += (long long)blockIdx.y * gridDim.x;
  const unsigned C = z.c, H = z.h, W = z.w;
  const unsigned total = (unsigned)z.d * H * W * C;
  double acc = 0.0;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned vox = i / C, c = i - vox * C;
    const unsigned row = vox / W, x = vox - row * W;
    const unsigned zz = row / H, y = row - zz * H;
    float h, g;
    pseudo_bernoulli_terms(z.p[vox_addr(z, item, zz, y, x) + c], h, g);
    acc += (double)h;
    dz.p[vox_addr(dz, item, zz, y, x) + c] = g * inv_count;
  }
  const double s = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// Categorical head: y = one-hot of the FIRST arg max, h = lse(z) - max z = log sum exp(z - max), g = softmax(z) - y.
__global__ __launch_bounds__(256) void pseudo_categorical_kernel(TV z, TV dz, double* partial, float inv_count) {
  __shared__ double sh[4];
  const int item = blockIdx.y, R = z.c;
  partial += (long long)blockIdx.y * gridDim.x;
  const unsigned H = z.h, W = z.w;
  const unsigned total = (unsigned)z.d * H * W;
  double acc = 0.0;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned row = i / W, x = i - row * W;
    const unsigned zz = row / H, y = row - zz * H;
    const float* zp = z.p + vox_addr(z, item, zz, y, x);
    float* gp = dz.p + vox_addr(dz, item, zz, y, x);
    float t[EATA_MAX_R];
    float m = -INFINITY;
    int arg = 0;
#pragma unroll
    for (int r = 0; r < EATA_MAX_R; ++r)
      if (r < R) {
        t[r] = zp[r];
        arg = t[r] > m ? r : arg;
        m = fmaxf(m, t[r]);
      }
    float se = 0.f;
#pragma unroll
    for (int r = 0; r < EATA_MAX_R; ++r)
      if (r < R) se += expf(t[r] - m);
    const float inv = 1.f / se;            // se >= 1: the maximum contributes exp(0)
    acc += (double)logf(se);
#pragma unroll
    for (int r = 0; r < EATA_MAX_R; ++r)
      if (r < R) gp[r] = (expf(t[r] - m) * inv - (r == arg ? 1.f : 0.f)) * inv_count;
  }
  const double s = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(64) void pseudo_finish_kernel(const double* partial, int nblocks, double inv_count, float* loss) {
  partial += (long long)blockIdx.x * nblocks;      // one workgroup per item
  double s = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 64) s += partial[i];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) loss[blockIdx.x] = (float)(s * inv_count);
}

// every offset inside one item fits 31 bits (the pseudo-label kernels index voxels with 32-bit arithmetic)
static bool eata_small_item(const mmtta_tensor* t) {
  const long long ld = t->sw > t->c ? t->sw : t->c;
  return t->d > 0 && t->h > 0 && t->w > 0 && t->c > 0 && (long long)t->d * t->h * t->w * (ld > 4 ? ld : 4) < (1ll << 31);
}

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
  return 2 * (int64_t)eata_blocks(logits) * logits->n;
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
  MMTTA_CHECK(logits->n <= EATA_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "entropy weighted: more than %d items in one call",
              EATA_MAX_GRID_Y);
  hipStream_t s = (hipStream_t)stream;
  const int items = logits->n;
  const int blocks = eata_blocks(logits);
  const dim3 grid(blocks, items);
  const long long* kd = (const long long*)kept;
  if (!softmax) {
    const bool vec = logits->c <= 4 && eata_dense16(logits) && eata_dense16(dlogits) &&
                     ((dlogits->flags & MMTTA_TENSOR_OWNS_PAD) || dlogits->c == 4);
    MMTTA_CHECK(is_f32(dlogits) || vec, MMTTA_ERR_UNSUPPORTED,
                "entropy weighted: a bf16-stored `dlogits` needs dense 4-channel voxel rows that own their pad");
    auto run = [&](double* part, const long long* kk) {
      if (vec && is_bf16(dlogits))
        hipLaunchKernelGGL(went_bernoulli_vec_kernel<true>, grid, dim3(256), 0, s, tv(logits), tv(dlogits), margin, keep_out, part, kk);
      else if (vec)
        hipLaunchKernelGGL(went_bernoulli_vec_kernel<false>, grid, dim3(256), 0, s, tv(logits), tv(dlogits), margin, keep_out, part, kk);
      else
        hipLaunchKernelGGL(went_bernoulli_kernel, grid, dim3(256), 0, s, tv(logits), tv(dlogits), margin, keep_out, part, kk);
    };
    run(partial, nullptr);
    int st = launch_status("entropy weighted bernoulli");
    if (st) return st;
    hipLaunchKernelGGL(went_finish_kernel, dim3(items), dim3(64), 0, s, partial, blocks, loss, (long long*)kept);
    st = launch_status("entropy weighted finish");
    if (st) return st;
    run(nullptr, kd);
    return launch_status("entropy weighted bernoulli gradient");
  }
  MMTTA_CHECK(logits->c <= EATA_MAX_R, MMTTA_ERR_UNSUPPORTED, "entropy weighted softmax: more than %d classes", EATA_MAX_R);
  MMTTA_CHECK(is_f32(dlogits), MMTTA_ERR_UNSUPPORTED, "entropy weighted softmax: `dlogits` must be fp32-stored");
  hipLaunchKernelGGL(went_categorical_kernel, grid, dim3(256), 0, s, tv(logits), tv(dlogits), margin, keep_out, partial,
                     (const long long*)nullptr);
  int st = launch_status("entropy weighted categorical");
  if (st) return st;
  hipLaunchKernelGGL(went_finish_kernel, dim3(items), dim3(64), 0, s, partial, blocks, loss, (long long*)kept);
  st = launch_status("entropy weighted finish");
  if (st) return st;
  hipLaunchKernelGGL(went_categorical_kernel, grid, dim3(256), 0, s, tv(logits), tv(dlogits), margin, keep_out, (double*)nullptr, kd);
  return launch_status("entropy weighted categorical gradient");
}

extern "C" int64_t mmtta_pseudo_label_partials(const mmtta_tensor* logits) {
  if (logits == nullptr || logits->n < 1) return -1;
  return (int64_t)eata_blocks(logits) * logits->n;
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
  MMTTA_CHECK(eata_small_item(logits) && eata_small_item(dlogits), MMTTA_ERR_UNSUPPORTED,
              "pseudo-label loss: an item of 2^31 elements or more");
  MMTTA_CHECK(logits->n <= EATA_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "pseudo-label loss: more than %d items in one call",
              EATA_MAX_GRID_Y);
  hipStream_t s = (hipStream_t)stream;
  const int items = logits->n;
  const int blocks = eata_blocks(logits);
  const long long nvox = (long long)logits->d * logits->h * logits->w;
  const dim3 grid(blocks, items);
  const double cnt = softmax ? (double)nvox : (double)nvox * logits->c;
  const float inv = (float)(1.0 / cnt);
  int st;
  if (!softmax) {
    const bool vec = logits->c <= 4 && eata_dense16(logits) && eata_dense16(dlogits) &&
                     ((dlogits->flags & MMTTA_TENSOR_OWNS_PAD) || dlogits->c == 4);
    MMTTA_CHECK(is_f32(dlogits) || vec, MMTTA_ERR_UNSUPPORTED,
                "pseudo-label loss: a bf16-stored `dlogits` needs dense 4-channel voxel rows that own their pad");
    if (vec && is_bf16(dlogits))
      hipLaunchKernelGGL(pseudo_bernoulli_vec_kernel<true>, grid, dim3(256), 0, s, (const float*)logits->ptr,
                         (float*)dlogits->ptr, (long long)logits->sn, (long long)dlogits->sn, (int)logits->c, (unsigned)nvox,
                         partial, inv);
    else if (vec)
      hipLaunchKernelGGL(pseudo_bernoulli_vec_kernel<false>, grid, dim3(256), 0, s, (const float*)logits->ptr,
                         (float*)dlogits->ptr, (long long)logits->sn, (long long)dlogits->sn, (int)logits->c, (unsigned)nvox,
                         partial, inv);
    else
      hipLaunchKernelGGL(pseudo_bernoulli_kernel, grid, dim3(256), 0, s, tv(logits), tv(dlogits), partial, inv);
    st = launch_status("pseudo-label bernoulli");
  } else {
    MMTTA_CHECK(logits->c <= EATA_MAX_R, MMTTA_ERR_UNSUPPORTED, "pseudo-label loss softmax: more than %d classes", EATA_MAX_R);
    MMTTA_CHECK(is_f32(dlogits), MMTTA_ERR_UNSUPPORTED, "pseudo-label loss softmax: `dlogits` must be fp32-stored");
    hipLaunchKernelGGL(pseudo_categorical_kernel, grid, dim3(256), 0, s, tv(logits), tv(dlogits), partial, inv);
    st = launch_status("pseudo-label categorical");
  }
  if (st) return st;
  hipLaunchKernelGGL(pseudo_finish_kernel, dim3(items), dim3(64), 0, s, partial, blocks, 1.0 / cnt, loss);
  return launch_status("pseudo-label finish");
}

extern "C" int mmtta_fisher_accumulate_sets(float* fisher, const float* grads, int64_t n, int sets, int64_t set_stride,
                                            void* stream) {
  MMTTA_CHECK(fisher && grads, MMTTA_ERR_INVALID, "fisher accumulate: null argument");
  MMTTA_CHECK(n >= 0, MMTTA_ERR_INVALID, "fisher accumulate: n = %lld", (long long)n);
  MMTTA_CHECK(sets >= 1 && sets <= EATA_MAX_GRID_Y, MMTTA_ERR_INVALID, "fisher accumulate: sets = %d (1 .. %d)", sets, EATA_MAX_GRID_Y);
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
  MMTTA_CHECK(sets >= 1 && sets <= replicas && sets <= EATA_MAX_GRID_Y && n <= set_stride, MMTTA_ERR_INVALID,
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
