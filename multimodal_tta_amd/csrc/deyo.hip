// DeYO (Lee et al., ICLR 2024, "Entropy is not Enough for Test-Time Adaptation") on gfx950: the patch-shuffled copy of a
// staged volume and the reliable entropy that is filtered and weighted by the pseudo-label probability difference (PLPD)
// between the logits of the volume and the logits of its shuffled copy.  Both are HBM-bound streams.  See include/mmtta.h
// for the contracts.
#include "common.h"

namespace mmtta {

constexpr int DEYO_MAX_BLOCKS = 2048;      // block partials per item (the entropy objective's figure)
constexpr int DEYO_MAX_R = 16;             // classes of the categorical path
constexpr int DEYO_MAX_GRID_Y = 65535;     // gridDim.y carries the item
constexpr int DEYO_MAX_PATCHES = 4096;     // 16 x 16 x 16

// The patch grid of one call: g* patches per axis of p* voxels each, P = gd * gh * gw slots in row-major order.
struct DeyoGrid {
  int gd, gh, gw, pd, ph, pw, P;
};

// The voxel that patch row[slot of (z, y, x)] holds at the same offset inside the patch.  With row = perm it is the source of
// a voxel of the shuffled copy, with row = the inverse it is where the content of a voxel of the volume went.  An entry
// outside [0, P) is clamped: the access stays inside the item whatever the table holds.
__device__ __forceinline__ void deyo_image(const DeyoGrid& g, const int* __restrict__ row, unsigned z, unsigned y, unsigned x,
                                           unsigned& iz, unsigned& iy, unsigned& ix) {
  const unsigned sz = z / (unsigned)g.pd, sy = y / (unsigned)g.ph, sx = x / (unsigned)g.pw;
  const unsigned slot = (sz * g.gh + sy) * g.gw + sx;      // < P: the grid divides the extents (checked on the host)
  const int e = row[slot];
  const unsigned j = (unsigned)min(max(e, 0), g.P - 1);
  const unsigned jr = j / (unsigned)g.gw, jx = j - jr * g.gw;
  const unsigned jz = jr / (unsigned)g.gh, jy = jr - jz * g.gh;      // jz < gd because j < P
  iz = jz * g.pd + (z - sz * g.pd);
  iy = jy * g.ph + (y - sy * g.ph);
  ix = jx * g.pw + (x - sx * g.pw);
}

// ------------------------------------------------------------------ the shuffled copy
// One thread per unit of T (16 / 8 / 4 / 2 bytes) of the output; the units of a voxel row and the rows of a run of W / gw
// voxels are consecutive on both sides, so the loads coalesce as the stores do.
template <class T>
__global__ __launch_bounds__(256) void deyo_shuffle_kernel(const T* __restrict__ x, T* __restrict__ y, long long xsn, long long ysn,
                                                           unsigned upr, unsigned D, unsigned H, unsigned W, DeyoGrid pg,
                                                           const int* __restrict__ table) {
  const int item = blockIdx.y;
  const int* perm = table + (long long)item * 2 * pg.P;
  const unsigned total = D * H * W * upr;
  const T* xb = x + (long long)item * xsn;
  T* yb = y + (long long)item * ysn;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned vox = i / upr, u = i - vox * upr;
    const unsigned r = vox / W, xx = vox - r * W;
    const unsigned zz = r / H, yy = r - zz * H;
    unsigned iz, iy, ix;
    deyo_image(pg, perm, zz, yy, xx, iz, iy, ix);
    yb[i] = xb[((iz * H + iy) * W + ix) * upr + u];
  }
}

// ------------------------------------------------------------------ PLPD-weighted reliable entropy
// The launch geometry, the mask layout and the entropy arithmetic of mmtta_entropy_weighted_items (eata.hip), hence of
// mmtta_entropy_filtered_items: keep1 = H < margin and its count come out bit for bit as that entry point's.  z'' is read from
// the shuffled logits at the mapped voxel (the inverse row of the table).  Pass 1 leaves the keep bytes and fp64 block
// partials of the kept sum of a H, of |keep| and of |keep1|; pass 2 writes dlogits = keep * a * dH/dz / kept[item].

// sigmoid(|t|) with the instructions of bernoulli_entropy_terms (the compiler shares them)
__device__ __forceinline__ float deyo_sigmoid_abs(float t) {
  const float e = __builtin_amdgcn_exp2f(-fabsf(t) * 1.4426950408889634f);
  return __builtin_amdgcn_rcpf(1.f + e);
}
// sigmoid(u), without a subtraction
__device__ __forceinline__ float deyo_sigmoid(float u) {
  const float e = __builtin_amdgcn_exp2f(-fabsf(u) * 1.4426950408889634f);
  const float r = __builtin_amdgcn_rcpf(1.f + e);
  return u >= 0.f ? r : e * r;
}

// Pass 1: fp64 block partials partial[item][0 / 1 / 2][block] = kept sum, |keep|, |keep1|.
__device__ __forceinline__ void deyo_store_partials(double acc, int cnt, int cnt1, double* partial, double* sh) {
  const double s = block_sum_d(acc, sh);
  __syncthreads();
  const double c = block_sum_d((double)cnt, sh);
  __syncthreads();
  const double c1 = block_sum_d((double)cnt1, sh);
  if (threadIdx.x == 0) {
    double* p = partial + (long long)blockIdx.y * 3 * gridDim.x;
    p[blockIdx.x] = s;
    p[gridDim.x + blockIdx.x] = c;
    p[2 * gridDim.x + blockIdx.x] = c1;
  }
}

struct DeyoArgs {
  float margin, margin0, threshold;
};

__global__ __launch_bounds__(256) void deyo_bernoulli_kernel(TV z, TV zs, TV dz, DeyoGrid pg, const int* __restrict__ table,
                                                             DeyoArgs a, unsigned char* kout, double* partial,
                                                             const long long* kept) {
  __shared__ double sh[4];
  const unsigned C = z.c, H = z.h, W = z.w;
  const unsigned total = (unsigned)z.d * H * W * C;
  const int* inv = table + ((long long)blockIdx.y * 2 + 1) * pg.P;
  z.p += (long long)blockIdx.y * z.sn;
  zs.p += (long long)blockIdx.y * zs.sn;
  kout += (long long)blockIdx.y * total;
  const bool grad = kept != nullptr;      // pass 2: kout is the mask pass 1 wrote
  if (grad) dz.p += (long long)blockIdx.y * dz.sn;
  const float scale = grad ? fent_scale(kept) : 0.f;
  double acc = 0.0;
  int cnt = 0, cnt1 = 0;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned vox = i / C, c = i - vox * C;
    const unsigned r = vox / W, x = vox - r * W;
    const unsigned zz = r / H, y = r - zz * H;
    unsigned iz, iy, ix;
    deyo_image(pg, inv, zz, y, x, iz, iy, ix);
    const float t = z.p[zz * z.sd + y * z.sh + x * z.sw + c];
    const float ts = zs.p[iz * zs.sd + iy * zs.sh + ix * zs.sw + c];
    const float e = expf(-fabsf(t));
    const float sig = t >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    const float softplus = fmaxf(t, 0.f) + log1pf(e);
    const float h = softplus - t * sig;
    const float u = t >= 0.f ? ts : -ts;
    const float eu = expf(-fabsf(u));
    const float plpd = 1.f / (1.f + e) - (u >= 0.f ? 1.f / (1.f + eu) : eu / (1.f + eu));
    const float wgt = expf(a.margin0 - fminf(h, a.margin)) + expf(plpd);
    if (grad) {
      dz.p[zz * dz.sd + y * dz.sh + x * dz.sw + c] = kout[i] ? wgt * (-t * sig * (1.f - sig)) * scale : 0.f;
      continue;
    }
    const bool keep1 = h < a.margin;
    const bool keep = keep1 && plpd > a.threshold;
    kout[i] = keep ? 1 : 0;
    cnt1 += keep1 ? 1 : 0;
    if (keep) { acc += (double)(wgt * h); ++cnt; }
  }
  if (!grad) deyo_store_partials(acc, cnt, cnt1, partial, sh);
}

// Fast path: <= 4 regions in dense 16-byte voxel rows of both logit tensors; a thread owns a voxel and reads one more row,
// the one of the mapped voxel.  OBF: bf16-stored gradient.
template <bool OBF>
__global__ __launch_bounds__(256) void deyo_bernoulli_vec_kernel(TV z, TV zs, TV dz, DeyoGrid pg, const int* __restrict__ table,
                                                                 DeyoArgs a, unsigned char* kout, double* partial,
                                                                 const long long* kept) {
  __shared__ double sh[4];
  const int C = z.c;
  const unsigned H = z.h, W = z.w;
  const unsigned total = (unsigned)z.d * H * W;
  const int* inv = table + ((long long)blockIdx.y * 2 + 1) * pg.P;
  z.p += (long long)blockIdx.y * z.sn;
  zs.p += (long long)blockIdx.y * zs.sn;
  kout += (long long)blockIdx.y * total * C;
  const bool grad = kept != nullptr;
  if (grad)
    dz.p = OBF ? reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(dz.p) + (long long)blockIdx.y * dz.sn)
               : dz.p + (long long)blockIdx.y * dz.sn;
  const float scale = grad ? fent_scale(kept) : 0.f;
  double acc = 0.0;
  int cnt = 0, cnt1 = 0;
  for (unsigned v = blockIdx.x * 256u + threadIdx.x; v < total; v += gridDim.x * 256u) {
    const unsigned r = v / W, x = v - r * W;
    const unsigned zz = r / H, y = r - zz * H;
    unsigned iz, iy, ix;
    deyo_image(pg, inv, zz, y, x, iz, iy, ix);
    const unsigned vs = (iz * H + iy) * W + ix;
    const float4 t4 = *reinterpret_cast<const float4*>(z.p + (long long)v * 4);
    const float4 s4 = *reinterpret_cast<const float4*>(zs.p + (long long)vs * 4);
    const float ts[4] = {t4.x, t4.y, t4.z, t4.w};
    const float ss[4] = {s4.x, s4.y, s4.z, s4.w};
    unsigned char km[4] = {0, 0, 0, 0};
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
        float hc, gc;
        bernoulli_entropy_terms(ts[c], hc, gc);
        const float plpd = deyo_sigmoid_abs(ts[c]) - deyo_sigmoid(ts[c] >= 0.f ? ss[c] : -ss[c]);
        const float wgt = __builtin_amdgcn_exp2f((a.margin0 - fminf(hc, a.margin)) * 1.4426950408889634f) +
                          __builtin_amdgcn_exp2f(plpd * 1.4426950408889634f);
        if (grad) {
          g[c] = km[c] ? wgt * gc * scale : 0.f;
        } else {
          const bool keep1 = hc < a.margin;
          const bool keep = keep1 && plpd > a.threshold;
          km[c] = keep ? 1 : 0;
          cnt1 += keep1 ? 1 : 0;
          if (keep) { h += wgt * hc; ++cnt; }
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
  if (!grad) deyo_store_partials(acc, cnt, cnt1, partial, sh);
}

// Categorical head: the element is the voxel, y^ the FIRST arg max of z, PLPD = softmax(z)[y^] - softmax(z'')[y^].
__global__ __launch_bounds__(256) void deyo_categorical_kernel(TV z, TV zs, TV dz, DeyoGrid pg, const int* __restrict__ table,
                                                               DeyoArgs a, unsigned char* kout, double* partial,
                                                               const long long* kept) {
  __shared__ double sh[4];
  const int R = z.c;
  const unsigned H = z.h, W = z.w;
  const unsigned total = (unsigned)z.d * H * W;
  const int* inv = table + ((long long)blockIdx.y * 2 + 1) * pg.P;
  z.p += (long long)blockIdx.y * z.sn;
  zs.p += (long long)blockIdx.y * zs.sn;
  kout += (long long)blockIdx.y * total;
  const bool grad = kept != nullptr;
  if (grad) dz.p += (long long)blockIdx.y * dz.sn;
  const float scale = grad ? fent_scale(kept) : 0.f;
  double acc = 0.0;
  int cnt = 0, cnt1 = 0;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned rr = i / W, x = i - rr * W;
    const unsigned zz = rr / H, y = rr - zz * H;
    unsigned iz, iy, ix;
    deyo_image(pg, inv, zz, y, x, iz, iy, ix);
    const float* zp = z.p + zz * z.sd + y * z.sh + x * z.sw;
    const float* sp = zs.p + iz * zs.sd + iy * zs.sh + ix * zs.sw;
    float t[DEYO_MAX_R], s[DEYO_MAX_R];
    float m = -INFINITY, ms = -INFINITY;
    int arg = 0;
#pragma unroll
    for (int r = 0; r < DEYO_MAX_R; ++r)
      if (r < R) {
        t[r] = zp[r];
        s[r] = sp[r];
        arg = t[r] > m ? r : arg;
        m = fmaxf(m, t[r]);
        ms = fmaxf(ms, s[r]);
      }
    float se = 0.f, ses = 0.f, sarg = 0.f;
#pragma unroll
    for (int r = 0; r < DEYO_MAX_R; ++r)
      if (r < R) {
        se += expf(t[r] - m);
        const float es = expf(s[r] - ms);
        ses += es;
        sarg = r == arg ? es : sarg;
      }
    const float lse = m + logf(se);
    float pz = 0.f;
#pragma unroll
    for (int r = 0; r < DEYO_MAX_R; ++r)
      if (r < R) pz += expf(t[r] - lse) * t[r];
    const float Hf = lse - pz;             // the filtered kernel's H: it decides keep1, bit for bit
    // loss, weight and gradient use H in the shifted form, as mmtta_entropy_weighted_items does (eata.hip has the account)
    const float lgs = logf(se);
    float pu = 0.f;
#pragma unroll
    for (int r = 0; r < DEYO_MAX_R; ++r)
      if (r < R) {
        const float u = t[r] - m;
        pu += expf(u - lgs) * u;
      }
    const float Hs = lgs - pu;
    const float plpd = 1.f / se - sarg / ses;      // softmax(z)[y^] = exp(0) / se
    const float wgt = expf(a.margin0 - fminf(Hs, a.margin)) + expf(plpd);
    if (grad) {
      float* gp = dz.p + zz * dz.sd + y * dz.sh + x * dz.sw;
      const bool keep = kout[i] != 0;
#pragma unroll
      for (int r = 0; r < DEYO_MAX_R; ++r)
        if (r < R) {
          const float logp = (t[r] - m) - lgs;
          gp[r] = keep ? wgt * (-expf(logp) * (logp + Hs)) * scale : 0.f;
        }
      continue;
    }
    const bool keep1 = Hf < a.margin;
    const bool keep = keep1 && plpd > a.threshold;
    kout[i] = keep ? 1 : 0;
    cnt1 += keep1 ? 1 : 0;
    if (keep) { acc += (double)(wgt * Hs); ++cnt; }
  }
  if (!grad) deyo_store_partials(acc, cnt, cnt1, partial, sh);
}

__global__ __launch_bounds__(64) void deyo_finish_kernel(const double* partial, int nblocks, float* loss, long long* kept,
                                                         long long* kept_entropy) {
  partial += (long long)blockIdx.x * 3 * nblocks;      // one workgroup per item
  double s = 0.0, c = 0.0, c1 = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 64) {
    s += partial[i];
    c += partial[nblocks + i];
    c1 += partial[2 * nblocks + i];
  }
  s = wave_sum_d(s);
  c = wave_sum_d(c);
  c1 = wave_sum_d(c1);
  if (threadIdx.x == 0) {
    kept[blockIdx.x] = (long long)c;
    kept_entropy[blockIdx.x] = (long long)c1;
    loss[blockIdx.x] = c > 0.0 ? (float)(s * (1.0 / c)) : __builtin_nanf("");
  }
}

static int deyo_blocks(const mmtta_tensor* z) {      // mmtta_entropy_filtered_partials' figure for ONE item
  const long long total = (long long)z->d * z->h * z->w * z->c;
  long long b = (total + 255) / 256;
  if (b < 1) b = 1;
  if (b > DEYO_MAX_BLOCKS) b = DEYO_MAX_BLOCKS;
  return (int)b;
}

static bool deyo_dense16(const mmtta_tensor* t) {
  return t->sc == 1 && t->sw == 4 && t->sh == (int64_t)t->w * 4 && t->sd == (int64_t)t->h * t->sh && t->sn % 4 == 0 &&
         ((uintptr_t)t->ptr) % 16 == 0;
}

// every offset inside one item fits 31 bits (the kernels index voxels with 32-bit arithmetic)
static bool deyo_small_item(const mmtta_tensor* t) {
  const long long ld = t->sw > t->c ? t->sw : t->c;
  return t->d > 0 && t->h > 0 && t->w > 0 && t->c > 0 && (long long)t->d * t->h * t->w * (ld > 4 ? ld : 4) < (1ll << 31) &&
         item_fits_31(t, ld);
}

// The patch grid of a call against the extents of `t`: counts >= 1 that divide them, 2 <= P <= DEYO_MAX_PATCHES.
static int deyo_grid_check(const char* what, const int32_t* grid, const mmtta_tensor* t, DeyoGrid& g) {
  MMTTA_CHECK(grid != nullptr, MMTTA_ERR_INVALID, "%s: null patch grid", what);
  MMTTA_CHECK(grid[0] >= 1 && grid[1] >= 1 && grid[2] >= 1 && grid[0] <= DEYO_MAX_PATCHES && grid[1] <= DEYO_MAX_PATCHES &&
                  grid[2] <= DEYO_MAX_PATCHES,
              MMTTA_ERR_INVALID, "%s: patch grid [%d, %d, %d] (counts of 1 .. %d)", what, grid[0], grid[1], grid[2],
              DEYO_MAX_PATCHES);
  const long long P = (long long)grid[0] * grid[1] * grid[2];
  MMTTA_CHECK(P >= 2 && P <= DEYO_MAX_PATCHES, MMTTA_ERR_INVALID, "%s: patch grid [%d, %d, %d] has %lld patches (2 .. %d)", what,
              grid[0], grid[1], grid[2], P, DEYO_MAX_PATCHES);
  MMTTA_CHECK(t->d >= 1 && t->h >= 1 && t->w >= 1 && t->d % grid[0] == 0 && t->h % grid[1] == 0 && t->w % grid[2] == 0,
              MMTTA_ERR_INVALID, "%s: patch grid [%d, %d, %d] does not divide the extents (%d, %d, %d)", what, grid[0], grid[1],
              grid[2], t->d, t->h, t->w);
  g.gd = grid[0]; g.gh = grid[1]; g.gw = grid[2];
  g.pd = t->d / grid[0]; g.ph = t->h / grid[1]; g.pw = t->w / grid[2];
  g.P = (int)P;
  return MMTTA_OK;
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int mmtta_patch_shuffle(const mmtta_tensor* x, const mmtta_tensor* y, const int32_t* grid, const int32_t* table,
                                   void* stream) {
  MMTTA_CHECK(x && y && x->ptr && y->ptr && table, MMTTA_ERR_INVALID, "patch shuffle: null argument");
  MMTTA_CHECK(same_shape(x, y) && x->dtype == y->dtype && x->n >= 1 && x->c >= 1, MMTTA_ERR_INVALID,
              "patch shuffle: shape mismatch");
  DeyoGrid pg;
  int st = deyo_grid_check("patch shuffle", grid, x, pg);
  if (st) return st;
  MMTTA_CHECK(x->dtype == MMTTA_F32 || x->dtype == MMTTA_BF16, MMTTA_ERR_UNSUPPORTED, "patch shuffle: fp32 or bf16 rows");
  auto dense = [](const mmtta_tensor* t) {
    return t->sc == 1 && t->sw >= t->c && t->sh == (int64_t)t->w * t->sw && t->sd == (int64_t)t->h * t->sh &&
           (t->n == 1 || t->sn >= (int64_t)t->d * t->sd);
  };
  MMTTA_CHECK(dense(x) && dense(y) && x->sw == y->sw, MMTTA_ERR_UNSUPPORTED, "patch shuffle: dense channels-last rows of one width");
  MMTTA_CHECK(y->sw == y->c || (y->flags & MMTTA_TENSOR_OWNS_PAD), MMTTA_ERR_UNSUPPORTED,
              "patch shuffle: `y` must own the pad lanes of its rows");
  MMTTA_CHECK(deyo_small_item(x), MMTTA_ERR_UNSUPPORTED, "patch shuffle: an item of 2^31 elements or more");
  MMTTA_CHECK(x->n <= DEYO_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "patch shuffle: more than %d items in one call", DEYO_MAX_GRID_Y);
  const long long esz = x->dtype == MMTTA_BF16 ? 2 : 4;
  {
    // a patch of the output is read from another patch of the input: the two may not share memory
    const uintptr_t xb = (uintptr_t)x->ptr, yb = (uintptr_t)y->ptr;
    const uintptr_t xe = xb + (uintptr_t)(((long long)(x->n - 1) * x->sn + (long long)x->d * x->sd) * esz);
    const uintptr_t ye = yb + (uintptr_t)(((long long)(y->n - 1) * y->sn + (long long)y->d * y->sd) * esz);
    MMTTA_CHECK(xe <= yb || ye <= xb, MMTTA_ERR_INVALID, "patch shuffle: in-place call (`x` and `y` overlap)");
  }
  const long long row = x->sw * esz;
  const uintptr_t both = (uintptr_t)x->ptr | (uintptr_t)y->ptr | (uintptr_t)(x->sn * esz) | (uintptr_t)(y->sn * esz) | (uintptr_t)row;
  const int unit = both % 16 == 0 ? 16 : (both % 8 == 0 ? 8 : (both % 4 == 0 ? 4 : 2));
  MMTTA_CHECK(unit >= esz && both % esz == 0, MMTTA_ERR_UNSUPPORTED, "patch shuffle: misaligned tensor");
  hipStream_t s = (hipStream_t)stream;
  const unsigned upr = (unsigned)(row / unit);
  const long long units = (long long)x->d * x->h * x->w * upr;
  long long b = (units + 255) / 256;
  if (b > 4096) b = 4096;
  const dim3 launch((unsigned)b, x->n);
  const long long xsn = x->sn * esz / unit, ysn = y->sn * esz / unit;
  const unsigned D = x->d, H = x->h, W = x->w;
#define DEYO_SHUFFLE(T) \
  hipLaunchKernelGGL((deyo_shuffle_kernel<T>), launch, dim3(256), 0, s, (const T*)x->ptr, (T*)y->ptr, xsn, ysn, upr, D, H, W, pg, (const int*)table)
  if (unit == 16) DEYO_SHUFFLE(uint4);
  else if (unit == 8) DEYO_SHUFFLE(uint2);
  else if (unit == 4) DEYO_SHUFFLE(unsigned);
  else DEYO_SHUFFLE(unsigned short);
#undef DEYO_SHUFFLE
  return launch_status("patch shuffle");
}

extern "C" int64_t mmtta_deyo_partials(const mmtta_tensor* logits) {
  if (logits == nullptr || logits->n < 1) return -1;
  return 3 * (int64_t)deyo_blocks(logits) * logits->n;
}

extern "C" int mmtta_deyo_loss_items(const mmtta_tensor* logits, const mmtta_tensor* logits_shuffled, const int32_t* grid,
                                     const int32_t* table, int softmax, float margin, float margin0, float plpd_threshold,
                                     uint8_t* keep_out, const mmtta_tensor* dlogits, double* partial, float* loss, int64_t* kept,
                                     int64_t* kept_entropy, void* stream) {
  MMTTA_CHECK(__builtin_isfinite(margin) && margin > 0.f, MMTTA_ERR_INVALID,
              "deyo loss: margin must be finite and positive, got %g", (double)margin);
  MMTTA_CHECK(__builtin_isfinite(margin0) && margin0 > 0.f, MMTTA_ERR_INVALID,
              "deyo loss: margin0 must be finite and positive, got %g", (double)margin0);
  MMTTA_CHECK(__builtin_isfinite(plpd_threshold) && plpd_threshold >= -1.f && plpd_threshold < 1.f, MMTTA_ERR_INVALID,
              "deyo loss: plpd_threshold must be finite with -1 <= threshold < 1, got %g", (double)plpd_threshold);
  MMTTA_CHECK(keep_out != nullptr, MMTTA_ERR_INVALID, "deyo loss: null mask output");
  MMTTA_CHECK(logits && logits_shuffled && dlogits && table && partial && loss && kept && kept_entropy && logits->ptr &&
                  logits_shuffled->ptr && dlogits->ptr,
              MMTTA_ERR_INVALID, "deyo loss: null argument");
  MMTTA_CHECK(same_shape(logits, dlogits) && same_shape(logits, logits_shuffled) && logits->n >= 1 && logits->c >= 1 &&
                  logits->d >= 1 && logits->h >= 1 && logits->w >= 1,
              MMTTA_ERR_INVALID, "deyo loss: shape mismatch");
  DeyoGrid pg;
  int st = deyo_grid_check("deyo loss", grid, logits, pg);
  if (st) return st;
  MMTTA_CHECK(logits->dtype == MMTTA_F32 && logits_shuffled->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED,
              "deyo loss: `logits` and `logits_shuffled` must be fp32-stored");
  MMTTA_CHECK(is_cl(logits) && is_cl(logits_shuffled) && is_cl(dlogits), MMTTA_ERR_UNSUPPORTED, "deyo loss: channels-last only");
  MMTTA_CHECK(deyo_small_item(logits) && deyo_small_item(logits_shuffled) && deyo_small_item(dlogits), MMTTA_ERR_UNSUPPORTED,
              "deyo loss: an item of 2^31 elements or more");
  MMTTA_CHECK(logits->n <= DEYO_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "deyo loss: more than %d items in one call", DEYO_MAX_GRID_Y);
  hipStream_t s = (hipStream_t)stream;
  const int items = logits->n;
  const int blocks = deyo_blocks(logits);
  const dim3 launch(blocks, items);
  const long long* kd = (const long long*)kept;
  const int* tb = (const int*)table;
  const DeyoArgs a = {margin, margin0, plpd_threshold};
  if (!softmax) {
    const bool vec = logits->c <= 4 && deyo_dense16(logits) && deyo_dense16(logits_shuffled) && deyo_dense16(dlogits) &&
                     ((dlogits->flags & MMTTA_TENSOR_OWNS_PAD) || dlogits->c == 4);
    MMTTA_CHECK(is_f32(dlogits) || vec, MMTTA_ERR_UNSUPPORTED,
                "deyo loss: a bf16-stored `dlogits` needs dense 4-channel voxel rows that own their pad");
    auto run = [&](double* part, const long long* kk) {
      if (vec && is_bf16(dlogits))
        hipLaunchKernelGGL(deyo_bernoulli_vec_kernel<true>, launch, dim3(256), 0, s, tv(logits), tv(logits_shuffled), tv(dlogits),
                           pg, tb, a, keep_out, part, kk);
      else if (vec)
        hipLaunchKernelGGL(deyo_bernoulli_vec_kernel<false>, launch, dim3(256), 0, s, tv(logits), tv(logits_shuffled), tv(dlogits),
                           pg, tb, a, keep_out, part, kk);
      else
        hipLaunchKernelGGL(deyo_bernoulli_kernel, launch, dim3(256), 0, s, tv(logits), tv(logits_shuffled), tv(dlogits), pg, tb, a,
                           keep_out, part, kk);
    };
    run(partial, nullptr);
    st = launch_status("deyo loss bernoulli");
    if (st) return st;
    hipLaunchKernelGGL(deyo_finish_kernel, dim3(items), dim3(64), 0, s, (const double*)partial, blocks, loss, (long long*)kept,
                       (long long*)kept_entropy);
    st = launch_status("deyo loss finish");
    if (st) return st;
    run(nullptr, kd);
    return launch_status("deyo loss bernoulli gradient");
  }
  MMTTA_CHECK(logits->c <= DEYO_MAX_R, MMTTA_ERR_UNSUPPORTED, "deyo loss softmax: more than %d classes", DEYO_MAX_R);
  MMTTA_CHECK(is_f32(dlogits), MMTTA_ERR_UNSUPPORTED, "deyo loss softmax: `dlogits` must be fp32-stored");
  hipLaunchKernelGGL(deyo_categorical_kernel, launch, dim3(256), 0, s, tv(logits), tv(logits_shuffled), tv(dlogits), pg, tb, a,
                     keep_out, partial, (const long long*)nullptr);
  st = launch_status("deyo loss categorical");
  if (st) return st;
  hipLaunchKernelGGL(deyo_finish_kernel, dim3(items), dim3(64), 0, s, (const double*)partial, blocks, loss, (long long*)kept,
                     (long long*)kept_entropy);
  st = launch_status("deyo loss finish");
  if (st) return st;
  hipLaunchKernelGGL(deyo_categorical_kernel, launch, dim3(256), 0, s, tv(logits), tv(logits_shuffled), tv(dlogits), pg, tb, a,
                     keep_out, (double*)nullptr, kd);
  return launch_status("deyo loss categorical gradient");
}
