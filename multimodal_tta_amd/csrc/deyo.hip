// DeYO (Lee et al., ICLR 2024, "Entropy is not Enough for Test-Time Adaptation") on gfx950: the patch-shuffled copy of a
// staged volume and the reliable entropy that is filtered and weighted by the pseudo-label probability difference (PLPD)
// between the logits of the volume and the logits of its shuffled copy.  Both are HBM-bound streams.  See include/mmtta.h
// for the contracts.
#include "voxel_loss.h"

namespace mmtta {

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
// The filtered walk of voxel_loss.h with three partial rows, hence the launch geometry and the mask layout of
// mmtta_entropy_weighted_items (eata.hip) and of mmtta_entropy_filtered_items, over the same entropy definitions: keep1 =
// H < margin and its count are those entry points'.  The second operand z'' is read from the shuffled logits at the mapped
// voxel (the inverse row of the table).  Pass 1 leaves the keep bytes and fp64 block partials of the kept sum of a H, of
// |keep| and of |keep1|; pass 2 writes dlogits = keep * a * dH/dz / kept[item].
struct DeyoLoss {
  static constexpr int ROWS = 3;
  float margin, margin0, threshold;
  TV zs;
  DeyoGrid pg;
  const int* inv;      // the call's table; item() moves it to the item's inverse row
  __device__ __forceinline__ void item(int n, long long) {
    zs.p += (long long)n * zs.sn;
    inv += ((long long)n * 2 + 1) * pg.P;
  }
  __device__ __forceinline__ bool allowed(long long) const { return true; }
  __device__ __forceinline__ long long mapped(unsigned z, unsigned y, unsigned x) const {
    unsigned iz, iy, ix;
    deyo_image(pg, inv, z, y, x, iz, iy, ix);
    return iz * zs.sd + iy * zs.sh + ix * zs.sw;
  }
  // dense rows: one more 16-byte load, the row of the mapped voxel
  __device__ __forceinline__ float4 row(unsigned v) const {
    const unsigned H = zs.h, W = zs.w;
    const unsigned r = v / W, x = v - r * W;
    const unsigned zz = r / H, y = r - zz * H;
    unsigned iz, iy, ix;
    deyo_image(pg, inv, zz, y, x, iz, iy, ix);
    const unsigned vs = (iz * H + iy) * W + ix;
    return *reinterpret_cast<const float4*>(zs.p + (long long)vs * 4);
  }
  __device__ __forceinline__ float at(const VoxPos& p, int c) const { return zs.p[mapped(p.z, p.y, p.x) + c]; }
  __device__ __forceinline__ const float* vox(const VoxPos& p) const { return zs.p + mapped(p.z, p.y, p.x); }

  __device__ __forceinline__ KeptTerms fast(float t, float s) const {
    float h, g;
    bernoulli_entropy_terms(t, h, g);
    const float u = t >= 0.f ? s : -s;
    const float plpd = sigmoid_pair(t, exp_neg_abs(t)).r - sigmoid_pair(u, exp_neg_abs(u)).p;      // sigmoid(|t|) - sigmoid(u)
    const float wgt = exp_fast(margin0 - fminf(h, margin)) + exp_fast(plpd);
    return {h, wgt * h, wgt * g, plpd > threshold};
  }
  __device__ __forceinline__ KeptTerms generic(float t, float s) const {
    const BernoulliLibm b = bernoulli_entropy_libm(t);
    const float u = t >= 0.f ? s : -s;
    const float eu = expf(-fabsf(u));
    const float plpd = 1.f / (1.f + b.e) - (u >= 0.f ? 1.f / (1.f + eu) : eu / (1.f + eu));
    const float wgt = expf(margin0 - fminf(b.h, margin)) + expf(plpd);
    return {b.h, wgt * b.h, wgt * b.g, plpd > threshold};
  }
  // Categorical head: the element is the voxel, y^ the FIRST arg max of z, PLPD = softmax(z)[y^] - softmax(z'')[y^].
  template <class F>
  __device__ __forceinline__ KeptTerms categorical(const float* zp, const float* sp, int R, F&& put) const {
    CategoricalVoxel v;
    categorical_entropy<true>(zp, R, v);
    const int arg = categorical_argmax(v, R);
    float s[LOSS_MAX_R];
    float ms = -INFINITY;
#pragma unroll
    for (int r = 0; r < LOSS_MAX_R; ++r)
      if (r < R) { s[r] = sp[r]; ms = fmaxf(ms, s[r]); }
    float ses = 0.f, sarg = 0.f;
#pragma unroll
    for (int r = 0; r < LOSS_MAX_R; ++r)
      if (r < R) {
        const float es = expf(s[r] - ms);
        ses += es;
        sarg = r == arg ? es : sarg;
      }
    const float plpd = 1.f / v.se - sarg / ses;      // softmax(z)[y^] = exp(0) / se
    const float wgt = expf(margin0 - fminf(v.Hs, margin)) + expf(plpd);
#pragma unroll
    for (int r = 0; r < LOSS_MAX_R; ++r)
      if (r < R) put(r, wgt * categorical_entropy_grad<true>(v, r));
    return {v.H, wgt * v.Hs, 0.f, plpd > threshold};
  }
};

// every offset inside one item fits 31 bits, the last voxel's included (the patch map reaches any voxel of the item)
static bool deyo_small_item(const mmtta_tensor* t) {
  return loss_small_item(t) && item_fits_31(t, t->sw > t->c ? t->sw : t->c);
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
  MMTTA_CHECK(x->n <= LOSS_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "patch shuffle: more than %d items in one call", LOSS_MAX_GRID_Y);
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
  return 3 * (int64_t)loss_blocks(logits) * logits->n;
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
  MMTTA_CHECK(logits->n <= LOSS_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "deyo loss: more than %d items in one call", LOSS_MAX_GRID_Y);
  DeyoLoss p = {margin, margin0, plpd_threshold, tv(logits_shuffled), pg, (const int*)table};
  return kept_launch<DeyoLoss, unsigned>({"deyo loss", "deyo loss", "deyo loss"}, logits, dlogits, softmax,
                                         loss_vec(logits, dlogits, logits_shuffled), keep_out, partial, loss, (long long*)kept,
                                         (long long*)kept_entropy, p, (hipStream_t)stream);
}
