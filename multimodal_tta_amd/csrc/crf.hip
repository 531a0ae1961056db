// CRF-regularised entropy on gfx950: the entropy objective of the adaptation step plus a pairwise grid-CRF (Potts) term over
// the 6 / 18 / 26 spatial neighbours (Tang et al., ECCV 2018, "On Regularized Losses for Weakly-supervised CNN Segmentation";
// the contour term of Hu et al., MICCAI 2021), loss and gradient in ONE pass over the logits:
//   L = H + weight * P,   P = 1 / (2 n E) sum_i sum_{j in N(i)} a_ij phi(p_i, p_j),   a_ij as in lame.hip.
// The gradient is a gather: every voxel needs the same stencil sums as its share of P (sum_j a_ij, sum_j a_ij p_j or
// sum_j a_ij (p_i - p_j)), so nothing is scattered and nothing is added atomically.  Two launches: the main pass (fp64 block
// partials of H and P, the whole gradient) and a per-item finish.  See include/mmtta.h for the contract.
#include "voxel_loss.h"

namespace mmtta {

constexpr int CRF_MAX_R = LOSS_MAX_R;     // regions / input channels of the generic path
constexpr int CRF_MAX_GRID_Y = 65535;     // gridDim.y carries the item
// The tile of the fast path is lame.hip's: 4 x 8 x 32 voxels per 256-thread workgroup (a thread owns one (y, x) column of 4),
// staged with a one-voxel halo as 6 x 10 x 34 rows of 16 bytes: 32,640 B of p and as many of x - two workgroups of the affinity
// form per CU, five of the sigma = 0 form.  A lane group of ds_read_b128 reads 16 consecutive rows (no conflicts).
constexpr int CRF_TD = 4, CRF_TH = 8, CRF_TW = 32;
constexpr int CRF_HD = CRF_TD + 2, CRF_HH = CRF_TH + 2, CRF_HW = CRF_TW + 2;
constexpr int CRF_HALO = CRF_HD * CRF_HH * CRF_HW;

// p of one voxel row of <= 4 regions (lanes >= R come out 0, whatever the pad holds: a 0 lane adds nothing to phi)
template <bool SOFTMAX>
__device__ __forceinline__ float4 crf_p4(float4 l, int R) {
  if (!SOFTMAX) {
    auto sg = [](float t) { return sigmoid_pair(t, exp_neg_abs(t)).p; };
    return make_float4(sg(l.x), R > 1 ? sg(l.y) : 0.f, R > 2 ? sg(l.z) : 0.f, R > 3 ? sg(l.w) : 0.f);
  }
  float m = l.x;
  if (R > 1) m = fmaxf(m, l.y);
  if (R > 2) m = fmaxf(m, l.z);
  if (R > 3) m = fmaxf(m, l.w);
  const float ex = exp_fast(l.x - m);
  const float ey = R > 1 ? exp_fast(l.y - m) : 0.f;
  const float ez = R > 2 ? exp_fast(l.z - m) : 0.f;
  const float ew = R > 3 ? exp_fast(l.w - m) : 0.f;
  const float s = (ex + ey) + (ez + ew);
  return make_float4(ex / s, ey / s, ez / s, ew / s);
}

// block partials partial[item][0][block] (entropy sum) and partial[item][1][block] (pair sum)
__device__ __forceinline__ void crf_store_partials(double hs, double ps, double* partial, double* sh) {
  const double h = block_sum_d(hs, sh);
  __syncthreads();
  const double p = block_sum_d(ps, sh);
  if (threadIdx.x == 0) {
    double* q = partial + (long long)blockIdx.y * 2 * gridDim.x;
    q[blockIdx.x] = h;
    q[gridDim.x + blockIdx.x] = p;
  }
}

struct CrfArgs {
  const float* l;        // logits: never written
  float* dl;             // dlogits (fp32 or bf16 elements)
  const float* x;        // staged input (fp32 or bf16 elements), null when sigma == 0
  long long lsn, dsn, xsn;      // item strides in elements
  int D, H, W, R;
  unsigned mask;         // present channels, already cut to the C channels of x
  int maxl1;             // |d|_1 <= 1 / 2 / 3 for connectivity 6 / 18 / 26
  float inv_e, cw, negk; // 1 / E;  weight / (n E);  -log2(e) / (2 sigma^2)
  int full_rows;         // dl rows are stored as one 16- / 8-byte access (R == 4 or the view owns its pad: pad lanes get 0)
  int tiles_x, tiles_y;
  double* partial;
};

// ------------------------------------------------------------------ tiled fast path: R <= 4, C <= 4, 16-byte logit rows
// FORM 0: Potts (the stencil sums are sum_j a_ij and sum_j a_ij p_j), 1: quadratic (sum_j a_ij (p_i - p_j) and its square
// form, taken as differences: equal neighbours give an exact 0).
template <bool AFF, bool SOFTMAX, bool XBF, bool OBF, int FORM>
__global__ __launch_bounds__(256) void crf_tiled_kernel(CrfArgs a) {
  __shared__ float4 ps[CRF_HALO];
  __shared__ float4 xs[AFF ? CRF_HALO : 1];
  __shared__ double shd[4];
  const int D = a.D, H = a.H, W = a.W, R = a.R;
  unsigned t = blockIdx.x;
  const int bx = (int)(t % (unsigned)a.tiles_x);
  t /= (unsigned)a.tiles_x;
  const int by = (int)(t % (unsigned)a.tiles_y), bz = (int)(t / (unsigned)a.tiles_y);
  const int x0 = bx * CRF_TW, y0 = by * CRF_TH, z0 = bz * CRF_TD;
  const float* lp = a.l + (long long)blockIdx.y * a.lsn;
  float* dl = grad_item<OBF>(a.dl, blockIdx.y, a.dsn);
  const float* xb = AFF ? item_base<XBF>(a.x, blockIdx.y, a.xsn) : nullptr;

  // stage p and x with the halo; a voxel outside the volume is p = 0, x = 0 and is kept out by its coordinates below
  for (int h = threadIdx.x; h < CRF_HALO; h += 256) {
    const int hx = h % CRF_HW, hr = h / CRF_HW;
    const int hy = hr % CRF_HH, hz = hr / CRF_HH;
    const int gx = x0 - 1 + hx, gy = y0 - 1 + hy, gz = z0 - 1 + hz;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f), xv = p;
    if ((unsigned)gx < (unsigned)W && (unsigned)gy < (unsigned)H && (unsigned)gz < (unsigned)D) {
      const unsigned v = ((unsigned)gz * H + gy) * W + gx;      // * 4 < 2^31: checked on the host
      p = crf_p4<SOFTMAX>(*reinterpret_cast<const float4*>(lp + v * 4u), R);
      if (AFF) {
        const float4 q = ld4_t<XBF>(xb, v * 4u);
        xv = make_float4((a.mask & 1u) ? q.x : 0.f, (a.mask & 2u) ? q.y : 0.f, (a.mask & 4u) ? q.z : 0.f,
                         (a.mask & 8u) ? q.w : 0.f);      // absent channels and pad lanes: no difference
      }
    }
    ps[h] = p;
    if (AFF) xs[h] = xv;
  }
  __syncthreads();

  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int gx = x0 + tx, gy = y0 + ty;
  double hsum = 0.0, psum = 0.0;
  if (gx < W && gy < H) {
    const bool xok[3] = {gx > 0, true, gx + 1 < W}, yok[3] = {gy > 0, true, gy + 1 < H};
    for (int tz = 0; tz < CRF_TD; ++tz) {
      const int gz = z0 + tz;
      if (gz >= D) break;
      const bool zok[3] = {gz > 0, true, gz + 1 < D};
      const int c = ((tz + 1) * CRF_HH + ty + 1) * CRF_HW + tx + 1;
      const float4 pi = ps[c];
      float4 xi = make_float4(0.f, 0.f, 0.f, 0.f);
      if (AFF) xi = xs[c];
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);      // sum_j a_ij p_j (Potts) or sum_j a_ij (p_i - p_j) (quadratic)
      float sw = 0.f, sq = 0.f;                          // sum_j a_ij;  sum_j a_ij |p_i - p_j|^2
#pragma unroll
      for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const int l1 = (dz != 0) + (dy != 0) + (dx != 0);
            if (l1 == 0 || l1 > a.maxl1) continue;      // (wave-uniform)
            const int j = c + (dz * CRF_HH + dy) * CRF_HW + dx;
            const float4 pj = ps[j];
            float w = 1.f;
            if (AFF) {
              const float4 xj = xs[j];
              const float ex = xi.x - xj.x, ey = xi.y - xj.y, ez = xi.z - xj.z, ew = xi.w - xj.w;
              const float d2 = fmaf(ew, ew, fmaf(ez, ez, fmaf(ey, ey, ex * ex)));
              w = __builtin_amdgcn_exp2f(d2 * a.negk);
            }
            w = (zok[dz + 1] && yok[dy + 1] && xok[dx + 1]) ? w : 0.f;      // a neighbour outside the volume adds nothing
            if (FORM == 0) {
              sw += w;
              acc.x = fmaf(w, pj.x, acc.x);
              acc.y = fmaf(w, pj.y, acc.y);
              acc.z = fmaf(w, pj.z, acc.z);
              acc.w = fmaf(w, pj.w, acc.w);
            } else {
              const float ex = pi.x - pj.x, ey = pi.y - pj.y, ez = pi.z - pj.z, ew = pi.w - pj.w;
              acc.x = fmaf(w, ex, acc.x);
              acc.y = fmaf(w, ey, acc.y);
              acc.z = fmaf(w, ez, acc.z);
              acc.w = fmaf(w, ew, acc.w);
              sq = fmaf(w, fmaf(ew, ew, fmaf(ez, ez, fmaf(ey, ey, ex * ex))), sq);
            }
          }
      const float pv[4] = {pi.x, pi.y, pi.z, pi.w}, av[4] = {acc.x, acc.y, acc.z, acc.w};
      // g = dP/dp of the voxel's lanes (before the weight / (n E) scale) and the voxel's share phi of the pair sum
      float g[4], phi;
      if (FORM == 1) {
        phi = sq;
#pragma unroll
        for (int r = 0; r < 4; ++r) g[r] = 2.f * av[r];
      } else if (SOFTMAX) {
        phi = sw - (fmaf(pv[0], av[0], pv[1] * av[1]) + fmaf(pv[2], av[2], pv[3] * av[3]));
#pragma unroll
        for (int r = 0; r < 4; ++r) g[r] = -av[r];
      } else {
        // sum_j a [p (1 - q) + (1 - p) q] = p sum_j a + (1 - 2 p) sum_j a q; pad lanes hold p = 0 and sum a q = 0
        phi = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          phi += fmaf(pv[r], sw, fmaf(-2.f * pv[r], av[r], av[r]));
          g[r] = fmaf(-2.f, av[r], sw);
        }
      }
      const unsigned v = ((unsigned)gz * H + gy) * W + gx;
      const float4 t4 = *reinterpret_cast<const float4*>(lp + v * 4u);
      const float ts[4] = {t4.x, t4.y, t4.z, t4.w};
      float o[4] = {0.f, 0.f, 0.f, 0.f};
      float hv = 0.f;
      if (!SOFTMAX) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (r < R) {
            float hr, gh;
            bernoulli_entropy_terms(ts[r], hr, gh);
            const SigmoidPair s = sigmoid_pair(ts[r], exp_neg_abs(ts[r]));
            hv += hr;
            o[r] = fmaf(a.cw * g[r], s.er * s.r, gh * a.inv_e);      // dP/dl = g p (1 - p)
          }
      } else {
        // the shifted form Hs = log se - sum p u: lse - sum p z carries the rounding of the largest logit (voxel_loss.h)
        CategoricalVoxel cv;
        categorical_entropy<true>(ts, R, cv);
        hv = cv.Hs;
        const float pg = fmaf(pv[0], g[0], pv[1] * g[1]) + fmaf(pv[2], g[2], pv[3] * g[3]);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (r < R) o[r] = fmaf(a.cw * pv[r], g[r] - pg, categorical_entropy_grad<true>(cv, r) * a.inv_e);
      }
      hsum += (double)hv;
      psum += (double)phi;
      if (a.full_rows) {
        st4_t<OBF>(dl, v * 4u, make_float4(o[0], o[1], o[2], o[3]));
      } else {
        st1_t<OBF>(dl, v * 4u, o[0]);
        if (R > 1) st1_t<OBF>(dl, v * 4u + 1, o[1]);
        if (R > 2) st1_t<OBF>(dl, v * 4u + 2, o[2]);
      }
    }
  }
  crf_store_partials(hsum, psum, a.partial, shd);
}

// ------------------------------------------------------------------ generic path: R <= 16, C <= 16, any channels-last rows
// One thread per voxel; the neighbours' p is recomputed from the logits in global memory (the rows come from L2); libm forms.
__device__ __forceinline__ float crf_sigmoid_libm(float t) {
  const float e = expf(-fabsf(t));
  return t >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

__global__ __launch_bounds__(256) void crf_generic_kernel(TV l, TV dl, TV x, int aff, int softmax, int form, unsigned mask, int maxl1,
                                                          float inv_e, float cw, float negk, double* partial) {
  __shared__ double shd[4];
  const int D = l.d, H = l.h, W = l.w, R = l.c, C = aff ? x.c : 0;
  const unsigned total = (unsigned)D * H * W;      // < 2^31: checked on the host
  const unsigned v = blockIdx.x * 256u + threadIdx.x;
  const float* lp = l.p + (long long)blockIdx.y * l.sn;
  float* dp = dl.p + (long long)blockIdx.y * dl.sn;
  const long long xitem = aff ? (long long)blockIdx.y * x.sn : 0;
  double hsum = 0.0, psum = 0.0;
  if (v < total) {
    const int gx = (int)(v % (unsigned)W), rr = (int)(v / (unsigned)W);
    const int gy = rr % H, gz = rr / H;
    const float* zp = lp + gz * l.sd + gy * l.sh + gx * l.sw;
    // the voxel's own p, entropy and entropy gradient
    float pi[CRF_MAX_R], gh[CRF_MAX_R], pq[CRF_MAX_R], acc[CRF_MAX_R], xi[CRF_MAX_R];
    float hv = 0.f;
    if (softmax) {
      CategoricalVoxel cv;
      categorical_entropy<true>(zp, R, cv);      // the shifted form, as in the tiled kernel
      hv = cv.Hs;
#pragma unroll
      for (int r = 0; r < CRF_MAX_R; ++r) {
        pi[r] = gh[r] = pq[r] = 0.f;
        if (r < R) {
          pi[r] = expf(cv.t[r] - cv.m) / cv.se;      // the form the neighbours' p takes below: equal logits, equal bits
          gh[r] = categorical_entropy_grad<true>(cv, r);
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < CRF_MAX_R; ++r) {
        pi[r] = gh[r] = pq[r] = 0.f;
        if (r < R) {
          const BernoulliLibm b = bernoulli_entropy_libm(zp[r]);
          hv += b.h;
          pi[r] = b.sig;
          gh[r] = b.g;
          pq[r] = b.sig * (1.f - b.sig);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < CRF_MAX_R; ++c) {
      acc[c] = 0.f;
      xi[c] = 0.f;
      if (c < C && ((mask >> c) & 1u)) xi[c] = ld1_any(x.p, xitem + gz * x.sd + gy * x.sh + gx * x.sw + c, x.bf);
    }
    float sw = 0.f, sq = 0.f;
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
        for (int c = 0; c < CRF_MAX_R; ++c)
          if (c < C && ((mask >> c) & 1u)) {
            const float e = xi[c] - ld1_any(x.p, xo + c, x.bf);
            d2 = fmaf(e, e, d2);
          }
        w = __builtin_amdgcn_exp2f(d2 * negk);
      }
      const float* np = lp + nz * l.sd + ny * l.sh + nx * l.sw;
      float pj[CRF_MAX_R];
      if (softmax) {
        CategoricalVoxel nv;
        categorical_load(np, R, nv);
#pragma unroll
        for (int r = 0; r < CRF_MAX_R; ++r) pj[r] = r < R ? expf(nv.t[r] - nv.m) / nv.se : 0.f;
      } else {
#pragma unroll
        for (int r = 0; r < CRF_MAX_R; ++r) pj[r] = r < R ? crf_sigmoid_libm(np[r]) : 0.f;
      }
      sw += w;
#pragma unroll
      for (int r = 0; r < CRF_MAX_R; ++r)
        if (r < R) {
          if (form == 0) {
            acc[r] = fmaf(w, pj[r], acc[r]);
          } else {
            const float e = pi[r] - pj[r];
            acc[r] = fmaf(w, e, acc[r]);
            sq = fmaf(w * e, e, sq);
          }
        }
    }
    float g[CRF_MAX_R];
    float phi = form == 1 ? sq : (softmax ? sw : 0.f), pg = 0.f;
#pragma unroll
    for (int r = 0; r < CRF_MAX_R; ++r) {
      g[r] = 0.f;
      if (r < R) {
        if (form == 1) {
          g[r] = 2.f * acc[r];
        } else if (softmax) {
          phi -= pi[r] * acc[r];
          g[r] = -acc[r];
        } else {
          phi += fmaf(pi[r], sw, fmaf(-2.f * pi[r], acc[r], acc[r]));
          g[r] = fmaf(-2.f, acc[r], sw);
        }
        pg = fmaf(pi[r], g[r], pg);
      }
    }
    float* op = dp + gz * dl.sd + gy * dl.sh + gx * dl.sw;
#pragma unroll
    for (int r = 0; r < CRF_MAX_R; ++r)
      if (r < R)      // pad lanes are left as they are
        op[r] = softmax ? fmaf(cw * pi[r], g[r] - pg, gh[r] * inv_e) : fmaf(cw * g[r], pq[r], gh[r] * inv_e);
    hsum = (double)hv;
    psum = (double)phi;
  }
  crf_store_partials(hsum, psum, partial, shd);
}

// loss[item] = H + weight * P, entropy[item] = H, pairwise[item] = P from the item's block partials, in a fixed order
__global__ __launch_bounds__(256) void crf_finish_kernel(const double* partial, int nblocks, double inv_e, double inv_pairs,
                                                         double weight, float* loss, float* entropy, float* pairwise) {
  __shared__ double shd[4];
  partial += (long long)blockIdx.x * 2 * nblocks;      // one workgroup per item
  double h = 0.0, p = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) {
    h += partial[i];
    p += partial[nblocks + i];
  }
  h = block_sum_d(h, shd);
  __syncthreads();
  p = block_sum_d(p, shd);
  if (threadIdx.x == 0) {
    const double H = h * inv_e, P = p * inv_pairs;
    loss[blockIdx.x] = (float)(H + weight * P);
    entropy[blockIdx.x] = (float)H;
    pairwise[blockIdx.x] = (float)P;
  }
}

static long long crf_tiles(const mmtta_tensor* t) {
  return (long long)((t->w + CRF_TW - 1) / CRF_TW) * ((t->h + CRF_TH - 1) / CRF_TH) * ((t->d + CRF_TD - 1) / CRF_TD);
}
static long long crf_generic_blocks(const mmtta_tensor* t) { return ((long long)t->d * t->h * t->w + 255) / 256; }

}  // namespace mmtta

using namespace mmtta;

// fp64 scratch of one call: [N][2][blocks] with the larger block count of the two routes
extern "C" int64_t mmtta_crf_partials(const mmtta_tensor* logits) {
  if (logits == nullptr || logits->n < 1 || logits->d < 1 || logits->h < 1 || logits->w < 1) return -1;
  const long long a = crf_tiles(logits), b = crf_generic_blocks(logits);
  return (int64_t)logits->n * 2 * (a > b ? a : b);
}

extern "C" int mmtta_crf_entropy_items(const mmtta_tensor* logits, const mmtta_tensor* x, uint32_t channel_mask, int softmax,
                                       int connectivity, int form, float weight, float sigma, const mmtta_tensor* dlogits,
                                       double* partial, float* loss, float* entropy, float* pairwise, void* stream) {
  MMTTA_CHECK(logits && logits->ptr, MMTTA_ERR_INVALID, "crf entropy: null `logits`");
  MMTTA_CHECK(dlogits && dlogits->ptr, MMTTA_ERR_INVALID, "crf entropy: null `dlogits`");
  MMTTA_CHECK(partial != nullptr, MMTTA_ERR_INVALID, "crf entropy: null `partial`");
  MMTTA_CHECK(loss != nullptr, MMTTA_ERR_INVALID, "crf entropy: null `loss`");
  MMTTA_CHECK(entropy != nullptr, MMTTA_ERR_INVALID, "crf entropy: null `entropy`");
  MMTTA_CHECK(pairwise != nullptr, MMTTA_ERR_INVALID, "crf entropy: null `pairwise`");
  MMTTA_CHECK(connectivity == 6 || connectivity == 18 || connectivity == 26, MMTTA_ERR_INVALID,
              "crf entropy: connectivity must be 6, 18 or 26, got %d", connectivity);
  MMTTA_CHECK(form == 0 || form == 1, MMTTA_ERR_INVALID, "crf entropy: form must be 0 (potts) or 1 (quadratic), got %d", form);
  MMTTA_CHECK(__builtin_isfinite(weight) && weight > 0.f && weight <= 16.f, MMTTA_ERR_INVALID,
              "crf entropy: weight must be finite and in (0, 16], got %g", (double)weight);
  MMTTA_CHECK(__builtin_isfinite(sigma) && sigma >= 0.f, MMTTA_ERR_INVALID,
              "crf entropy: sigma must be finite and >= 0, got %g", (double)sigma);
  const bool aff = sigma > 0.f;
  // the kernels multiply the squared distance by -log2(e) / (2 sigma^2) in fp32: an infinite factor would turn equal inputs into NaN
  MMTTA_CHECK(!aff || __builtin_isfinite((float)(1.4426950408889634 / (2.0 * (double)sigma * (double)sigma))), MMTTA_ERR_INVALID,
              "crf entropy: sigma %g is too small, 1 / (2 sigma^2) overflows fp32 (sigma 0 switches the affinity off)", (double)sigma);
  MMTTA_CHECK(!aff || (x && x->ptr), MMTTA_ERR_INVALID, "crf entropy: null `x` with sigma > 0");
  MMTTA_CHECK(logits->n >= 1 && logits->c >= 1 && logits->d >= 1 && logits->h >= 1 && logits->w >= 1, MMTTA_ERR_INVALID,
              "crf entropy: empty `logits`");
  MMTTA_CHECK(same_shape(logits, dlogits), MMTTA_ERR_INVALID, "crf entropy: shape mismatch between `logits` and `dlogits`");
  MMTTA_CHECK(logits->sw == dlogits->sw, MMTTA_ERR_INVALID, "crf entropy: row width mismatch between `logits` and `dlogits`");
  MMTTA_CHECK(!aff || (x->n == logits->n && x->d == logits->d && x->h == logits->h && x->w == logits->w && x->c >= 1),
              MMTTA_ERR_INVALID, "crf entropy: shape mismatch between `x` and `logits`");
  MMTTA_CHECK(logits->c <= CRF_MAX_R, MMTTA_ERR_UNSUPPORTED, "crf entropy: more than %d regions", CRF_MAX_R);
  MMTTA_CHECK(!aff || x->c <= CRF_MAX_R, MMTTA_ERR_UNSUPPORTED, "crf entropy: more than %d input channels", CRF_MAX_R);
  const uint32_t mask = aff ? (channel_mask & ((1u << x->c) - 1u)) : 0u;
  MMTTA_CHECK(!aff || mask != 0u, MMTTA_ERR_INVALID,
              "crf entropy: channel_mask 0x%x names none of the %d channels of `x` (sigma > 0)", channel_mask, aff ? x->c : 0);
  MMTTA_CHECK(is_f32(logits), MMTTA_ERR_UNSUPPORTED, "crf entropy: `logits` must be fp32-stored");
  MMTTA_CHECK(is_f32(dlogits) || is_bf16(dlogits), MMTTA_ERR_UNSUPPORTED, "crf entropy: `dlogits` must be fp32 or bf16");
  MMTTA_CHECK(!aff || x->dtype == MMTTA_F32 || x->dtype == MMTTA_BF16, MMTTA_ERR_UNSUPPORTED, "crf entropy: `x` must be fp32 or bf16");
  auto cl = [](const mmtta_tensor* t) { return t->sc == 1 && t->sw >= t->c && t->sh >= 0 && t->sd >= 0 && t->sn >= 0; };
  MMTTA_CHECK(cl(logits) && cl(dlogits) && (!aff || cl(x)), MMTTA_ERR_UNSUPPORTED, "crf entropy: channels-last only");
  MMTTA_CHECK(!loss_overlap(logits, dlogits), MMTTA_ERR_INVALID, "crf entropy: `dlogits` must not overlap `logits` (aliased)");
  MMTTA_CHECK(!aff || !loss_overlap(x, dlogits), MMTTA_ERR_INVALID, "crf entropy: `x` is aliased by `dlogits`");
  // the kernels index the voxels and the elements of one item with 32-bit arithmetic
  auto small = [](const mmtta_tensor* t) {
    const long long ld = t->sw > 4 ? t->sw : 4;
    return (long long)t->d * t->h * t->w * ld < (1ll << 31) && item_fits_31(t, ld);
  };
  MMTTA_CHECK(small(logits) && small(dlogits) && (!aff || small(x)), MMTTA_ERR_UNSUPPORTED,
              "crf entropy: an item of 2^31 elements or more");
  MMTTA_CHECK(logits->n <= CRF_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "crf entropy: more than %d items in one call", CRF_MAX_GRID_Y);
  const int R = logits->c;
  const bool tiled = R <= 4 && loss_dense4(logits) && loss_dense4(dlogits) && (!aff || (x->c <= 4 && loss_dense4(x)));
  MMTTA_CHECK(is_f32(dlogits) || (tiled && !softmax), MMTTA_ERR_UNSUPPORTED,
              "crf entropy: a bf16-stored `dlogits` needs the sigmoid head on the tiled route (<= 4 regions and channels in "
              "dense 4-element voxel rows)");

  hipStream_t s = (hipStream_t)stream;
  const int items = logits->n;
  const int maxl1 = connectivity == 6 ? 1 : (connectivity == 18 ? 2 : 3);
  const double E = (double)logits->d * logits->h * logits->w * (softmax ? 1 : R);
  const float inv_e = (float)(1.0 / E);
  const float cw = (float)((double)weight / ((double)connectivity * E));
  const float negk = aff ? (float)(-1.4426950408889634 / (2.0 * (double)sigma * (double)sigma)) : 0.f;
  long long blocks;
  if (tiled) {
    CrfArgs a;
    a.l = (const float*)logits->ptr; a.dl = (float*)dlogits->ptr; a.x = aff ? (const float*)x->ptr : nullptr;
    a.lsn = logits->sn; a.dsn = dlogits->sn; a.xsn = aff ? x->sn : 0;
    a.D = logits->d; a.H = logits->h; a.W = logits->w; a.R = R;
    a.mask = mask; a.maxl1 = maxl1; a.inv_e = inv_e; a.cw = cw; a.negk = negk;
    a.full_rows = (R == 4 || (dlogits->flags & MMTTA_TENSOR_OWNS_PAD)) ? 1 : 0;
    a.tiles_x = (a.W + CRF_TW - 1) / CRF_TW; a.tiles_y = (a.H + CRF_TH - 1) / CRF_TH;
    a.partial = partial;
    blocks = crf_tiles(logits);      // < 2^31 / 4
    const dim3 launch((unsigned)blocks, items);
    const bool xbf = aff && x->dtype == MMTTA_BF16, obf = is_bf16(dlogits);
#define CRF_TILED(AFF, SM, XBF, OBF) \
  do { \
    if (form == 0) hipLaunchKernelGGL((crf_tiled_kernel<AFF, SM, XBF, OBF, 0>), launch, dim3(256), 0, s, a); \
    else hipLaunchKernelGGL((crf_tiled_kernel<AFF, SM, XBF, OBF, 1>), launch, dim3(256), 0, s, a); \
  } while (0)
#define CRF_TILED_HEAD(AFF, XBF) \
  do { \
    if (softmax) CRF_TILED(AFF, true, XBF, false); \
    else if (obf) CRF_TILED(AFF, false, XBF, true); \
    else CRF_TILED(AFF, false, XBF, false); \
  } while (0)
    if (!aff) CRF_TILED_HEAD(false, false);
    else if (xbf) CRF_TILED_HEAD(true, true);
    else CRF_TILED_HEAD(true, false);
#undef CRF_TILED_HEAD
#undef CRF_TILED
  } else {
    blocks = crf_generic_blocks(logits);
    hipLaunchKernelGGL(crf_generic_kernel, dim3((unsigned)blocks, items), dim3(256), 0, s, tv(logits), tv(dlogits),
                       aff ? tv(x) : tv(logits), aff ? 1 : 0, softmax ? 1 : 0, form, mask, maxl1, inv_e, cw, negk, partial);
  }
  int st = launch_status("crf entropy");
  if (st) return st;
  hipLaunchKernelGGL(crf_finish_kernel, dim3(items), dim3(256), 0, s, (const double*)partial, (int)blocks, 1.0 / E,
                     1.0 / (2.0 * (double)connectivity * E), (double)weight, loss, entropy, pairwise);
  return launch_status("crf entropy finish");
}
