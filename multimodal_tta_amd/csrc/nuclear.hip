// Entropy minus a regional nuclear-norm term on gfx950 (Cui et al., CVPR 2020, "Towards Discriminability and Diversity: Batch
// Nuclear-norm Maximization"; the regional nuclear norm of Hu et al., MICCAI 2021, "Fully Test-time Adaptation for Image
// Segmentation"): per batch item, over a grid of boxes of `block` voxels,
//   L = entropy_weight * H - weight * N,   N = 1/Q sum_A nu(A),   nu(A) = sum_k sqrt(lambda_k(A^T A) + eps m) / sqrt(m min(m, K)).
// The loss of a voxel depends on a matrix statistic of its whole box, so the pass has three parts - a reduction (fp64
// partials of the box's Gram entries and of the entropy), a small dense eigenproblem per box, and a gradient pass that
// reads the result back - and a per-item finish: four launches, whatever the data and the block size.  Nothing is
// scattered and nothing is added atomically; every sum is taken in a fixed order.  See include/mmtta.h for the contract.
#include "voxel_loss.h"

namespace mmtta {

constexpr int NUC_MAX_R = LOSS_MAX_R;
constexpr int NUC_MAX_GRID_Y = LOSS_MAX_GRID_Y;      // gridDim.y carries the item
constexpr int NUC_THREADS = 256;
constexpr int NUC_PER_THREAD = 4;
constexpr int NUC_CHUNK = NUC_THREADS * NUC_PER_THREAD;      // voxels of one box that one workgroup owns
constexpr int NUC_MAX_S = NUC_MAX_R * (NUC_MAX_R + 1) / 2 + 1;      // sums of one partial row: the upper Gram entries, the entropy

// The geometry of one item.  A box b (z-major over the grid of boxes) has `cpb` chunks, whatever its own size: a border box
// is smaller, and its last chunks are empty (they write zero partials).  Scratch of one item, in doubles:
//   [B * cpb][S] partial rows | [Q] nu | [B] entropy sums | coefficients (fp32: K * K per box, or (c0, c1) per (box, region))
struct NucGeo {
  int D, H, W, R;
  int bd, bh, bw;      // the box, entries of 0 and entries past the extent replaced by the extent
  int nbh, nbw;        // boxes along y and x
  int B, cpb, S, CF;   // boxes; chunks per box; sums per partial row; coefficient floats per box
  long long Q;         // matrices of the item
  long long off_nu, off_h, off_cf, item;
};

struct NucBox {
  int z0, y0, x0, my, mx, m;
};
__device__ __forceinline__ NucBox nuc_box(const NucGeo& g, unsigned b) {
  NucBox q;
  const unsigned bx = b % (unsigned)g.nbw, t = b / (unsigned)g.nbw;
  const unsigned by = t % (unsigned)g.nbh, bz = t / (unsigned)g.nbh;
  q.z0 = (int)bz * g.bd; q.y0 = (int)by * g.bh; q.x0 = (int)bx * g.bw;
  const int mz = min(g.bd, g.D - q.z0);
  q.my = min(g.bh, g.H - q.y0);
  q.mx = min(g.bw, g.W - q.x0);
  q.m = mz * q.my * q.mx;
  return q;
}
// voxel j < m of a box (x fastest) -> its coordinates in the volume
__device__ __forceinline__ void nuc_voxel_pos(const NucBox& q, unsigned j, int& z, int& y, int& x) {
  const unsigned lx = j % (unsigned)q.mx, t = j / (unsigned)q.mx;
  x = q.x0 + (int)lx;
  y = q.y0 + (int)(t % (unsigned)q.my);
  z = q.z0 + (int)(t / (unsigned)q.my);
}

// One voxel: p (and q = 1 - p on the sigmoid head, not formed by subtraction), its entropy h, dh/dl and, on the sigmoid
// head, p (1 - p).  FAST: v_exp_f32 / v_rcp_f32 / v_log_f32, the forms of the entropy fast path; otherwise libm's.  Lanes
// >= R come out 0.  Both passes call this, so the gradient pass meets the p the Gram pass summed.
template <int MAXR>
struct NucVoxel {
  float p[MAXR], q[MAXR], gh[MAXR], pq[MAXR];
  float h;
};
template <bool SOFTMAX, bool FAST, int MAXR>
__device__ __forceinline__ void nuc_voxel(const float (&t)[MAXR], int R, NucVoxel<MAXR>& v) {
  v.h = 0.f;
  if (!SOFTMAX) {
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
      v.p[r] = v.q[r] = v.gh[r] = v.pq[r] = 0.f;
      if (r < R) {
        if (FAST) {
          const float e = exp_neg_abs(t[r]);
          const SigmoidPair s = sigmoid_pair(t[r], e);
          v.p[r] = s.p;
          v.q[r] = s.q;
          v.pq[r] = s.er * s.r;
          v.h += fmaxf(t[r], 0.f) + log1p_unit(e) - t[r] * s.p;
          v.gh[r] = -t[r] * v.pq[r];
        } else {
          const BernoulliLibm b = bernoulli_entropy_libm(t[r]);
          const float other = t[r] >= 0.f ? b.e / (1.f + b.e) : 1.f / (1.f + b.e);
          v.p[r] = b.sig;
          v.q[r] = other;
          v.pq[r] = b.sig * other;
          v.h += b.h;
          v.gh[r] = -t[r] * v.pq[r];
        }
      }
    }
    return;
  }
  float m = -INFINITY;
#pragma unroll
  for (int r = 0; r < MAXR; ++r)
    if (r < R) m = fmaxf(m, t[r]);
  float u[MAXR], se = 0.f;
#pragma unroll
  for (int r = 0; r < MAXR; ++r) {
    u[r] = 0.f;
    v.p[r] = 0.f;
    if (r < R) {
      u[r] = t[r] - m;
      v.p[r] = FAST ? exp_fast(u[r]) : expf(u[r]);
      se += v.p[r];
    }
  }
  // the shifted form Hs = log se - sum p u of voxel_loss.h
  const float lg = FAST ? __builtin_amdgcn_logf(se) * 0.6931471805599453f : logf(se);
  float pu = 0.f;
#pragma unroll
  for (int r = 0; r < MAXR; ++r) {
    v.p[r] = v.p[r] / se;
    pu = fmaf(v.p[r], u[r], pu);
  }
  v.h = lg - pu;
#pragma unroll
  for (int r = 0; r < MAXR; ++r) {
    v.q[r] = v.pq[r] = 0.f;
    v.gh[r] = r < R ? -v.p[r] * ((u[r] - lg) + v.h) : 0.f;
  }
}

// the logits of voxel (z, y, x): one 16-byte load on the fast route
template <bool FAST, int MAXR>
__device__ __forceinline__ void nuc_load(const float* lp, const NucGeo& g, long long sd, long long sh, long long sw, int z, int y,
                                         int x, float (&t)[MAXR]) {
  if constexpr (FAST) {
    const unsigned v = ((unsigned)z * g.H + y) * g.W + x;      // * 4 < 2^31: checked on the host
    const float4 t4 = *reinterpret_cast<const float4*>(lp + v * 4u);
    t[0] = t4.x; t[1] = t4.y; t[2] = t4.z; t[3] = t4.w;
  } else {
    const float* zp = lp + z * sd + y * sh + x * sw;
#pragma unroll
    for (int r = 0; r < MAXR; ++r) t[r] = r < g.R ? zp[r] : 0.f;
  }
}

// index of entry (a, b), a <= b, among the upper entries of a K x K matrix, row by row
__host__ __device__ __forceinline__ int nuc_tri(int a, int b, int K) { return a * K - a * (a - 1) / 2 + (b - a); }

// ------------------------------------------------------------------ stage 1: the Gram pass
// Fast route (R <= 4, 16-byte rows): a thread sums its four voxels in fp32, the workgroup adds them up in fp64.  The
// accumulators take the 4-lane layout (pad lanes hold p = 0) and are mapped to the row of the R-lane layout at the store.
template <bool SOFTMAX>
__global__ __launch_bounds__(NUC_THREADS) void nuc_gram_fast_kernel(const float* l, long long lsn, NucGeo g, double* scratch) {
  constexpr int NS = SOFTMAX ? 11 : 13;
  __shared__ double sh[4][NS];
  const unsigned b = blockIdx.x / (unsigned)g.cpb, chunk = blockIdx.x % (unsigned)g.cpb;
  const NucBox box = nuc_box(g, b);
  const float* lp = l + (long long)blockIdx.y * lsn;
  float acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.f;
#pragma unroll
  for (int i = 0; i < NUC_PER_THREAD; ++i) {
    const unsigned j = chunk * NUC_CHUNK + i * NUC_THREADS + threadIdx.x;
    if (j < (unsigned)box.m) {
      int z, y, x;
      nuc_voxel_pos(box, j, z, y, x);
      float t[4];
      nuc_load<true, 4>(lp, g, 0, 0, 0, z, y, x, t);
      NucVoxel<4> v;
      nuc_voxel<SOFTMAX, true, 4>(t, g.R, v);
      if (SOFTMAX) {
        int s = 0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int c = a; c < 4; ++c) {
            acc[s] = fmaf(v.p[a], v.p[c], acc[s]);
            ++s;
          }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          acc[3 * r] = fmaf(v.p[r], v.p[r], acc[3 * r]);
          acc[3 * r + 1] = fmaf(v.p[r], v.q[r], acc[3 * r + 1]);
          acc[3 * r + 2] = fmaf(v.q[r], v.q[r], acc[3 * r + 2]);
        }
      }
      acc[NS - 1] += v.h;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const double w = wave_sum_d((double)acc[s]);
    if (lane == 0) sh[wave][s] = w;
  }
  __syncthreads();
  if ((int)threadIdx.x < g.S) {
    const int s = threadIdx.x;
    int src = s;
    if (s == g.S - 1) {
      src = NS - 1;
    } else if (SOFTMAX) {
      int a = 0, rest = s;      // entry s of the R-lane layout is (a, c)
      while (rest >= g.R - a) { rest -= g.R - a; ++a; }
      src = nuc_tri(a, a + rest, 4);
    }
    double* part = scratch + (long long)blockIdx.y * g.item + (long long)blockIdx.x * g.S;
    part[s] = (sh[0][src] + sh[1][src]) + (sh[2][src] + sh[3][src]);
  }
}

// Generic route (R <= 16, any channels-last rows): the workgroup stages 256 voxels' p (and q) in LDS, and thread s adds up
// entry s of the row over them in fp64, in voxel order.
template <bool SOFTMAX>
__global__ __launch_bounds__(NUC_THREADS) void nuc_gram_generic_kernel(TV l, NucGeo g, double* scratch) {
  constexpr int LD = (SOFTMAX ? NUC_MAX_R : 2 * NUC_MAX_R) + 1;
  __shared__ float ps[NUC_THREADS][LD];
  __shared__ double shd[4];
  const unsigned b = blockIdx.x / (unsigned)g.cpb, chunk = blockIdx.x % (unsigned)g.cpb;
  const NucBox box = nuc_box(g, b);
  const float* lp = l.p + (long long)blockIdx.y * l.sn;
  const int R = g.R, s = threadIdx.x;
  // the two columns of ps that entry s multiplies
  int ca = 0, cb = 0;
  if (s < g.S - 1) {
    if (SOFTMAX) {
      int a = 0, rest = s;
      while (rest >= R - a) { rest -= R - a; ++a; }
      ca = a; cb = a + rest;
    } else {
      const int r = s / 3, k = s % 3;      // p p, p q, q q of region r: columns 2 r (p) and 2 r + 1 (q)
      ca = 2 * r + (k == 2 ? 1 : 0);
      cb = 2 * r + (k == 0 ? 0 : 1);
    }
  }
  double sum = 0.0, hsum = 0.0;
  for (int i = 0; i < NUC_PER_THREAD; ++i) {
    const unsigned j = chunk * NUC_CHUNK + i * NUC_THREADS + threadIdx.x;
    NucVoxel<NUC_MAX_R> v;
    if (j < (unsigned)box.m) {
      int z, y, x;
      nuc_voxel_pos(box, j, z, y, x);
      float t[NUC_MAX_R];
      nuc_load<false, NUC_MAX_R>(lp, g, l.sd, l.sh, l.sw, z, y, x, t);
      nuc_voxel<SOFTMAX, false, NUC_MAX_R>(t, R, v);
      hsum += (double)v.h;
    } else {
#pragma unroll
      for (int r = 0; r < NUC_MAX_R; ++r) v.p[r] = v.q[r] = 0.f;
    }
#pragma unroll
    for (int r = 0; r < NUC_MAX_R; ++r) {
      if (SOFTMAX) {
        ps[threadIdx.x][r] = v.p[r];
      } else {
        ps[threadIdx.x][2 * r] = v.p[r];
        ps[threadIdx.x][2 * r + 1] = v.q[r];
      }
    }
    __syncthreads();
    if (s < g.S - 1)
      for (int k = 0; k < NUC_THREADS; ++k) sum += (double)(ps[k][ca] * ps[k][cb]);
    __syncthreads();
  }
  const double h = block_sum_d(hsum, shd);
  double* part = scratch + (long long)blockIdx.y * g.item + (long long)blockIdx.x * g.S;
  if (s < g.S - 1) part[s] = sum;
  if (s == 0) part[g.S - 1] = h;
}

// ------------------------------------------------------------------ stage 2: the spectrum pass
// One workgroup per box: its threads add the box's partial rows up (rows t, t + 256, ... each, then across the workgroup), and
//   sigmoid head  thread r < R takes the 2 x 2 matrix of region r in closed form: with X = G + eps m I and s1, s2 the roots of
//                 its eigenvalues, X^(-1/2) = adj(X + s1 s2 I) / (s1 s2 (s1 + s2)) - no division by s1 - s2;
//   softmax head  thread 0 diagonalises the K x K matrix with cyclic Jacobi rotations in LDS.
// Written: nu per matrix, the box's entropy sum, and the coefficients of (weight / Q) M as fp32 - K x K per box, or per
// (box, region) c0 = M00 - M01 and c1 = M01 - M11, so that g = [(A M)_0 - (A M)_1] weight / Q = c0 p + c1 q.
template <bool SOFTMAX>
__global__ __launch_bounds__(256) void nuc_spectrum_kernel(NucGeo g, double eps, double scale, double* scratch) {
  constexpr int KK = SOFTMAX ? NUC_MAX_R : 1;
  __shared__ double sums[NUC_MAX_S], waves[4][NUC_MAX_S];
  __shared__ double gs[KK * KK], vs[KK * KK], ds[KK];
  const unsigned b = blockIdx.x;
  const NucBox box = nuc_box(g, b);
  double* item = scratch + (long long)blockIdx.y * g.item;
  const double* part = item + (long long)b * g.cpb * g.S;
  const int lane = threadIdx.x, R = g.R;      // (the index in the workgroup)
  for (int s = 0; s < g.S; ++s) {
    double t = 0.0;
    for (int row = lane; row < g.cpb; row += 256) t += part[(long long)row * g.S + s];
    t = wave_sum_d(t);
    if ((lane & 63) == 0) waves[lane >> 6][s] = t;
  }
  __syncthreads();
  if (lane < g.S) sums[lane] = (waves[0][lane] + waves[1][lane]) + (waves[2][lane] + waves[3][lane]);
  __syncthreads();
  const double m = (double)box.m, em = eps * m;
  float* cf = reinterpret_cast<float*>(item + g.off_cf) + (long long)b * g.CF;
  if (lane == 0) item[g.off_h + b] = sums[g.S - 1];
  if (!SOFTMAX) {
    if (lane < R) {
      const double c = 1.0 / sqrt(m * (box.m < 2 ? 1.0 : 2.0));
      const double a = sums[3 * lane], o = sums[3 * lane + 1], d = sums[3 * lane + 2];
      const double hm = 0.5 * (a + d), hd = 0.5 * (a - d);
      const double l1 = hm + sqrt(hd * hd + o * o);
      const double l2 = l1 > 0.0 ? fmax((a * d - o * o) / l1, 0.0) : 0.0;
      const double s1 = sqrt(fmax(l1, 0.0) + em), s2 = sqrt(l2 + em);
      const double ss = s1 * s2, inv = c / (ss * (s1 + s2));
      const double m00 = (d + em + ss) * inv, m01 = -o * inv, m11 = (a + em + ss) * inv;
      item[g.off_nu + (long long)b * R + lane] = c * (s1 + s2);
      cf[2 * lane] = (float)((m00 - m01) * scale);
      cf[2 * lane + 1] = (float)((m01 - m11) * scale);
    }
    return;
  }
  const int K = R;
  if (lane == 0) {
    for (int a = 0; a < K; ++a)
      for (int c = a; c < K; ++c) {
        const double v = sums[nuc_tri(a, c, K)];
        gs[a * K + c] = v;
        gs[c * K + a] = v;
        vs[a * K + c] = vs[c * K + a] = a == c ? 1.0 : 0.0;
      }
    double tr = 0.0;
    for (int a = 0; a < K; ++a) tr += gs[a * K + a];
    for (int sweep = 0; sweep < 40; ++sweep) {
      double off = 0.0;
      for (int p = 0; p < K; ++p)
        for (int q = p + 1; q < K; ++q) off += gs[p * K + q] * gs[p * K + q];
      if (off <= 1e-30 * tr * tr) break;      // off-diagonal norm below 1e-15 of the trace: the sweeps converge quadratically
      for (int p = 0; p < K; ++p)
        for (int q = p + 1; q < K; ++q) {
          const double gpq = gs[p * K + q];
          if (gpq == 0.0) continue;
          const double tau = (gs[q * K + q] - gs[p * K + p]) / (2.0 * gpq);
          const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
          const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
          for (int k = 0; k < K; ++k) {      // columns p, q
            const double x = gs[k * K + p], y = gs[k * K + q];
            gs[k * K + p] = c * x - s * y;
            gs[k * K + q] = s * x + c * y;
          }
          for (int k = 0; k < K; ++k) {      // rows p, q
            const double x = gs[p * K + k], y = gs[q * K + k];
            gs[p * K + k] = c * x - s * y;
            gs[q * K + k] = s * x + c * y;
          }
          for (int k = 0; k < K; ++k) {
            const double x = vs[k * K + p], y = vs[k * K + q];
            vs[k * K + p] = c * x - s * y;
            vs[k * K + q] = s * x + c * y;
          }
        }
    }
    const double c = 1.0 / sqrt(m * (double)(box.m < K ? box.m : K));
    double nu = 0.0;
    for (int k = 0; k < K; ++k) {
      const double r = sqrt(fmax(gs[k * K + k], 0.0) + em);
      nu += r;
      ds[k] = c / r;
    }
    item[g.off_nu + b] = c * nu;
  }
  __syncthreads();
  for (int e = lane; e < K * K; e += 256) {
    const int a = e / K, c = e % K;
    double v = 0.0;
    for (int k = 0; k < K; ++k) v += vs[a * K + k] * ds[k] * vs[c * K + k];
    cf[e] = (float)(v * scale);
  }
}

// ------------------------------------------------------------------ stage 3: the gradient pass
// The traversal of the Gram pass.  The coefficients of the workgroup's box go through LDS once (every lane reads the same
// address: a broadcast); dlogits = entropy_weight / E * dh/dl - dN/dl with the weight / Q scale already in the coefficients.
template <bool SOFTMAX, bool FAST, bool OBF>
__global__ __launch_bounds__(NUC_THREADS) void nuc_grad_kernel(TV l, TV dl, NucGeo g, float ewe, int full_rows, const double* scratch) {
  constexpr int MAXR = FAST ? 4 : NUC_MAX_R;
  __shared__ float cs[SOFTMAX ? MAXR * MAXR : 2 * MAXR];
  const unsigned b = blockIdx.x / (unsigned)g.cpb, chunk = blockIdx.x % (unsigned)g.cpb;
  const NucBox box = nuc_box(g, b);
  const int R = g.R;
  const float* cf = reinterpret_cast<const float*>(scratch + (long long)blockIdx.y * g.item + g.off_cf) + (long long)b * g.CF;
  if ((int)threadIdx.x < g.CF) cs[threadIdx.x] = cf[threadIdx.x];
  __syncthreads();
  const float* lp = l.p + (long long)blockIdx.y * l.sn;
  float* dp = grad_item<OBF>(dl.p, blockIdx.y, dl.sn);
#pragma unroll
  for (int i = 0; i < NUC_PER_THREAD; ++i) {
    const unsigned j = chunk * NUC_CHUNK + i * NUC_THREADS + threadIdx.x;
    if (j >= (unsigned)box.m) continue;
    int z, y, x;
    nuc_voxel_pos(box, j, z, y, x);
    float t[MAXR];
    nuc_load<FAST, MAXR>(lp, g, l.sd, l.sh, l.sw, z, y, x, t);
    NucVoxel<MAXR> v;
    nuc_voxel<SOFTMAX, FAST, MAXR>(t, R, v);
    float o[MAXR];
    if (SOFTMAX) {
      float gk[MAXR], pg = 0.f;
#pragma unroll
      for (int k = 0; k < MAXR; ++k) {
        gk[k] = 0.f;
        if (k < R) {
#pragma unroll
          for (int a = 0; a < MAXR; ++a)
            if (a < R) gk[k] = fmaf(v.p[a], cs[a * R + k], gk[k]);
          pg = fmaf(v.p[k], gk[k], pg);
        }
      }
#pragma unroll
      for (int k = 0; k < MAXR; ++k) o[k] = k < R ? fmaf(ewe, v.gh[k], -(v.p[k] * (gk[k] - pg))) : 0.f;
    } else {
#pragma unroll
      for (int r = 0; r < MAXR; ++r) {
        o[r] = 0.f;
        if (r < R) {
          const float gr = fmaf(v.p[r], cs[2 * r], v.q[r] * cs[2 * r + 1]);
          o[r] = fmaf(ewe, v.gh[r], -(gr * v.pq[r]));
        }
      }
    }
    if constexpr (FAST) {
      const unsigned vx = ((unsigned)z * g.H + y) * g.W + x;
      if (full_rows) {
        st4_t<OBF>(dp, vx * 4u, make_float4(o[0], o[1], o[2], o[3]));
      } else {
        st1_t<OBF>(dp, vx * 4u, o[0]);
        if (R > 1) st1_t<OBF>(dp, vx * 4u + 1, o[1]);
        if (R > 2) st1_t<OBF>(dp, vx * 4u + 2, o[2]);
      }
    } else {
      float* op = dp + z * dl.sd + y * dl.sh + x * dl.sw;
#pragma unroll
      for (int r = 0; r < MAXR; ++r)
        if (r < R) op[r] = o[r];      // pad lanes are left as they are
    }
  }
}

// loss[item] = entropy_weight * H - weight * N, entropy[item] = H, nuclear[item] = N from the boxes' sums, in a fixed order
__global__ __launch_bounds__(256) void nuc_finish_kernel(NucGeo g, const double* scratch, double inv_e, double entropy_weight,
                                                         double weight, float* loss, float* entropy, float* nuclear) {
  __shared__ double shd[4];
  const double* item = scratch + (long long)blockIdx.x * g.item;      // one workgroup per item
  double h = 0.0, n = 0.0;
  for (int i = threadIdx.x; i < g.B; i += 256) h += item[g.off_h + i];
  for (long long i = threadIdx.x; i < g.Q; i += 256) n += item[g.off_nu + i];
  h = block_sum_d(h, shd);
  __syncthreads();
  n = block_sum_d(n, shd);
  if (threadIdx.x == 0) {
    const double H = h * inv_e, N = n / (double)g.Q;
    loss[blockIdx.x] = (float)(entropy_weight * H - weight * N);
    entropy[blockIdx.x] = (float)H;
    nuclear[blockIdx.x] = (float)N;
  }
}

// the geometry of one item of `t`; false: an empty tensor, more than NUC_MAX_R regions, a negative block entry or sizes
// past what an int64 count of doubles holds
static bool nuc_geometry(const mmtta_tensor* t, int softmax, int bd, int bh, int bw, NucGeo& g) {
  if (t->n < 1 || t->c < 1 || t->c > NUC_MAX_R || t->d < 1 || t->h < 1 || t->w < 1 || bd < 0 || bh < 0 || bw < 0) return false;
  auto whole = [](int b, int extent) { return (b == 0 || b >= extent) ? extent : b; };
  g.D = t->d; g.H = t->h; g.W = t->w; g.R = t->c;
  g.bd = whole(bd, g.D); g.bh = whole(bh, g.H); g.bw = whole(bw, g.W);
  const long long nbd = (g.D + g.bd - 1) / g.bd;
  g.nbh = (g.H + g.bh - 1) / g.bh;
  g.nbw = (g.W + g.bw - 1) / g.bw;
  const long long B = nbd * g.nbh * g.nbw, full = (long long)g.bd * g.bh * g.bw, cpb = (full + NUC_CHUNK - 1) / NUC_CHUNK;
  if ((double)t->d * t->h * t->w >= 9e15 || B * cpb >= (1ll << 31)) return false;
  g.B = (int)B;
  g.cpb = (int)cpb;
  g.S = (softmax ? g.R * (g.R + 1) / 2 : 3 * g.R) + 1;
  g.CF = softmax ? g.R * g.R : 2 * g.R;
  g.Q = softmax ? B : B * g.R;
  g.off_nu = B * cpb * g.S;
  g.off_h = g.off_nu + g.Q;
  g.off_cf = g.off_h + B;
  g.item = g.off_cf + (B * g.CF + 1) / 2;
  return true;
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int64_t mmtta_nuclear_scratch(const mmtta_tensor* logits, int softmax, int bd, int bh, int bw) {
  NucGeo g;
  if (logits == nullptr || !nuc_geometry(logits, softmax, bd, bh, bw, g)) return -1;
  return (int64_t)logits->n * g.item;
}

extern "C" int mmtta_nuclear_entropy_items(const mmtta_tensor* logits, int softmax, int bd, int bh, int bw, float entropy_weight,
                                           float weight, float eps, const mmtta_tensor* dlogits, double* scratch, float* loss,
                                           float* entropy, float* nuclear, void* stream) {
  MMTTA_CHECK(logits && logits->ptr, MMTTA_ERR_INVALID, "nuclear entropy: null `logits`");
  MMTTA_CHECK(dlogits && dlogits->ptr, MMTTA_ERR_INVALID, "nuclear entropy: null `dlogits`");
  MMTTA_CHECK(scratch != nullptr, MMTTA_ERR_INVALID, "nuclear entropy: null `scratch`");
  MMTTA_CHECK(loss != nullptr, MMTTA_ERR_INVALID, "nuclear entropy: null `loss`");
  MMTTA_CHECK(entropy != nullptr, MMTTA_ERR_INVALID, "nuclear entropy: null `entropy`");
  MMTTA_CHECK(nuclear != nullptr, MMTTA_ERR_INVALID, "nuclear entropy: null `nuclear`");
  MMTTA_CHECK(bd >= 0 && bh >= 0 && bw >= 0, MMTTA_ERR_INVALID,
              "nuclear entropy: block entries must be >= 0 (0: the whole extent), got [%d, %d, %d]", bd, bh, bw);
  MMTTA_CHECK(__builtin_isfinite(weight) && weight > 0.f && weight <= 16.f, MMTTA_ERR_INVALID,
              "nuclear entropy: weight must be finite and in (0, 16], got %g", (double)weight);
  MMTTA_CHECK(__builtin_isfinite(entropy_weight) && entropy_weight >= 0.f && entropy_weight <= 16.f, MMTTA_ERR_INVALID,
              "nuclear entropy: entropy_weight must be finite and in [0, 16], got %g", (double)entropy_weight);
  MMTTA_CHECK(__builtin_isfinite(eps) && eps >= 1e-6f && eps <= 0.1f, MMTTA_ERR_INVALID,
              "nuclear entropy: eps must be finite and in [1e-6, 0.1], got %g", (double)eps);
  MMTTA_CHECK(logits->n >= 1 && logits->c >= 1 && logits->d >= 1 && logits->h >= 1 && logits->w >= 1, MMTTA_ERR_INVALID,
              "nuclear entropy: empty `logits`");
  MMTTA_CHECK(same_shape(logits, dlogits), MMTTA_ERR_INVALID, "nuclear entropy: shape mismatch between `logits` and `dlogits`");
  MMTTA_CHECK(logits->sw == dlogits->sw, MMTTA_ERR_INVALID, "nuclear entropy: row width mismatch between `logits` and `dlogits`");
  MMTTA_CHECK(logits->c <= NUC_MAX_R, MMTTA_ERR_UNSUPPORTED, "nuclear entropy: more than %d regions", NUC_MAX_R);
  MMTTA_CHECK(is_f32(logits), MMTTA_ERR_UNSUPPORTED, "nuclear entropy: `logits` must be fp32-stored");
  MMTTA_CHECK(is_f32(dlogits) || is_bf16(dlogits), MMTTA_ERR_UNSUPPORTED, "nuclear entropy: `dlogits` must be fp32 or bf16");
  auto cl = [](const mmtta_tensor* t) { return t->sc == 1 && t->sw >= t->c && t->sh >= 0 && t->sd >= 0 && t->sn >= 0; };
  MMTTA_CHECK(cl(logits) && cl(dlogits), MMTTA_ERR_UNSUPPORTED, "nuclear entropy: channels-last only");
  MMTTA_CHECK(!loss_overlap(logits, dlogits), MMTTA_ERR_INVALID, "nuclear entropy: `dlogits` must not overlap `logits` (aliased)");
  // the kernels index the voxels and the elements of one item with 32-bit arithmetic
  auto small = [](const mmtta_tensor* t) {
    const long long ld = t->sw > 4 ? t->sw : 4;
    return (long long)t->d * t->h * t->w * ld < (1ll << 31) && item_fits_31(t, ld);
  };
  MMTTA_CHECK(small(logits) && small(dlogits), MMTTA_ERR_UNSUPPORTED, "nuclear entropy: an item of 2^31 elements or more");
  MMTTA_CHECK(logits->n <= NUC_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "nuclear entropy: more than %d items in one call", NUC_MAX_GRID_Y);
  NucGeo g;
  MMTTA_CHECK(nuc_geometry(logits, softmax, bd, bh, bw, g) && (long long)logits->n * g.item < (1ll << 31), MMTTA_ERR_UNSUPPORTED,
              "nuclear entropy: a scratch of 2^31 fp64 elements or more");
  const int R = logits->c;
  const bool fast = R <= 4 && loss_dense16(logits) && loss_dense4(dlogits);
  MMTTA_CHECK(is_f32(dlogits) || (fast && !softmax), MMTTA_ERR_UNSUPPORTED,
              "nuclear entropy: a bf16-stored `dlogits` needs the sigmoid head on the fast route (<= 4 regions in dense "
              "4-element voxel rows)");

  hipStream_t s = (hipStream_t)stream;
  const int items = logits->n;
  const double E = (double)logits->d * logits->h * logits->w * (softmax ? 1 : R);
  const float ewe = (float)((double)entropy_weight / E);
  const dim3 units((unsigned)g.B * (unsigned)g.cpb, items), boxes((unsigned)g.B, items);
  if (fast) {
    if (softmax) hipLaunchKernelGGL(nuc_gram_fast_kernel<true>, units, dim3(NUC_THREADS), 0, s, (const float*)logits->ptr, (long long)logits->sn, g, scratch);
    else hipLaunchKernelGGL(nuc_gram_fast_kernel<false>, units, dim3(NUC_THREADS), 0, s, (const float*)logits->ptr, (long long)logits->sn, g, scratch);
  } else {
    if (softmax) hipLaunchKernelGGL(nuc_gram_generic_kernel<true>, units, dim3(NUC_THREADS), 0, s, tv(logits), g, scratch);
    else hipLaunchKernelGGL(nuc_gram_generic_kernel<false>, units, dim3(NUC_THREADS), 0, s, tv(logits), g, scratch);
  }
  int st = launch_status("nuclear entropy gram");
  if (st) return st;
  const double scale = (double)weight / (double)g.Q;
  if (softmax) hipLaunchKernelGGL(nuc_spectrum_kernel<true>, boxes, dim3(256), 0, s, g, (double)eps, scale, scratch);
  else hipLaunchKernelGGL(nuc_spectrum_kernel<false>, boxes, dim3(256), 0, s, g, (double)eps, scale, scratch);
  st = launch_status("nuclear entropy spectrum");
  if (st) return st;
  const int full_rows = (R == 4 || (dlogits->flags & MMTTA_TENSOR_OWNS_PAD)) ? 1 : 0;
#define NUC_GRAD(SM, FAST, OBF) \
  hipLaunchKernelGGL((nuc_grad_kernel<SM, FAST, OBF>), units, dim3(NUC_THREADS), 0, s, tv(logits), tv(dlogits), g, ewe, full_rows, (const double*)scratch)
  if (!fast) {
    if (softmax) NUC_GRAD(true, false, false);
    else NUC_GRAD(false, false, false);
  } else if (softmax) {
    NUC_GRAD(true, true, false);
  } else if (is_bf16(dlogits)) {
    NUC_GRAD(false, true, true);
  } else {
    NUC_GRAD(false, true, false);
  }
#undef NUC_GRAD
  st = launch_status("nuclear entropy gradient");
  if (st) return st;
  hipLaunchKernelGGL(nuc_finish_kernel, dim3(items), dim3(256), 0, s, g, (const double*)scratch, 1.0 / E, (double)entropy_weight,
                     (double)weight, loss, entropy, nuclear);
  return launch_status("nuclear entropy finish");
}
