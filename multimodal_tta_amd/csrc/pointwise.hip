// HBM-bound kernels of the adaptation path (gfx950): layout copies, norm statistics and the
// norm(+ReLU) backward, the residual "combine", trilinear x2 and its adjoint, linear
// combinations (modality means).  All tensors are channels-last unless noted; channel is the
// fastest thread index so a wave touches 256 contiguous bytes (4 B/lane) or 1 KiB (16 B/lane,
// the float4 paths) per instruction.  Reductions are two-stage and deterministic: partial slabs
// [rows][2][C] in fp32, combined in fp64 - no float atomics anywhere.
#include "common.h"

namespace mmtta {
MMTTA_ACT_NS_OPEN


// ------------------------------------------------------------------ strided copy
template <bool DBF>
__global__ void copy_strided_kernel(TV s, TV d) {
  const long long total = (long long)d.n * d.c * d.d * d.h * d.w;
  // iterate in the destination's fastest order: if dst is channels-last, c fastest; else x fastest
  const bool cl = d.sc == 1;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    int n, c, z, y, x;
    long long t = i;
    if (cl) {
      c = (int)(t % d.c); t /= d.c;
      x = (int)(t % d.w); t /= d.w;
      y = (int)(t % d.h); t /= d.h;
      z = (int)(t % d.d); n = (int)(t / d.d);
    } else {
      x = (int)(t % d.w); t /= d.w;
      y = (int)(t % d.h); t /= d.h;
      z = (int)(t % d.d); t /= d.d;
      c = (int)(t % d.c); n = (int)(t / d.c);
    }
    st1_any(d.p, vox_addr(d, n, z, y, x) + (long long)c * d.sc, s.p[vox_addr(s, n, z, y, x) + (long long)c * s.sc], DBF);
  }
}

// ------------------------------------------------------------------ two-stage channel reductions
// Block layout: cpl channel lanes (power of two >= min(C,256)) x (256/cpl) voxel lanes.
// MODE 0: (sum x, sum x^2).  MODE 1: norm backward (sum dz, sum dz*xhat).
struct RedArgs {
  TV x;        // MODE 0: tensor ; MODE 1: y (pre-norm)
  TV dout;     // MODE 1
  NL t;        // MODE 1
  int per_item; // MODE 1: t's gamma / beta are [N*C] (mmtta_norm_on_load.per_item)
  float* part; // [N*rows_per_n][2][C]
  int rows_per_n;
  long long vox_per_row;
};

// VEC = 4: every thread owns 4 consecutive channels (16-byte loads); VEC = 1: scalar fallback.
// `regular` tensors (dense voxel order: sh == W*sw, sd == H*sh) are addressed as voxel*sw, no div/mod.
// XBF / DBF: storage of x (the activation) and of dout (the gradient: bf16 when method.grad_storage stores gradients so)
template <int MODE, int VEC, bool XBF = false, bool DBF = false>
__global__ __launch_bounds__(256) void channel_reduce_kernel(RedArgs a) {
  __shared__ float red[2][VEC][256];
  const int C = a.x.c;
  const int CV = (C + VEC - 1) / VEC;          // channel vectors
  int cpl = 1;
  while (cpl < CV && cpl < 256) cpl <<= 1;
  const int nvl = 256 / cpl;
  const int cl = threadIdx.x % cpl, vl = threadIdx.x / cpl;
  const int n = blockIdx.x / a.rows_per_n, row = blockIdx.x % a.rows_per_n;
  const long long dhw = (long long)a.x.d * a.x.h * a.x.w;
  const long long v0 = row * a.vox_per_row;
  const long long v1 = (v0 + a.vox_per_row < dhw) ? v0 + a.vox_per_row : dhw;
  const bool regx = a.x.sh == (long long)a.x.w * a.x.sw && a.x.sd == (long long)a.x.h * a.x.sh;
  const bool regd = a.dout.sh == (long long)a.dout.w * a.dout.sw && a.dout.sd == (long long)a.dout.h * a.dout.sh;
  for (int cb = 0; cb < CV; cb += cpl) {
    const int c0 = (cb + cl) * VEC;
    float s0[VEC], s1[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { s0[j] = 0.f; s1[j] = 0.f; }
    if (c0 < C) {
      float mu[VEC], rs[VEC], g[VEC], b[VEC];
      const int ab = a.per_item ? n * C : 0;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        mu[j] = 0.f; rs[j] = 1.f; g[j] = 1.f; b[j] = 0.f;
        if (MODE == 1 && a.t.mean && c0 + j < C) {
          mu[j] = a.t.mean[n * C + c0 + j]; rs[j] = a.t.rstd[n * C + c0 + j];
          if (a.t.gamma) g[j] = a.t.gamma[ab + c0 + j];
          if (a.t.beta) b[j] = a.t.beta[ab + c0 + j];
        }
      }
      for (long long v = v0 + vl; v < v1; v += nvl) {
        long long ax, ad;
        if (regx && regd) {
          ax = (long long)n * a.x.sn + v * a.x.sw;
          ad = (long long)n * a.dout.sn + v * a.dout.sw;
        } else {
          long long t = v;
          const int xx = (int)(t % a.x.w); t /= a.x.w;
          const int yy = (int)(t % a.x.h);
          const int zz = (int)(t / a.x.h);
          ax = vox_addr(a.x, n, zz, yy, xx);
          ad = vox_addr(a.dout, n, zz, yy, xx);
        }
        float xv[VEC], dv[VEC];
        if (VEC == 4) {
          const float4 t4 = ld4_t<XBF>(a.x.p, ax + c0);               // the pre-norm activation may be bf16-stored
          xv[0] = t4.x; xv[1] = t4.y; xv[2] = t4.z; xv[3] = t4.w;
          if (MODE == 1) {
            const float4 d4 = ld4_t<DBF>(a.dout.p, ad + c0);
            dv[0] = d4.x; dv[1] = d4.y; dv[2] = d4.z; dv[3] = d4.w;
          }
        } else {
          xv[0] = ld1_t<XBF>(a.x.p, ax + c0);
          if (MODE == 1) dv[0] = ld1_t<DBF>(a.dout.p, ad + c0);
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          if (MODE == 0) {
            s0[j] += xv[j];
            s1[j] += xv[j] * xv[j];
          } else {
            const float xhat = (xv[j] - mu[j]) * rs[j];
            float dz = dv[j];
            MMTTA_ACT_BWD(dz, a.t.relu, fmaf(g[j], xhat, b[j]));
            s0[j] += dz;
            s1[j] += dz * xhat;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) { red[0][j][threadIdx.x] = s0[j]; red[1][j][threadIdx.x] = s1[j]; }
    __syncthreads();
    if (vl == 0 && c0 < C) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        if (c0 + j < C) {
          float t0 = 0.f, t1 = 0.f;
          for (int q = 0; q < nvl; ++q) { t0 += red[0][j][q * cpl + cl]; t1 += red[1][j][q * cpl + cl]; }
          a.part[((long long)blockIdx.x * 2 + 0) * C + c0 + j] = t0;
          a.part[((long long)blockIdx.x * 2 + 1) * C + c0 + j] = t1;
        }
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ the same reduction, streamed
// channel_reduce_kernel<MODE, 4> for voxel-dense tensors with C <= 1024 and 32-bit element offsets inside a batch item.
// `part` holds bit for bit what that kernel writes: the rows, cpl / nvl, the voxels of a lane and their order, the order
// of the lane partials and the expressions per element are its own.  What differs is the schedule:
//   - a workgroup walks `rows_per_block` consecutive rows of one item and loads its 16 coefficients once;
//   - a lane's trips are cut into chunks of IT whose loads (clamped addresses, masked adds) are all issued before the
//     first use, and the next chunk's - the next row's, at a row's end - are in flight under the current one's adds;
//   - the lane partials of a row are added by one thread per (sum, channel), sequentially in q as before, from an LDS
//     image [sum][q][channel] that is double-buffered over the rows: one barrier per row, and only the threads that own
//     a chain stay behind for it.
struct RedSArgs {
  const float* x; const float* dout;      // MODE 0: x only
  long long xsn, dsn;
  unsigned xsw, dsw;
  unsigned C, dhw, vox_per_row;
  unsigned rows_per_n, rows_per_block;
  const float* mean; const float* rstd; const float* gamma; const float* beta;   // MODE 1
  act_t relu;
  int per_item;
  float* part;
};

// 4 consecutive channels as loaded (converted when they are used, like Oct8)
template <bool BF> struct Quad4 { float4 v; };
template <> struct Quad4<true> { uint2 q; };
template <bool BF>
__device__ __forceinline__ Quad4<BF> quad4_ld(const float* base, unsigned eoff) {
  Quad4<BF> r;
  if constexpr (BF) r.q = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(base) + eoff);
  else r.v = *reinterpret_cast<const float4*>(base + eoff);
  return r;
}
__device__ __forceinline__ void quad4_f4(const Quad4<false>& r, float (&v)[4]) { v[0] = r.v.x; v[1] = r.v.y; v[2] = r.v.z; v[3] = r.v.w; }
__device__ __forceinline__ void quad4_f4(const Quad4<true>& r, float (&v)[4]) {
  v[0] = bf16_bits_to_f32(r.q.x & 0xffffu); v[1] = __uint_as_float(r.q.x & 0xffff0000u);
  v[2] = bf16_bits_to_f32(r.q.y & 0xffffu); v[3] = __uint_as_float(r.q.y & 0xffff0000u);
}

template <int MODE, int IT, bool XBF = false, bool DBF = false>
__global__ __launch_bounds__(256) void channel_reduce_stream_kernel(RedSArgs a) {
  __shared__ float red[2][2][1024];                     // [row parity][sum][voxel lane q][4 * cpl channels]
  const unsigned n = blockIdx.y;
  const unsigned C = a.C, CV = (C + 3) / 4;
  unsigned cpl = 1;
  while (cpl < CV) cpl <<= 1;                           // CV <= 256 (host)
  const unsigned nvl = 256u / cpl, W = 4 * cpl;
  const unsigned cl = threadIdx.x & (cpl - 1), vl = threadIdx.x / cpl;
  const bool live = cl * 4 < C;                         // an idle channel lane sums channel quad 0: nobody reads its partials
  const unsigned c0 = live ? cl * 4 : 0;
  const float* xp = item_base<XBF>(a.x, n, a.xsn);
  const float* dp = MODE == 1 ? item_base<DBF>(a.dout, n, a.dsn) : nullptr;
  float mu[4], rs[4], g[4], b[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { mu[j] = 0.f; rs[j] = 1.f; g[j] = 1.f; b[j] = 0.f; }
  if (MODE == 1) {
    // (the pad lanes of a quad read channel C-1's coefficients: their sums are never written)
    unsigned pc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) pc[j] = min(c0 + j, C - 1);
    const unsigned ab = a.per_item ? n * C : 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { mu[j] = a.mean[n * C + pc[j]]; rs[j] = a.rstd[n * C + pc[j]]; }
    if (a.gamma) {
#pragma unroll
      for (int j = 0; j < 4; ++j) g[j] = a.gamma[ab + pc[j]];
    }
    if (a.beta) {
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = a.beta[ab + pc[j]];
    }
  }
  const unsigned row_lo = blockIdx.x * a.rows_per_block;
  const unsigned row_hi = min(row_lo + a.rows_per_block, a.rows_per_n);
  const unsigned nchunk = ((a.vox_per_row + nvl - 1) / nvl + IT - 1) / IT;     // chunks of IT trips per row
  Quad4<XBF> xn[IT];
  Quad4<DBF> dn[IT];
  auto issue = [&](unsigned row, unsigned chunk) {
    const unsigned vb = row * a.vox_per_row + chunk * (IT * nvl) + vl;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const unsigned v = min(vb + i * nvl, a.dhw - 1);
      xn[i] = quad4_ld<XBF>(xp, v * a.xsw + c0);
      if (MODE == 1) dn[i] = quad4_ld<DBF>(dp, v * a.dsw + c0);
    }
  };
  float s0[4], s1[4];
  // one voxel quad into the sums; `ok` false leaves them as they are (skipped, not + 0.f: -0.f stays -0.f)
  auto add = [&](const Quad4<XBF>& xr, const Quad4<DBF>& dr, bool ok) {
    float xv[4], dv[4];
    quad4_f4(xr, xv);
    if (MODE == 1) quad4_f4(dr, dv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float t0, t1;
      if (MODE == 0) {
        t0 = s0[j] + xv[j];
        t1 = s1[j] + xv[j] * xv[j];
      } else {
        const float xhat = (xv[j] - mu[j]) * rs[j];
        float dz = dv[j];
        MMTTA_ACT_BWD(dz, a.relu, fmaf(g[j], xhat, b[j]));
        t0 = s0[j] + dz;
        t1 = s1[j] + dz * xhat;
      }
      s0[j] = ok ? t0 : s0[j];
      s1[j] = ok ? t1 : s1[j];
    }
  };
  issue(row_lo, 0);
  for (unsigned row = row_lo; row < row_hi; ++row) {
    const unsigned v0 = row * a.vox_per_row;
    const unsigned v1 = min(v0 + a.vox_per_row, a.dhw);
#pragma unroll
    for (int j = 0; j < 4; ++j) { s0[j] = 0.f; s1[j] = 0.f; }
    for (unsigned chunk = 0; chunk < nchunk; ++chunk) {
      Quad4<XBF> xq[IT];
      Quad4<DBF> dq[IT];
#pragma unroll
      for (int i = 0; i < IT; ++i) {
        xq[i] = xn[i];
        if (MODE == 1) dq[i] = dn[i];
      }
      // the next chunk, of the next row behind a row's last; behind the workgroup's last the same chunk once more (cache
      // hits nobody waits for), so that no branch stands between these loads and the adds below
      const bool last_c = chunk + 1 == nchunk, last_r = row + 1 == row_hi;
      issue(last_c && !last_r ? row + 1 : row, last_c ? (last_r ? chunk : 0u) : chunk + 1);
      const unsigned cb = v0 + chunk * (IT * nvl);
      if (cb + IT * nvl <= v1) {                          // every lane's IT voxels are inside the row (workgroup-uniform)
#pragma unroll
        for (int i = 0; i < IT; ++i) add(xq[i], dq[i], true);
      } else {
#pragma unroll
        for (int i = 0; i < IT; ++i) add(xq[i], dq[i], cb + vl + i * nvl < v1);
      }
    }
    float (&rb)[2][1024] = red[row & 1];
    *reinterpret_cast<float4*>(&rb[0][vl * W + cl * 4]) = make_float4(s0[0], s0[1], s0[2], s0[3]);
    *reinterpret_cast<float4*>(&rb[1][vl * W + cl * 4]) = make_float4(s1[0], s1[1], s1[2], s1[3]);
    __syncthreads();
    // chain e = (sum, channel).  Its buffer is written again two rows on, behind the next row's barrier, which this
    // thread reaches only after the chain.
    for (unsigned e = threadIdx.x; e < 2 * W; e += 256) {
      const unsigned sm = e / W, c = e & (W - 1);
      if (c < C) {
        float t = 0.f;
#pragma unroll 8
        for (unsigned q = 0; q < nvl; ++q) t += rb[sm][q * W + c];
        a.part[(((long long)n * a.rows_per_n + row) * 2 + sm) * C + c] = t;
      }
    }
  }
}

// stage 2a: one wave per (n,c): fp64 sum over the partial rows -> tot[n*C+c][2]
__global__ __launch_bounds__(64) void rows_reduce_kernel(const float* part, int rows_per_n, int C, double* tot) {
  const int n = blockIdx.x / C, c = blockIdx.x % C;
  double s0 = 0.0, s1 = 0.0;
  for (int r = threadIdx.x; r < rows_per_n; r += 64) {
    const long long row = (long long)n * rows_per_n + r;
    s0 += (double)part[(row * 2 + 0) * C + c];
    s1 += (double)part[(row * 2 + 1) * C + c];
  }
  s0 = wave_sum_d(s0);
  s1 = wave_sum_d(s1);
  if (threadIdx.x == 0) {
    tot[((long long)n * C + c) * 2 + 0] = s0;
    tot[((long long)n * C + c) * 2 + 1] = s1;
  }
}

// Norm parameter sets (mmtta_norm_sets) on the device: item n reads set q = n / ips, whose affines sit q * astride and
// whose running statistics sit q * sstride elements behind set 0's.  The plain entry points run the same kernels with ONE
// set spanning the batch (ips = N, strides 0), so both forms share every summation order.
struct NSets {
  int ips;
  long long astride, sstride;
};
inline NSets nsets_plain(int n) { NSets r; r.ips = n; r.astride = 0; r.sstride = 0; return r; }

// InstanceNorm fast path: one wave per (n,c) reduces the partial rows AND finishes the statistics
// (no cross-(n,c) coupling), one launch instead of two.  gi / bi (optional): item n's copy of its set's gamma / beta.
__global__ __launch_bounds__(64) void instance_stats_kernel(const float* part, int rows_per_n, int C, double count, float eps,
                                                            float* mean, float* rstd, const float* gamma, const float* beta,
                                                            float* scale, float* shift, NSets ns, float* gi, float* bi) {
  const int n = blockIdx.x / C, c = blockIdx.x % C;
  const long long ab = (long long)(n / ns.ips) * ns.astride;
  if (gamma) gamma += ab;
  if (beta) beta += ab;
  double s0 = 0.0, s1 = 0.0;
  for (int r = threadIdx.x; r < rows_per_n; r += 64) {
    const long long row = (long long)n * rows_per_n + r;
    s0 += (double)part[(row * 2 + 0) * C + c];
    s1 += (double)part[(row * 2 + 1) * C + c];
  }
  s0 = wave_sum_d(s0);
  s1 = wave_sum_d(s1);
  if (threadIdx.x == 0) {
    const double mu = s0 / count;
    double var = s1 / count - mu * mu;
    if (var < 0.0) var = 0.0;
    const float rs = (float)(1.0 / sqrt(var + (double)eps));
    mean[blockIdx.x] = (float)mu;
    rstd[blockIdx.x] = rs;
    if (scale != nullptr) {
      const float sc = rs * (gamma ? gamma[c] : 1.f);
      scale[blockIdx.x] = sc;
      shift[blockIdx.x] = (beta ? beta[c] : 0.f) - (float)mu * sc;
    }
    if (gi != nullptr) gi[blockIdx.x] = gamma[c];
    if (bi != nullptr) bi[blockIdx.x] = beta[c];
  }
}

__global__ __launch_bounds__(64) void instance_bwd_kernel(const float* part, int rows_per_n, int C, double count,
                                                          const float* gamma, float* m1, float* m2, NSets ns) {
  const int n = blockIdx.x / C, c = blockIdx.x % C;
  if (gamma) gamma += (long long)(n / ns.ips) * ns.astride;
  double s0 = 0.0, s1 = 0.0;
  for (int r = threadIdx.x; r < rows_per_n; r += 64) {
    const long long row = (long long)n * rows_per_n + r;
    s0 += (double)part[(row * 2 + 0) * C + c];
    s1 += (double)part[(row * 2 + 1) * C + c];
  }
  s0 = wave_sum_d(s0);
  s1 = wave_sum_d(s1);
  if (threadIdx.x == 0) {
    const double g = gamma ? (double)gamma[c] : 1.0;
    m1[blockIdx.x] = (float)(g * s0 / count);
    m2[blockIdx.x] = (float)(g * s1 / count);
  }
}

struct StatFinArgs {
  int kind, groups, N, C;
  double count;
  float eps;
  int training;
  float* running_mean; float* running_var; float momentum;
  float* mean; float* rstd;
  const float* gamma; const float* beta; float* scale; float* shift;
  const double* tot;
  NSets ns;
  float* gi; float* bi;   // optional per-item copies of the set's gamma / beta
};

__global__ void stats_finalize_kernel(StatFinArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.N * a.C) return;
  const int n = i / a.C, c = i % a.C;
  const int q = n / a.ns.ips, m0 = q * a.ns.ips;          // this item's set and its first item
  const float* gamma = a.gamma ? a.gamma + q * a.ns.astride : nullptr;
  const float* beta = a.beta ? a.beta + q * a.ns.astride : nullptr;
  float* running_mean = a.running_mean ? a.running_mean + q * a.ns.sstride : nullptr;
  float* running_var = a.running_var ? a.running_var + q * a.ns.sstride : nullptr;
  if (a.gi != nullptr) a.gi[i] = gamma[c];
  if (a.bi != nullptr) a.bi[i] = beta[c];
  double S = 0.0, Q = 0.0, cnt = 0.0;
  if (a.kind == MMTTA_NORM_INSTANCE) {
    S = a.tot[(long long)i * 2]; Q = a.tot[(long long)i * 2 + 1]; cnt = a.count;
  } else if (a.kind == MMTTA_NORM_BATCH) {
    if (!a.training) {
      a.mean[i] = running_mean[c];
      a.rstd[i] = (float)(1.0 / sqrt((double)running_var[c] + (double)a.eps));
      if (a.scale != nullptr) {
        const float sc = a.rstd[i] * (gamma ? gamma[c] : 1.f);
        a.scale[i] = sc;
        a.shift[i] = (beta ? beta[c] : 0.f) - a.mean[i] * sc;
      }
      return;
    }
    for (int m = m0; m < m0 + a.ns.ips; ++m) { S += a.tot[((long long)m * a.C + c) * 2]; Q += a.tot[((long long)m * a.C + c) * 2 + 1]; }
    cnt = a.count * a.ns.ips;
  } else {
    const int cg = a.C / a.groups, g0 = (c / cg) * cg;
    for (int k = g0; k < g0 + cg; ++k) { S += a.tot[((long long)n * a.C + k) * 2]; Q += a.tot[((long long)n * a.C + k) * 2 + 1]; }
    cnt = a.count * cg;
  }
  const double mu = S / cnt;
  double var = Q / cnt - mu * mu;
  if (var < 0.0) var = 0.0;
  a.mean[i] = (float)mu;
  a.rstd[i] = (float)(1.0 / sqrt(var + (double)a.eps));
  if (a.scale != nullptr) {
    const float sc = a.rstd[i] * (gamma ? gamma[c] : 1.f);
    a.scale[i] = sc;
    a.shift[i] = (beta ? beta[c] : 0.f) - a.mean[i] * sc;
  }
  if (a.kind == MMTTA_NORM_BATCH && a.training && n == m0 && running_mean != nullptr) {
    const double unb = cnt > 1.0 ? var * cnt / (cnt - 1.0) : var;
    running_mean[c] = (float)((1.0 - a.momentum) * running_mean[c] + a.momentum * mu);
    running_var[c] = (float)((1.0 - a.momentum) * running_var[c] + a.momentum * unb);
  }
}

struct BwdFinArgs {
  int kind, groups, N, C;
  double count;
  const float* gamma;
  int training;
  float* m1; float* m2; float* dgamma; float* dbeta; int accumulate;
  const double* tot;
  NSets ns;
};

__global__ void bwd_finalize_kernel(BwdFinArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.N * a.C) return;
  const int n = i / a.C, c = i % a.C;
  const int q = n / a.ns.ips, m0 = q * a.ns.ips;          // this item's set and its first item
  const float* gamma = a.gamma ? a.gamma + q * a.ns.astride : nullptr;
  double A = 0.0, B = 0.0, cnt = 1.0;
  if (a.kind == MMTTA_NORM_INSTANCE) {
    const double g = gamma ? (double)gamma[c] : 1.0;
    A = g * a.tot[(long long)i * 2]; B = g * a.tot[(long long)i * 2 + 1]; cnt = a.count;
  } else if (a.kind == MMTTA_NORM_BATCH) {
    const double g = gamma ? (double)gamma[c] : 1.0;
    for (int m = m0; m < m0 + a.ns.ips; ++m) { A += g * a.tot[((long long)m * a.C + c) * 2]; B += g * a.tot[((long long)m * a.C + c) * 2 + 1]; }
    cnt = a.count * a.ns.ips;
  } else {
    const int cg = a.C / a.groups, g0 = (c / cg) * cg;
    for (int k = g0; k < g0 + cg; ++k) {
      const double g = gamma ? (double)gamma[k] : 1.0;
      A += g * a.tot[((long long)n * a.C + k) * 2]; B += g * a.tot[((long long)n * a.C + k) * 2 + 1];
    }
    cnt = a.count * cg;
  }
  const bool frozen = (a.kind == MMTTA_NORM_BATCH && !a.training);
  a.m1[i] = frozen ? 0.f : (float)(A / cnt);
  a.m2[i] = frozen ? 0.f : (float)(B / cnt);
  if (n == m0 && a.dgamma != nullptr) {
    double dg = 0.0, db = 0.0;
    for (int m = m0; m < m0 + a.ns.ips; ++m) { db += a.tot[((long long)m * a.C + c) * 2]; dg += a.tot[((long long)m * a.C + c) * 2 + 1]; }
    float* dgamma = a.dgamma + q * a.ns.astride;
    dgamma[c] = a.accumulate ? dgamma[c] + (float)dg : (float)dg;
    if (a.dbeta) {
      float* dbeta = a.dbeta + q * a.ns.astride;
      dbeta[c] = a.accumulate ? dbeta[c] + (float)db : (float)db;
    }
  }
}

// ------------------------------------------------------------------ elementwise (channel fastest)
struct EwArgs {
  TV a, b, o;
  NL ta, tb;
  const float* m1; const float* m2;
  int hasb;
  int pa, pb;   // ta / tb carry per-item gamma / beta [N*C] (mmtta_norm_on_load.per_item)
};

// item n's view of a norm-on-load whose gamma / beta are per item ([N*C]): the [C] vectors of that item
__device__ __forceinline__ NL nl_item(NL t, int per_item, int n, int C) {
  if (per_item) {
    if (t.gamma) t.gamma += (long long)n * C;
    if (t.beta) t.beta += (long long)n * C;
  }
  return t;
}

// MODE 0: combine  out = Ta(a) + Tb(b)
// MODE 1: norm bwd apply: a = dout, b = y, T = ta(on y)   out = rstd*(g*dz - m1 - xhat*m2)
template <int MODE, int VEC, bool ABF = false, bool BBF = false, bool OBF = false>
__global__ __launch_bounds__(256) void elementwise_kernel(EwArgs e) {
  const int C = e.o.c;
  const int CV = (C + VEC - 1) / VEC;
  const long long nvox = (long long)e.o.n * e.o.d * e.o.h * e.o.w;
  const long long total = nvox * CV;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c0 = (int)(i % CV) * VEC;
    const long long v = i / CV;
    int n, z, y, x;
    vox_decompose(e.o, v, n, z, y, x);
    float av[VEC], bv[VEC], ov[VEC];
    const long long ao = vox_addr(e.a, n, z, y, x) + c0;
    const long long bo = e.hasb ? vox_addr(e.b, n, z, y, x) + c0 : 0;
    const bool bp = e.hasb != 0;
    if (VEC == 4) {
      const float4 t = ld4_t<ABF>(e.a.p, ao);
      av[0] = t.x; av[1] = t.y; av[2] = t.z; av[3] = t.w;
      if (bp) { const float4 u = ld4_t<BBF>(e.b.p, bo); bv[0] = u.x; bv[1] = u.y; bv[2] = u.z; bv[3] = u.w; }
    } else {
      av[0] = ld1_t<ABF>(e.a.p, ao);
      if (bp) bv[0] = ld1_t<BBF>(e.b.p, bo);
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int c = c0 + j;
      if (MODE == 0) {
        float sa, ha;
        nl_coeff(nl_item(e.ta, e.pa, n, C), n, C, min(c, C - 1), sa, ha);
        float r = nl_apply(av[j], sa, ha, e.ta.relu);
        if (bp) {
          float sb, hb;
          nl_coeff(nl_item(e.tb, e.pb, n, C), n, C, min(c, C - 1), sb, hb);
          r += nl_apply(bv[j], sb, hb, e.tb.relu);
        }
        ov[j] = r;
      } else {
        const int cc = min(c, C - 1);                 // pad lanes of a padded row compute on channel C-1's values
        const float mu = e.ta.mean[n * C + cc], rs = e.ta.rstd[n * C + cc];
        const int ab = e.pa ? n * C : 0;
        const float g = e.ta.gamma ? e.ta.gamma[ab + cc] : 1.f;
        const float bt = e.ta.beta ? e.ta.beta[ab + cc] : 0.f;
        const float xhat = (bv[j] - mu) * rs;
        float dz = av[j];
        MMTTA_ACT_BWD(dz, e.ta.relu, fmaf(g, xhat, bt));
        ov[j] = rs * (g * dz - e.m1[n * C + cc] - xhat * e.m2[n * C + cc]);
      }
    }
    const long long oo = vox_addr(e.o, n, z, y, x) + c0;
    if (VEC == 4) st4_t<OBF>(e.o.p, oo, make_float4(ov[0], ov[1], ov[2], ov[3]));
    else st1_t<OBF>(e.o.p, oo, ov[0]);
  }
}

// ------------------------------------------------------------------ norm backward apply, 8 channels per thread
// The same arithmetic as elementwise_kernel<1, ...> for voxel-dense tensors with C a power of two >= 8: a thread keeps ONE
// channel octet (its 48 coefficients are loaded once, as 16-byte loads) and walks IT voxels whose loads are all issued before
// the first use; 32-bit element offsets from the batch item's base, no division per element.
struct Nb8Args {
  const float* dout; const float* y; float* o;
  long long dsn, ysn, osn;
  unsigned dsw, ysw, osw;
  int C;
  act_t relu;
  unsigned dhw;
  const float* mean; const float* rstd; const float* gamma; const float* beta; const float* m1; const float* m2;
  int per_item;   // gamma / beta [N*C] (mmtta_norm_on_load.per_item)
};

template <bool YBF, int IT, bool DBF = false>
__global__ __launch_bounds__(256) void norm_bwd_apply8_kernel(Nb8Args a) {
  const int n = blockIdx.y;
  const unsigned CG = (unsigned)a.C >> 3, nvl = 256u / CG;
  const unsigned cg = threadIdx.x & (CG - 1), vl = threadIdx.x / CG;   // CG is a power of two
  const unsigned c0 = cg * 8;
  const float* dp = item_base<DBF>(a.dout, n, a.dsn);                 // gradient in / out share one storage type (DBF)
  const float* yp = item_base<YBF>(a.y, n, a.ysn);
  float* op = const_cast<float*>(item_base<DBF>(a.o, n, a.osn));
  const unsigned v0 = blockIdx.x * (nvl * IT) + vl;
  Oct8<YBF> yr[IT];
  Oct8<DBF> dr[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const unsigned v = min(v0 + i * nvl, a.dhw - 1);                   // clamped address, masked store
    yr[i] = oct8_ld<YBF>(yp, v * a.ysw + c0, v * a.ysw + c0 + 4);
    dr[i] = oct8_ld<DBF>(dp, v * a.dsw + c0, v * a.dsw + c0 + 4);
  }
  float mu[8], rs[8], g[8], bt[8], m1[8], m2[8];
  {
    const unsigned pc = (unsigned)n * a.C + c0;
    auto ld8 = [](const float* p, unsigned off, float (&r)[8]) {
      const float4 lo = *reinterpret_cast<const float4*>(p + off), hi = *reinterpret_cast<const float4*>(p + off + 4);
      r[0] = lo.x; r[1] = lo.y; r[2] = lo.z; r[3] = lo.w; r[4] = hi.x; r[5] = hi.y; r[6] = hi.z; r[7] = hi.w;
    };
    ld8(a.mean, pc, mu); ld8(a.rstd, pc, rs); ld8(a.m1, pc, m1); ld8(a.m2, pc, m2);
    const unsigned ac = a.per_item ? pc : c0;
    if (a.gamma) ld8(a.gamma, ac, g);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = 1.f;
    }
    if (a.beta) ld8(a.beta, ac, bt);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) bt[j] = 0.f;
    }
  }
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    float yv[8], ov[8], dv[8];
    oct8_f8(yr[i], yv);
    oct8_f8(dr[i], dv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xhat = (yv[j] - mu[j]) * rs[j];
      float dz = dv[j];
      MMTTA_ACT_BWD(dz, a.relu, fmaf(g[j], xhat, bt[j]));
      ov[j] = rs[j] * (g[j] * dz - m1[j] - xhat * m2[j]);
    }
    const unsigned v = v0 + i * nvl;
    if (v < a.dhw) oct8_st<DBF>(op, v * a.osw + c0, ov);
  }
}

// ------------------------------------------------------------------ whole instance-norm backward of a small tensor
// The deep levels (<= 16^3 voxels) ran reduce -> finalize -> apply as three launches of a few microseconds each, all of
// them launch latency.  Here one workgroup owns 32 channels of one batch item: pass 1 sums dz and dz * xhat over all
// voxels (a thread keeps one channel octet, 64 voxel lanes), the 64 partials of a channel are added in a fixed order
// in fp64 (like instance_bwd_kernel), pass 2 re-reads the two tensors (L2 hits) and writes dy.  No affine gradients.
struct NbsArgs {
  const float* dout; const float* y; float* o;
  long long dsn, ysn, osn;
  unsigned dsw, ysw, osw;
  int C;
  act_t relu;
  unsigned dhw;
  double count;
  const float* mean; const float* rstd; const float* gamma; const float* beta;
  int per_item;   // gamma / beta [N*C] (mmtta_norm_on_load.per_item)
};

template <bool YBF, bool DBF = false>
__global__ __launch_bounds__(256) void norm_bwd_small_kernel(NbsArgs a) {
  __shared__ float part[2][8][256];
  __shared__ float mm[2][32];
  const int n = blockIdx.y;
  const unsigned cg = threadIdx.x & 3, vl = threadIdx.x >> 2;
  const unsigned c0 = blockIdx.x * 32 + cg * 8;
  const float* dp = item_base<DBF>(a.dout, n, a.dsn);
  const float* yp = item_base<YBF>(a.y, n, a.ysn);
  float* op = const_cast<float*>(item_base<DBF>(a.o, n, a.osn));
  float mu[8], rs[8], g[8], bt[8];
  {
    const unsigned pc = (unsigned)n * a.C + c0;
    auto ld8 = [](const float* p, unsigned off, float (&r)[8]) {
      const float4 lo = *reinterpret_cast<const float4*>(p + off), hi = *reinterpret_cast<const float4*>(p + off + 4);
      r[0] = lo.x; r[1] = lo.y; r[2] = lo.z; r[3] = lo.w; r[4] = hi.x; r[5] = hi.y; r[6] = hi.z; r[7] = hi.w;
    };
    ld8(a.mean, pc, mu); ld8(a.rstd, pc, rs);
    const unsigned ac = a.per_item ? pc : c0;
    if (a.gamma) ld8(a.gamma, ac, g);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = 1.f;
    }
    if (a.beta) ld8(a.beta, ac, bt);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) bt[j] = 0.f;
    }
  }
  constexpr int IT = 2;
  float s0[8], s1[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { s0[j] = 0.f; s1[j] = 0.f; }
  for (unsigned vb = vl; vb < a.dhw; vb += 64 * IT) {
    Oct8<YBF> yr[IT];
    Oct8<DBF> dr[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const unsigned v = min(vb + 64 * i, a.dhw - 1);
      yr[i] = oct8_ld<YBF>(yp, v * a.ysw + c0, v * a.ysw + c0 + 4);
      dr[i] = oct8_ld<DBF>(dp, v * a.dsw + c0, v * a.dsw + c0 + 4);
    }
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      float yv[8], dv[8];
      oct8_f8(yr[i], yv);
      oct8_f8(dr[i], dv);
      const bool live = vb + 64 * i < a.dhw;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xhat = (yv[j] - mu[j]) * rs[j];
        float dz = live ? dv[j] : 0.f;
        MMTTA_ACT_BWD(dz, a.relu, fmaf(g[j], xhat, bt[j]));
        s0[j] += dz;
        s1[j] += dz * xhat;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { part[0][j][threadIdx.x] = s0[j]; part[1][j][threadIdx.x] = s1[j]; }
  __syncthreads();
  if (threadIdx.x < 64) {                        // thread -> (k, octet, j): the 64 voxel-lane partials of one channel
    const int k = threadIdx.x >> 5, q = (threadIdx.x >> 3) & 3, j = threadIdx.x & 7;
    double t = 0.0;
    for (int l = 0; l < 64; ++l) t += (double)part[k][j][l * 4 + q];
    const int c = blockIdx.x * 32 + q * 8 + j;
    const double gm = a.gamma ? (double)a.gamma[(a.per_item ? n * a.C : 0) + c] : 1.0;
    mm[k][q * 8 + j] = (float)(gm * t / a.count);
  }
  __syncthreads();
  float m1[8], m2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { m1[j] = mm[0][cg * 8 + j]; m2[j] = mm[1][cg * 8 + j]; }
  for (unsigned vb = vl; vb < a.dhw; vb += 64 * IT) {
    Oct8<YBF> yr[IT];
    Oct8<DBF> dr[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const unsigned v = min(vb + 64 * i, a.dhw - 1);
      yr[i] = oct8_ld<YBF>(yp, v * a.ysw + c0, v * a.ysw + c0 + 4);
      dr[i] = oct8_ld<DBF>(dp, v * a.dsw + c0, v * a.dsw + c0 + 4);
    }
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      float yv[8], ov[8], dv[8];
      oct8_f8(yr[i], yv);
      oct8_f8(dr[i], dv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xhat = (yv[j] - mu[j]) * rs[j];
        float dz = dv[j];
        MMTTA_ACT_BWD(dz, a.relu, fmaf(g[j], xhat, bt[j]));
        ov[j] = rs[j] * (g[j] * dz - m1[j] - xhat * m2[j]);
      }
      const unsigned v = vb + 64 * i;
      if (v < a.dhw) oct8_st<DBF>(op, v * a.osw + c0, ov);
    }
  }
}

// ------------------------------------------------------------------ combine, 8 channels per thread
// out = Ta(a) + Tb(b) for voxel-dense tensors of one storage type with C a power of two >= 8: the same arithmetic as
// elementwise_kernel<0, ...>, a thread's 16 coefficient pairs computed once, IT voxels' loads issued before the first use.
struct Cb8Args {
  const float* a; const float* b; float* o;
  long long asn, bsn, osn;
  unsigned asw, bsw, osw;
  int C;
  unsigned dhw;
  NL ta, tb;
  int pa, pb;   // per-item gamma / beta of ta / tb
};

template <bool BF, bool HASB, int IT>
__global__ __launch_bounds__(256) void combine8_kernel(Cb8Args e) {
  const int n = blockIdx.y;
  const unsigned CG = (unsigned)e.C >> 3, nvl = 256u / CG;
  const unsigned cg = threadIdx.x & (CG - 1), vl = threadIdx.x / CG;   // CG is a power of two
  const unsigned c0 = cg * 8;
  auto item = [&](const float* p, long long sn) {
    return BF ? reinterpret_cast<const float*>(reinterpret_cast<const unsigned short*>(p) + (long long)n * sn) : p + (long long)n * sn;
  };
  const float* ap = item(e.a, e.asn);
  const float* bp = HASB ? item(e.b, e.bsn) : ap;
  float* op = const_cast<float*>(item(e.o, e.osn));
  const unsigned v0 = blockIdx.x * (nvl * IT) + vl;
  Oct8<BF> ar[IT], br[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const unsigned v = min(v0 + i * nvl, e.dhw - 1);                   // clamped address, masked store
    ar[i] = oct8_ld<BF>(ap, v * e.asw + c0, v * e.asw + c0 + 4);
    if (HASB) br[i] = oct8_ld<BF>(bp, v * e.bsw + c0, v * e.bsw + c0 + 4);
  }
  float sa[8], ha[8], sb[8], hb[8];
  nl_coeff_vec<8>(nl_item(e.ta, e.pa, n, e.C), n, e.C, (int)c0, sa, ha);
  if (HASB) nl_coeff_vec<8>(nl_item(e.tb, e.pb, n, e.C), n, e.C, (int)c0, sb, hb);
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    float av[8], bv[8], ov[8];
    oct8_f8(ar[i], av);
    if (HASB) oct8_f8(br[i], bv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float r = nl_apply(av[j], sa[j], ha[j], e.ta.relu);
      if (HASB) r += nl_apply(bv[j], sb[j], hb[j], e.tb.relu);
      ov[j] = r;
    }
    const unsigned v = v0 + i * nvl;
    if (v < e.dhw) {
      if constexpr (BF) {
        uint4 q;
        q.x = f32x2_to_bf16x2(ov[0], ov[1]); q.y = f32x2_to_bf16x2(ov[2], ov[3]);
        q.z = f32x2_to_bf16x2(ov[4], ov[5]); q.w = f32x2_to_bf16x2(ov[6], ov[7]);
        *reinterpret_cast<uint4*>(reinterpret_cast<unsigned short*>(op) + v * e.osw + c0) = q;
      } else {
        *reinterpret_cast<float4*>(op + v * e.osw + c0) = make_float4(ov[0], ov[1], ov[2], ov[3]);
        *reinterpret_cast<float4*>(op + v * e.osw + c0 + 4) = make_float4(ov[4], ov[5], ov[6], ov[7]);
      }
    }
  }
}

template <bool BF, bool HASB>
static void launch_combine8(const Cb8Args& q, const mmtta_pointwise_route_t& r, hipStream_t s) {
  const dim3 g8((unsigned)r.grid_x, (unsigned)r.grid_y);
  if (r.it == 4) hipLaunchKernelGGL((combine8_kernel<BF, HASB, 4>), g8, dim3(256), 0, s, q);
  else hipLaunchKernelGGL((combine8_kernel<BF, HASB, 2>), g8, dim3(256), 0, s, q);
}

// ------------------------------------------------------------------ linear combination
struct LinArgs {
  TV in[8];
  float w[8];
  int count;
  TV o;
  int accumulate;
};

// COUNT inputs are a template parameter: their loads are straight-line (a load behind a run-time `k < count`
// branch is waited for before the next one is issued)
// IBF / OBF: storage of the inputs (all alike) and of the output (bf16: the wide forward activations of bf16 precision)
template <int VEC, int COUNT, bool IBF = false, bool OBF = false>
__global__ __launch_bounds__(256) void lincomb_kernel(LinArgs e) {
  const int C = e.o.c;
  const int CV = (C + VEC - 1) / VEC;
  const long long nvox = (long long)e.o.n * e.o.d * e.o.h * e.o.w;
  const long long total = nvox * CV;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c0 = (int)(i % CV) * VEC;
    const long long v = i / CV;
    int n, z, y, x;
    vox_decompose(e.o, v, n, z, y, x);
    float acc[VEC];
    const long long oo = vox_addr(e.o, n, z, y, x) + c0;          // element offsets: the same code addresses 2- and 4-byte elements
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
    if (e.accumulate) {
      if (VEC == 4) { const float4 t = ld4_t<OBF>(e.o.p, oo); acc[0] = t.x; acc[1] = t.y; acc[2] = t.z; acc[3] = t.w; }
      else acc[0] = ld1_t<OBF>(e.o.p, oo);
    }
    float4 tv4[COUNT];
    float ts[COUNT];
#pragma unroll
    for (int k = 0; k < COUNT; ++k) {
      const long long io = vox_addr(e.in[k], n, z, y, x) + c0;
      if (VEC == 4) tv4[k] = ld4_t<IBF>(e.in[k].p, io);
      else ts[k] = ld1_t<IBF>(e.in[k].p, io);
    }
#pragma unroll
    for (int k = 0; k < COUNT; ++k) {
      if (VEC == 4) {
        acc[0] = fmaf(e.w[k], tv4[k].x, acc[0]); acc[1] = fmaf(e.w[k], tv4[k].y, acc[1]);
        acc[2] = fmaf(e.w[k], tv4[k].z, acc[2]); acc[3] = fmaf(e.w[k], tv4[k].w, acc[3]);
      } else {
        acc[0] = fmaf(e.w[k], ts[k], acc[0]);
      }
    }
    if (VEC == 4) st4_t<OBF>(e.o.p, oo, make_float4(acc[0], acc[1], acc[2], acc[3]));
    else st1_t<OBF>(e.o.p, oo, acc[0]);
  }
}

// ------------------------------------------------------------------ trilinear x2 (align_corners=True)
__device__ __forceinline__ void src_index(int dst, int in, int out, int& i0, int& i1, float& lam) {
  // torch: scale = (in-1)/(out-1) (0 when out == 1); src = scale*dst; i0 = floor; i1 = min(i0+1, in-1)
  const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  const float src = scale * (float)dst;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  lam = src - (float)i0;
}

// VEC = 4: a thread owns 4 consecutive channels of one output voxel (16-byte accesses, index arithmetic amortised);
// VEC = 1: scalar fallback for unaligned views.
template <int VEC, bool BF = false>
__global__ __launch_bounds__(256) void upsample_fwd_kernel(TV x, TV y) {
  const int C = y.c;
  const int CV = (C + VEC - 1) / VEC;
  const long long total = (long long)y.n * y.d * y.h * y.w * CV;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % CV) * VEC;
    int n, oz, oy, ox;
    vox_decompose(y, i / CV, n, oz, oy, ox);
    int z0, z1, y0, y1, x0, x1;
    float lz, ly, lx;
    src_index(oz, x.d, y.d, z0, z1, lz);
    src_index(oy, x.h, y.h, y0, y1, ly);
    src_index(ox, x.w, y.w, x0, x1, lx);
    const float* xp = x.p;
    const long long xb = (long long)n * x.sn + c;                 // element offset of (item, channel): x and y share one storage (BF)
    const float wz0 = 1.f - lz, wy0 = 1.f - ly, wx0 = 1.f - lx;
    const long long o00 = (long long)z0 * x.sd + (long long)y0 * x.sh, o01 = (long long)z0 * x.sd + (long long)y1 * x.sh;
    const long long o10 = (long long)z1 * x.sd + (long long)y0 * x.sh, o11 = (long long)z1 * x.sd + (long long)y1 * x.sh;
    const long long a0 = (long long)x0 * x.sw, a1 = (long long)x1 * x.sw;
    const long long oo = vox_addr(y, n, oz, oy, ox) + c;
    if (VEC == 4) {
      const float4 v000 = ld4_t<BF>(xp, xb + o00 + a0), v001 = ld4_t<BF>(xp, xb + o00 + a1);
      const float4 v010 = ld4_t<BF>(xp, xb + o01 + a0), v011 = ld4_t<BF>(xp, xb + o01 + a1);
      const float4 v100 = ld4_t<BF>(xp, xb + o10 + a0), v101 = ld4_t<BF>(xp, xb + o10 + a1);
      const float4 v110 = ld4_t<BF>(xp, xb + o11 + a0), v111 = ld4_t<BF>(xp, xb + o11 + a1);
#define MMTTA_TRI(f) (wz0 * (wy0 * (wx0 * v000.f + lx * v001.f) + ly * (wx0 * v010.f + lx * v011.f)) + \
                      lz * (wy0 * (wx0 * v100.f + lx * v101.f) + ly * (wx0 * v110.f + lx * v111.f)))
      st4_t<BF>(y.p, oo, make_float4(MMTTA_TRI(x), MMTTA_TRI(y), MMTTA_TRI(z), MMTTA_TRI(w)));
#undef MMTTA_TRI
    } else {
      auto X = [&](long long o) { return ld1_t<BF>(xp, xb + o); };
      const float v = wz0 * (wy0 * (wx0 * X(o00 + a0) + lx * X(o00 + a1)) + ly * (wx0 * X(o01 + a0) + lx * X(o01 + a1))) +
                      lz * (wy0 * (wx0 * X(o10 + a0) + lx * X(o10 + a1)) + ly * (wx0 * X(o11 + a0) + lx * X(o11 + a1)));
      st1_t<BF>(y.p, oo, v);
    }
  }
}

// adjoint as a gather: for input index i the outputs that touch it lie in [2i-2, 2i+2]
__device__ __forceinline__ int axis_weights(int i, int in, int out, int* os, float* ws) {
  int cnt = 0;
  int lo = 2 * i - 2, hi = 2 * i + 2;
  if (lo < 0) lo = 0;
  if (hi > out - 1) hi = out - 1;
  for (int o = lo; o <= hi; ++o) {
    int i0, i1;
    float lam;
    src_index(o, in, out, i0, i1, lam);
    float w = 0.f;
    if (i0 == i) w += 1.f - lam;
    if (i1 == i) w += lam;   // i0 == i1 == i at the last sample: (1-lam) + lam = 1
    if (i0 == i1 && i0 == i) w = 1.f;
    if (w != 0.f) { os[cnt] = o; ws[cnt] = w; ++cnt; }
  }
  return cnt;
}

// BF: both gradients bf16-stored (method.grad_storage; offsets are elements either way)
template <int VEC, bool BF = false>
__global__ __launch_bounds__(256) void upsample_bwd_kernel(TV dy, TV dx, int accumulate) {
  const int C = dx.c;
  const int CV = (C + VEC - 1) / VEC;
  const long long total = (long long)dx.n * dx.d * dx.h * dx.w * CV;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % CV) * VEC;
    int n, iz, iy, ix;
    vox_decompose(dx, i / CV, n, iz, iy, ix);
    int oz[5], oy[5], ox[5];
    float wz[5], wy[5], wx[5];
    const int nz = axis_weights(iz, dx.d, dy.d, oz, wz);
    const int ny = axis_weights(iy, dx.h, dy.h, oy, wy);
    const int nx = axis_weights(ix, dx.w, dy.w, ox, wx);
    const long long gbase = (long long)n * dy.sn + c;
    float s[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) s[j] = 0.f;
    for (int a = 0; a < nz; ++a)
      for (int b = 0; b < ny; ++b) {
        const float wzy = wz[a] * wy[b];
        const long long row = gbase + (long long)oz[a] * dy.sd + (long long)oy[b] * dy.sh;
        for (int k = 0; k < nx; ++k) {
          const float wgt = wzy * wx[k];
          if (VEC == 4) {
            const float4 g4 = ld4_any(dy.p, row + (long long)ox[k] * dy.sw, BF);
            s[0] = fmaf(wgt, g4.x, s[0]); s[1] = fmaf(wgt, g4.y, s[1]); s[2] = fmaf(wgt, g4.z, s[2]); s[3] = fmaf(wgt, g4.w, s[3]);
          } else {
            s[0] += wgt * ld1_any(dy.p, row + (long long)ox[k] * dy.sw, BF);
          }
        }
      }
    const long long o = vox_addr(dx, n, iz, iy, ix) + c;
    if (VEC == 4) {
      float4 r = make_float4(s[0], s[1], s[2], s[3]);
      if (accumulate) { const float4 t = ld4_any(dx.p, o, BF); r.x += t.x; r.y += t.y; r.z += t.z; r.w += t.w; }
      st4_any(dx.p, o, r, BF);
    } else {
      st1_any(dx.p, o, accumulate ? ld1_any(dx.p, o, BF) + s[0] : s[0], BF);
    }
  }
}

static inline int grid_for(long long total, int cap = 8192) {
  long long b = (total + 255) / 256;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}

// 16-byte access to 4 channels at a time.  C need not be a multiple of 4 when the voxel row is padded to one
// (sw >= roundup(C,4)): READING the pad lanes is always harmless; WRITING them needs a view that owns its pad.
static inline bool vec4_rd(const mmtta_tensor* t) {
  return quad_aligned(t, quad_bytes(t)) && t->sc == 1 && (t->c % 4 == 0 || t->sw >= (t->c + 3) / 4 * 4);
}
static inline bool vec4_wr(const mmtta_tensor* t) {
  return vec4_rd(t) && (t->c % 4 == 0 || (t->flags & MMTTA_TENSOR_OWNS_PAD));
}

static void rows_geometry(const mmtta_tensor* t, int& rows_per_n, long long& vox_per_row) {
  const long long dhw = (long long)t->d * t->h * t->w;
  long long vpr = (dhw + 1023) / 1024;     // at most 1024 rows per batch item
  if (vpr < 32) vpr = 32;
  rows_per_n = (int)((dhw + vpr - 1) / vpr);
  if (rows_per_n < 1) rows_per_n = 1;
  vox_per_row = vpr;
}

// ---- the streamed two-stage reduction (channel_reduce_stream_kernel): which operands take it, and its launch
static inline bool dense_voxels(const mmtta_tensor* t) { return t->sh == (int64_t)t->w * t->sw && t->sd == (int64_t)t->h * t->sh; }
// `d`: the second tensor of MODE 1 (null for MODE 0).  Voxel-dense 4-channel-vector operands, one pass over the channel
// lanes (C <= 1024), 32-bit element offsets inside an item; everything else keeps channel_reduce_kernel.
static bool reduce_stream_ok(const mmtta_tensor* x, const mmtta_tensor* d) {
  const int64_t pad = (x->c + 3) / 4 * 4;
  auto ok = [pad](const mmtta_tensor* t) { return vec4_rd(t) && dense_voxels(t) && item_fits_31(t, pad); };
  const int64_t dhw = (int64_t)x->d * x->h * x->w;
  return ok(x) && (!d || ok(d)) && x->c >= 1 && x->c <= 1024 && dhw >= 1 && dhw < ((int64_t)1 << 31) && x->n >= 1 && x->n <= 65535;
}

// ---- host-side planning: which kernel an entry point runs and on what launch geometry.  The launchers below and
// mmtta_pointwise_route call the same functions, so the answer of the query is the launch (tests assert the route first).
typedef mmtta_pointwise_route_t PwRoute;

static inline long long vox_count(const mmtta_tensor* t) { return (long long)t->d * t->h * t->w; }

// a grid-stride kernel: `total` work items on at most `cap` workgroups of 256
static inline void route_grid_stride(PwRoute& r, long long total, int cap = 8192) {
  r.work_items = total;
  r.grid_x = grid_for(total, cap);
  r.grid_y = 1;
  r.second_trip = total > r.grid_x * 256 ? 1 : 0;
}

// the octet kernels (combine8 / norm_bwd_apply8 / norm_bwd_small): 16-byte aligned octets of a voxel-dense tensor
static inline bool oct_aligned(const mmtta_tensor* t) {
  const int per = is_bf16(t) ? 8 : 4;
  return ((uintptr_t)t->ptr) % 16 == 0 && t->sw % per == 0 && t->sn % per == 0;
}
static inline bool oct_channels(int C) { return C >= 8 && C <= 2048 && (C & (C - 1)) == 0; }
static inline bool null_or_16(const void* p) { return p == nullptr || ((uintptr_t)p) % 16 == 0; }
// voxels per thread (IT 4 from 1024 workgroups per item on) and the grid of combine8 / norm_bwd_apply8
static inline void route_octets(PwRoute& r, int C, long long dhw, int n) {
  const long long nvl = 256 / (C / 8);
  const bool four = dhw / (nvl * 4) >= 1024;
  const long long per = nvl * (four ? 4 : 2);
  r.vec = 8; r.it = four ? 4 : 2; r.cpl = C / 8; r.nvl = (int)nvl; r.trips = 1;
  r.grid_x = (dhw + per - 1) / per; r.grid_y = n;
  r.work_items = dhw * n * (C / 8);
}

// the streamed reduction's schedule
struct StreamGeo { unsigned cpl, nvl, trips, it, rpb; };
static inline StreamGeo stream_geometry(unsigned C, unsigned vox_per_row, unsigned rows_per_n, int n) {
  StreamGeo g;
  g.cpl = 1;
  while (g.cpl < (C + 3) / 4) g.cpl <<= 1;
  g.nvl = 256u / g.cpl;
  g.trips = (vox_per_row + g.nvl - 1) / g.nvl;
  // Rows per workgroup.  A row of several chunks overlaps its own loads and adds, and one row per workgroup balances best
  // (measured, groups of 8: 64^3 x 32 and 128^3 x 3 are fastest at 1).  A row of ONE chunk has nothing to overlap with but
  // the next row: 4 rows per workgroup (32^3 x 64: 23 us at 1, 14 us at 4), fewer where the launch would shrink below
  // 512 workgroups.
  g.it = g.trips >= 4 ? 4 : (g.trips >= 2 ? 2 : 1);
  const unsigned chunks = (g.trips + g.it - 1) / g.it, total = (unsigned)n * rows_per_n;
  g.rpb = 1;
  if (chunks == 1) g.rpb = total / 512 < 1 ? 1 : (total / 512 > 4 ? 4 : total / 512);
  return g;
}

// MODE 0 (`d` null): channel sums of x.  MODE 1: the norm-backward sums of (y = x, dout = d).
static inline PwRoute reduce_plan(const mmtta_tensor* x, const mmtta_tensor* d) {
  PwRoute r = {};
  r.mode = d ? 1 : 0;
  r.bf16_a = is_bf16(x) ? 1 : 0; r.bf16_b = d && is_bf16(d) ? 1 : 0;
  int rows; long long vpr;
  rows_geometry(x, rows, vpr);
  r.rows_per_n = rows; r.vox_per_row = vpr;
  if (reduce_stream_ok(x, d)) {
    const StreamGeo g = stream_geometry((unsigned)x->c, (unsigned)vpr, (unsigned)rows, x->n);
    r.family = MMTTA_PW_REDUCE_STREAM; r.vec = 4; r.it = (int)g.it;
    r.cpl = (int)g.cpl; r.nvl = (int)g.nvl; r.trips = (int)g.trips; r.rows_per_block = (int)g.rpb; r.cb_passes = 1;
    r.grid_x = (rows + g.rpb - 1) / g.rpb; r.grid_y = x->n;
  } else {
    const bool v4 = vec4_rd(x) && (!d || vec4_rd(d));
    r.family = MMTTA_PW_REDUCE; r.vec = v4 ? 4 : 1; r.it = 1;
    const int cv = (x->c + r.vec - 1) / r.vec;
    int cpl = 1;
    while (cpl < cv && cpl < 256) cpl <<= 1;            // channel_reduce_kernel's own block layout
    r.cpl = cpl; r.nvl = 256 / cpl; r.trips = (int)((vpr + r.nvl - 1) / r.nvl);
    r.rows_per_block = 1; r.cb_passes = (cv + cpl - 1) / cpl;
    r.grid_x = (long long)x->n * rows; r.grid_y = 1;
  }
  r.work_items = (long long)x->n * vox_count(x) * ((x->c + r.vec - 1) / r.vec);
  return r;
}

static inline int combine_check(const mmtta_tensor* a, const mmtta_tensor* b, const mmtta_tensor* out) {
  MMTTA_CHECK(a && out && a->ptr && out->ptr, MMTTA_ERR_INVALID, "combine: null tensor");
  MMTTA_CHECK(same_shape(a, out) && (!b || same_shape(b, out)), MMTTA_ERR_INVALID, "combine: shape mismatch");
  MMTTA_CHECK(is_cl(a) && is_cl(out) && (!b || is_cl(b)), MMTTA_ERR_UNSUPPORTED, "combine: channels-last only");
  // storage: all fp32, or all bf16 (the wide forward activations of bf16 precision)
  const bool abf = is_bf16(a), bbf = b ? is_bf16(b) : abf, obf = is_bf16(out);
  MMTTA_CHECK((abf == bbf && bbf == obf), MMTTA_ERR_UNSUPPORTED, "combine: operands must share one storage type");
  return MMTTA_OK;
}
static inline bool combine_v4(const mmtta_tensor* a, const mmtta_tensor* b, const mmtta_tensor* out) {
  return vec4_rd(a) && vec4_wr(out) && (!b || vec4_rd(b));
}
// octet form: C a power of two in [8, 2048], voxel-dense tensors, 16-byte aligned octets, 32-bit offsets inside an item
static inline bool combine_ok8(const mmtta_tensor* a, const mmtta_tensor* b, const mmtta_tensor* out) {
  return combine_v4(a, b, out) && oct_channels(out->c) && dense_voxels(a) && dense_voxels(out) && oct_aligned(a) &&
         oct_aligned(out) && (!b || (dense_voxels(b) && oct_aligned(b))) &&
         vox_count(out) * std::max(std::max(a->sw, out->sw), b ? b->sw : (int64_t)0) < (1LL << 31);
}
static inline PwRoute combine_plan(const mmtta_tensor* a, const mmtta_tensor* b, const mmtta_tensor* out) {
  PwRoute r = {};
  r.mode = 0; r.has_b = b ? 1 : 0;
  r.bf16_a = r.bf16_b = r.bf16_o = is_bf16(out) ? 1 : 0;
  if (combine_ok8(a, b, out)) {
    r.family = MMTTA_PW_COMBINE8;
    route_octets(r, out->c, vox_count(out), out->n);
    return r;
  }
  const bool v4 = combine_v4(a, b, out);
  r.family = MMTTA_PW_ELEMENTWISE; r.vec = v4 ? 4 : 1;
  route_grid_stride(r, (long long)out->n * vox_count(out) * (v4 ? (out->c + 3) / 4 : out->c));
  return r;
}

static inline int norm_bwd_reduce_check(const mmtta_tensor* dout, const mmtta_tensor* y, const mmtta_norm_on_load* t) {
  MMTTA_CHECK(dout && y && t && dout->ptr && y->ptr && t->mean && t->rstd, MMTTA_ERR_INVALID, "norm bwd reduce: null argument");
  // (a bf16-stored gradient sits next to a bf16-stored activation - or, <= 4 channels, next to an fp32-stored one: the thin
  // full-resolution tensors keep their activations fp32, round 3)
  MMTTA_CHECK(!is_bf16(dout) || is_bf16(y) || y->c <= 4, MMTTA_ERR_UNSUPPORTED, "norm bwd reduce: a bf16-stored gradient needs a bf16-stored activation");
  MMTTA_CHECK(same_shape(dout, y) && is_cl(dout) && is_cl(y), MMTTA_ERR_INVALID, "norm bwd reduce: shape/layout mismatch");
  return MMTTA_OK;
}

static inline int norm_bwd_apply_check(const mmtta_tensor* dout, const mmtta_tensor* y, const mmtta_norm_on_load* t,
                                       const float* m1, const float* m2, const mmtta_tensor* dy) {
  MMTTA_CHECK(dout && y && t && dy && m1 && m2 && t->mean && t->rstd, MMTTA_ERR_INVALID, "norm bwd apply: null argument");
  MMTTA_CHECK(dout->dtype == dy->dtype && (!is_bf16(dout) || is_bf16(y) || y->c <= 4), MMTTA_ERR_UNSUPPORTED,
              "norm bwd apply: `dout` and `dy` share one storage type (bf16 only next to a bf16-stored activation)");
  MMTTA_CHECK(same_shape(dout, y) && same_shape(dy, y), MMTTA_ERR_INVALID, "norm bwd apply: shape mismatch");
  MMTTA_CHECK(is_cl(dout) && is_cl(y) && is_cl(dy), MMTTA_ERR_UNSUPPORTED, "norm bwd apply: channels-last only");
  return MMTTA_OK;
}
static inline bool norm_bwd_apply_v4(const mmtta_tensor* dout, const mmtta_tensor* y, const mmtta_tensor* dy) {
  return vec4_rd(dout) && vec4_rd(y) && vec4_wr(dy);
}
// octet form: as combine_ok8, and the [N*C] coefficient vectors on 16 bytes
static inline bool norm_bwd_apply_ok8(const mmtta_tensor* dout, const mmtta_tensor* y, const mmtta_norm_on_load* t,
                                      const float* m1, const float* m2, const mmtta_tensor* dy) {
  return norm_bwd_apply_v4(dout, y, dy) && oct_channels(y->c) && dense_voxels(dout) && dense_voxels(y) && dense_voxels(dy) &&
         oct_aligned(dout) && oct_aligned(dy) && oct_aligned(y) && ((uintptr_t)t->mean % 16 == 0) &&
         ((uintptr_t)t->rstd % 16 == 0) && ((uintptr_t)m1 % 16 == 0) && ((uintptr_t)m2 % 16 == 0) && null_or_16(t->gamma) &&
         null_or_16(t->beta) && vox_count(y) * std::max(std::max(dout->sw, y->sw), dy->sw) < (1LL << 31);
}
static inline PwRoute norm_bwd_apply_plan(const mmtta_tensor* dout, const mmtta_tensor* y, const mmtta_norm_on_load* t,
                                          const float* m1, const float* m2, const mmtta_tensor* dy) {
  PwRoute r = {};
  r.mode = 1; r.has_b = 1;
  r.bf16_a = r.bf16_o = is_bf16(dout) ? 1 : 0; r.bf16_b = is_bf16(y) ? 1 : 0;
  if (norm_bwd_apply_ok8(dout, y, t, m1, m2, dy)) {
    r.family = MMTTA_PW_NORM_BWD_APPLY8;
    route_octets(r, y->c, vox_count(y), y->n);
    return r;
  }
  const bool v4 = norm_bwd_apply_v4(dout, y, dy);
  r.family = MMTTA_PW_ELEMENTWISE; r.vec = v4 ? 4 : 1;
  route_grid_stride(r, (long long)y->n * vox_count(y) * (v4 ? (y->c + 3) / 4 : y->c));
  return r;
}

static RedSArgs reduce_stream_args(const mmtta_tensor* x, const mmtta_tensor* d, const mmtta_norm_on_load* t, float* part) {
  RedSArgs q;
  q.x = (const float*)x->ptr; q.dout = d ? (const float*)d->ptr : nullptr;
  q.xsn = x->sn; q.dsn = d ? d->sn : 0;
  q.xsw = (unsigned)x->sw; q.dsw = d ? (unsigned)d->sw : 0u;
  q.C = (unsigned)x->c; q.dhw = (unsigned)((int64_t)x->d * x->h * x->w);
  int rows; long long vpr;
  rows_geometry(x, rows, vpr);
  q.rows_per_n = (unsigned)rows; q.vox_per_row = (unsigned)vpr; q.rows_per_block = 1;
  q.mean = t ? t->mean : nullptr; q.rstd = t ? t->rstd : nullptr; q.gamma = t ? t->gamma : nullptr; q.beta = t ? t->beta : nullptr;
  q.relu = act_arg(t); q.per_item = t && t->per_item != 0 ? 1 : 0;
  q.part = part;
  return q;
}

template <int MODE, bool XBF, bool DBF>
static void launch_reduce_stream(RedSArgs q, const PwRoute& r, hipStream_t s) {
  q.rows_per_block = (unsigned)r.rows_per_block;
  const dim3 grid((unsigned)r.grid_x, (unsigned)r.grid_y);
  const int it = r.it;
  if (it == 4) hipLaunchKernelGGL((channel_reduce_stream_kernel<MODE, 4, XBF, DBF>), grid, dim3(256), 0, s, q);
  else if (it == 2) hipLaunchKernelGGL((channel_reduce_stream_kernel<MODE, 2, XBF, DBF>), grid, dim3(256), 0, s, q);
  else hipLaunchKernelGGL((channel_reduce_stream_kernel<MODE, 1, XBF, DBF>), grid, dim3(256), 0, s, q);
}

int channel_partial_rows(const mmtta_tensor* t) {
  int r; long long v;
  rows_geometry(t, r, v);
  return r;
}

int launch_channel_sums(const mmtta_tensor* x, float* part, hipStream_t s) {
  RedArgs a;
  a.x = tv(x); a.dout = tv(x); a.t = nl(nullptr); a.per_item = 0; a.part = part;
  rows_geometry(x, a.rows_per_n, a.vox_per_row);
  const PwRoute r = reduce_plan(x, nullptr);
  const dim3 grid((unsigned)r.grid_x);
  if (r.family == MMTTA_PW_REDUCE_STREAM) {
    const RedSArgs q = reduce_stream_args(x, nullptr, nullptr, part);
    MMTTA_BF_DISPATCH(is_bf16(x), XBF, { launch_reduce_stream<0, XBF, false>(q, r, s); });
    return launch_status("channel sums");
  }
  const bool v4 = r.vec == 4;
  if (is_bf16(x)) {
    if (v4) hipLaunchKernelGGL((channel_reduce_kernel<0, 4, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((channel_reduce_kernel<0, 1, true>), grid, dim3(256), 0, s, a);
  } else {
    if (v4) hipLaunchKernelGGL((channel_reduce_kernel<0, 4>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((channel_reduce_kernel<0, 1>), grid, dim3(256), 0, s, a);
  }
  return launch_status("channel sums");
}

// ---- entry bodies (the C entry points below check the norm-on-load descriptors and pick the activation instantiation)
int combine_body(const mmtta_tensor* a, const mmtta_norm_on_load* ta, const mmtta_tensor* b,
                 const mmtta_norm_on_load* tb, const mmtta_tensor* out, void* stream) {
  const int st = combine_check(a, b, out);
  if (st) return st;
  EwArgs e;
  e.a = tv(a); e.b = b ? tv(b) : tv(a); e.o = tv(out); e.ta = nl(ta); e.tb = nl(tb); e.m1 = e.m2 = nullptr; e.hasb = b ? 1 : 0;
  e.pa = ta && ta->per_item ? 1 : 0;
  e.pb = b && tb && tb->per_item ? 1 : 0;
  const PwRoute r = combine_plan(a, b, out);
  const bool v4 = r.vec == 4, abf = is_bf16(a);
  const dim3 grid((unsigned)r.grid_x);
  hipStream_t s = (hipStream_t)stream;
  {
    if (r.family == MMTTA_PW_COMBINE8) {
      const int C = out->c;
      const long long dhw = vox_count(out);
      Cb8Args q;
      q.a = (const float*)a->ptr; q.b = b ? (const float*)b->ptr : nullptr; q.o = (float*)out->ptr;
      q.asn = a->sn; q.bsn = b ? b->sn : 0; q.osn = out->sn;
      q.asw = (unsigned)a->sw; q.bsw = b ? (unsigned)b->sw : 0u; q.osw = (unsigned)out->sw;
      q.C = C; q.dhw = (unsigned)dhw; q.ta = e.ta; q.tb = e.tb; q.pa = e.pa; q.pb = e.pb;
      if (abf) { if (b) launch_combine8<true, true>(q, r, s); else launch_combine8<true, false>(q, r, s); }
      else { if (b) launch_combine8<false, true>(q, r, s); else launch_combine8<false, false>(q, r, s); }
      return launch_status("combine");
    }
  }
  if (abf) {
    if (v4) hipLaunchKernelGGL((elementwise_kernel<0, 4, true, true, true>), grid, dim3(256), 0, s, e);
    else hipLaunchKernelGGL((elementwise_kernel<0, 1, true, true, true>), grid, dim3(256), 0, s, e);
  } else {
    if (v4) hipLaunchKernelGGL((elementwise_kernel<0, 4>), grid, dim3(256), 0, s, e);
    else hipLaunchKernelGGL((elementwise_kernel<0, 1>), grid, dim3(256), 0, s, e);
  }
  return launch_status("combine");
}

int norm_bwd_reduce_body(const mmtta_tensor* dout, const mmtta_tensor* y, const mmtta_norm_on_load* t,
                         float* part, void* stream) {
  MMTTA_CHECK(part != nullptr, MMTTA_ERR_INVALID, "norm bwd reduce: null argument");
  const int st = norm_bwd_reduce_check(dout, y, t);
  if (st) return st;
  RedArgs a;
  a.x = tv(y); a.dout = tv(dout); a.t = nl(t); a.per_item = t->per_item != 0 ? 1 : 0; a.part = part;
  rows_geometry(y, a.rows_per_n, a.vox_per_row);
  const PwRoute r = reduce_plan(y, dout);
  const dim3 grid((unsigned)r.grid_x);
  hipStream_t s = (hipStream_t)stream;
  const bool v4 = r.vec == 4;
  if (r.family == MMTTA_PW_REDUCE_STREAM) {
    const RedSArgs q = reduce_stream_args(y, dout, t, part);
    MMTTA_BF_DISPATCH(is_bf16(y), XBF, {
      if (is_bf16(dout)) launch_reduce_stream<1, XBF, true>(q, r, s);
      else launch_reduce_stream<1, XBF, false>(q, r, s);
    });
    return launch_status("norm bwd reduce");
  }
  if (is_bf16(dout) && !is_bf16(y)) {
    if (v4) hipLaunchKernelGGL((channel_reduce_kernel<1, 4, false, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((channel_reduce_kernel<1, 1, false, true>), grid, dim3(256), 0, s, a);
  } else if (is_bf16(dout)) {
    if (v4) hipLaunchKernelGGL((channel_reduce_kernel<1, 4, true, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((channel_reduce_kernel<1, 1, true, true>), grid, dim3(256), 0, s, a);
  } else if (is_bf16(y)) {
    if (v4) hipLaunchKernelGGL((channel_reduce_kernel<1, 4, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((channel_reduce_kernel<1, 1, true>), grid, dim3(256), 0, s, a);
  } else {
    if (v4) hipLaunchKernelGGL((channel_reduce_kernel<1, 4>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((channel_reduce_kernel<1, 1>), grid, dim3(256), 0, s, a);
  }
  return launch_status("norm bwd reduce");
}

int norm_bwd_apply_body(const mmtta_tensor* dout, const mmtta_tensor* y, const mmtta_norm_on_load* t,
                        const float* m1, const float* m2, const mmtta_tensor* dy, void* stream) {
  const int st = norm_bwd_apply_check(dout, y, t, m1, m2, dy);
  if (st) return st;
  const bool dbf = is_bf16(dout);
  EwArgs e;
  e.a = tv(dout); e.b = tv(y); e.o = tv(dy); e.ta = nl(t); e.tb = nl(nullptr); e.m1 = m1; e.m2 = m2; e.hasb = 1;
  e.pa = t->per_item ? 1 : 0; e.pb = 0;
  const PwRoute r = norm_bwd_apply_plan(dout, y, t, m1, m2, dy);
  const bool v4 = r.vec == 4;
  const dim3 grid((unsigned)r.grid_x);
  hipStream_t s = (hipStream_t)stream;
  {
    if (r.family == MMTTA_PW_NORM_BWD_APPLY8) {
      const int C = y->c;
      const long long dhw = vox_count(y);
      Nb8Args q;
      q.dout = (const float*)dout->ptr; q.y = (const float*)y->ptr; q.o = (float*)dy->ptr;
      q.dsn = dout->sn; q.ysn = y->sn; q.osn = dy->sn;
      q.dsw = (unsigned)dout->sw; q.ysw = (unsigned)y->sw; q.osw = (unsigned)dy->sw;
      q.C = C; q.relu = act_arg(t); q.dhw = (unsigned)dhw;
      q.mean = t->mean; q.rstd = t->rstd; q.gamma = t->gamma; q.beta = t->beta; q.m1 = m1; q.m2 = m2;
      q.per_item = t->per_item != 0 ? 1 : 0;
      const bool four = r.it == 4;
      const dim3 g8((unsigned)r.grid_x, (unsigned)r.grid_y);
      if (dbf) {
        if (four) hipLaunchKernelGGL((norm_bwd_apply8_kernel<true, 4, true>), g8, dim3(256), 0, s, q);
        else hipLaunchKernelGGL((norm_bwd_apply8_kernel<true, 2, true>), g8, dim3(256), 0, s, q);
      } else if (is_bf16(y)) {
        if (four) hipLaunchKernelGGL((norm_bwd_apply8_kernel<true, 4>), g8, dim3(256), 0, s, q);
        else hipLaunchKernelGGL((norm_bwd_apply8_kernel<true, 2>), g8, dim3(256), 0, s, q);
      } else {
        if (four) hipLaunchKernelGGL((norm_bwd_apply8_kernel<false, 4>), g8, dim3(256), 0, s, q);
        else hipLaunchKernelGGL((norm_bwd_apply8_kernel<false, 2>), g8, dim3(256), 0, s, q);
      }
      return launch_status("norm bwd apply");
    }
  }
  if (dbf && !is_bf16(y)) {          // thin tensors: bf16-stored gradients next to an fp32-stored activation
    if (v4) hipLaunchKernelGGL((elementwise_kernel<1, 4, true, false, true>), grid, dim3(256), 0, s, e);
    else hipLaunchKernelGGL((elementwise_kernel<1, 1, true, false, true>), grid, dim3(256), 0, s, e);
  } else if (dbf) {
    if (v4) hipLaunchKernelGGL((elementwise_kernel<1, 4, true, true, true>), grid, dim3(256), 0, s, e);
    else hipLaunchKernelGGL((elementwise_kernel<1, 1, true, true, true>), grid, dim3(256), 0, s, e);
  } else if (is_bf16(y)) {
    if (v4) hipLaunchKernelGGL((elementwise_kernel<1, 4, false, true, false>), grid, dim3(256), 0, s, e);
    else hipLaunchKernelGGL((elementwise_kernel<1, 1, false, true, false>), grid, dim3(256), 0, s, e);
  } else {
    if (v4) hipLaunchKernelGGL((elementwise_kernel<1, 4>), grid, dim3(256), 0, s, e);
    else hipLaunchKernelGGL((elementwise_kernel<1, 1>), grid, dim3(256), 0, s, e);
  }
  return launch_status("norm bwd apply");
}

// eligibility of the one-launch backward (host-only): instance statistics of a small voxel-dense tensor, channels in whole
// groups of 32, 16-byte aligned octets
bool nbs_ok(const mmtta_tensor* dout, const mmtta_tensor* y, const mmtta_norm_on_load* t, const mmtta_tensor* dy) {
  if (!dout || !y || !t || !dy || !t->mean || !t->rstd) return false;
  if (dout->dtype != dy->dtype || (is_bf16(dout) && !is_bf16(y))) return false;
  if (!same_shape(dout, y) || !same_shape(dy, y) || !is_cl(dout) || !is_cl(y) || !is_cl(dy)) return false;
  const long long dhw = vox_count(y);
  return y->c % 32 == 0 && dhw >= 1 && dhw <= 4096 && dense_voxels(dout) && dense_voxels(y) && dense_voxels(dy) &&
         oct_aligned(dout) && oct_aligned(dy) && oct_aligned(y) && null_or_16(t->mean) && null_or_16(t->rstd) &&
         null_or_16(t->gamma) && null_or_16(t->beta);
}

// one workgroup per 32 channels of an item: 4 channel octets x 64 voxel lanes, 2 voxels in flight per lane
PwRoute norm_bwd_small_plan(const mmtta_tensor* dout, const mmtta_tensor* y) {
  PwRoute r = {};
  r.family = MMTTA_PW_NORM_BWD_SMALL; r.mode = 1; r.has_b = 1; r.vec = 8; r.it = 2;
  r.bf16_a = r.bf16_o = is_bf16(dout) ? 1 : 0; r.bf16_b = is_bf16(y) ? 1 : 0;
  const long long dhw = vox_count(y);
  r.cpl = 4; r.nvl = 64; r.trips = (int)((dhw + 127) / 128) * 2;
  r.rows_per_n = 1; r.rows_per_block = 1; r.vox_per_row = dhw; r.cb_passes = 1;
  r.grid_x = y->c / 32; r.grid_y = y->n;
  r.work_items = dhw * y->n * (y->c / 8);
  return r;
}

int norm_bwd_small_body(const mmtta_tensor* dout, const mmtta_tensor* y, const mmtta_norm_on_load* t,
                        int64_t count, const mmtta_tensor* dy, void* stream) {
  MMTTA_CHECK(nbs_ok(dout, y, t, dy), MMTTA_ERR_UNSUPPORTED, "norm bwd (one launch): tensors not eligible (mmtta_norm_bwd_small_ok)");
  MMTTA_CHECK(count > 0, MMTTA_ERR_INVALID, "norm bwd (one launch): count must be positive");
  NbsArgs q;
  q.dout = (const float*)dout->ptr; q.y = (const float*)y->ptr; q.o = (float*)dy->ptr;
  q.dsn = dout->sn; q.ysn = y->sn; q.osn = dy->sn;
  q.dsw = (unsigned)dout->sw; q.ysw = (unsigned)y->sw; q.osw = (unsigned)dy->sw;
  q.C = y->c; q.relu = act_arg(t); q.dhw = (unsigned)((long long)y->d * y->h * y->w); q.count = (double)count;
  q.mean = t->mean; q.rstd = t->rstd; q.gamma = t->gamma; q.beta = t->beta;
  q.per_item = t->per_item != 0 ? 1 : 0;
  const PwRoute r = norm_bwd_small_plan(dout, y);
  const dim3 grid((unsigned)r.grid_x, (unsigned)r.grid_y);
  if (is_bf16(dout)) hipLaunchKernelGGL((norm_bwd_small_kernel<true, true>), grid, dim3(256), 0, (hipStream_t)stream, q);
  else if (is_bf16(y)) hipLaunchKernelGGL(norm_bwd_small_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, q);
  else hipLaunchKernelGGL(norm_bwd_small_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, q);
  return launch_status("norm bwd (one launch)");
}

MMTTA_ACT_NS_CLOSE
}  // namespace mmtta

#ifndef MMTTA_ACT_LEAKY_TU
using namespace mmtta;

extern "C" int mmtta_copy_strided(const mmtta_tensor* src, const mmtta_tensor* dst, void* stream) {
  MMTTA_CHECK(src == nullptr || src->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "mmtta_copy_strided: `src` must be fp32-stored");
  MMTTA_CHECK(src && dst && src->ptr && dst->ptr, MMTTA_ERR_INVALID, "copy: null tensor");
  MMTTA_CHECK(same_shape(src, dst), MMTTA_ERR_INVALID, "copy: shape mismatch");
  const long long total = (long long)dst->n * dst->c * dst->d * dst->h * dst->w;
  // (dst may be bf16-stored: the network input of bf16 precision is rounded once here instead of by every consumer)
  if (is_bf16(dst)) hipLaunchKernelGGL(copy_strided_kernel<true>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, tv(src), tv(dst));
  else hipLaunchKernelGGL(copy_strided_kernel<false>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, tv(src), tv(dst));
  return launch_status("copy_strided");
}

extern "C" int mmtta_reduce_rows_per_n(const mmtta_tensor* t) {
  if (t == nullptr) return -1;
  int r; long long v;
  rows_geometry(t, r, v);
  return r;
}

extern "C" int mmtta_channel_stats(const mmtta_tensor* x, float* part, void* stream) {
  MMTTA_CHECK(x && x->ptr && part, MMTTA_ERR_INVALID, "channel_stats: null argument");
  MMTTA_CHECK(is_cl(x), MMTTA_ERR_UNSUPPORTED, "channel_stats: tensor must be channels-last");
  return launch_channel_sums(x, part, (hipStream_t)stream);
}

// host-side check of a norm-sets descriptor against a batch of n items (mmtta_norm_sets)
// (with several sets, written affine gradients / running statistics must not overlap: each set's first item writes its own
// [C] vectors, a stride below C would make the writers of two sets race on one element)
static int nsets_validate(const mmtta_norm_sets* g, int n, int c, bool writes_affine, bool has_stats, const char* what) {
  MMTTA_CHECK(g != nullptr, MMTTA_ERR_INVALID, "%s: null norm-sets descriptor", what);
  MMTTA_CHECK(g->items_per_set >= 1, MMTTA_ERR_INVALID, "%s: items_per_set %d (>= 1)", what, g->items_per_set);
  MMTTA_CHECK(n > 0 && n % g->items_per_set == 0, MMTTA_ERR_INVALID, "%s: batch %d is no multiple of items_per_set %d", what, n,
              g->items_per_set);
  MMTTA_CHECK(g->affine_stride >= 0 && g->stats_stride >= 0 && g->affine_stride % 4 == 0 && g->stats_stride % 4 == 0,
              MMTTA_ERR_INVALID, "%s: strides must be non-negative and keep 16-byte alignment (affine %lld, stats %lld)", what,
              (long long)g->affine_stride, (long long)g->stats_stride);
  if (n / g->items_per_set > 1) {
    MMTTA_CHECK(!writes_affine || g->affine_stride >= c, MMTTA_ERR_INVALID,
                "%s: affine_stride %lld < C %d: the affine gradients of the sets would overlap", what, (long long)g->affine_stride, c);
    MMTTA_CHECK(!has_stats || g->stats_stride >= c, MMTTA_ERR_INVALID,
                "%s: stats_stride %lld < C %d: the running statistics of the sets would overlap", what, (long long)g->stats_stride, c);
  }
  return MMTTA_OK;
}
static NSets nsets(const mmtta_norm_sets* g) {
  NSets r; r.ips = g->items_per_set; r.astride = g->affine_stride; r.sstride = g->stats_stride; return r;
}

static int stats_finalize(int kind, int groups, const float* part, int rows_per_n, int n, int c, int64_t count, float eps,
                          int training, float* running_mean, float* running_var, float momentum, float* mean, float* rstd,
                          const float* gamma, const float* beta, float* scale, float* shift, float* gi, float* bi,
                          double* scratch, NSets ns, void* stream) {
  MMTTA_CHECK(kind >= 0 && kind <= 2, MMTTA_ERR_INVALID, "norm: bad kind %d", kind);
  MMTTA_CHECK(mean && rstd && n > 0 && c > 0 && count > 0, MMTTA_ERR_INVALID, "norm finalize: bad argument");
  MMTTA_CHECK((scale == nullptr) == (shift == nullptr), MMTTA_ERR_INVALID, "norm finalize: scale and shift go together");
  MMTTA_CHECK(scratch != nullptr, MMTTA_ERR_INVALID, "norm finalize: null scratch");
  double* g_tot = scratch;
  if (kind == MMTTA_NORM_GROUP) MMTTA_CHECK(groups > 0 && c % groups == 0, MMTTA_ERR_INVALID, "group norm: C %% groups != 0");
  if (kind == MMTTA_NORM_BATCH && !training) MMTTA_CHECK(running_mean && running_var, MMTTA_ERR_INVALID, "batch norm eval needs running stats");
  hipStream_t s = (hipStream_t)stream;
  if (kind == MMTTA_NORM_INSTANCE) {
    MMTTA_CHECK(part != nullptr && rows_per_n > 0, MMTTA_ERR_INVALID, "norm finalize: null partials");
    hipLaunchKernelGGL(instance_stats_kernel, dim3(n * c), dim3(64), 0, s, part, rows_per_n, c, (double)count, eps, mean, rstd,
                       gamma, beta, scale, shift, ns, gi, bi);
    return launch_status("instance norm stats");
  }
  const bool need_rows = !(kind == MMTTA_NORM_BATCH && !training);
  if (need_rows) {
    MMTTA_CHECK(part != nullptr && rows_per_n > 0, MMTTA_ERR_INVALID, "norm finalize: null partials");
    hipLaunchKernelGGL(rows_reduce_kernel, dim3(n * c), dim3(64), 0, s, part, rows_per_n, c, g_tot);
    int st = launch_status("norm rows reduce");
    if (st) return st;
  }
  StatFinArgs a;
  a.kind = kind; a.groups = groups; a.N = n; a.C = c; a.count = (double)count; a.eps = eps; a.training = training;
  a.running_mean = running_mean; a.running_var = running_var; a.momentum = momentum; a.mean = mean; a.rstd = rstd;
  a.gamma = gamma; a.beta = beta; a.scale = scale; a.shift = shift;
  a.tot = g_tot;
  a.ns = ns; a.gi = gi; a.bi = bi;
  hipLaunchKernelGGL(stats_finalize_kernel, dim3((n * c + 63) / 64), dim3(64), 0, s, a);
  return launch_status("norm stats finalize");
}

extern "C" int mmtta_norm_stats_finalize(int kind, int groups, const float* part, int rows_per_n, int n, int c,
                                         int64_t count, float eps, int training, float* running_mean,
                                         float* running_var, float momentum, float* mean, float* rstd,
                                         const float* gamma, const float* beta, float* scale, float* shift,
                                         double* scratch, void* stream) {
  return stats_finalize(kind, groups, part, rows_per_n, n, c, count, eps, training, running_mean, running_var, momentum, mean,
                        rstd, gamma, beta, scale, shift, nullptr, nullptr, scratch, nsets_plain(n > 0 ? n : 1), stream);
}

extern "C" int mmtta_norm_stats_finalize_sets(int kind, int groups, const float* part, int rows_per_n, int n, int c,
                                              int64_t count, float eps, int training, float* running_mean,
                                              float* running_var, float momentum, float* mean, float* rstd,
                                              const float* gamma, const float* beta, float* scale, float* shift,
                                              float* gamma_items, float* beta_items, double* scratch,
                                              const mmtta_norm_sets* sets, void* stream) {
  const int st = nsets_validate(sets, n, c, false, running_mean != nullptr, "norm finalize (sets)");
  if (st) return st;
  MMTTA_CHECK((gamma_items == nullptr || gamma != nullptr) && (beta_items == nullptr || beta != nullptr), MMTTA_ERR_INVALID,
              "norm finalize (sets): gamma_items / beta_items need gamma / beta");
  MMTTA_CHECK((running_mean == nullptr) == (running_var == nullptr), MMTTA_ERR_INVALID,
              "norm finalize (sets): running_mean and running_var go together");
  return stats_finalize(kind, groups, part, rows_per_n, n, c, count, eps, training, running_mean, running_var, momentum, mean,
                        rstd, gamma, beta, scale, shift, gamma_items, beta_items, scratch, nsets(sets), stream);
}

static int bwd_finalize(int kind, int groups, const float* part, int rows_per_n, int n, int c, int64_t count,
                        const float* gamma, int training, float* m1, float* m2, float* dgamma, float* dbeta, int accumulate,
                        double* scratch, NSets ns, void* stream) {
  MMTTA_CHECK(kind >= 0 && kind <= 2, MMTTA_ERR_INVALID, "norm: bad kind %d", kind);
  MMTTA_CHECK(part && m1 && m2 && n > 0 && c > 0 && count > 0 && rows_per_n > 0, MMTTA_ERR_INVALID, "norm bwd finalize: bad argument");
  MMTTA_CHECK(scratch != nullptr, MMTTA_ERR_INVALID, "norm bwd finalize: null scratch");
  double* g_tot = scratch;
  if (kind == MMTTA_NORM_GROUP) MMTTA_CHECK(groups > 0 && c % groups == 0, MMTTA_ERR_INVALID, "group norm: C %% groups != 0");
  hipStream_t s = (hipStream_t)stream;
  if (kind == MMTTA_NORM_INSTANCE && dgamma == nullptr) {
    hipLaunchKernelGGL(instance_bwd_kernel, dim3(n * c), dim3(64), 0, s, part, rows_per_n, c, (double)count, gamma, m1, m2, ns);
    return launch_status("instance norm bwd finalize");
  }
  hipLaunchKernelGGL(rows_reduce_kernel, dim3(n * c), dim3(64), 0, s, part, rows_per_n, c, g_tot);
  int st = launch_status("norm bwd rows reduce");
  if (st) return st;
  BwdFinArgs a;
  a.kind = kind; a.groups = groups; a.N = n; a.C = c; a.count = (double)count; a.gamma = gamma; a.training = training;
  a.m1 = m1; a.m2 = m2; a.dgamma = dgamma; a.dbeta = dbeta; a.accumulate = accumulate; a.tot = g_tot;
  a.ns = ns;
  hipLaunchKernelGGL(bwd_finalize_kernel, dim3((n * c + 63) / 64), dim3(64), 0, s, a);
  return launch_status("norm bwd finalize");
}

extern "C" int mmtta_norm_bwd_finalize(int kind, int groups, const float* part, int rows_per_n, int n, int c,
                                       int64_t count, const float* gamma, int training, float* m1, float* m2,
                                       float* dgamma, float* dbeta, int accumulate, double* scratch, void* stream) {
  return bwd_finalize(kind, groups, part, rows_per_n, n, c, count, gamma, training, m1, m2, dgamma, dbeta, accumulate, scratch,
                      nsets_plain(n > 0 ? n : 1), stream);
}

extern "C" int mmtta_norm_bwd_finalize_sets(int kind, int groups, const float* part, int rows_per_n, int n, int c,
                                            int64_t count, const float* gamma, int training, float* m1, float* m2,
                                            float* dgamma, float* dbeta, int accumulate, double* scratch,
                                            const mmtta_norm_sets* sets, void* stream) {
  const int st = nsets_validate(sets, n, c, dgamma != nullptr || dbeta != nullptr, false, "norm bwd finalize (sets)");
  if (st) return st;
  MMTTA_CHECK(dbeta == nullptr || dgamma != nullptr, MMTTA_ERR_INVALID, "norm bwd finalize (sets): dbeta needs dgamma");
  return bwd_finalize(kind, groups, part, rows_per_n, n, c, count, gamma, training, m1, m2, dgamma, dbeta, accumulate, scratch,
                      nsets(sets), stream);
}

extern "C" int mmtta_combine(const mmtta_tensor* a, const mmtta_norm_on_load* ta, const mmtta_tensor* b,
                             const mmtta_norm_on_load* tb, const mmtta_tensor* out, void* stream) {
  int st = nl_act_check(ta, "combine (ta)");
  if (st) return st;
  if (b) {
    st = nl_act_check(tb, "combine (tb)");
    if (st) return st;
  }
  if (nl_leaky(ta) || (b && nl_leaky(tb))) return leaky::combine_body(a, ta, b, tb, out, stream);
  return combine_body(a, ta, b, tb, out, stream);
}

extern "C" int mmtta_norm_bwd_reduce(const mmtta_tensor* dout, const mmtta_tensor* y, const mmtta_norm_on_load* t,
                                     float* part, void* stream) {
  const int st = nl_act_check(t, "norm bwd reduce");
  if (st) return st;
  return nl_leaky(t) ? leaky::norm_bwd_reduce_body(dout, y, t, part, stream) : norm_bwd_reduce_body(dout, y, t, part, stream);
}

extern "C" int mmtta_norm_bwd_apply(const mmtta_tensor* dout, const mmtta_tensor* y, const mmtta_norm_on_load* t,
                                    const float* m1, const float* m2, const mmtta_tensor* dy, void* stream) {
  const int st = nl_act_check(t, "norm bwd apply");
  if (st) return st;
  return nl_leaky(t) ? leaky::norm_bwd_apply_body(dout, y, t, m1, m2, dy, stream) : norm_bwd_apply_body(dout, y, t, m1, m2, dy, stream);
}

extern "C" int mmtta_norm_bwd_small_ok(const mmtta_tensor* dout, const mmtta_tensor* y, const mmtta_norm_on_load* t,
                                       const mmtta_tensor* dy) {
  return nbs_ok(dout, y, t, dy) ? 1 : 0;
}

extern "C" int mmtta_norm_bwd_small(const mmtta_tensor* dout, const mmtta_tensor* y, const mmtta_norm_on_load* t,
                                    int64_t count, const mmtta_tensor* dy, void* stream) {
  const int st = nl_act_check(t, "norm bwd (one launch)");
  if (st) return st;
  return nl_leaky(t) ? leaky::norm_bwd_small_body(dout, y, t, count, dy, stream) : norm_bwd_small_body(dout, y, t, count, dy, stream);
}

static int upsample_fwd_check(const mmtta_tensor* x, const mmtta_tensor* y) {
  MMTTA_CHECK(x && y && x->ptr && y->ptr, MMTTA_ERR_INVALID, "upsample: null tensor");
  MMTTA_CHECK(x->dtype == y->dtype, MMTTA_ERR_UNSUPPORTED, "mmtta_upsample2x_fwd: `x` and `y` must share one storage type");
  MMTTA_CHECK(y->n == x->n && y->c == x->c && y->d == 2 * x->d && y->h == 2 * x->h && y->w == 2 * x->w, MMTTA_ERR_INVALID,
              "upsample: y must be exactly 2x of x");
  MMTTA_CHECK(is_cl(x) && is_cl(y), MMTTA_ERR_UNSUPPORTED, "upsample: channels-last only");
  return MMTTA_OK;
}
static int upsample_bwd_check(const mmtta_tensor* dy, const mmtta_tensor* dx) {
  MMTTA_CHECK(dx && dy && dx->ptr && dy->ptr, MMTTA_ERR_INVALID, "upsample bwd: null tensor");
  MMTTA_CHECK(dy->dtype == dx->dtype, MMTTA_ERR_UNSUPPORTED, "mmtta_upsample2x_bwd: `dy` and `dx` must share one storage type");
  MMTTA_CHECK(dy->n == dx->n && dy->c == dx->c && dy->d == 2 * dx->d && dy->h == 2 * dx->h && dy->w == 2 * dx->w,
              MMTTA_ERR_INVALID, "upsample bwd: dy must be exactly 2x of dx");
  MMTTA_CHECK(is_cl(dx) && is_cl(dy), MMTTA_ERR_UNSUPPORTED, "upsample bwd: channels-last only");
  return MMTTA_OK;
}
// both directions: one thread per (voxel, channel vector) of the tensor written, `src` the tensor read
static PwRoute upsample_plan(int family, const mmtta_tensor* src, const mmtta_tensor* dst) {
  PwRoute r = {};
  const bool v4 = vec4_rd(src) && vec4_wr(dst);
  r.family = family; r.vec = v4 ? 4 : 1;
  r.bf16_a = r.bf16_o = is_bf16(dst) ? 1 : 0;
  route_grid_stride(r, (long long)dst->n * vox_count(dst) * (v4 ? (dst->c + 3) / 4 : dst->c), 16384);
  return r;
}

extern "C" int mmtta_upsample2x_fwd(const mmtta_tensor* x, const mmtta_tensor* y, void* stream) {
  const int st = upsample_fwd_check(x, y);
  if (st) return st;
  const PwRoute r = upsample_plan(MMTTA_PW_UPSAMPLE_FWD, x, y);
  const bool v4 = r.vec == 4;
  const dim3 ug((unsigned)r.grid_x);
  if (is_bf16(x)) {
    if (v4) hipLaunchKernelGGL((upsample_fwd_kernel<4, true>), ug, dim3(256), 0, (hipStream_t)stream, tv(x), tv(y));
    else hipLaunchKernelGGL((upsample_fwd_kernel<1, true>), ug, dim3(256), 0, (hipStream_t)stream, tv(x), tv(y));
  } else {
    if (v4) hipLaunchKernelGGL(upsample_fwd_kernel<4>, ug, dim3(256), 0, (hipStream_t)stream, tv(x), tv(y));
    else hipLaunchKernelGGL(upsample_fwd_kernel<1>, ug, dim3(256), 0, (hipStream_t)stream, tv(x), tv(y));
  }
  return launch_status("upsample fwd");
}

extern "C" int mmtta_upsample2x_bwd(const mmtta_tensor* dy, const mmtta_tensor* dx, int accumulate, void* stream) {
  const int st = upsample_bwd_check(dy, dx);
  if (st) return st;
  const PwRoute r = upsample_plan(MMTTA_PW_UPSAMPLE_BWD, dy, dx);
  const bool v4 = r.vec == 4;
  const dim3 ug((unsigned)r.grid_x);
  if (is_bf16(dy)) {
    if (v4) hipLaunchKernelGGL((upsample_bwd_kernel<4, true>), ug, dim3(256), 0, (hipStream_t)stream, tv(dy), tv(dx), accumulate);
    else hipLaunchKernelGGL((upsample_bwd_kernel<1, true>), ug, dim3(256), 0, (hipStream_t)stream, tv(dy), tv(dx), accumulate);
  } else {
    if (v4) hipLaunchKernelGGL(upsample_bwd_kernel<4>, ug, dim3(256), 0, (hipStream_t)stream, tv(dy), tv(dx), accumulate);
    else hipLaunchKernelGGL(upsample_bwd_kernel<1>, ug, dim3(256), 0, (hipStream_t)stream, tv(dy), tv(dx), accumulate);
  }
  return launch_status("upsample bwd");
}

static int lincomb_check(int count, const mmtta_tensor* const* in, const mmtta_tensor* out) {
  MMTTA_CHECK(count >= 1 && count <= 8 && in && out && out->ptr, MMTTA_ERR_INVALID, "lincomb: bad argument");
  for (int i = 0; i < count; ++i)
    MMTTA_CHECK(in[i] != nullptr && in[i]->dtype == in[0]->dtype, MMTTA_ERR_UNSUPPORTED, "lincomb: the inputs must share one storage type");
  for (int k = 0; k < count; ++k)
    MMTTA_CHECK(in[k] && in[k]->ptr && same_shape(in[k], out) && is_cl(in[k]), MMTTA_ERR_INVALID, "lincomb: input %d mismatch", k);
  MMTTA_CHECK(is_cl(out), MMTTA_ERR_UNSUPPORTED, "lincomb: channels-last only");
  return MMTTA_OK;
}
static PwRoute lincomb_plan(int count, const mmtta_tensor* const* in, const mmtta_tensor* out) {
  PwRoute r = {};
  bool v4 = vec4_wr(out);
  for (int k = 0; k < count; ++k) v4 = v4 && vec4_rd(in[k]);
  r.family = MMTTA_PW_LINCOMB; r.vec = v4 ? 4 : 1; r.count = count;
  r.bf16_a = is_bf16(in[0]) ? 1 : 0; r.bf16_o = is_bf16(out) ? 1 : 0;
  route_grid_stride(r, (long long)out->n * vox_count(out) * (v4 ? (out->c + 3) / 4 : out->c));
  return r;
}

extern "C" int mmtta_lincomb(int count, const mmtta_tensor* const* in, const float* w, const mmtta_tensor* out,
                             int accumulate, void* stream) {
  MMTTA_CHECK(w != nullptr, MMTTA_ERR_INVALID, "lincomb: bad argument");
  const int cs = lincomb_check(count, in, out);
  if (cs) return cs;
  const PwRoute r = lincomb_plan(count, in, out);
  const bool ibf = r.bf16_a != 0, obf = r.bf16_o != 0, v4 = r.vec == 4;
  LinArgs e;
  for (int k = 0; k < count; ++k) {
    e.in[k] = tv(in[k]);
    e.w[k] = w[k];
  }
  for (int k = count; k < 8; ++k) { e.in[k] = e.in[0]; e.w[k] = 0.f; }
  e.count = count; e.o = tv(out); e.accumulate = accumulate;
  const dim3 grid((unsigned)r.grid_x), block(256);
  hipStream_t st = (hipStream_t)stream;
#define MMTTA_LINCOMB_S(N, I, O) \
  do { if (v4) hipLaunchKernelGGL((lincomb_kernel<4, N, I, O>), grid, block, 0, st, e); \
       else hipLaunchKernelGGL((lincomb_kernel<1, N, I, O>), grid, block, 0, st, e); } while (0)
#define MMTTA_LINCOMB(N) \
  case N: if (ibf && obf) MMTTA_LINCOMB_S(N, true, true); else if (obf) MMTTA_LINCOMB_S(N, false, true); \
          else if (ibf) MMTTA_LINCOMB_S(N, true, false); else MMTTA_LINCOMB_S(N, false, false); break;
  switch (count) {
    MMTTA_LINCOMB(1) MMTTA_LINCOMB(2) MMTTA_LINCOMB(3) MMTTA_LINCOMB(4)
    MMTTA_LINCOMB(5) MMTTA_LINCOMB(6) MMTTA_LINCOMB(7) MMTTA_LINCOMB(8)
  }
#undef MMTTA_LINCOMB
#undef MMTTA_LINCOMB_S
  return launch_status("lincomb");
}

extern "C" int mmtta_pointwise_route(int op, const mmtta_tensor* const* operands, int count, const mmtta_norm_on_load* t,
                                     const mmtta_norm_on_load* t2, const float* m1, const float* m2,
                                     mmtta_pointwise_route_t* out) {
  MMTTA_CHECK(operands && out && count >= 1 && count <= 9, MMTTA_ERR_INVALID, "pointwise route: bad argument");
  for (int i = 0; i < count; ++i) MMTTA_CHECK(operands[i] != nullptr, MMTTA_ERR_INVALID, "pointwise route: null operand %d", i);
  auto wants = [&](int k) { return count == k; };
  int st = MMTTA_OK;
  PwRoute r = {};
  switch (op) {
    case MMTTA_PW_OP_CHANNEL_STATS:
      MMTTA_CHECK(wants(1), MMTTA_ERR_INVALID, "pointwise route: channel stats takes {x}");
      MMTTA_CHECK(operands[0]->ptr, MMTTA_ERR_INVALID, "channel_stats: null argument");
      MMTTA_CHECK(is_cl(operands[0]), MMTTA_ERR_UNSUPPORTED, "channel_stats: tensor must be channels-last");
      r = reduce_plan(operands[0], nullptr);
      break;
    case MMTTA_PW_OP_NORM_BWD_REDUCE:
      MMTTA_CHECK(wants(2), MMTTA_ERR_INVALID, "pointwise route: norm bwd reduce takes {dout, y}");
      if ((st = nl_act_check(t, "norm bwd reduce")) || (st = norm_bwd_reduce_check(operands[0], operands[1], t))) return st;
      r = reduce_plan(operands[1], operands[0]);
      r.leaky = nl_leaky(t) ? 1 : 0;
      break;
    case MMTTA_PW_OP_NORM_BWD_APPLY:
      MMTTA_CHECK(wants(3), MMTTA_ERR_INVALID, "pointwise route: norm bwd apply takes {dout, y, dy}");
      if ((st = nl_act_check(t, "norm bwd apply")) || (st = norm_bwd_apply_check(operands[0], operands[1], t, m1, m2, operands[2])))
        return st;
      r = norm_bwd_apply_plan(operands[0], operands[1], t, m1, m2, operands[2]);
      r.leaky = nl_leaky(t) ? 1 : 0;
      break;
    case MMTTA_PW_OP_NORM_BWD_SMALL:
      MMTTA_CHECK(wants(3), MMTTA_ERR_INVALID, "pointwise route: norm bwd (one launch) takes {dout, y, dy}");
      if ((st = nl_act_check(t, "norm bwd (one launch)"))) return st;
      MMTTA_CHECK(nbs_ok(operands[0], operands[1], t, operands[2]), MMTTA_ERR_UNSUPPORTED,
                  "norm bwd (one launch): tensors not eligible (mmtta_norm_bwd_small_ok)");
      r = norm_bwd_small_plan(operands[0], operands[1]);
      r.leaky = nl_leaky(t) ? 1 : 0;
      break;
    case MMTTA_PW_OP_COMBINE: {
      MMTTA_CHECK(wants(2) || wants(3), MMTTA_ERR_INVALID, "pointwise route: combine takes {a, out} or {a, b, out}");
      const mmtta_tensor* b = count == 3 ? operands[1] : nullptr;
      if ((st = nl_act_check(t, "combine (ta)")) || (b && (st = nl_act_check(t2, "combine (tb)")))) return st;
      if ((st = combine_check(operands[0], b, operands[count - 1]))) return st;
      r = combine_plan(operands[0], b, operands[count - 1]);
      r.leaky = nl_leaky(t) || (b && nl_leaky(t2)) ? 1 : 0;
      break;
    }
    case MMTTA_PW_OP_LINCOMB:
      MMTTA_CHECK(count >= 2, MMTTA_ERR_INVALID, "pointwise route: lincomb takes {in[0..k-1], out}");
      if ((st = lincomb_check(count - 1, operands, operands[count - 1]))) return st;
      r = lincomb_plan(count - 1, operands, operands[count - 1]);
      break;
    case MMTTA_PW_OP_UPSAMPLE_FWD:
      MMTTA_CHECK(wants(2), MMTTA_ERR_INVALID, "pointwise route: upsample takes {x, y}");
      if ((st = upsample_fwd_check(operands[0], operands[1]))) return st;
      r = upsample_plan(MMTTA_PW_UPSAMPLE_FWD, operands[0], operands[1]);
      break;
    case MMTTA_PW_OP_UPSAMPLE_BWD:
      MMTTA_CHECK(wants(2), MMTTA_ERR_INVALID, "pointwise route: upsample bwd takes {dy, dx}");
      if ((st = upsample_bwd_check(operands[0], operands[1]))) return st;
      r = upsample_plan(MMTTA_PW_UPSAMPLE_BWD, operands[0], operands[1]);
      break;
    default:
      MMTTA_CHECK(false, MMTTA_ERR_INVALID, "pointwise route: op %d", op);
  }
  *out = r;
  return MMTTA_OK;
}
#endif  // MMTTA_ACT_LEAKY_TU
