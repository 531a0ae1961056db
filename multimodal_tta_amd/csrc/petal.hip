// PETAL's data-driven restore (Brahma & Rai, CVPR 2023, "A Probabilistic Framework for Lifelong Test-Time Adaptation") on the
// flat arena (gfx950): per parameter tensor and weight replica the order statistic of the gradient magnitudes - a radix
// select over the 31 key bits, 11 / 10 / 10 bits per pass - and the pass that follows the student's optimizer step: the
// teacher's exponential moving average (mmtta_cotta_update_sets' arithmetic) and the return to the source of every element
// whose key lies below its tensor's threshold.  See include/mmtta.h for the contract of the entry points.
//
// The tensors are the rows (start, length, rank) of a segment table, relative to a replica.  Rows of up to SEL_SMALL_MAX
// elements are selected by one workgroup with their keys in LDS; longer rows are cut into chunks of SEL_CHUNK elements, one
// workgroup each: per pass an LDS histogram of the chunk's elements under the prefix found so far, its non-empty bins added
// to the row's global table with integer atomics, then one workgroup per row that finds the bin of the rank, narrows the
// prefix and clears the table.  Seven launches whatever the data and the number of replicas; integer sums only, so the
// result does not depend on the order in which the workgroups arrive.
#include "common.h"

namespace mmtta {

constexpr int SEL_SMALL_MAX = 8192;       // longest row one workgroup selects with its keys in LDS (32 KB)
constexpr int SEL_CHUNK = 16384;          // elements of a long row per workgroup and pass: 16 quads per thread
constexpr int SEL_BINS = 2048;            // bins of the first digit (bits 30..20); the other two digits use 1024 of them
constexpr int SEL_THREADS = 256;
constexpr int PETAL_MAX_ROWS = 1 << 20;
constexpr int PETAL_MAX_SETS = 65535;     // grid.y
constexpr int UPD_BLOCK = 4096;           // elements per workgroup of the update: 4 quads per thread
constexpr int UPD_ROWS = UPD_BLOCK / 4 + 1;      // rows that can meet a block: starts are distinct multiples of 4, + one from before
constexpr unsigned KEY_MASK = 0x7fffffffu;

// digit of pass P: (shift, bits) and the bits the passes before it fixed
template <int P> struct Digit;
template <> struct Digit<0> { static constexpr int shift = 20, bins = 2048; static constexpr unsigned done = 0u; };
template <> struct Digit<1> { static constexpr int shift = 10, bins = 1024; static constexpr unsigned done = 0x7ff00000u; };
template <> struct Digit<2> { static constexpr int shift = 0, bins = 1024; static constexpr unsigned done = 0x7ffffc00u; };

// The bin that holds the k-th smallest (0-based) of the elements counted in hist[0, BINS) (LDS), and k inside that bin.
// Called by all SEL_THREADS threads; k < the sum of the bins.  `sh`: 8 words of LDS.
template <int BINS>
__device__ __forceinline__ void pick_bin(const unsigned* hist, unsigned k, unsigned* sh, unsigned& bin, unsigned& krest) {
  constexpr int PER = BINS / SEL_THREADS;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  unsigned own = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) own += hist[t * PER + j];
  unsigned incl = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) sh[wave] = incl;
  if (t == 0) { sh[4] = BINS - 1; sh[5] = 0; }
  __syncthreads();
  for (int w = 0; w < wave; ++w) incl += sh[w];
  unsigned c = incl - own;
  if (c <= k && k < incl) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const unsigned h = hist[t * PER + j];
      if (k < c + h) { sh[4] = t * PER + j; sh[5] = k - c; break; }
      c += h;
    }
  }
  __syncthreads();
  bin = sh[4];
  krest = sh[5];
  __syncthreads();
}

template <int P>
__device__ __forceinline__ void count_key(unsigned* hist, unsigned bits, unsigned prefix) {
  const unsigned key = bits & KEY_MASK;
  if ((key & Digit<P>::done) == prefix) atomicAdd(&hist[(key >> Digit<P>::shift) & (Digit<P>::bins - 1)], 1u);
}

template <int P>
__device__ __forceinline__ void small_pass(const unsigned* keys, int len, unsigned* hist, unsigned* sh, unsigned& prefix, unsigned& k) {
  for (int i = threadIdx.x; i < Digit<P>::bins; i += SEL_THREADS) hist[i] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < len; i += SEL_THREADS) count_key<P>(hist, keys[i], prefix);
  __syncthreads();
  unsigned bin;
  pick_bin<Digit<P>::bins>(hist, k, sh, bin, k);
  prefix |= bin << Digit<P>::shift;
}

// One workgroup per (row, replica).  A short row is selected here, start to end; for a long row this launch clears the
// row's global table and sets its state (prefix 0, the rank), so that the scratch needs no preparation by the caller.
__global__ __launch_bounds__(SEL_THREADS) void select_small_kernel(const float* __restrict__ g, const long long* __restrict__ table,
                                                                   int count, long long stride, unsigned* __restrict__ gamma,
                                                                   unsigned* __restrict__ ghist, unsigned* __restrict__ state) {
  __shared__ unsigned keys[SEL_SMALL_MAX];
  __shared__ unsigned hist[SEL_BINS];
  __shared__ unsigned sh[8];
  const int r = blockIdx.x, s = blockIdx.y;
  const long long start = table[3 * r], len = table[3 * r + 1], rank = table[3 * r + 2];
  const long long slot = (long long)s * count + r;
  if (len > SEL_SMALL_MAX) {
    for (int i = threadIdx.x; i < SEL_BINS; i += SEL_THREADS) ghist[slot * SEL_BINS + i] = 0;
    if (threadIdx.x == 0) { state[2 * slot] = 0; state[2 * slot + 1] = (unsigned)rank; }
    return;
  }
  const unsigned* src = reinterpret_cast<const unsigned*>(g) + (long long)s * stride + start;
  const int n = (int)len;
  for (int i = threadIdx.x; i < n; i += SEL_THREADS) keys[i] = src[i] & KEY_MASK;
  unsigned prefix = 0, k = (unsigned)rank;
  small_pass<0>(keys, n, hist, sh, prefix, k);
  small_pass<1>(keys, n, hist, sh, prefix, k);
  small_pass<2>(keys, n, hist, sh, prefix, k);
  if (threadIdx.x == 0) gamma[slot] = prefix;
}

// Pass P over the long rows: workgroup c of a replica owns chunk c of the running chunk count cum[] (table + 3 count).
template <int P>
__global__ __launch_bounds__(SEL_THREADS) void select_hist_kernel(const float* __restrict__ g, const long long* __restrict__ table,
                                                                  int count, long long stride, unsigned* __restrict__ ghist,
                                                                  const unsigned* __restrict__ state) {
  __shared__ unsigned hist[Digit<P>::bins];
  const long long* cum = table + 3ll * count;
  const long long c = blockIdx.x;
  int lo = 0, hi = count;          // the last row with cum[row] <= c: the row of chunk c (short rows have no chunks)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cum[mid] <= c) lo = mid; else hi = mid;
  }
  const int r = lo, s = blockIdx.y;
  const long long start = table[3 * r], len = table[3 * r + 1];
  const long long off = (c - cum[r]) * SEL_CHUNK;
  const long long slot = (long long)s * count + r;
  const unsigned prefix = P == 0 ? 0u : state[2 * slot];
  for (int i = threadIdx.x; i < Digit<P>::bins; i += SEL_THREADS) hist[i] = 0;
  __syncthreads();
  const unsigned* src = reinterpret_cast<const unsigned*>(g) + (long long)s * stride + start + off;
  const int m = (int)(len - off < SEL_CHUNK ? len - off : SEL_CHUNK);
  const int nq = m >> 2;
#pragma unroll 4
  for (int q = threadIdx.x; q < nq; q += SEL_THREADS) {
    const uint4 u = reinterpret_cast<const uint4*>(src)[q];
    count_key<P>(hist, u.x, prefix);
    count_key<P>(hist, u.y, prefix);
    count_key<P>(hist, u.z, prefix);
    count_key<P>(hist, u.w, prefix);
  }
  for (int i = (nq << 2) + threadIdx.x; i < m; i += SEL_THREADS) count_key<P>(hist, src[i], prefix);
  __syncthreads();
  unsigned* gh = ghist + slot * SEL_BINS;
  for (int i = threadIdx.x; i < Digit<P>::bins; i += SEL_THREADS) {
    const unsigned h = hist[i];
    if (h != 0) atomicAdd(&gh[i], h);
  }
}

// After pass P: one workgroup per (long row, replica) finds the rank's bin in the row's table, clears the table and
// narrows the state - or, after the last pass, writes the threshold.
template <int P>
__global__ __launch_bounds__(SEL_THREADS) void select_pick_kernel(const long long* __restrict__ table, int count,
                                                                  unsigned* __restrict__ gamma, unsigned* __restrict__ ghist,
                                                                  unsigned* __restrict__ state) {
  __shared__ unsigned hist[Digit<P>::bins];
  __shared__ unsigned sh[8];
  const int r = blockIdx.x, s = blockIdx.y;
  if (table[3 * r + 1] <= SEL_SMALL_MAX) return;
  const long long slot = (long long)s * count + r;
  unsigned* gh = ghist + slot * SEL_BINS;
  for (int i = threadIdx.x; i < Digit<P>::bins; i += SEL_THREADS) {
    hist[i] = gh[i];
    gh[i] = 0;
  }
  __syncthreads();
  unsigned bin, k;
  pick_bin<Digit<P>::bins>(hist, state[2 * slot + 1], sh, bin, k);
  if (threadIdx.x == 0) {
    const unsigned prefix = state[2 * slot] | (bin << Digit<P>::shift);
    if (P == 2) {
      gamma[slot] = prefix;
    } else {
      state[2 * slot] = prefix;
      state[2 * slot + 1] = k;
    }
  }
}

// ------------------------------------------------------------------ teacher EMA + ranked restore
// One pass over [sets][n]: w' <- a w' + b w, then w_i <- w0_i where key(g_i) < gamma of i's row.  A workgroup owns UPD_BLOCK
// consecutive elements; it finds the rows that meet them by two searches of the table (workgroup-uniform), keeps their
// bounds and thresholds in LDS, and every thread places each of its quads among them there.  Row starts are multiples of 4,
// so a quad meets one row at the most: its first `cnt` elements.  Elements of no row (alignment padding) and rows with
// gamma == 0 are never restored and their gradient is not read.
__global__ __launch_bounds__(256) void petal_update_kernel(float* __restrict__ w, float* __restrict__ teacher,
                                                           const float* __restrict__ source, const float* __restrict__ g,
                                                           const unsigned* __restrict__ gamma, const long long* __restrict__ table,
                                                           int count, long long n, long long w_stride, long long t_stride,
                                                           long long g_stride, float a, float b, long long* partial) {
  __shared__ int rs[UPD_ROWS], re[UPD_ROWS];
  __shared__ unsigned rg[UPD_ROWS];
  __shared__ int sh[4];
  const int s = blockIdx.y;
  w += (long long)s * w_stride;
  teacher += (long long)s * t_stride;
  g += (long long)s * g_stride;
  gamma += (long long)s * count;
  const long long b0 = (long long)blockIdx.x * UPD_BLOCK;
  const long long b1 = b0 + UPD_BLOCK < n ? b0 + UPD_BLOCK : n;
  int lo = -1, hi = count;          // j0: the first row that ends behind b0
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (table[3 * mid] + table[3 * mid + 1] > b0) hi = mid; else lo = mid;
  }
  const int j0 = hi;
  lo = j0 - 1; hi = count;          // j1: the first row that starts at b1 or behind it
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (table[3 * mid] >= b1) hi = mid; else lo = mid;
  }
  int m = hi - j0;
  if (m > UPD_ROWS) m = UPD_ROWS;          // (cannot happen for a table that passed the checks)
  for (int j = threadIdx.x; j < m; j += 256) {
    const long long st = table[3 * (j0 + j)] - b0, en = st + table[3 * (j0 + j) + 1];
    rs[j] = (int)(st > 0 ? st : 0);
    re[j] = (int)(en < UPD_BLOCK ? en : UPD_BLOCK);
    rg[j] = gamma[j0 + j];
  }
  __syncthreads();
  const bool ema = !(a == 1.f && b == 0.f);      // alpha = 1: the teacher keeps its bits (-0 included) and is not written
  int restored = 0;
#pragma unroll
  for (int v = 0; v < UPD_BLOCK / 4 / 256; ++v) {
    const int e = (v * 256 + (int)threadIdx.x) << 2;
    const long long i = b0 + e;
    if (i >= n) continue;
    int cnt = 0;
    unsigned gam = 0;
    if (m > 0 && rs[0] <= e) {
      int l = 0, h = m;          // the last row that starts at e or before it
      while (h - l > 1) {
        const int mid = (l + h) >> 1;
        if (rs[mid] <= e) l = mid; else h = mid;
      }
      cnt = re[l] - e;
      cnt = cnt < 0 ? 0 : (cnt > 4 ? 4 : cnt);
      gam = rg[l];
    }
    const bool pick = cnt > 0 && gam != 0u;
    if (i + 4 <= n) {
      float4 wq = *reinterpret_cast<const float4*>(w + i);
      if (ema) {
        const float4 tq = *reinterpret_cast<const float4*>(teacher + i);
        *reinterpret_cast<float4*>(teacher + i) =
            make_float4(__fadd_rn(__fmul_rn(a, tq.x), __fmul_rn(b, wq.x)), __fadd_rn(__fmul_rn(a, tq.y), __fmul_rn(b, wq.y)),
                        __fadd_rn(__fmul_rn(a, tq.z), __fmul_rn(b, wq.z)), __fadd_rn(__fmul_rn(a, tq.w), __fmul_rn(b, wq.w)));
      }
      if (pick) {
        const uint4 gq = *reinterpret_cast<const uint4*>(g + i);
        const bool r0 = (gq.x & KEY_MASK) < gam, r1 = cnt > 1 && (gq.y & KEY_MASK) < gam, r2 = cnt > 2 && (gq.z & KEY_MASK) < gam,
                   r3 = cnt > 3 && (gq.w & KEY_MASK) < gam;
        if (r0 | r1 | r2 | r3) {
          const float4 sq = *reinterpret_cast<const float4*>(source + i);
          wq.x = r0 ? sq.x : wq.x; wq.y = r1 ? sq.y : wq.y; wq.z = r2 ? sq.z : wq.z; wq.w = r3 ? sq.w : wq.w;
          *reinterpret_cast<float4*>(w + i) = wq;
          restored += (int)r0 + (int)r1 + (int)r2 + (int)r3;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        if (i + j < n) {
          const float wi = w[i + j];
          if (ema) teacher[i + j] = __fadd_rn(__fmul_rn(a, teacher[i + j]), __fmul_rn(b, wi));
          if (pick && j < cnt && (__float_as_uint(g[i + j]) & KEY_MASK) < gam) { w[i + j] = source[i + j]; ++restored; }
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) restored += __shfl_xor(restored, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = restored;
  __syncthreads();
  if (threadIdx.x == 0) partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = (long long)sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(64) void petal_finish_kernel(const long long* partial, long long nblocks, long long* restored) {
  partial += (long long)blockIdx.x * nblocks;      // one workgroup per parameter set
  long long s = 0;
  for (long long i = threadIdx.x; i < nblocks; i += 64) s += partial[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) restored[blockIdx.x] = s;
}

static int64_t select_chunks(int64_t length) { return length <= SEL_SMALL_MAX ? 0 : (length + SEL_CHUNK - 1) / SEL_CHUNK; }
static int64_t update_blocks(int64_t n) { return n < 1 ? 1 : (n + UPD_BLOCK - 1) / UPD_BLOCK; }

// The host copy of the table: [count][3] (start, length, rank), then the [count + 1] running chunk counts.  Rows ascending
// and disjoint inside [0, limit).
static int check_table(const char* what, const int64_t* t, int count, int64_t limit) {
  MMTTA_CHECK(count >= 1, MMTTA_ERR_INVALID, "%s: count = %d (>= 1)", what, count);
  MMTTA_CHECK(count <= PETAL_MAX_ROWS, MMTTA_ERR_UNSUPPORTED, "%s: count = %d rows (at most %d)", what, count, PETAL_MAX_ROWS);
  const int64_t* cum = t + 3ll * count;
  MMTTA_CHECK(cum[0] == 0, MMTTA_ERR_INVALID, "%s: the chunk counts of the table do not start at 0", what);
  int64_t end = 0;
  for (int r = 0; r < count; ++r) {
    const int64_t start = t[3 * r], len = t[3 * r + 1], rank = t[3 * r + 2];
    MMTTA_CHECK(start >= end && start % 4 == 0, MMTTA_ERR_INVALID,
                "%s: row %d starts at %lld (a multiple of 4, not before %lld: rows ascending and disjoint)", what, r,
                (long long)start, (long long)end);
    MMTTA_CHECK(len >= 1, MMTTA_ERR_INVALID, "%s: row %d has length %lld (>= 1)", what, r, (long long)len);
    MMTTA_CHECK(rank >= 0 && rank < len, MMTTA_ERR_INVALID, "%s: row %d has rank %lld (0 <= rank < length %lld)", what, r,
                (long long)rank, (long long)len);
    MMTTA_CHECK(len < (1ll << 31), MMTTA_ERR_UNSUPPORTED, "%s: row %d has 2^31 elements or more", what, r);
    MMTTA_CHECK(start <= limit - len, MMTTA_ERR_INVALID, "%s: row %d ends at %lld, behind the %lld elements of a set", what, r,
                (long long)(start + len), (long long)limit);
    MMTTA_CHECK(cum[r + 1] - cum[r] == select_chunks(len), MMTTA_ERR_INVALID,
                "%s: the chunk counts of the table do not match row %d (mmtta_magnitude_select_chunks)", what, r);
    end = start + len;
  }
  MMTTA_CHECK(cum[count] < (1ll << 31), MMTTA_ERR_UNSUPPORTED, "%s: 2^31 chunks or more", what);
  return MMTTA_OK;
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int mmtta_magnitude_select_class(int64_t length) {
  if (length < 1) return -1;
  return length <= SEL_SMALL_MAX ? 0 : 1;
}

extern "C" int64_t mmtta_magnitude_select_chunks(int64_t length) {
  if (length < 1) return -1;
  return select_chunks(length);
}

extern "C" int64_t mmtta_magnitude_select_scratch_bytes(int count, int sets) {
  if (count < 1 || sets < 1) return -1;
  return (int64_t)sets * count * (SEL_BINS + 2) * (int64_t)sizeof(unsigned);
}

extern "C" int mmtta_magnitude_select_sets(const float* g, const int64_t* table, const int64_t* table_host, int count, int sets,
                                           int64_t set_stride, uint32_t* gamma_out, void* scratch, void* stream) {
  MMTTA_CHECK(g && table && table_host && gamma_out && scratch, MMTTA_ERR_INVALID, "magnitude select: null argument");
  MMTTA_CHECK(sets >= 1, MMTTA_ERR_INVALID, "magnitude select: sets = %d (>= 1)", sets);
  MMTTA_CHECK(sets <= PETAL_MAX_SETS, MMTTA_ERR_UNSUPPORTED, "magnitude select: sets = %d (at most %d)", sets, PETAL_MAX_SETS);
  MMTTA_CHECK(set_stride >= 0 && set_stride % 4 == 0, MMTTA_ERR_INVALID, "magnitude select: a stride of %lld between the sets (a multiple of 4)",
              (long long)set_stride);
  int st = check_table("magnitude select", table_host, count, set_stride);
  if (st) return st;
  MMTTA_CHECK(((uintptr_t)g | (uintptr_t)scratch) % 16 == 0, MMTTA_ERR_UNSUPPORTED, "magnitude select: buffers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const long long* tb = (const long long*)table;
  unsigned* ghist = (unsigned*)scratch;
  unsigned* state = ghist + (long long)sets * count * SEL_BINS;
  unsigned* gamma = (unsigned*)gamma_out;
  const unsigned chunks = (unsigned)table_host[3ll * count + count];
  const dim3 rows((unsigned)count, (unsigned)sets), blk(SEL_THREADS);
  hipLaunchKernelGGL(select_small_kernel, rows, blk, 0, s, g, tb, count, (long long)set_stride, gamma, ghist, state);
  if ((st = launch_status("magnitude select (short rows)"))) return st;
  if (chunks == 0) return MMTTA_OK;          // (a property of the table, not of the data: the launch count stays fixed per table)
  const dim3 cgrid(chunks, (unsigned)sets);
  hipLaunchKernelGGL(select_hist_kernel<0>, cgrid, blk, 0, s, g, tb, count, (long long)set_stride, ghist, (const unsigned*)state);
  hipLaunchKernelGGL(select_pick_kernel<0>, rows, blk, 0, s, tb, count, gamma, ghist, state);
  hipLaunchKernelGGL(select_hist_kernel<1>, cgrid, blk, 0, s, g, tb, count, (long long)set_stride, ghist, (const unsigned*)state);
  hipLaunchKernelGGL(select_pick_kernel<1>, rows, blk, 0, s, tb, count, gamma, ghist, state);
  hipLaunchKernelGGL(select_hist_kernel<2>, cgrid, blk, 0, s, g, tb, count, (long long)set_stride, ghist, (const unsigned*)state);
  hipLaunchKernelGGL(select_pick_kernel<2>, rows, blk, 0, s, tb, count, gamma, ghist, state);
  return launch_status("magnitude select (long rows)");
}

extern "C" int64_t mmtta_petal_update_partials(int64_t n, int sets) {
  if (n < 0 || sets < 1) return -1;
  return update_blocks(n) * sets;
}

extern "C" int mmtta_petal_update_sets(float* w, float* teacher, const float* source, const float* g, const uint32_t* gamma,
                                       const int64_t* table, const int64_t* table_host, int count, int64_t n, int sets,
                                       int64_t w_stride, int64_t teacher_stride, int64_t g_stride, double alpha,
                                       int64_t* partial, int64_t* restored, void* stream) {
  MMTTA_CHECK(w && teacher && source && g && gamma && table && table_host && partial && restored, MMTTA_ERR_INVALID,
              "petal update: null argument");
  MMTTA_CHECK(n >= 0 && n <= (1ll << 34), MMTTA_ERR_INVALID, "petal update: n = %lld (0 .. 2^34)", (long long)n);
  MMTTA_CHECK(sets >= 1, MMTTA_ERR_INVALID, "petal update: sets = %d (>= 1)", sets);
  MMTTA_CHECK(sets <= PETAL_MAX_SETS, MMTTA_ERR_UNSUPPORTED, "petal update: sets = %d (at most %d)", sets, PETAL_MAX_SETS);
  MMTTA_CHECK(w_stride % 4 == 0 && teacher_stride % 4 == 0 && g_stride % 4 == 0 && w_stride >= n && teacher_stride >= n && g_stride >= n,
              MMTTA_ERR_INVALID, "petal update: strides %lld / %lld / %lld (n = %lld; multiples of 4, >= n)", (long long)w_stride,
              (long long)teacher_stride, (long long)g_stride, (long long)n);
  MMTTA_CHECK(alpha >= 0.0 && alpha <= 1.0, MMTTA_ERR_INVALID, "petal update: alpha = %g (0 <= alpha <= 1)", alpha);
  int st = check_table("petal update", table_host, count, n);
  if (st) return st;
  const bool al = ((uintptr_t)w | (uintptr_t)teacher | (uintptr_t)source | (uintptr_t)g) % 16 == 0;
  MMTTA_CHECK(al, MMTTA_ERR_UNSUPPORTED, "petal update: buffers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const long long blocks = update_blocks(n);
  const dim3 grid((unsigned)blocks, (unsigned)sets);
  hipLaunchKernelGGL(petal_update_kernel, grid, dim3(256), 0, s, w, teacher, source, g, (const unsigned*)gamma,
                     (const long long*)table, count, (long long)n, (long long)w_stride, (long long)teacher_stride,
                     (long long)g_stride, (float)alpha, (float)(1.0 - alpha), (long long*)partial);
  if ((st = launch_status("petal update"))) return st;
  hipLaunchKernelGGL(petal_finish_kernel, dim3(sets), dim3(64), 0, s, (const long long*)partial, blocks, (long long*)restored);
  return launch_status("petal finish");
}
