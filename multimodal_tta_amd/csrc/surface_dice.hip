// Normalised surface Dice (NSD) of the evaluation tail, region-wise and lesion-wise (the BraTS-2024 pair is lesion-wise Dice
// + lesion-wise NSD): the share of each surface that lies within a tolerance tau (mm) of the other surface.  MONAI's
// SurfaceDiceMetric on the package's own edges (voxel counts, not Nikolov's surface-element areas):
//
//   edge(X)   = X & ~erode6(X), outside the volume counts as background (the edges of surface.hip)
//   d(v, u)   = (float)sqrt(fma(dz sd, dz sd, fma(dy sh, dy sh, (dx sw)^2)))      fp64 inside, the arithmetic of surface.hip
//   hit       v of edge(A) against B at tau: some u of edge(B) has d(v, u) <= (float)tau
//   NSD_tau   = (hits(edge P -> edge G) + hits(edge G -> edge P)) / (|edge P| + |edge G|)
//
// NSD needs no distance, only one bit per surface voxel, and for the tolerances in use the search is a window of a few
// voxels: per axis r = the largest k with (float)sqrt((k s)^2) <= (float)tau_max, found by a loop on the host.  Every term
// of the squared distance is monotone in |offset|, rounding included, so the window holds every offset that can be a hit;
// the minimum over the window then decides every tau <= tau_max at once.  r <= SD_MAX_R on every axis.
//
//   S1 edges    both edge sets bit-packed: one 64-bit word per 64 voxels of a row (a wave's ballot), bits beyond W are 0.
//               |edge P| and |edge G| from the popcounts.
//   S2 window   a wave owns one word = 64 voxels of one row; it walks the (2 rz + 1)(2 ry + 1) rows of the window (the walk
//               is the same for every lane, so the three words of a row that can hold the window are one address per wave),
//               a lane cuts its 2 rx + 1 bits out of them by shifts and evaluates the fp64 distance only for set bits.  A
//               voxel whose own position is an edge of the other set is a hit at every tau without a search.
//               Counts: wave popcounts, LDS sums, one integer atomic per block and column.
//               The bit planes stay in global memory: a 128^3 mask is 256 KB per set, resident in L2, and a row's words are
//               read by whole waves at one address; they are not staged through LDS.
//
// The lesion-wise pass runs behind mmtta_lesionwise_scores and only reads its scratch (lesionwise.h), like
// lesionwise_hd95.hip: per kept, found lesion g, A_g = its own voxels, P_g = the union of the components matched to it,
//   nsd_{g,tau} = (hits(edge A_g -> edge P_g) + hits(edge P_g -> edge A_g)) / (|edge A_g| + |edge P_g|)
// where only voxels of P_g are candidates for A_g and the reverse: a candidate counts iff the pair (component, lesion) is
// in the pair table.
//   L1 edges    as S1 from the mask and the G bit of the Gd byte; edge voxels per component root (cntP) and per lesion root
//               (den), one atomic per distinct root of a wave.
//   L2 window   direction A -> P: the minimum over the candidates whose component is matched to the voxel's lesion.
//               Direction P -> A: a predicted edge voxel can lie within tau of several lesions and is then a hit for each
//               of them once per tau: a list of LN_LIST (lesion root, smallest d^2) per thread; when a window holds more
//               lesions the list is dropped, the voxel is marked in a third bit plane and a launch of its own walks the
//               window of the marked voxels once per lesion, in the order of the roots (exact for any number of lesions).
//               Both directions add into hits[tau][lesion root].
//   L3 lengths  walk of the pair table: every pair (c, g) adds cntP[c] to den[g]; a component counts once per lesion it matches.
//   L4 finish   per scored lesion root: q = round(hits / den * 2^30) in integers, rounded once, summed per (mask, tau).
// Everything on the device is an integer count, so two calls agree bit for bit and a batch gives what its items give alone;
// the launch sequence depends on the shape and the window alone.
#include "lesionwise.h"

namespace mmtta {

constexpr int SD_MAX_T = 4;                 // tolerances per call
constexpr int SD_MAX_R = 8;                 // window radius per axis (LW_MAX_IT of lesionwise.hip)
constexpr int SD_MAX_DIM = 1024;            // the extent limit of mmtta_surface_distances
constexpr int LN_LIST = 2;                  // lesions a thread of the P -> A direction keeps before it falls back
static_assert(2 * SD_MAX_R + 1 <= 32, "a window row is cut out of three words with shifts below 64");

struct SdWin {
  int rz, ry, rx, T;
  float tau[SD_MAX_T];
  float tau_max;
  double d2_skip;              // above this squared distance (float)sqrt(d2) > tau_max for certain: no sqrt needed
  double sd, sh, sw;
};

struct SdArgs {
  const unsigned char* pred;   // [M][V]
  TV lab;
  int M, D, H, W, WW;          // WW words per row
  long long V, words;          // words per mask = D * H * WW
  unsigned long long* ep;      // [M][words] edges of the prediction
  unsigned long long* eg;      // [M][words] edges of the ground truth
  unsigned long long* counts;  // [M][T][4]
  SdWin win;
};

struct SdPos {
  bool valid;                  // the wave's word exists
  bool in;                     // and the lane's voxel lies in the row
  int j, y, z, x, lane;
  long long wi;
};

// a wave per word: 4 words per workgroup of 256
__device__ inline SdPos sd_pos(long long words, int WW, int H, int W) {
  SdPos p;
  p.lane = threadIdx.x & 63;
  p.wi = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  p.valid = p.wi < words;
  const long long wc = p.valid ? p.wi : 0;
  p.j = (int)(wc % WW);
  const long long row = wc / WW;
  p.y = (int)(row % H);
  p.z = (int)(row / H);
  p.x = p.j * 64 + p.lane;
  p.in = p.valid && p.x < W;
  return p;
}

// The window of the voxel at bit `b` of word j, cut out of the row's words j - 1, j, j + 1: bit k <-> dx = k - rx.
__device__ inline unsigned int sd_cut(unsigned long long wm, unsigned long long w0, unsigned long long wp, int b, int rx) {
  unsigned long long v;
  if (b >= rx) {
    v = w0 >> (b - rx);
    const int up = 64 - b + rx;                    // first window bit that comes from word j + 1
    if (up <= 2 * rx) v |= wp << up;               // up >= rx + 1 >= 1, below 64
  } else {
    const int s = rx - b;                          // 1 ... rx
    v = (w0 << s) | (wm >> (64 - s));
  }
  return (unsigned int)(v & ((1ull << (2 * rx + 1)) - 1ull));
}

// Walks the window of voxel (z, y, bit b of word j) over the bit plane `plane` and calls visit(d2, dz, dy, dx) for every set
// bit.  The rows are walked alike by every lane of a wave.
template <typename F>
__device__ inline void sd_walk(const unsigned long long* plane, const SdWin& w, int D, int H, int WW, int z, int y, int j, int b,
                               bool active, F&& visit) {
  for (int dz = -w.rz; dz <= w.rz; ++dz) {
    const int zz = z + dz;
    if (zz < 0 || zz >= D) continue;
    const double fd = (double)dz * w.sd;
    for (int dy = -w.ry; dy <= w.ry; ++dy) {
      const int yy = y + dy;
      if (yy < 0 || yy >= H) continue;
      const unsigned long long* rowp = plane + ((long long)zz * H + yy) * WW;
      const unsigned long long w0 = rowp[j];
      const unsigned long long wm = j > 0 ? rowp[j - 1] : 0ull;
      const unsigned long long wp = j + 1 < WW ? rowp[j + 1] : 0ull;
      if ((w0 | wm | wp) == 0ull || !active) continue;
      unsigned int bits = sd_cut(wm, w0, wp, b, w.rx);
      const double fh = (double)dy * w.sh;
      while (bits != 0u) {
        const int k = __ffs((int)bits) - 1;
        bits &= bits - 1u;
        const int dx = k - w.rx;
        const double fw = (double)dx * w.sw;
        visit(fma(fd, fd, fma(fh, fh, fw * fw)), dz, dy, dx);
      }
    }
  }
}

// The lesion-wise window kernels hold more wave-uniform values than there are scalar registers; the window's constants are
// uniform but cheap to keep per lane, so they are moved to vector registers rather than spilled there by the allocator.
// This leans on the register allocator of the compiler at hand: with ROCm 7.2.0 (AMD clang 22.0.0git) the three kernels have
// 2 / 9 / 22 SGPR spills (A -> P, P -> A, marked voxels) without it and none with it.  tests/test_surface_dice_host.py reads the figures of
// the built library, so another compiler that spills after all, or no longer needs this, is noticed there.
template <typename T>
__device__ inline T sd_vreg(T v) {
  asm volatile("" : "+v"(v));
  return v;
}

__device__ inline SdWin sd_win_vreg(const SdWin& w) {
  SdWin o = w;
  o.sd = sd_vreg(w.sd); o.sh = sd_vreg(w.sh); o.sw = sd_vreg(w.sw);
  o.d2_skip = sd_vreg(w.d2_skip);
  o.tau_max = sd_vreg(w.tau_max);
#pragma unroll
  for (int t = 0; t < SD_MAX_T; ++t) o.tau[t] = sd_vreg(w.tau[t]);
  return o;
}

// S1
__global__ __launch_bounds__(256) void sd_edges_kernel(SdArgs a) {
  __shared__ unsigned int s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  const int m = blockIdx.y;
  const SdPos p = sd_pos(a.words, a.WW, a.H, a.W);
  const int x = p.in ? p.x : 0, y = p.y, z = p.z;
  const int n = m / a.lab.c, r = m % a.lab.c;
  const unsigned char* pm = a.pred + (long long)m * a.V;
  const float* lp = a.lab.p + (long long)n * a.lab.sn + (long long)r * a.lab.sc;
  // all 7 + 7 loads from clamped coordinates; a neighbour outside the volume is background
  const int zs[7] = {z, z > 0 ? z - 1 : z, z + 1 < a.D ? z + 1 : z, z, z, z, z};
  const int ys[7] = {y, y, y, y > 0 ? y - 1 : y, y + 1 < a.H ? y + 1 : y, y, y};
  const int xs[7] = {x, x, x, x, x, x > 0 ? x - 1 : x, x + 1 < a.W ? x + 1 : x};
  const bool inb[7] = {true, z > 0, z + 1 < a.D, y > 0, y + 1 < a.H, x > 0, x + 1 < a.W};
  bool pv[7], gv[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    pv[k] = pm[((long long)zs[k] * a.H + ys[k]) * a.W + xs[k]] != 0;
    gv[k] = lp[(long long)zs[k] * a.lab.sd + (long long)ys[k] * a.lab.sh + (long long)xs[k] * a.lab.sw] > 0.5f;
  }
  bool pin = true, gin = true;
#pragma unroll
  for (int k = 1; k < 7; ++k) {
    pin = pin && inb[k] && pv[k];
    gin = gin && inb[k] && gv[k];
  }
  const unsigned long long bp = __ballot(p.in && pv[0] && !pin);
  const unsigned long long bg = __ballot(p.in && gv[0] && !gin);
  if (p.valid && p.lane == 0) {
    a.ep[(long long)m * a.words + p.wi] = bp;
    a.eg[(long long)m * a.words + p.wi] = bg;
    if (bp != 0ull) atomicAdd(&s_cnt[0], (unsigned int)__popcll(bp));
    if (bg != 0ull) atomicAdd(&s_cnt[1], (unsigned int)__popcll(bg));
  }
  __syncthreads();
  // |edge P| -> column 1, |edge G| -> column 3 of every tolerance
  if (threadIdx.x < 2 * a.win.T) {
    const int t = threadIdx.x >> 1, c = threadIdx.x & 1;
    if (s_cnt[c] != 0u) atomicAdd(a.counts + ((long long)m * a.win.T + t) * 4 + 1 + 2 * c, (unsigned long long)s_cnt[c]);
  }
}

// S2: blockIdx.z = direction, 0: edge P -> edge G (column 0), 1: edge G -> edge P (column 2)
__global__ __launch_bounds__(256) void sd_window_kernel(SdArgs a) {
  __shared__ unsigned int s_hit[SD_MAX_T];
  if (threadIdx.x < SD_MAX_T) s_hit[threadIdx.x] = 0u;
  __syncthreads();
  const int m = blockIdx.y, dir = blockIdx.z;
  const SdPos p = sd_pos(a.words, a.WW, a.H, a.W);
  const unsigned long long* src = (dir == 0 ? a.ep : a.eg) + (long long)m * a.words;
  const unsigned long long* oth = (dir == 0 ? a.eg : a.ep) + (long long)m * a.words;
  const unsigned long long ws = p.valid ? src[p.wi] : 0ull;
  const unsigned long long wo = p.valid ? oth[p.wi] : 0ull;
  const bool edge = ((ws >> p.lane) & 1ull) != 0ull;
  const bool same = edge && ((wo >> p.lane) & 1ull) != 0ull;      // the position itself is an edge of the other set
  const bool search = edge && !same;
  double best = INFINITY;
  if ((ws & ~wo) != 0ull)      // some lane of the wave has to search
    sd_walk(oth, a.win, a.D, a.H, a.WW, p.z, p.y, p.j, p.lane, search,
            [&](double d2, int, int, int) { best = d2 < best ? d2 : best; });
  const float dist = same ? 0.0f : (float)sqrt(best);
  for (int t = 0; t < a.win.T; ++t) {
    const unsigned long long bal = __ballot(edge && dist <= a.win.tau[t]);
    if (p.lane == 0 && bal != 0ull) atomicAdd(&s_hit[t], (unsigned int)__popcll(bal));
  }
  __syncthreads();
  if (threadIdx.x < a.win.T && s_hit[threadIdx.x] != 0u)
    atomicAdd(a.counts + ((long long)m * a.win.T + threadIdx.x) * 4 + 2 * dir, (unsigned long long)s_hit[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------ lesion-wise
struct LnArgs {
  const unsigned char* pred;    // [M][V]
  const unsigned char* gd;      // [M][V] bit 0: Gd, bit 1: G
  const int* LG;                // [M][V]
  const int* LP;                // [M][V]
  const unsigned int* pg;       // [M][V] at a lesion root
  const unsigned int* own;      // [M][V] at a lesion root
  const unsigned char* matched; // [M][V] at a component root
  const unsigned long long* table;       // [M][cap]
  unsigned long long cap;
  int logcap;
  int M, R, D, H, W, WW;
  long long V, words;
  unsigned long long* ep;       // [M][words]
  unsigned long long* eg;       // [M][words]
  unsigned long long* ovf;      // [M][words] edge voxels of P whose window holds more lesions than LN_LIST (every word written)
  unsigned int* cntP;           // [M][V] at a component root: its edge voxels                        (zeroed)
  unsigned int* den;            // [M][V] at a lesion root: |edge A_g| + |edge P_g|                  (zeroed)
  unsigned int* hits;           // [M][T][V] at a lesion root: hits of both directions               (zeroed)
  unsigned long long* stats;    // [M][T]
  float* lesion_nsd;            // [M][T][V] or nullptr
  SdWin win;
  unsigned long long min_voxels[CC_MAX_R];
};

// Is (component c, lesion g) in the mask's pair table?  Key and probing of lw_pair_kernel (lesionwise.hip); the table is at
// most half full, so a probe ends on the key or on an empty slot.
struct LnTable {
  const unsigned long long* tab;      // the mask's table
  unsigned long long cap;
  int shift;                          // 64 - log2(cap)
};

__device__ inline LnTable ln_table(const LnArgs& a, int m) {
  LnTable t;
  t.tab = sd_vreg(a.table + (unsigned long long)m * a.cap);
  t.cap = sd_vreg(a.cap);
  t.shift = sd_vreg(64 - a.logcap);
  return t;
}

__device__ inline bool ln_pair(const LnTable& t, int c, int g) {
  const unsigned long long key = ((unsigned long long)(unsigned int)(c + 1) << 32) | (unsigned long long)(unsigned int)(g + 1);
  unsigned long long idx = (key * 0x9E3779B97F4A7C15ull) >> t.shift;
  for (unsigned long long probe = 0; probe < t.cap; ++probe) {
    const unsigned long long k = t.tab[idx];
    if (k == key) return true;
    if (k == 0ull) return false;
    idx = (idx + 1) & (t.cap - 1);
  }
  return false;
}

// Adds the hits of the wave's lanes to hits[t][root]: one atomic per distinct root and tolerance.  Every lane of the wave calls it.
__device__ inline void ln_emit(const LnArgs& a, int m, int lane, bool active, int root, unsigned int hitmask) {
  unsigned long long todo = __ballot(active && hitmask != 0u);
  while (todo != 0ull) {
    const int lead = __ffsll((long long)todo) - 1;
    const int r = __shfl(root, lead);
    const bool mine = active && hitmask != 0u && root == r;
    const unsigned long long same = __ballot(mine);
    for (int t = 0; t < a.win.T; ++t) {
      const unsigned long long bal = __ballot(mine && ((hitmask >> t) & 1u) != 0u);
      if (lane == lead && bal != 0ull) atomicAdd(a.hits + ((long long)m * a.win.T + t) * a.V + r, (unsigned int)__popcll(bal));
    }
    todo &= ~same;
  }
}

__device__ inline unsigned int ln_hitmask(const SdWin& w, double d2) {
  const float dist = (float)sqrt(d2);
  unsigned int hm = 0u;
#pragma unroll
  for (int t = 0; t < SD_MAX_T; ++t) hm |= dist <= w.tau[t] ? (1u << t) : 0u;      // tau[t] = -1 beyond the T in use
  return hm;
}

// L1
__global__ __launch_bounds__(256) void ln_edges_kernel(LnArgs a) {
  const int m = blockIdx.y;
  const SdPos p = sd_pos(a.words, a.WW, a.H, a.W);
  const long long mv = (long long)m * a.V;
  const int x = p.in ? p.x : 0, y = p.y, z = p.z;
  const long long hw = (long long)a.H * a.W;
  const long long vc = ((long long)z * a.H + y) * a.W + x;
  const unsigned char* pm = a.pred + mv;
  const unsigned char* gm = a.gd + mv;
  const long long nb[6] = {z > 0 ? vc - hw : vc, z + 1 < a.D ? vc + hw : vc, y > 0 ? vc - a.W : vc, y + 1 < a.H ? vc + a.W : vc,
                           x > 0 ? vc - 1 : vc, x + 1 < a.W ? vc + 1 : vc};
  const bool inb[6] = {z > 0, z + 1 < a.D, y > 0, y + 1 < a.H, x > 0, x + 1 < a.W};
  const bool pv = p.in && pm[vc] != 0;
  const bool gv = p.in && (gm[vc] & 2u) != 0u;
  bool pin = true, gin = true;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    pin = pin && inb[k] && pm[nb[k]] != 0;
    gin = gin && inb[k] && (gm[nb[k]] & 2u) != 0u;
  }
  const bool ep = pv && !pin, eg = gv && !gin;
  const unsigned long long bp = __ballot(ep), bg = __ballot(eg);
  if (p.valid && p.lane == 0) {
    a.ep[(long long)m * a.words + p.wi] = bp;
    a.eg[(long long)m * a.words + p.wi] = bg;
  }
  const int lg = eg ? a.LG[mv + vc] : -1;
  const int lp = ep ? a.LP[mv + vc] : -1;
  unsigned long long todo = bg;
  while (todo != 0ull) {
    const int lead = __ffsll((long long)todo) - 1;
    const int root = __shfl(lg, lead);
    const unsigned long long same = __ballot(eg && lg == root);
    if (p.lane == lead) atomicAdd(a.den + mv + root, (unsigned int)__popcll(same));
    todo &= ~same;
  }
  todo = bp;
  while (todo != 0ull) {
    const int lead = __ffsll((long long)todo) - 1;
    const int root = __shfl(lp, lead);
    const unsigned long long same = __ballot(ep && lp == root);
    if (p.lane == lead) atomicAdd(a.cntP + mv + root, (unsigned int)__popcll(same));
    todo &= ~same;
  }
}

// L2, direction A -> P: a wave per word of edge(G)
__global__ __launch_bounds__(256) void ln_window_a_kernel(LnArgs a) {
  const SdWin win = sd_win_vreg(a.win);
  const LnTable tab = ln_table(a, blockIdx.y);
  const int m = blockIdx.y, r = m % a.R;
  const SdPos p = sd_pos(a.words, a.WW, a.H, a.W);
  const long long mv = (long long)m * a.V;
  const long long hw = (long long)a.H * a.W;
  const unsigned long long ws = p.valid ? a.eg[(long long)m * a.words + p.wi] : 0ull;
  if (ws == 0ull) return;      // the whole wave
  const unsigned long long wo = a.ep[(long long)m * a.words + p.wi];
  const long long v = ((long long)p.z * a.H + p.y) * a.W + (p.in ? p.x : 0);
  const bool edge = ((ws >> p.lane) & 1ull) != 0ull;
  const int g = edge ? a.LG[mv + v] : -1;
  const bool scored = edge && (unsigned long long)a.own[mv + g] >= a.min_voxels[r] && a.pg[mv + g] != 0u;      // kept and found
  // the voxel itself is an edge voxel of P: it lies in P and in lesion g, so its component is matched to g
  const bool same = scored && ((wo >> p.lane) & 1ull) != 0ull;
  const bool search = scored && !same;
  double best = INFINITY;
  if (__ballot(search) != 0ull) {
    int lastc = -1;
    bool lastok = false;
    sd_walk(a.ep + (long long)m * a.words, win, a.D, a.H, a.WW, p.z, p.y, p.j, p.lane, search,
            [&](double d2, int dz, int dy, int dx) {
              if (d2 > win.d2_skip || d2 >= best) return;
              const int c = a.LP[mv + v + (long long)dz * hw + (long long)dy * a.W + dx];
              if (c != lastc) { lastc = c; lastok = ln_pair(tab, c, g); }
              if (lastok) best = d2;
            });
  }
  const unsigned int hm = same ? ((1u << win.T) - 1u) : (search ? ln_hitmask(win, best) : 0u);
  ln_emit(a, m, p.lane, scored, g, hm);
}

// L2, direction P -> A: a wave per word of edge(P)
__global__ __launch_bounds__(256) void ln_window_p_kernel(LnArgs a) {
  const SdWin win = sd_win_vreg(a.win);
  const LnTable tab = ln_table(a, blockIdx.y);
  const int m = blockIdx.y;
  const SdPos p = sd_pos(a.words, a.WW, a.H, a.W);
  const long long mv = sd_vreg((long long)m * a.V);
  const long long hw = sd_vreg((long long)a.H * a.W), lw = sd_vreg((long long)a.W);
  const unsigned long long ws = p.valid ? a.ep[(long long)m * a.words + p.wi] : 0ull;
  if (ws == 0ull) {            // the whole wave
    if (p.valid && p.lane == 0) a.ovf[(long long)m * a.words + p.wi] = 0ull;
    return;
  }
  const long long v = ((long long)p.z * a.H + p.y) * a.W + (p.in ? p.x : 0);
  const bool edge = ((ws >> p.lane) & 1ull) != 0ull;
  const int c = edge ? a.LP[mv + v] : -1;
  const bool search = edge && a.matched[mv + c] != 0;
  const unsigned long long* plane = a.eg + (long long)m * a.words;
  int lg[LN_LIST];
  double ld[LN_LIST];
#pragma unroll
  for (int i = 0; i < LN_LIST; ++i) { lg[i] = -1; ld[i] = INFINITY; }
  bool overflow = false;
  if (__ballot(search) != 0ull) {
    int lastg = -1;
    bool lastok = false;
    sd_walk(plane, win, a.D, a.H, a.WW, p.z, p.y, p.j, p.lane, search, [&](double d2, int dz, int dy, int dx) {
      if (d2 > win.d2_skip || !((float)sqrt(d2) <= win.tau_max)) return;
      const int g = a.LG[mv + v + (long long)dz * hw + (long long)dy * lw + dx];
      if (g != lastg) { lastg = g; lastok = ln_pair(tab, c, g); }
      if (!lastok) return;
      bool placed = false;
#pragma unroll
      for (int i = 0; i < LN_LIST; ++i) {
        if (!placed && (lg[i] == g || lg[i] < 0)) {
          lg[i] = g;
          ld[i] = d2 < ld[i] ? d2 : ld[i];
          placed = true;
        }
      }
      if (!placed) overflow = true;
    });
  }
#pragma unroll
  for (int i = 0; i < LN_LIST; ++i) {
    const bool have = search && !overflow && lg[i] >= 0;
    ln_emit(a, m, p.lane, have, lg[i], have ? ln_hitmask(win, ld[i]) : 0u);
  }
  const unsigned long long bo = __ballot(search && overflow);
  if (p.lane == 0) a.ovf[(long long)m * a.words + p.wi] = bo;
}

// L2, direction P -> A, the voxels whose window holds more lesions than the list: one walk per lesion, in the order of the
// roots; `cur` is the lesion whose minimum the walk takes, `next` the smallest root above it that the walk meets
__global__ __launch_bounds__(256) void ln_window_f_kernel(LnArgs a) {
  const SdWin win = sd_win_vreg(a.win);
  const LnTable tab = ln_table(a, blockIdx.y);
  const int m = blockIdx.y;
  const SdPos p = sd_pos(a.words, a.WW, a.H, a.W);
  const long long mv = sd_vreg((long long)m * a.V);
  const long long hw = sd_vreg((long long)a.H * a.W), lw = sd_vreg((long long)a.W);
  const unsigned long long ws = p.valid ? a.ovf[(long long)m * a.words + p.wi] : 0ull;
  if (((ws >> p.lane) & 1ull) == 0ull) return;
  const long long v = ((long long)p.z * a.H + p.y) * a.W + p.x;
  const int c = a.LP[mv + v];
  const unsigned long long* plane = a.eg + (long long)m * a.words;
  int cur = -1;
  for (;;) {
    int next = 0x7fffffff;
    double best = INFINITY;
    int lastg = -1;
    bool lastok = false;
    sd_walk(plane, win, a.D, a.H, a.WW, p.z, p.y, p.j, p.lane, true, [&](double d2, int dz, int dy, int dx) {
      if (d2 > win.d2_skip || !((float)sqrt(d2) <= win.tau_max)) return;
      const int g = a.LG[mv + v + (long long)dz * hw + (long long)dy * lw + dx];
      if (g < cur || (g > cur && g >= next)) return;
      if (g != lastg) { lastg = g; lastok = ln_pair(tab, c, g); }
      if (!lastok) return;
      if (g == cur) best = d2 < best ? d2 : best;
      else next = g;
    });
    if (cur >= 0) {
      const unsigned int hm = ln_hitmask(win, best);
      for (int t = 0; t < win.T; ++t)
        if ((hm >> t) & 1u) atomicAdd(a.hits + ((long long)m * win.T + t) * a.V + cur, 1u);
    }
    if (next == 0x7fffffff) break;
    cur = next;
  }
}

// L3
__global__ __launch_bounds__(256) void ln_lengths_kernel(LnArgs a) {
  const int m = blockIdx.y;
  const unsigned long long slot = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (slot >= a.cap) return;
  const unsigned long long key = a.table[(unsigned long long)m * a.cap + slot];
  if (key == 0ull) return;
  const long long mv = (long long)m * a.V;
  const long long c = (long long)(key >> 32) - 1, g = (long long)(key & 0xffffffffull) - 1;
  atomicAdd(a.den + mv + g, a.cntP[mv + c]);
}

// L4
__global__ __launch_bounds__(256) void ln_finish_kernel(LnArgs a) {
  __shared__ unsigned long long s_sum[SD_MAX_T];
  if (threadIdx.x < SD_MAX_T) s_sum[threadIdx.x] = 0ull;
  __syncthreads();
  const int m = blockIdx.y, r = m % a.R;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long mv = (long long)m * a.V;
  if (v < a.V && (a.gd[mv + v] & 1u) && a.LG[mv + v] == (int)v &&
      (unsigned long long)a.own[mv + v] >= a.min_voxels[r] && a.pg[mv + v] != 0u) {
    const unsigned long long den = a.den[mv + v];      // >= 1: a scored lesion has own voxels, hence an edge voxel
    for (int t = 0; t < a.win.T; ++t) {
      const long long at = ((long long)m * a.win.T + t) * a.V + v;
      const unsigned long long num = a.hits[at];       // <= den < 2^33
      const unsigned long long q = ((num << 30) + den / 2) / den;
      if (q != 0ull) atomicAdd(&s_sum[t], q);
      if (a.lesion_nsd != nullptr) a.lesion_nsd[at] = (float)((double)num / (double)den);
    }
  }
  __syncthreads();
  if (threadIdx.x < a.win.T && s_sum[threadIdx.x] != 0ull) atomicAdd(a.stats + (long long)m * a.win.T + threadIdx.x, s_sum[threadIdx.x]);
}

// largest k >= 0 with (float)sqrt((k s)^2) <= tau, or SD_MAX_R + 1 when that is above SD_MAX_R
static int sd_radius(double s, float tau) {
  int k = 0;
  while (k <= SD_MAX_R) {
    const double f = (double)(k + 1) * s;
    if (!((float)sqrt(f * f) <= tau)) break;
    ++k;
  }
  return k;
}

// The checks on spacing and tolerances that both entry points make, and the window; 0 or the status to return.
static int sd_window(const char* who, const double* spacing, const double* tolerances, int n_tolerances, SdWin& w) {
  MMTTA_CHECK(spacing != nullptr, MMTTA_ERR_INVALID, "%s: null `spacing`", who);
  MMTTA_CHECK(tolerances != nullptr, MMTTA_ERR_INVALID, "%s: null `tolerances`", who);
  MMTTA_CHECK(n_tolerances >= 1 && n_tolerances <= SD_MAX_T, MMTTA_ERR_INVALID, "%s: n_tolerances = %d (1 ... %d `tolerances` per call)",
              who, n_tolerances, SD_MAX_T);
  for (int i = 0; i < 3; ++i)
    MMTTA_CHECK(spacing[i] > 0.0 && spacing[i] <= 1.7976931348623157e308, MMTTA_ERR_INVALID,
                "%s: spacing[%d] = %g must be positive and finite", who, i, spacing[i]);
  w.T = n_tolerances;
  w.tau_max = 0.0f;
  for (int t = 0; t < SD_MAX_T; ++t) w.tau[t] = -1.0f;
  for (int t = 0; t < n_tolerances; ++t) {
    MMTTA_CHECK(tolerances[t] >= 0.0 && tolerances[t] <= 1.7976931348623157e308, MMTTA_ERR_INVALID,
                "%s: tolerances[%d] = %g must be finite and >= 0", who, t, tolerances[t]);
    w.tau[t] = (float)tolerances[t];
    w.tau_max = w.tau[t] > w.tau_max ? w.tau[t] : w.tau_max;
  }
  w.sd = spacing[0]; w.sh = spacing[1]; w.sw = spacing[2];
  w.rz = sd_radius(w.sd, w.tau_max); w.ry = sd_radius(w.sh, w.tau_max); w.rx = sd_radius(w.sw, w.tau_max);
  MMTTA_CHECK(w.rz <= SD_MAX_R && w.ry <= SD_MAX_R && w.rx <= SD_MAX_R, MMTTA_ERR_UNSUPPORTED,
              "%s: the largest of `tolerances`, %g, needs a search window of more than %d voxels at spacing (%g, %g, %g); "
              "mmtta_surface_distances (HD95 / ASD) is the tool for large distances",
              who, (double)w.tau_max, SD_MAX_R, w.sd, w.sh, w.sw);
  // (float)sqrt(d2) <= tau_max implies sqrt(d2) < tau_max (1 + 2^-23), so d2 < tau_max^2 (1 + 2^-22): anything above
  // tau_max^2 (1 + 2^-20) is no hit (a subnormal tau_max has no such relative bound: the smallest normal float stands in)
  const double tm = (double)w.tau_max > 1.17549435e-38 ? (double)w.tau_max : 1.17549435e-38;
  w.d2_skip = tm * tm * (1.0 + 9.5367431640625e-07);
  return MMTTA_OK;
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int64_t mmtta_surface_dice_scratch_bytes(int64_t n_masks, int64_t d, int64_t h, int64_t w) {
  if (n_masks < 1 || n_masks > 65535 || d < 1 || h < 1 || w < 1 || d > SD_MAX_DIM || h > SD_MAX_DIM || w > SD_MAX_DIM) return -1;
  const size_t words = (size_t)d * h * ((w + 63) / 64);
  return (int64_t)(2 * lw_align((size_t)n_masks * words * 8));
}

extern "C" int mmtta_surface_dice(const uint8_t* pred_mask, const mmtta_tensor* label, const double* spacing,
                                  const double* tolerances, int n_tolerances, int64_t* counts, void* scratch, void* stream) {
  MMTTA_CHECK(pred_mask != nullptr, MMTTA_ERR_INVALID, "surface_dice: null `pred_mask`");
  MMTTA_CHECK(label != nullptr, MMTTA_ERR_INVALID, "surface_dice: null `label`");
  MMTTA_CHECK(counts != nullptr, MMTTA_ERR_INVALID, "surface_dice: null `counts`");
  MMTTA_CHECK(scratch != nullptr, MMTTA_ERR_INVALID, "surface_dice: null `scratch`");
  SdArgs a;
  int st = sd_window("surface_dice", spacing, tolerances, n_tolerances, a.win);
  if (st) return st;
  MMTTA_CHECK(label->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "mmtta_surface_dice: `label` must be fp32-stored");
  MMTTA_CHECK(label->ptr != nullptr, MMTTA_ERR_INVALID, "surface_dice: null `label` data");
  MMTTA_CHECK(label->n >= 1 && label->c >= 1 && label->d >= 1 && label->h >= 1 && label->w >= 1, MMTTA_ERR_INVALID,
              "surface_dice: every extent of `label` must be >= 1");
  MMTTA_CHECK(label->d <= SD_MAX_DIM && label->h <= SD_MAX_DIM && label->w <= SD_MAX_DIM, MMTTA_ERR_UNSUPPORTED,
              "surface_dice: spatial extent %d x %d x %d above %d", label->d, label->h, label->w, SD_MAX_DIM);
  const long long M = (long long)label->n * label->c;
  MMTTA_CHECK(M <= 65535, MMTTA_ERR_UNSUPPORTED, "surface_dice: more than 65535 masks per call");
  hipStream_t s = (hipStream_t)stream;
  a.pred = pred_mask;
  a.lab = tv(label);
  a.M = (int)M; a.D = label->d; a.H = label->h; a.W = label->w;
  a.WW = (a.W + 63) / 64;
  a.V = (long long)a.D * a.H * a.W;
  a.words = (long long)a.D * a.H * a.WW;
  a.ep = (unsigned long long*)scratch;
  a.eg = (unsigned long long*)((char*)scratch + lw_align((size_t)M * (size_t)a.words * 8));
  a.counts = (unsigned long long*)counts;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)M * a.win.T * 4 * sizeof(int64_t), s);
  MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "surface_dice: memset failed: %s", hipGetErrorString(e));
  const dim3 grid((unsigned)((a.words + 3) / 4), (unsigned)M);
  hipLaunchKernelGGL(sd_edges_kernel, grid, dim3(256), 0, s, a);
  st = launch_status("surface_dice edges");
  if (st) return st;
  hipLaunchKernelGGL(sd_window_kernel, dim3(grid.x, grid.y, 2), dim3(256), 0, s, a);
  return launch_status("surface_dice window");
}

namespace mmtta {

struct LnLayout {
  size_t zero_bytes, cntP, den, hits, ep, eg, ovf, total;
};

// [cntP | den | hits] are zeroed by one memset; sized for SD_MAX_T tolerances, so a function of the shape alone
static LnLayout ln_layout(int64_t M, int64_t V, int64_t words) {
  LnLayout l;
  const size_t mv = (size_t)M * (size_t)V;
  size_t o = 0;
  l.cntP = o; o += lw_align(mv * 4);
  l.den = o; o += lw_align(mv * 4);
  l.hits = o; o += lw_align(mv * 4 * SD_MAX_T);
  l.zero_bytes = o;
  l.ep = o; o += lw_align((size_t)M * (size_t)words * 8);
  l.eg = o; o += lw_align((size_t)M * (size_t)words * 8);
  l.ovf = o; o += lw_align((size_t)M * (size_t)words * 8);
  l.total = o;
  return l;
}

}  // namespace mmtta

extern "C" int mmtta_lesionwise_nsd_list_slots(void) { return LN_LIST; }

extern "C" int64_t mmtta_lesionwise_nsd_scratch_bytes(int64_t n_masks, int64_t d, int64_t h, int64_t w) {
  if (!lw_extent_ok(n_masks, d, h, w)) return -1;
  return (int64_t)ln_layout(n_masks, d * h * w, d * h * ((w + 63) / 64)).total;
}

extern "C" int mmtta_lesionwise_nsd(const uint8_t* mask, int n, int r, int d, int h, int w, const double* spacing,
                                    const double* tolerances, int n_tolerances, const int64_t* min_lesion_voxels,
                                    const void* lesionwise_scratch, int64_t* nsd_stats, float* lesion_nsd, void* scratch,
                                    void* stream) {
  MMTTA_CHECK(mask != nullptr, MMTTA_ERR_INVALID, "lesionwise_nsd: null `mask`");
  MMTTA_CHECK(min_lesion_voxels != nullptr, MMTTA_ERR_INVALID, "lesionwise_nsd: null `min_lesion_voxels`");
  MMTTA_CHECK(lesionwise_scratch != nullptr, MMTTA_ERR_INVALID, "lesionwise_nsd: null `lesionwise_scratch`");
  MMTTA_CHECK(nsd_stats != nullptr, MMTTA_ERR_INVALID, "lesionwise_nsd: null `nsd_stats`");
  MMTTA_CHECK(scratch != nullptr, MMTTA_ERR_INVALID, "lesionwise_nsd: null `scratch`");
  LnArgs a;
  int st = sd_window("lesionwise_nsd", spacing, tolerances, n_tolerances, a.win);
  if (st) return st;
  MMTTA_CHECK(n >= 1 && r >= 1 && d >= 1 && h >= 1 && w >= 1, MMTTA_ERR_INVALID,
              "lesionwise_nsd: every extent must be >= 1, got %d %d %d %d %d", n, r, d, h, w);
  MMTTA_CHECK(r <= CC_MAX_R, MMTTA_ERR_UNSUPPORTED, "lesionwise_nsd: r = %d regions, at most %d", r, CC_MAX_R);
  MMTTA_CHECK(lw_extent_ok((int64_t)n * r, d, h, w), MMTTA_ERR_UNSUPPORTED,
              "lesionwise_nsd: %d x %d masks of %d x %d x %d voxels are beyond the limits of mmtta_lesionwise_scores", n, r, d, h, w);
  for (int i = 0; i < CC_MAX_R; ++i) a.min_voxels[i] = 0ull;
  for (int i = 0; i < r; ++i) {
    MMTTA_CHECK(min_lesion_voxels[i] >= 0, MMTTA_ERR_INVALID, "lesionwise_nsd: min_lesion_voxels[%d] = %lld is negative", i,
                (long long)min_lesion_voxels[i]);
    a.min_voxels[i] = (unsigned long long)min_lesion_voxels[i];
  }
  hipStream_t s = (hipStream_t)stream;
  const long long V = (long long)d * h * w, M = (long long)n * r;
  a.cap = lw_table_slots(d, h, w, a.logcap);
  const LwLayout lw = lw_layout(M, V, a.cap);
  const char* lbase = (const char*)lesionwise_scratch;
  a.pred = mask;
  a.gd = (const unsigned char*)(lbase + lw.gd);
  a.LG = (const int*)(lbase + lw.LG);
  a.LP = (const int*)(lbase + lw.LP);
  a.pg = (const unsigned int*)(lbase + lw.pg);
  a.own = (const unsigned int*)(lbase + lw.own);
  a.matched = (const unsigned char*)(lbase + lw.matched);
  a.table = (const unsigned long long*)(lbase + lw.table);
  a.M = (int)M; a.R = r; a.D = d; a.H = h; a.W = w; a.V = V;
  a.WW = (w + 63) / 64;
  a.words = (long long)d * h * a.WW;
  const LnLayout l = ln_layout(M, V, a.words);
  char* base = (char*)scratch;
  a.cntP = (unsigned int*)(base + l.cntP);
  a.den = (unsigned int*)(base + l.den);
  a.hits = (unsigned int*)(base + l.hits);
  a.ep = (unsigned long long*)(base + l.ep);
  a.eg = (unsigned long long*)(base + l.eg);
  a.ovf = (unsigned long long*)(base + l.ovf);
  a.stats = (unsigned long long*)nsd_stats;
  a.lesion_nsd = lesion_nsd;

  const size_t mv = (size_t)M * (size_t)V;
  hipError_t e = hipMemsetAsync(base, 0, l.hits + mv * 4 * a.win.T, s);      // cntP, den and the hits of the T tolerances in use
  MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "lesionwise_nsd: memset failed: %s", hipGetErrorString(e));
  e = hipMemsetAsync(nsd_stats, 0, (size_t)M * a.win.T * sizeof(int64_t), s);
  MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "lesionwise_nsd: memset failed: %s", hipGetErrorString(e));
  if (lesion_nsd != nullptr) {
    e = hipMemsetD32Async((hipDeviceptr_t)lesion_nsd, 0x7fc00000, mv * a.win.T, s);      // quiet NaN
    MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "lesionwise_nsd: memset failed: %s", hipGetErrorString(e));
  }
  const dim3 wgrid((unsigned)((a.words + 3) / 4), (unsigned)M);
  const dim3 vox((unsigned)((V + 255) / 256), (unsigned)M);
  const dim3 slots((unsigned)((a.cap + 255) / 256), (unsigned)M);
  hipLaunchKernelGGL(ln_edges_kernel, wgrid, dim3(256), 0, s, a);
  st = launch_status("lesionwise_nsd edges");
  if (st) return st;
  hipLaunchKernelGGL(ln_window_a_kernel, wgrid, dim3(256), 0, s, a);
  st = launch_status("lesionwise_nsd window a");
  if (st) return st;
  hipLaunchKernelGGL(ln_window_p_kernel, wgrid, dim3(256), 0, s, a);
  st = launch_status("lesionwise_nsd window p");
  if (st) return st;
  hipLaunchKernelGGL(ln_window_f_kernel, wgrid, dim3(256), 0, s, a);
  st = launch_status("lesionwise_nsd window p, many lesions");
  if (st) return st;
  hipLaunchKernelGGL(ln_lengths_kernel, slots, dim3(256), 0, s, a);
  st = launch_status("lesionwise_nsd lengths");
  if (st) return st;
  hipLaunchKernelGGL(ln_finish_kernel, vox, dim3(256), 0, s, a);
  return launch_status("lesionwise_nsd finish");
}
