// Lesion-wise HD95 of the evaluation tail (the other half of the BraTS-2023 lesion-wise score): per kept, found lesion g
// the percentile Hausdorff distance between the surface of its own voxels A_g and the surface of P_g, the union of the
// predicted components matched to it.  Runs right behind mmtta_lesionwise_scores on the same stream and only reads what
// that call left in its scratch (lesionwise.h): Gd / G, the lesion and component roots, own-voxel counts, |P_g|, the
// matched flags and the table of distinct (component, lesion) pairs.  Nothing is labelled twice.
//
//   K1 edges    edge(X) = X & ~erode6(X) of G and of P in one pass (6-adjacent voxels of G lie in one lesion, those of P in
//               one component, so edge(A_g) = edge(G) within lesion g and edge(P_g) = edge(P) within the matched
//               components); edge voxels counted per lesion root and per component root, one atomic per distinct root of
//               a wave.
//   K2 roots    per lesion root: kept and found?  then its segment of the A-side lists (bump allocation; at most V entries
//               per mask, every edge voxel of G lies in one lesion).  Per matched component root: its segment of the
//               component lists (likewise at most V).
//   K3 lengths  walk of the pair table: every occupied slot (c, g) of a kept lesion adds edges(c) to g's P-side length and
//               to the mask's total; what the length was before is the slot's offset inside the lesion's segment.
//   K4 pool     per scored lesion: its segment of the P-side pool (2 V entries per mask), or, when the mask's total does
//               not fit, nothing: the mask's `overflow` counts its unscored lesions and none of it is scored (the total is
//               a sum, so whether a mask overflows does not depend on scheduling).  Scored lesions join a compact list.
//   K5 fill     packed coordinates (10 bits per axis) of the edge voxels into the A-side and the component lists.
//   K6 gather   second walk of the pair table, a wave per 64 slots and HD_GATHER_Z workgroups per wave of slots, each of
//               which copies its slice of every list: the component's list goes into its piece of the lesion's pool
//               segment, so that P_g's surface is ONE contiguous list.  (This replaces per-pair distance sets combined by
//               an atomic minimum: a lesion's two directions become plain brute-force passes between two lists and no
//               distance is written twice.)
//   K7 nearest  brute force, N-body style: work units are (lesion, direction, chunk of HD_SRC sources), dealt round-robin
//               to a fixed grid, so one large lesion spreads over the whole chip.  A source sits in registers, candidates
//               are staged through LDS as doubles in tiles of HD_TILE.  The arithmetic is surface.hip's: the squared
//               distance in fp64 as fma(dz sd, dz sd, fma(dy sh, dy sh, (dx sw)^2)), the minimum over every candidate,
//               then sqrt to float32.  A tile is staged with its bounding box; the same expression of a source's
//               distance to the box bounds every candidate of the tile from below (each term is monotone in |d|, rounding
//               included), so a tile that no source of the workgroup can gain from is skipped: the minimum is still the
//               minimum over every candidate.  The lists are roughly in voxel order, so the walk starts at the tile where
//               the first source's z suggests its neighbours lie and wraps around.
//   K8 select   one workgroup per lesion of the compact list, grid-striding: the two radix-select quantiles
//               (surface_quantile.h), the larger one is hd_g, rounded once in fp64 to 2^-20 and summed as an integer.
//
// Cost: sum over pairs of |edge(c)| |edge(A_g)| distance evaluations per direction.  Segments are handed out by atomic
// bumps: their placement and the order inside a list depend on scheduling, the multisets of distances do not, and the
// radix select and the integer sum see only those.  The launch sequence depends on the shape alone.
#include "lesionwise.h"
#include "surface_quantile.h"

namespace mmtta {

constexpr int HD_MAX_DIM = 1024;               // 10 bits per axis in a packed coordinate
constexpr int HD_SRC = 128;                    // sources of a work unit = threads of a K7 workgroup
constexpr int HD_TILE = 512;                   // candidates staged in LDS at a time (12 KB)
constexpr int HD_NEAR_BLOCKS = 1024;           // K7 workgroups per mask
constexpr int HD_SELECT_BLOCKS = 64;           // K8 workgroups per mask
constexpr int HD_GATHER_Z = 16;                // K6 workgroups that share the lists of one wave of slots
constexpr unsigned int HD_NONE = 0xffffffffu;  // at a root: no segment (lesion not scored, component not matched)
constexpr double HD_Q_ONE = 1048576.0;         // 2^20

struct HdHead {                 // per mask, zeroed by the call
  unsigned long long ptotal;    // sum over the pairs of kept lesions of edges(c)
  unsigned int nles;            // scored lesions in the compact list
  unsigned int poolA, poolC, poolP;      // bump cursors
  unsigned int pad[2];
};

struct HdArgs {
  const unsigned char* pred;    // [M][V]
  const unsigned char* gd;      // [M][V] bit 0: Gd, bit 1: G
  const int* LG;                // [M][V]
  const int* LP;                // [M][V]
  const unsigned int* pg;       // [M][V] at a lesion root
  const unsigned int* own;      // [M][V] at a lesion root
  const unsigned char* matched; // [M][V] at a component root
  const unsigned long long* table;       // [M][cap]
  unsigned long long cap;
  int M, R, D, H, W;
  long long V;
  double sd, sh, sw;
  float q;
  HdHead* head;                 // [M]
  unsigned char* edge;          // [M][V] bit 0: edge of P, bit 1: edge of G
  unsigned int* cntG;           // [M][V] at a lesion root: edge voxels of A_g          (zeroed)
  unsigned int* cntP;           // [M][V] at a component root: its edge voxels           (zeroed)
  unsigned int* plen;           // [M][V] at a lesion root: edge voxels of P_g           (zeroed)
  unsigned int* offG;           // [M][V] at a lesion root: start of its A-side segment, or HD_NONE
  unsigned int* offP;           // [M][V] at a component root: start of its list, or HD_NONE
  unsigned int* curG;           // [M][V] fill cursors, set to 0 at the roots by K2
  unsigned int* curP;
  unsigned int* pstart;         // [M][V] at a scored lesion's root: start of its pool segment
  unsigned int* rel;            // [M][cap] per occupied slot of a kept lesion: offset of the pair inside the lesion's segment
  unsigned int* list;           // [M][V] roots of the scored lesions
  unsigned int* coordA;         // [M][V] packed coordinates, A side
  unsigned int* coordC;         // [M][V] packed coordinates per component
  float* distA;                 // [M][V] d(A_g -> P_g)
  unsigned int* poolC;          // [M][2V] packed coordinates of P_g per lesion
  float* poolD;                 // [M][2V] d(P_g -> A_g)
  unsigned long long* stats;    // [M][3] hd_q, lesions scored, overflow
  float* lesion_hd;             // [M][V] or nullptr
  unsigned long long min_voxels[CC_MAX_R];
};

__device__ inline unsigned int hd_pack(int z, int y, int x) { return ((unsigned int)z << 20) | ((unsigned int)y << 10) | (unsigned int)x; }

// K1
__global__ __launch_bounds__(256) void hd_edges_kernel(HdArgs a) {
  const int m = blockIdx.y;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool in = v < a.V;
  const long long mv = (long long)m * a.V;
  const long long vc = in ? v : 0;
  long long t = vc;
  const int x = (int)(t % a.W); t /= a.W;
  const int y = (int)(t % a.H);
  const int z = (int)(t / a.H);
  const unsigned char* pm = a.pred + mv;
  const unsigned char* gm = a.gd + mv;
  const long long hw = (long long)a.H * a.W;
  // the six neighbours from clamped coordinates; one outside the volume is background
  const long long nb[6] = {z > 0 ? vc - hw : vc, z + 1 < a.D ? vc + hw : vc, y > 0 ? vc - a.W : vc, y + 1 < a.H ? vc + a.W : vc,
                           x > 0 ? vc - 1 : vc, x + 1 < a.W ? vc + 1 : vc};
  const bool inb[6] = {z > 0, z + 1 < a.D, y > 0, y + 1 < a.H, x > 0, x + 1 < a.W};
  const bool p = in && pm[vc] != 0;
  const bool g = in && (gm[vc] & 2u) != 0u;
  bool pin = true, gin = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    pin = pin && inb[j] && pm[nb[j]] != 0;
    gin = gin && inb[j] && (gm[nb[j]] & 2u) != 0u;
  }
  const bool ep = p && !pin, eg = g && !gin;
  if (in) a.edge[mv + v] = (unsigned char)((ep ? 1 : 0) | (eg ? 2 : 0));
  const int lane = threadIdx.x & 63;
  const int lg = eg ? a.LG[mv + vc] : -1;
  const int lp = ep ? a.LP[mv + vc] : -1;
  unsigned long long todo = __ballot(eg);
  while (todo != 0ull) {
    const int lead = __ffsll((long long)todo) - 1;
    const int root = __shfl(lg, lead);
    const unsigned long long same = __ballot(eg && lg == root);
    if (lane == lead) atomicAdd(a.cntG + mv + root, (unsigned int)__popcll(same));
    todo &= ~same;
  }
  todo = __ballot(ep);
  while (todo != 0ull) {
    const int lead = __ffsll((long long)todo) - 1;
    const int root = __shfl(lp, lead);
    const unsigned long long same = __ballot(ep && lp == root);
    if (lane == lead) atomicAdd(a.cntP + mv + root, (unsigned int)__popcll(same));
    todo &= ~same;
  }
}

// K2
__global__ __launch_bounds__(256) void hd_roots_kernel(HdArgs a) {
  const int m = blockIdx.y, r = m % a.R;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= a.V) return;
  const long long at = (long long)m * a.V + v;
  HdHead* hd = a.head + m;
  if ((a.gd[at] & 1u) && a.LG[at] == (int)v) {
    const bool scored = (unsigned long long)a.own[at] >= a.min_voxels[r] && a.pg[at] != 0u;      // kept and found
    a.offG[at] = scored ? atomicAdd(&hd->poolA, a.cntG[at]) : HD_NONE;
    a.curG[at] = 0u;
  }
  if (a.LP[at] == (int)v) {
    a.offP[at] = a.matched[at] != 0 ? atomicAdd(&hd->poolC, a.cntP[at]) : HD_NONE;
    a.curP[at] = 0u;
  }
}

// K3
__global__ __launch_bounds__(256) void hd_lengths_kernel(HdArgs a) {
  const int m = blockIdx.y;
  const unsigned long long slot = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (slot >= a.cap) return;
  const unsigned long long key = a.table[(unsigned long long)m * a.cap + slot];
  if (key == 0ull) return;
  const long long mv = (long long)m * a.V;
  const long long c = (long long)(key >> 32) - 1, g = (long long)(key & 0xffffffffull) - 1;
  if (a.offG[mv + g] == HD_NONE) return;
  const unsigned int n = a.cntP[mv + c];      // >= 1: a component has an edge voxel
  a.rel[(unsigned long long)m * a.cap + slot] = atomicAdd(a.plen + mv + g, n);
  atomicAdd(&a.head[m].ptotal, (unsigned long long)n);
}

// K4
__global__ __launch_bounds__(256) void hd_pool_kernel(HdArgs a) {
  const int m = blockIdx.y;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= a.V) return;
  const long long at = (long long)m * a.V + v;
  if (!((a.gd[at] & 1u) && a.LG[at] == (int)v) || a.offG[at] == HD_NONE) return;
  HdHead* hd = a.head + m;
  if (hd->ptotal > 2ull * (unsigned long long)a.V) {      // the mask's lists do not fit: none of it is scored
    atomicAdd(a.stats + (long long)m * 3 + 2, 1ull);
    return;
  }
  a.pstart[at] = atomicAdd(&hd->poolP, a.plen[at]);
  a.list[(long long)m * a.V + atomicAdd(&hd->nles, 1u)] = (unsigned int)v;
}

// K5
__global__ __launch_bounds__(256) void hd_fill_kernel(HdArgs a) {
  const int m = blockIdx.y;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool in = v < a.V;
  const long long mv = (long long)m * a.V;
  const long long vc = in ? v : 0;
  long long t = vc;
  const int x = (int)(t % a.W); t /= a.W;
  const int y = (int)(t % a.H);
  const int z = (int)(t / a.H);
  const unsigned int e = in ? a.edge[mv + vc] : 0u;
  const int lg = (e & 2u) ? a.LG[mv + vc] : -1;
  const int lp = (e & 1u) ? a.LP[mv + vc] : -1;
  const unsigned int og = lg >= 0 ? a.offG[mv + lg] : HD_NONE;
  const unsigned int op = lp >= 0 ? a.offP[mv + lp] : HD_NONE;
  const bool fg = og != HD_NONE, fp = op != HD_NONE;
  const unsigned int packed = hd_pack(z, y, x);
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned long long todo = __ballot(fg);
  while (todo != 0ull) {
    const int lead = __ffsll((long long)todo) - 1;
    const int root = __shfl(lg, lead);
    const unsigned long long same = __ballot(fg && lg == root);
    unsigned int base = 0;
    if (lane == lead) base = atomicAdd(a.curG + mv + root, (unsigned int)__popcll(same));
    base = __shfl(base, lead);
    if (fg && lg == root) a.coordA[mv + og + base + (unsigned int)__popcll(same & below)] = packed;      // < offG + cntG <= V
    todo &= ~same;
  }
  todo = __ballot(fp);
  while (todo != 0ull) {
    const int lead = __ffsll((long long)todo) - 1;
    const int root = __shfl(lp, lead);
    const unsigned long long same = __ballot(fp && lp == root);
    unsigned int base = 0;
    if (lane == lead) base = atomicAdd(a.curP + mv + root, (unsigned int)__popcll(same));
    base = __shfl(base, lead);
    if (fp && lp == root) a.coordC[mv + op + base + (unsigned int)__popcll(same & below)] = packed;      // < offP + cntP <= V
    todo &= ~same;
  }
}

// K6: a wave per 64 slots; the wave copies its slice (blockIdx.z of HD_GATHER_Z) of the list of every pair it holds
__global__ __launch_bounds__(256) void hd_gather_kernel(HdArgs a) {
  const int m = blockIdx.y;
  const unsigned long long slot = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  const long long mv = (long long)m * a.V;
  const bool fits = a.head[m].ptotal <= 2ull * (unsigned long long)a.V;
  const unsigned long long key = slot < a.cap ? a.table[(unsigned long long)m * a.cap + slot] : 0ull;
  const long long c = (long long)(key >> 32) - 1, g = (long long)(key & 0xffffffffull) - 1;
  const bool use = fits && key != 0ull && a.offG[mv + g] != HD_NONE;
  unsigned int n = 0, src = 0, dst = 0;
  if (use) {
    n = a.cntP[mv + c];
    src = a.offP[mv + c];      // matched, so it has a list
    dst = a.pstart[mv + g] + a.rel[(unsigned long long)m * a.cap + slot];      // dst + n <= pstart + plen <= 2 V
  }
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(use);
  const unsigned int* from = a.coordC + mv;
  unsigned int* to = a.poolC + 2 * mv;
  while (todo != 0ull) {
    const int lead = __ffsll((long long)todo) - 1;
    const unsigned int nn = __shfl(n, lead), s0 = __shfl(src, lead), d0 = __shfl(dst, lead);
    for (unsigned int i = blockIdx.z * 64 + lane; i < nn; i += 64 * HD_GATHER_Z) to[d0 + i] = from[s0 + i];
    todo &= todo - 1ull;
  }
}

// K7
__global__ __launch_bounds__(HD_SRC) void hd_nearest_kernel(HdArgs a) {
  __shared__ double cz[HD_TILE], cy[HD_TILE], cx[HD_TILE];
  __shared__ int bb[6];      // bounding box of the staged tile: min z, y, x, max z, y, x
  const int m = blockIdx.y;
  const long long mv = (long long)m * a.V;
  const unsigned int nles = a.head[m].nles;
  const unsigned int* list = a.list + mv;
  unsigned long long u = 0;      // units before the current lesion
  for (unsigned int li = 0; li < nles; ++li) {
    const unsigned int g = list[li];
    const unsigned int nA = a.cntG[mv + g], nP = a.plen[mv + g];
    const unsigned int uA = (nA + HD_SRC - 1) / HD_SRC, uP = (nP + HD_SRC - 1) / HD_SRC;
    const unsigned int units = uA + uP;
    unsigned int k = (unsigned int)((blockIdx.x + gridDim.x - u % gridDim.x) % gridDim.x);
    u += units;
    if (k >= units) continue;
    const unsigned int* listA = a.coordA + mv + a.offG[mv + g];
    const unsigned int* listP = a.poolC + 2 * mv + a.pstart[mv + g];
    float* outA = a.distA + mv + a.offG[mv + g];
    float* outP = a.poolD + 2 * mv + a.pstart[mv + g];
    for (; k < units; k += gridDim.x) {
      const bool fromA = k < uA;      // direction A_g -> P_g, else P_g -> A_g
      const unsigned int* src = fromA ? listA : listP;
      const unsigned int* cand = fromA ? listP : listA;
      const unsigned int nsrc = fromA ? nA : nP, ncand = fromA ? nP : nA;
      float* out = fromA ? outA : outP;
      const unsigned int i0 = (fromA ? k : k - uA) * HD_SRC;      // < nsrc
      const unsigned int i = i0 + threadIdx.x;
      const unsigned int s = src[i < nsrc ? i : nsrc - 1];
      const int zi = (int)(s >> 20), yi = (int)((s >> 10) & 1023u), xi = (int)(s & 1023u);
      const double z = (double)zi, y = (double)yi, x = (double)xi;
      const unsigned int ntiles = (ncand + HD_TILE - 1) / HD_TILE;
      unsigned int first = (unsigned int)(((unsigned long long)(src[i0] >> 20) * ntiles) / (unsigned int)a.D);      // uniform
      first = first < ntiles ? first : ntiles - 1;
      double best = INFINITY;
      for (unsigned int tt = 0; tt < ntiles; ++tt) {
        const unsigned int t0 = ((first + tt) % ntiles) * HD_TILE;
        const unsigned int nt = ncand - t0 < (unsigned int)HD_TILE ? ncand - t0 : (unsigned int)HD_TILE;
        __syncthreads();      // the previous tile and its box have been read
        if (threadIdx.x < 6) bb[threadIdx.x] = threadIdx.x < 3 ? HD_MAX_DIM : -1;
        __syncthreads();
        int lo[3] = {HD_MAX_DIM, HD_MAX_DIM, HD_MAX_DIM}, hi[3] = {-1, -1, -1};
        for (unsigned int j = threadIdx.x; j < nt; j += HD_SRC) {
          const unsigned int cc = cand[t0 + j];
          const int c3[3] = {(int)(cc >> 20), (int)((cc >> 10) & 1023u), (int)(cc & 1023u)};
          cz[j] = (double)c3[0]; cy[j] = (double)c3[1]; cx[j] = (double)c3[2];
#pragma unroll
          for (int ax = 0; ax < 3; ++ax) { lo[ax] = c3[ax] < lo[ax] ? c3[ax] : lo[ax]; hi[ax] = c3[ax] > hi[ax] ? c3[ax] : hi[ax]; }
        }
        if (threadIdx.x < nt) {
#pragma unroll
          for (int ax = 0; ax < 3; ++ax) { atomicMin(&bb[ax], lo[ax]); atomicMax(&bb[3 + ax], hi[ax]); }
        }
        __syncthreads();
        // the source's distance to the box, per axis; 0 inside
        const int gz = zi < bb[0] ? bb[0] - zi : zi > bb[3] ? zi - bb[3] : 0;
        const int gy = yi < bb[1] ? bb[1] - yi : yi > bb[4] ? yi - bb[4] : 0;
        const int gx = xi < bb[2] ? bb[2] - xi : xi > bb[5] ? xi - bb[5] : 0;
        const double bd = (double)gz * a.sd, bh = (double)gy * a.sh, bw = (double)gx * a.sw;
        const double bound = fma(bd, bd, fma(bh, bh, bw * bw));
        if (!__syncthreads_or(bound < best ? 1 : 0)) continue;      // no source of the workgroup can gain from this tile
#pragma unroll 4
        for (unsigned int j = 0; j < nt; ++j) {
          const double fd = (z - cz[j]) * a.sd, fh = (y - cy[j]) * a.sh, fw = (x - cx[j]) * a.sw;      // integer differences: exact
          const double val = fma(fd, fd, fma(fh, fh, fw * fw));
          best = fmin(best, val);
        }
      }
      if (i < nsrc) out[i] = (float)sqrt(best);
    }
  }
}

// K8
__global__ __launch_bounds__(1024) void hd_select_kernel(HdArgs a, int use_max) {
  __shared__ unsigned int hist[256];
  __shared__ unsigned int sh[2];
  const int m = blockIdx.y;
  const long long mv = (long long)m * a.V;
  const unsigned int nles = a.head[m].nles;
  const float qq = use_max ? 1.0f : a.q;
  unsigned long long sum = 0ull, cnt = 0ull;
  for (unsigned int li = blockIdx.x; li < nles; li += gridDim.x) {
    const unsigned int g = a.list[mv + li];
    const float q0 = surf_quantile(a.poolD + 2 * mv + a.pstart[mv + g], a.plen[mv + g], qq, hist, sh);
    const float q1 = surf_quantile(a.distA + mv + a.offG[mv + g], a.cntG[mv + g], qq, hist, sh);
    const float hd = q0 > q1 ? q0 : q1;
    sum += (unsigned long long)rint((double)hd * HD_Q_ONE);
    ++cnt;
    if (threadIdx.x == 0 && a.lesion_hd != nullptr) a.lesion_hd[mv + g] = hd;
  }
  if (threadIdx.x == 0 && cnt != 0ull) {
    atomicAdd(a.stats + (long long)m * 3, sum);
    atomicAdd(a.stats + (long long)m * 3 + 1, cnt);
  }
}

struct HdLayout {
  size_t zero_bytes, cntG, cntP, plen, offG, offP, curG, curP, pstart, rel, list, coordA, coordC, distA, edge, poolC, poolD, total;
};

// [heads | cntG | cntP | plen] are zeroed by one memset
static HdLayout hd_layout(int64_t M, int64_t V, unsigned long long cap) {
  HdLayout l;
  const size_t mv = (size_t)M * (size_t)V;
  size_t o = lw_align((size_t)M * sizeof(HdHead));
  l.cntG = o; o += lw_align(mv * 4);
  l.cntP = o; o += lw_align(mv * 4);
  l.plen = o; o += lw_align(mv * 4);
  l.zero_bytes = o;
  l.offG = o; o += lw_align(mv * 4);
  l.offP = o; o += lw_align(mv * 4);
  l.curG = o; o += lw_align(mv * 4);
  l.curP = o; o += lw_align(mv * 4);
  l.pstart = o; o += lw_align(mv * 4);
  l.rel = o; o += lw_align((size_t)M * (size_t)cap * 4);
  l.list = o; o += lw_align(mv * 4);
  l.coordA = o; o += lw_align(mv * 4);
  l.coordC = o; o += lw_align(mv * 4);
  l.distA = o; o += lw_align(mv * 4);
  l.edge = o; o += lw_align(mv);
  l.poolC = o; o += lw_align(mv * 8);
  l.poolD = o; o += lw_align(mv * 8);
  l.total = o;
  return l;
}

static bool hd_extent_ok(int64_t n_masks, int64_t d, int64_t h, int64_t w) {
  return lw_extent_ok(n_masks, d, h, w) && d <= HD_MAX_DIM && h <= HD_MAX_DIM && w <= HD_MAX_DIM;
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int64_t mmtta_lesionwise_hd95_scratch_bytes(int64_t n_masks, int64_t d, int64_t h, int64_t w) {
  if (!hd_extent_ok(n_masks, d, h, w)) return -1;
  int logcap;
  return (int64_t)hd_layout(n_masks, d * h * w, lw_table_slots(d, h, w, logcap)).total;
}

extern "C" int mmtta_lesionwise_hd95(const uint8_t* mask, const mmtta_tensor* label, int n, int r, int d, int h, int w,
                                     const double* spacing, double percentile, const int64_t* min_lesion_voxels,
                                     const void* lesionwise_scratch, int64_t* hd_stats, float* lesion_hd, void* scratch,
                                     void* stream) {
  MMTTA_CHECK(mask != nullptr, MMTTA_ERR_INVALID, "lesionwise_hd95: null `mask`");
  MMTTA_CHECK(label != nullptr, MMTTA_ERR_INVALID, "lesionwise_hd95: null `label`");
  MMTTA_CHECK(spacing != nullptr, MMTTA_ERR_INVALID, "lesionwise_hd95: null `spacing`");
  MMTTA_CHECK(min_lesion_voxels != nullptr, MMTTA_ERR_INVALID, "lesionwise_hd95: null `min_lesion_voxels`");
  MMTTA_CHECK(lesionwise_scratch != nullptr, MMTTA_ERR_INVALID, "lesionwise_hd95: null `lesionwise_scratch`");
  MMTTA_CHECK(hd_stats != nullptr, MMTTA_ERR_INVALID, "lesionwise_hd95: null `hd_stats`");
  MMTTA_CHECK(scratch != nullptr, MMTTA_ERR_INVALID, "lesionwise_hd95: null `scratch`");
  MMTTA_CHECK(n >= 1 && r >= 1 && d >= 1 && h >= 1 && w >= 1, MMTTA_ERR_INVALID,
              "lesionwise_hd95: every extent must be >= 1, got %d %d %d %d %d", n, r, d, h, w);
  MMTTA_CHECK(r <= CC_MAX_R, MMTTA_ERR_UNSUPPORTED, "lesionwise_hd95: r = %d regions, at most %d", r, CC_MAX_R);
  MMTTA_CHECK(d <= HD_MAX_DIM && h <= HD_MAX_DIM && w <= HD_MAX_DIM, MMTTA_ERR_UNSUPPORTED,
              "lesionwise_hd95: spatial extent %d x %d x %d above %d", d, h, w, HD_MAX_DIM);
  MMTTA_CHECK(hd_extent_ok((int64_t)n * r, d, h, w), MMTTA_ERR_UNSUPPORTED,
              "lesionwise_hd95: %d x %d masks of %d x %d x %d voxels are beyond the limits of mmtta_lesionwise_scores", n, r, d, h, w);
  for (int i = 0; i < 3; ++i)
    MMTTA_CHECK(spacing[i] > 0.0 && spacing[i] <= 1.7976931348623157e308, MMTTA_ERR_INVALID,
                "lesionwise_hd95: spacing[%d] = %g must be positive and finite", i, spacing[i]);
  MMTTA_CHECK(percentile >= 0.0 && percentile <= 100.0, MMTTA_ERR_INVALID,
              "lesionwise_hd95: percentile should be within [0, 100], got %g", percentile);
  MMTTA_CHECK(label->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "mmtta_lesionwise_hd95: `label` must be fp32-stored");
  MMTTA_CHECK(label->ptr != nullptr, MMTTA_ERR_INVALID, "lesionwise_hd95: null `label` data");
  MMTTA_CHECK(label->n == n && label->c == r && label->d == d && label->h == h && label->w == w, MMTTA_ERR_INVALID,
              "lesionwise_hd95: `label` shape differs from the mask's");
  HdArgs a;
  for (int i = 0; i < CC_MAX_R; ++i) a.min_voxels[i] = 0ull;
  for (int i = 0; i < r; ++i) {
    MMTTA_CHECK(min_lesion_voxels[i] >= 0, MMTTA_ERR_INVALID, "lesionwise_hd95: min_lesion_voxels[%d] = %lld is negative", i,
                (long long)min_lesion_voxels[i]);
    a.min_voxels[i] = (unsigned long long)min_lesion_voxels[i];
  }
  hipStream_t s = (hipStream_t)stream;
  const long long V = (long long)d * h * w, M = (long long)n * r;
  int logcap;
  a.cap = lw_table_slots(d, h, w, logcap);
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
  a.sd = spacing[0]; a.sh = spacing[1]; a.sw = spacing[2];
  a.q = (float)(percentile / 100.0);
  const HdLayout l = hd_layout(M, V, a.cap);
  char* base = (char*)scratch;
  a.head = (HdHead*)base;
  a.cntG = (unsigned int*)(base + l.cntG);
  a.cntP = (unsigned int*)(base + l.cntP);
  a.plen = (unsigned int*)(base + l.plen);
  a.offG = (unsigned int*)(base + l.offG);
  a.offP = (unsigned int*)(base + l.offP);
  a.curG = (unsigned int*)(base + l.curG);
  a.curP = (unsigned int*)(base + l.curP);
  a.pstart = (unsigned int*)(base + l.pstart);
  a.rel = (unsigned int*)(base + l.rel);
  a.list = (unsigned int*)(base + l.list);
  a.coordA = (unsigned int*)(base + l.coordA);
  a.coordC = (unsigned int*)(base + l.coordC);
  a.distA = (float*)(base + l.distA);
  a.edge = (unsigned char*)(base + l.edge);
  a.poolC = (unsigned int*)(base + l.poolC);
  a.poolD = (float*)(base + l.poolD);
  a.stats = (unsigned long long*)hd_stats;
  a.lesion_hd = lesion_hd;

  hipError_t e = hipMemsetAsync(base, 0, l.zero_bytes, s);
  MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "lesionwise_hd95: memset failed: %s", hipGetErrorString(e));
  e = hipMemsetAsync(hd_stats, 0, (size_t)M * 3 * sizeof(int64_t), s);
  MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "lesionwise_hd95: memset failed: %s", hipGetErrorString(e));
  if (lesion_hd != nullptr) {
    e = hipMemsetD32Async((hipDeviceptr_t)lesion_hd, 0x7fc00000, (size_t)M * (size_t)V, s);      // quiet NaN
    MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "lesionwise_hd95: memset failed: %s", hipGetErrorString(e));
  }
  const dim3 vox((unsigned)((V + 255) / 256), (unsigned)M);
  const dim3 slots((unsigned)((a.cap + 255) / 256), (unsigned)M);
  hipLaunchKernelGGL(hd_edges_kernel, vox, dim3(256), 0, s, a);
  int st = launch_status("lesionwise_hd95 edges");
  if (st) return st;
  hipLaunchKernelGGL(hd_roots_kernel, vox, dim3(256), 0, s, a);
  st = launch_status("lesionwise_hd95 roots");
  if (st) return st;
  hipLaunchKernelGGL(hd_lengths_kernel, slots, dim3(256), 0, s, a);
  st = launch_status("lesionwise_hd95 lengths");
  if (st) return st;
  hipLaunchKernelGGL(hd_pool_kernel, vox, dim3(256), 0, s, a);
  st = launch_status("lesionwise_hd95 pool");
  if (st) return st;
  hipLaunchKernelGGL(hd_fill_kernel, vox, dim3(256), 0, s, a);
  st = launch_status("lesionwise_hd95 fill");
  if (st) return st;
  hipLaunchKernelGGL(hd_gather_kernel, dim3(slots.x, slots.y, HD_GATHER_Z), dim3(256), 0, s, a);
  st = launch_status("lesionwise_hd95 gather");
  if (st) return st;
  const long long near = HD_NEAR_BLOCKS * M <= CC_MAX_BLOCKS ? HD_NEAR_BLOCKS : CC_MAX_BLOCKS / M;      // >= 256: M <= 65535
  hipLaunchKernelGGL(hd_nearest_kernel, dim3((unsigned)near, (unsigned)M), dim3(HD_SRC), 0, s, a);
  st = launch_status("lesionwise_hd95 nearest");
  if (st) return st;
  hipLaunchKernelGGL(hd_select_kernel, dim3(HD_SELECT_BLOCKS, (unsigned)M), dim3(1024), 0, s, a, percentile >= 100.0 ? 1 : 0);
  return launch_status("lesionwise_hd95 select");
}
