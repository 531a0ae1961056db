// Hole filling and region nesting of the evaluation tail: the step after the component filter in common BraTS / HECKTOR
// post-processing (scipy.ndimage.binary_fill_holes over a copied mask, then a nesting fix on the host), without a copy to
// the host.  No counterpart in the reference evaluator.
//
// A hole is a component of the BACKGROUND (mask == 0, connectivity 6 / 18 / 26) that touches no face of the volume.  The
// background of a tumour mask is about 99 % of the volume in one component, so the complement gets a tile pass of its own:
//   K1 tile     the labeller's tile geometry and parent convention (components.h) over mask == 0.  A tile whose in-volume
//               voxels are all background (nearly every tile of a real volume) is a box and therefore one component at every
//               connectivity: all of its voxels take the tile's first voxel as parent, and the LDS union-find with its up to
//               13 neighbour visits per voxel is skipped.
//   K2 merge    cc_merge_kernel   } of components.hip, unchanged, with maxn of `fill_connectivity`: L = root of every
//   K3 flatten  cc_flatten_kernel } background voxel, size[root] = voxels of the component
//   K4 border   every background voxel on a face of the volume marks its root open: a plain byte store of 1 (every racing
//               writer stores the same value)
//   K5 finish   one thread per (n, voxel) walks the R regions: fill decision from (root, open, size, cap), then the
//               nesting chain over the filled bits (a 64-bit word, one bit per region), the final mask in place, and per
//               region inter / psum / gsum, holes, holes filled (both at root voxels), filled voxels and nest-changed
//               voxels: ballot popcounts -> LDS counters -> one integer atomic per block, region and column.
// The launch sequence depends on the shape alone; all sums are integers and a root is the smallest index of its component,
// so results do not depend on scheduling.
#include <cstdlib>

#include "components.h"

namespace mmtta {

struct FhArgs {
  unsigned char* mask;             // [N][R][V], read by K1, written by K5
  TV lab;                          // ground truth, used when counts != nullptr
  int N, R, D, H, W, maxn;         // maxn: largest |dz| + |dy| + |dx| of a neighbour (1, 2, 3)
  int tz, ty, tx;
  long long tiles, V;
  int* L;                          // [M][V] root of a background voxel, -1 on the mask
  const unsigned int* size;        // [M][V] voxels of a background component, at its root
  unsigned char* open;             // [M][V] at a root: 1 = the component touches a face of the volume
  unsigned long long* counts;      // [M][3] or nullptr
  unsigned long long* stats;       // [M][4]
  unsigned long long fill;         // bit r: region r fills its holes
  int chain_len, grow;
  unsigned char chain[CC_MAX_R];   // innermost first
  unsigned long long cap[CC_MAX_R];      // 0 = no cap
};

// K1.  UNIFORM = false is the measurement arm without the uniform-tile path (MMTTA_FILL_UNIFORM_TILES=0).
template <bool UNIFORM>
__global__ __launch_bounds__(256) void fh_tile_kernel(FhArgs a) {
  __shared__ int lab[CC_TILE];
  const int m = blockIdx.y;
  const unsigned char* pm = a.mask + (long long)m * a.V;
  int* L = a.L + (long long)m * a.V;
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    long long t = tile;
    const int x0 = (int)(t % a.tx) * CC_TX; t /= a.tx;
    const int y0 = (int)(t % a.ty) * CC_TY;
    const int z0 = (int)(t / a.ty) * CC_TZ;
    bool bg[CC_TILE / 256];
    bool all = true;
#pragma unroll
    for (int k = 0; k < CC_TILE / 256; ++k) {
      const int i = threadIdx.x + k * 256;
      const int z = z0 + i / (CC_TY * CC_TX), y = y0 + (i / CC_TX) % CC_TY, x = x0 + i % CC_TX;
      const bool in = z < a.D && y < a.H && x < a.W;
      const long long v = ((long long)(in ? z : 0) * a.H + (in ? y : 0)) * a.W + (in ? x : 0);
      bg[k] = in && pm[v] == 0;
      all = all && (bg[k] || !in);
    }
    if (UNIFORM && __syncthreads_and(all ? 1 : 0)) {      // a box of background: one component, its first voxel the root
      const int g = (int)(((long long)z0 * a.H + y0) * a.W + x0);
#pragma unroll
      for (int k = 0; k < CC_TILE / 256; ++k) {
        const int i = threadIdx.x + k * 256;
        const int z = z0 + i / (CC_TY * CC_TX), y = y0 + (i / CC_TX) % CC_TY, x = x0 + i % CC_TX;
        if (z < a.D && y < a.H && x < a.W) L[((long long)z * a.H + y) * a.W + x] = g;
      }
      continue;      // the LDS tile was not touched
    }
#pragma unroll
    for (int k = 0; k < CC_TILE / 256; ++k) lab[threadIdx.x + k * 256] = bg[k] ? threadIdx.x + k * 256 : -1;
    __syncthreads();
    for (int i = threadIdx.x; i < CC_TILE; i += 256) {
      if (lab[i] < 0) continue;
      const int lz = i / (CC_TY * CC_TX), ly = (i / CC_TX) % CC_TY, lx = i % CC_TX;
#pragma unroll
      for (int j = 0; j < 13; ++j) {
        const int dz = j / 9 - 1, dy = (j / 3) % 3 - 1, dx = j % 3 - 1;
        if ((dz != 0) + (dy != 0) + (dx != 0) > a.maxn) continue;
        const int nz = lz + dz, ny = ly + dy, nx = lx + dx;
        if (nz < 0 || ny < 0 || ny >= CC_TY || nx < 0 || nx >= CC_TX) continue;      // another tile: K2
        const int nb = (nz * CC_TY + ny) * CC_TX + nx;
        if (((volatile int*)lab)[nb] < 0) continue;
        // lock-free union in LDS, as cc_tile_kernel does it: the larger root goes under the smaller one
        int p = i, q = nb;
        for (;;) {
          for (int u; (u = ((volatile int*)lab)[p]) != p; p = u) {}
          for (int u; (u = ((volatile int*)lab)[q]) != q; q = u) {}
          if (p == q) break;
          if (p < q) { const int s = p; p = q; q = s; }
          const int old = atomicMin(lab + p, q);
          if (old == p) break;
          p = old;
        }
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CC_TILE; i += 256) {
      const int z = z0 + i / (CC_TY * CC_TX), y = y0 + (i / CC_TX) % CC_TY, x = x0 + i % CC_TX;
      if (!(z < a.D && y < a.H && x < a.W)) continue;
      int g = -1;
      if (lab[i] >= 0) {
        int r = i;
        for (int u; (u = ((volatile int*)lab)[r]) != r; r = u) {}
        const int rz = z0 + r / (CC_TY * CC_TX), ry = y0 + (r / CC_TX) % CC_TY, rx = x0 + r % CC_TX;
        g = (int)(((long long)rz * a.H + ry) * a.W + rx);
      }
      L[((long long)z * a.H + y) * a.W + x] = g;
    }
    __syncthreads();      // the LDS tile is reused by the next round
  }
}

// K4: only voxels on a face read their root
__global__ __launch_bounds__(256) void fh_border_kernel(FhArgs a) {
  const int m = blockIdx.y;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= a.V) return;
  long long t = v;
  const int x = (int)(t % a.W); t /= a.W;
  const int y = (int)(t % a.H);
  const int z = (int)(t / a.H);
  if (!(z == 0 || z == a.D - 1 || y == 0 || y == a.H - 1 || x == 0 || x == a.W - 1)) return;
  const int root = a.L[(long long)m * a.V + v];
  if (root >= 0) a.open[(long long)m * a.V + root] = 1;
}

constexpr int FH_COLS = 8;      // LDS counters per region: inter, psum, gsum, holes, holes filled, filled voxels, nest-changed, (unused)

__global__ __launch_bounds__(256) void fh_finish_kernel(FhArgs a) {
  __shared__ unsigned int s_cnt[CC_MAX_R * FH_COLS];
  const int n = blockIdx.y;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  for (int i = threadIdx.x; i < a.R * FH_COLS; i += 256) s_cnt[i] = 0u;
  __syncthreads();
  const bool in = v < a.V;
  const long long vc = in ? v : 0;
  const bool lead = (threadIdx.x & 63) == 0;
  // after filling: bit r = region r's mask at this voxel
  unsigned long long old = 0ull;
  for (int r = 0; r < a.R; ++r) {
    const long long mv = ((long long)n * a.R + r) * a.V;
    const int root = in ? a.L[mv + vc] : -1;
    const bool fg = in && root < 0;
    const bool hole = root >= 0 && a.open[mv + (root >= 0 ? root : 0)] == 0;
    bool filled = hole && ((a.fill >> r) & 1ull) != 0ull;
    if (filled && a.cap[r] != 0ull) filled = (unsigned long long)a.size[mv + root] <= a.cap[r];
    if (fg || filled) old |= 1ull << r;
    const bool isroot = hole && root == (int)v;
    const bool conds[3] = {isroot, isroot && filled, filled};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const unsigned long long bal = __ballot(conds[k]);
      if (lead && bal != 0ull) atomicAdd(&s_cnt[r * FH_COLS + 3 + k], (unsigned int)__popcll(bal));
    }
  }
  // the chain, innermost first: clip = AND with every region further out, grow = OR with every region further in
  unsigned long long fin = old;
  if (a.grow) {
    unsigned long long acc = 0ull;
    for (int i = 0; i < a.chain_len; ++i) {
      const int c = a.chain[i];
      acc |= (old >> c) & 1ull;
      fin = (fin & ~(1ull << c)) | (acc << c);
    }
  } else {
    unsigned long long acc = 1ull;
    for (int i = a.chain_len - 1; i >= 0; --i) {
      const int c = a.chain[i];
      acc &= (old >> c) & 1ull;
      fin = (fin & ~(1ull << c)) | (acc << c);
    }
  }
  long long lz = 0;
  if (a.counts != nullptr) {
    long long t = vc;
    const int x = (int)(t % a.W); t /= a.W;
    const int y = (int)(t % a.H);
    const int z = (int)(t / a.H);
    lz = (long long)n * a.lab.sn + (long long)z * a.lab.sd + (long long)y * a.lab.sh + (long long)x * a.lab.sw;
  }
  for (int r = 0; r < a.R; ++r) {
    const bool p = ((fin >> r) & 1ull) != 0ull;
    const bool changed = (((fin ^ old) >> r) & 1ull) != 0ull;
    if (in) a.mask[((long long)n * a.R + r) * a.V + v] = (unsigned char)(p ? 1 : 0);
    const bool g = a.counts != nullptr && in && a.lab.p[lz + (long long)r * a.lab.sc] > 0.5f;
    const bool conds[4] = {p && g, p, g, changed};
    const int col[4] = {0, 1, 2, 6};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned long long bal = __ballot(conds[k]);
      if (lead && bal != 0ull) atomicAdd(&s_cnt[r * FH_COLS + col[k]], (unsigned int)__popcll(bal));
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < a.R * FH_COLS; i += 256) {
    const unsigned int c = s_cnt[i];
    if (c == 0u) continue;
    const int r = i / FH_COLS, k = i % FH_COLS;
    const long long m = (long long)n * a.R + r;
    if (k < 3) {
      if (a.counts != nullptr) atomicAdd(a.counts + m * 3 + k, (unsigned long long)c);
    } else if (k < 7) {
      atomicAdd(a.stats + m * 4 + (k - 3), (unsigned long long)c);
    }
  }
}

static size_t fh_align(size_t v) { return (v + 255) & ~(size_t)255; }

static bool fh_extent_ok(int64_t n_masks, int64_t d, int64_t h, int64_t w) {
  if (n_masks < 1 || n_masks > 65535 || d < 1 || h < 1 || w < 1) return false;
  if (d > CC_MAX_V || h > CC_MAX_V || w > CC_MAX_V || d * h > CC_MAX_V || d * h * w > CC_MAX_V) return false;
  return n_masks * ((d * h * w + 255) / 256) <= CC_MAX_BLOCKS;
}

// A/B switch read from the environment once: MMTTA_FILL_UNIFORM_TILES=0 labels every tile through the LDS union-find
static const bool g_uniform_tiles = !(getenv("MMTTA_FILL_UNIFORM_TILES") && atoi(getenv("MMTTA_FILL_UNIFORM_TILES")) == 0);

}  // namespace mmtta

using namespace mmtta;

// [per-mask header | sizes | open flags] are zeroed by one memset; then the parent volume
extern "C" int64_t mmtta_mask_fill_nest_scratch_bytes(int64_t n_masks, int64_t d, int64_t h, int64_t w) {
  if (!fh_extent_ok(n_masks, d, h, w)) return -1;
  const size_t mv = (size_t)n_masks * (size_t)(d * h * w);
  return (int64_t)(fh_align((size_t)n_masks * 4) + fh_align(mv * 4) + fh_align(mv) + fh_align(mv * 4));
}

extern "C" int mmtta_mask_fill_nest(uint8_t* mask, const mmtta_tensor* label, int n, int r, int d, int h, int w,
                                    int fill_connectivity, const int32_t* fill_holes, const int64_t* max_hole_voxels,
                                    const int32_t* chain, int chain_len, int nest_mode, int64_t* counts, int64_t* stats,
                                    void* scratch, void* stream) {
  MMTTA_CHECK(mask && fill_holes && max_hole_voxels && stats && scratch, MMTTA_ERR_INVALID, "fill_nest: null argument");
  MMTTA_CHECK(fill_connectivity == 6 || fill_connectivity == 18 || fill_connectivity == 26, MMTTA_ERR_INVALID,
              "fill_nest: fill_connectivity %d (6, 18 or 26)", fill_connectivity);
  MMTTA_CHECK(n >= 1 && r >= 1 && d >= 1 && h >= 1 && w >= 1, MMTTA_ERR_INVALID,
              "fill_nest: every extent must be >= 1, got %d %d %d %d %d", n, r, d, h, w);
  MMTTA_CHECK(r <= CC_MAX_R, MMTTA_ERR_UNSUPPORTED, "fill_nest: r = %d regions, at most %d", r, CC_MAX_R);
  MMTTA_CHECK((long long)n * r <= 65535, MMTTA_ERR_UNSUPPORTED, "fill_nest: more than 65535 masks per call");
  const long long dh = (long long)d * h;      // each factor below 2^31: no overflow before the checks
  MMTTA_CHECK(dh <= CC_MAX_V && dh * w <= CC_MAX_V, MMTTA_ERR_UNSUPPORTED,
              "fill_nest: d*h*w = %d*%d*%d voxels, at most 2^31 - 2", d, h, w);
  const long long V = dh * w, M = (long long)n * r;
  MMTTA_CHECK(M * ((V + 255) / 256) <= CC_MAX_BLOCKS, MMTTA_ERR_UNSUPPORTED,
              "fill_nest: %lld masks of %lld voxels in one call, at most 2^32 - 256 voxels (rounded up to 256 per mask): split the batch",
              M, V);
  MMTTA_CHECK(nest_mode == 0 || nest_mode == 1, MMTTA_ERR_INVALID, "fill_nest: nest_mode %d (0 clip, 1 grow)", nest_mode);
  MMTTA_CHECK(chain_len == 0 || (chain_len >= 2 && chain_len <= r), MMTTA_ERR_INVALID,
              "fill_nest: chain_len %d (0, or 2 ... %d distinct regions)", chain_len, r);
  MMTTA_CHECK(chain_len == 0 || chain != nullptr, MMTTA_ERR_INVALID, "fill_nest: null chain of length %d", chain_len);
  MMTTA_CHECK(label != nullptr || counts == nullptr, MMTTA_ERR_INVALID, "fill_nest: `counts` needs a `label` (label is NULL)");
  if (label != nullptr) {
    MMTTA_CHECK(label->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "mmtta_mask_fill_nest: `label` must be fp32-stored");
    MMTTA_CHECK(label->ptr != nullptr, MMTTA_ERR_INVALID, "fill_nest: null label data");
    MMTTA_CHECK(label->n == n && label->c == r && label->d == d && label->h == h && label->w == w, MMTTA_ERR_INVALID,
                "fill_nest: label shape differs from the mask's");
  }
  FhArgs a;
  a.fill = 0ull;
  for (int i = 0; i < CC_MAX_R; ++i) { a.cap[i] = 0ull; a.chain[i] = 0; }
  for (int i = 0; i < r; ++i) {
    MMTTA_CHECK(max_hole_voxels[i] >= 0, MMTTA_ERR_INVALID, "fill_nest: max_hole_voxels[%d] = %lld is negative", i,
                (long long)max_hole_voxels[i]);
    a.cap[i] = (unsigned long long)max_hole_voxels[i];
    if (fill_holes[i]) a.fill |= 1ull << i;
  }
  unsigned long long seen = 0ull;
  for (int i = 0; i < chain_len; ++i) {
    MMTTA_CHECK(chain[i] >= 0 && chain[i] < r, MMTTA_ERR_INVALID, "fill_nest: chain[%d] = %d is no region index (0 ... %d)", i,
                (int)chain[i], r - 1);
    MMTTA_CHECK(((seen >> chain[i]) & 1ull) == 0ull, MMTTA_ERR_INVALID, "fill_nest: chain[%d] = %d is repeated", i, (int)chain[i]);
    seen |= 1ull << chain[i];
    a.chain[i] = (unsigned char)chain[i];
  }
  hipStream_t s = (hipStream_t)stream;
  a.mask = mask;
  if (label != nullptr) a.lab = tv(label);
  else a.lab = TV{};
  a.N = n; a.R = r; a.D = d; a.H = h; a.W = w; a.V = V;
  a.tz = (d + CC_TZ - 1) / CC_TZ; a.ty = (h + CC_TY - 1) / CC_TY; a.tx = (w + CC_TX - 1) / CC_TX;
  a.tiles = (long long)a.tz * a.ty * a.tx;
  a.chain_len = chain_len; a.grow = nest_mode;
  a.maxn = fill_connectivity == 6 ? 1 : fill_connectivity == 18 ? 2 : 3;
  const size_t mv = (size_t)M * (size_t)V;
  char* base = (char*)scratch;
  const size_t head = fh_align((size_t)M * 4);
  unsigned int* ncomp = (unsigned int*)base;
  unsigned int* size = (unsigned int*)(base + head);
  a.size = size;
  a.open = (unsigned char*)(base + head + fh_align(mv * 4));
  a.L = (int*)(base + head + fh_align(mv * 4) + fh_align(mv));
  a.counts = counts != nullptr ? (unsigned long long*)counts : nullptr;
  a.stats = (unsigned long long*)stats;

  // what the labeller's merge and flatten passes read: geometry, maxn, the parent volume, sizes and the component counter
  CcArgs c;
  c.mask_in = mask; c.mask_out = nullptr; c.lab = TV{};
  c.M = (int)M; c.R = r; c.D = d; c.H = h; c.W = w; c.V = V; c.maxn = a.maxn;
  c.tz = a.tz; c.ty = a.ty; c.tx = a.tx; c.tiles = a.tiles;
  c.L = a.L; c.size = size; c.best = nullptr; c.ncomp = ncomp; c.nkept = nullptr;
  c.counts = nullptr; c.stats = nullptr; c.labels_out = nullptr;
  c.keep_largest = 0ull;
  for (int i = 0; i < CC_MAX_R; ++i) c.min_voxels[i] = 0ull;

  hipError_t e = hipMemsetAsync(base, 0, head + fh_align(mv * 4) + mv, s);      // header, sizes, open flags
  MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "fill_nest: memset failed: %s", hipGetErrorString(e));
  if (counts != nullptr) {
    e = hipMemsetAsync(counts, 0, (size_t)M * 3 * sizeof(int64_t), s);
    MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "fill_nest: memset failed: %s", hipGetErrorString(e));
  }
  e = hipMemsetAsync(stats, 0, (size_t)M * 4 * sizeof(int64_t), s);
  MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "fill_nest: memset failed: %s", hipGetErrorString(e));

  const long long tblocks = a.tiles < CC_MAX_BLOCKS / M ? a.tiles : CC_MAX_BLOCKS / M;      // >= 1; further tiles loop
  const dim3 vox((unsigned)((V + 255) / 256), (unsigned)M);
  if (g_uniform_tiles) hipLaunchKernelGGL(fh_tile_kernel<true>, dim3((unsigned)tblocks, (unsigned)M), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(fh_tile_kernel<false>, dim3((unsigned)tblocks, (unsigned)M), dim3(256), 0, s, a);
  int st = launch_status("fill_nest tile");
  if (st) return st;
  hipLaunchKernelGGL(cc_merge_kernel, vox, dim3(256), 0, s, c);
  st = launch_status("fill_nest merge");
  if (st) return st;
  hipLaunchKernelGGL(cc_flatten_kernel, vox, dim3(256), 0, s, c);
  st = launch_status("fill_nest flatten");
  if (st) return st;
  hipLaunchKernelGGL(fh_border_kernel, vox, dim3(256), 0, s, a);
  st = launch_status("fill_nest border");
  if (st) return st;
  hipLaunchKernelGGL(fh_finish_kernel, dim3((unsigned)((V + 255) / 256), (unsigned)n), dim3(256), 0, s, a);
  return launch_status("fill_nest finish");
}
