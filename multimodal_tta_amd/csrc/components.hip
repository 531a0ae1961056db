// Connected-component filtering of the evaluation tail: 3-D labelling of every (volume, region) mask, component sizes,
// a size / largest-component filter and the Dice counts of the filtered mask, without a copy to the host.  No
// counterpart in the reference evaluator; published BraTS / HECKTOR pipelines do this with scipy.ndimage.label on a
// copied mask.
//
// Block-based union-find (Komura / Playne-Hawick form), labels = 0-based linear voxel index inside the own (n, r)
// volume, -1 = background, parent <= child always:
//   K1 tile     a CC_TZ x CC_TY x CC_TX tile is labelled in LDS (union by atomicMin on the root, then flatten) and written
//               to the int32 label volume as the GLOBAL index of the tile-local root.  Tile-local order and global order
//               agree (both lexicographic in z, y, x), so the local minimum is the global minimum of the tile's part.
//   K2 merge    every foreground voxel unites with its backward neighbours that sit in ANOTHER tile: find both roots,
//               atomicMin the smaller onto the larger root, retry with what the atomic returned.  Labels only decrease,
//               so every loop ends on its own thread's progress; no workgroup waits for another one.
//   K3 flatten  label[v] = root(v); size[root] += 1 (one atomic per distinct root of a wave); roots counted per block.
//   K4 select   per root: survives `min_voxels`?  kept count; with `keep_largest` one 64-bit atomicMax of
//               (size << 32) | ~label, so equal sizes go to the smaller label.
//   K5 final    filtered mask, optional labels (root + 1, 0 = background), inter / psum / gsum and removed voxels: wave
//               popcounts -> LDS -> one integer atomic per block and counter.
// Only the backward half of the neighbourhood is visited (3 / 9 / 13 neighbours for connectivity 6 / 18 / 26); neighbour
// tests are on (z, y, x), never on the linear index.  The launch sequence depends on the shape alone; all sums are integers
// and a root is the smallest index of its component, so results do not depend on scheduling.
// K1 - K3 are also the labeller of the lesion-wise scores (lesionwise.hip) through cc_label (components.h).
#include "components.h"

namespace mmtta {

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x: parents are strictly smaller than their children, so the walk ends
template <bool LDS>
__device__ __forceinline__ int cc_find(int* L, int x) {
  for (;;) {
    const int p = LDS ? ((volatile int*)L)[x] : cc_load(L + x);
    if (p == x) return x;
    x = p;
  }
}

// lock-free union: the larger root is hung under the smaller one; when the larger one stopped being a root in the
// meantime the atomic tells what it points to now, and that node is united instead (it is smaller: progress)
template <bool LDS>
__device__ __forceinline__ void cc_unite(int* L, int a, int b) {
  for (;;) {
    a = cc_find<LDS>(L, a);
    b = cc_find<LDS>(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(L + a, b);
    if (old == a) return;
    a = old;
  }
}

// backward neighbour j = 0..12 of the 3x3x3 block in scan order (13 is the centre)
__device__ __forceinline__ void cc_offset(int j, int& dz, int& dy, int& dx) {
  dz = j / 9 - 1; dy = (j / 3) % 3 - 1; dx = j % 3 - 1;
}
__device__ __forceinline__ int cc_iabs(int v) { return v < 0 ? -v : v; }

__global__ __launch_bounds__(256) void cc_tile_kernel(CcArgs a) {
  __shared__ int lab[CC_TILE];
  const int m = blockIdx.y;
  const unsigned char* pm = a.mask_in + (long long)m * a.V;
  int* L = a.L + (long long)m * a.V;
  // one tile per workgroup; only a volume one voxel thin along two axes has more tiles than a launch has workgroups
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
  long long t = tile;
  const int x0 = (int)(t % a.tx) * CC_TX; t /= a.tx;
  const int y0 = (int)(t % a.ty) * CC_TY;
  const int z0 = (int)(t / a.ty) * CC_TZ;
  for (int i = threadIdx.x; i < CC_TILE; i += 256) {
    const int z = z0 + i / (CC_TY * CC_TX), y = y0 + (i / CC_TX) % CC_TY, x = x0 + i % CC_TX;
    const bool in = z < a.D && y < a.H && x < a.W;
    const long long v = ((long long)(in ? z : 0) * a.H + (in ? y : 0)) * a.W + (in ? x : 0);
    lab[i] = (in && pm[v] != 0) ? i : -1;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CC_TILE; i += 256) {
    if (lab[i] < 0) continue;
    const int lz = i / (CC_TY * CC_TX), ly = (i / CC_TX) % CC_TY, lx = i % CC_TX;
#pragma unroll
    for (int j = 0; j < 13; ++j) {
      int dz, dy, dx;
      cc_offset(j, dz, dy, dx);
      if (cc_iabs(dz) + cc_iabs(dy) + cc_iabs(dx) > a.maxn) continue;
      const int nz = lz + dz, ny = ly + dy, nx = lx + dx;
      if (nz < 0 || ny < 0 || ny >= CC_TY || nx < 0 || nx >= CC_TX) continue;      // another tile: K2 (out of the volume: background)
      const int nb = (nz * CC_TY + ny) * CC_TX + nx;
      if (((volatile int*)lab)[nb] >= 0) cc_unite<true>(lab, i, nb);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CC_TILE; i += 256) {
    const int z = z0 + i / (CC_TY * CC_TX), y = y0 + (i / CC_TX) % CC_TY, x = x0 + i % CC_TX;
    if (!(z < a.D && y < a.H && x < a.W)) continue;
    int g = -1;
    if (lab[i] >= 0) {
      const int r = cc_find<true>(lab, i);
      const int rz = z0 + r / (CC_TY * CC_TX), ry = y0 + (r / CC_TX) % CC_TY, rx = x0 + r % CC_TX;
      g = (int)(((long long)rz * a.H + ry) * a.W + rx);
    }
    L[((long long)z * a.H + y) * a.W + x] = g;
  }
  __syncthreads();      // the LDS tile is reused by the next round
  }
}

__global__ __launch_bounds__(256) void cc_merge_kernel(CcArgs a) {
  const int m = blockIdx.y;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= a.V) return;
  int* L = a.L + (long long)m * a.V;
  if (cc_load(L + v) < 0) return;
  long long t = v;
  const int x = (int)(t % a.W); t /= a.W;
  const int y = (int)(t % a.H);
  const int z = (int)(t / a.H);
#pragma unroll
  for (int j = 0; j < 13; ++j) {
    int dz, dy, dx;
    cc_offset(j, dz, dy, dx);
    if (cc_iabs(dz) + cc_iabs(dy) + cc_iabs(dx) > a.maxn) continue;
    const int nz = z + dz, ny = y + dy, nx = x + dx;
    if (nz < 0 || ny < 0 || ny >= a.H || nx < 0 || nx >= a.W) continue;
    if (nz / CC_TZ == z / CC_TZ && ny / CC_TY == y / CC_TY && nx / CC_TX == x / CC_TX) continue;      // same tile: done in K1
    const long long nb = ((long long)nz * a.H + ny) * a.W + nx;
    if (cc_load(L + nb) >= 0) cc_unite<false>(L, (int)v, (int)nb);
  }
}

__global__ __launch_bounds__(256) void cc_flatten_kernel(CcArgs a) {
  __shared__ unsigned int s_roots;
  const int m = blockIdx.y;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x == 0) s_roots = 0u;
  __syncthreads();
  int* L = a.L + (long long)m * a.V;
  const bool fg = v < a.V && cc_load(L + (v < a.V ? v : 0)) >= 0;
  int root = -1;
  if (fg) {
    root = cc_find<false>(L, (int)v);
    L[v] = root;               // a concurrent find reads the old parent or the root: both are ancestors
  }
  // one size atomic per distinct root of the wave (a wave covers a run of 64 voxels: few roots)
  const int lane = threadIdx.x & 63;
  unsigned int* sz = a.size + (long long)m * a.V;
  unsigned long long todo = __ballot(fg);
  while (todo != 0ull) {
    const int lead = __ffsll((long long)todo) - 1;
    const int lr = __shfl(root, lead);
    const unsigned long long same = __ballot(fg && root == lr);
    if (lane == lead) atomicAdd(sz + lr, (unsigned int)__popcll(same));
    todo &= ~same;
  }
  const unsigned long long isroot = __ballot(fg && root == (int)v);
  if (lane == 0 && isroot != 0ull) atomicAdd(&s_roots, (unsigned int)__popcll(isroot));
  __syncthreads();
  if (threadIdx.x == 0 && s_roots != 0u) atomicAdd(a.ncomp + m, s_roots);
}

__global__ __launch_bounds__(256) void cc_select_kernel(CcArgs a) {
  __shared__ unsigned int s_kept;
  const int m = blockIdx.y, r = m % a.R;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x == 0) s_kept = 0u;
  __syncthreads();
  const long long vc = v < a.V ? v : 0;
  const bool isroot = v < a.V && a.L[(long long)m * a.V + vc] == (int)v;
  const unsigned int s = a.size[(long long)m * a.V + vc];
  const bool ok = isroot && (unsigned long long)s >= a.min_voxels[r];
  if (ok && ((a.keep_largest >> r) & 1ull))
    atomicMax(a.best + m, ((unsigned long long)s << 32) | (unsigned long long)(~(unsigned int)(v + 1)));
  const unsigned long long bal = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && bal != 0ull) atomicAdd(&s_kept, (unsigned int)__popcll(bal));
  __syncthreads();
  if (threadIdx.x == 0 && s_kept != 0u) atomicAdd(a.nkept + m, s_kept);
}

__global__ __launch_bounds__(256) void cc_final_kernel(CcArgs a) {
  __shared__ unsigned int s_cnt[4];      // inter, psum, gsum, removed
  const int m = blockIdx.y, r = m % a.R, n = m / a.R;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  const bool in = v < a.V;
  const long long vc = in ? v : 0;
  const int root = in ? a.L[(long long)m * a.V + vc] : -1;
  const bool fg = root >= 0;
  const bool largest = ((a.keep_largest >> r) & 1ull) != 0ull;
  const unsigned long long best = a.best[m];
  bool keep = fg && (unsigned long long)a.size[(long long)m * a.V + (fg ? root : 0)] >= a.min_voxels[r];
  if (largest) keep = keep && best != 0ull && (unsigned int)(root + 1) == ~(unsigned int)(best & 0xffffffffull);
  bool g = false;
  if (a.counts != nullptr && in) {
    long long t = v;
    const int x = (int)(t % a.W); t /= a.W;
    const int y = (int)(t % a.H);
    const int z = (int)(t / a.H);
    g = a.lab.p[(long long)n * a.lab.sn + (long long)r * a.lab.sc + (long long)z * a.lab.sd + (long long)y * a.lab.sh +
                (long long)x * a.lab.sw] > 0.5f;
  }
  if (in) {
    a.mask_out[(long long)m * a.V + v] = (unsigned char)(keep ? 1 : 0);
    if (a.labels_out != nullptr) a.labels_out[(long long)m * a.V + v] = fg ? root + 1 : 0;
  }
  const bool conds[4] = {keep && g, keep, g, fg && !keep};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long bal = __ballot(conds[k]);
    if ((threadIdx.x & 63) == 0 && bal != 0ull) atomicAdd(&s_cnt[k], (unsigned int)__popcll(bal));
  }
  __syncthreads();
  if (threadIdx.x < 3 && a.counts != nullptr && s_cnt[threadIdx.x] != 0u)
    atomicAdd(a.counts + (long long)m * 3 + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
  if (threadIdx.x == 3 && a.stats != nullptr && s_cnt[3] != 0u) atomicAdd(a.stats + (long long)m * 3 + 2, (unsigned long long)s_cnt[3]);
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.stats != nullptr) {      // slots 0 and 1 have one writer; slot 2 is summed above
    a.stats[(long long)m * 3 + 0] = a.ncomp[m];
    a.stats[(long long)m * 3 + 1] = largest ? (best != 0ull ? 1ull : 0ull) : (unsigned long long)a.nkept[m];
  }
}

// K1 - K3 on `s`: a.L holds the root of every foreground voxel (-1 background), a.size the voxels of a component at its root
// (added to what is there: the caller zeroes it), a.ncomp the components per mask (likewise).  Reads a.mask_in, the geometry
// and a.maxn; shared with lesionwise.hip.
int cc_label(const CcArgs& a, hipStream_t s) {
  const long long M = a.M;
  const long long tblocks = a.tiles < CC_MAX_BLOCKS / M ? a.tiles : CC_MAX_BLOCKS / M;      // >= 1: M <= 65535; further tiles loop
  const dim3 vox((unsigned)((a.V + 255) / 256), (unsigned)M);
  hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)tblocks, (unsigned)M), dim3(256), 0, s, a);
  int st = launch_status("components tile");
  if (st) return st;
  hipLaunchKernelGGL(cc_merge_kernel, vox, dim3(256), 0, s, a);
  st = launch_status("components merge");
  if (st) return st;
  hipLaunchKernelGGL(cc_flatten_kernel, vox, dim3(256), 0, s, a);
  return launch_status("components flatten");
}

static size_t cc_align(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace mmtta

using namespace mmtta;

extern "C" int64_t mmtta_components_scratch_bytes(int64_t n_masks, int64_t d, int64_t h, int64_t w) {
  if (n_masks < 1 || n_masks > 65535 || d < 1 || h < 1 || w < 1) return -1;
  if (d > CC_MAX_V || h > CC_MAX_V || w > CC_MAX_V || d * h > CC_MAX_V || d * h * w > CC_MAX_V) return -1;
  if (n_masks * ((d * h * w + 255) / 256) > CC_MAX_BLOCKS) return -1;
  const size_t mv = (size_t)n_masks * (size_t)(d * h * w);
  return (int64_t)(cc_align((size_t)n_masks * 16) + cc_align(mv * 4) + cc_align(mv * 4));
}

extern "C" int mmtta_components_filter(const uint8_t* mask_in, uint8_t* mask_out, const mmtta_tensor* label, int n, int r, int d,
                                       int h, int w, int connectivity, const int64_t* min_voxels, const int32_t* keep_largest,
                                       int64_t* counts, int64_t* stats, int32_t* labels, void* scratch, void* stream) {
  MMTTA_CHECK(mask_in && mask_out && min_voxels && keep_largest && scratch, MMTTA_ERR_INVALID, "components: null argument");
  MMTTA_CHECK(connectivity == 6 || connectivity == 18 || connectivity == 26, MMTTA_ERR_INVALID,
              "components: connectivity %d (6, 18 or 26)", connectivity);
  MMTTA_CHECK(n >= 1 && r >= 1 && d >= 1 && h >= 1 && w >= 1, MMTTA_ERR_INVALID, "components: every extent must be >= 1, got %d %d %d %d %d",
              n, r, d, h, w);
  MMTTA_CHECK(r <= CC_MAX_R, MMTTA_ERR_UNSUPPORTED, "components: r = %d regions, at most %d", r, CC_MAX_R);
  MMTTA_CHECK((long long)n * r <= 65535, MMTTA_ERR_UNSUPPORTED, "components: more than 65535 masks per call");
  const long long dh = (long long)d * h;      // each factor below 2^31: no overflow before the checks
  MMTTA_CHECK(dh <= CC_MAX_V && dh * w <= CC_MAX_V, MMTTA_ERR_UNSUPPORTED,
              "components: d*h*w = %d*%d*%d voxels, at most 2^31 - 2", d, h, w);
  const long long V = dh * w;
  MMTTA_CHECK(label != nullptr || counts == nullptr, MMTTA_ERR_INVALID, "components: `counts` needs a `label` (label is NULL)");
  if (label != nullptr) {
    MMTTA_CHECK(label->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "mmtta_components_filter: `label` must be fp32-stored");
    MMTTA_CHECK(label->ptr != nullptr, MMTTA_ERR_INVALID, "components: null label data");
    MMTTA_CHECK(label->n == n && label->c == r && label->d == d && label->h == h && label->w == w, MMTTA_ERR_INVALID,
                "components: label shape differs from the mask's");
  }
  CcArgs a;
  a.keep_largest = 0ull;
  for (int i = 0; i < CC_MAX_R; ++i) a.min_voxels[i] = 0ull;
  for (int i = 0; i < r; ++i) {
    MMTTA_CHECK(min_voxels[i] >= 0, MMTTA_ERR_INVALID, "components: min_voxels[%d] = %lld is negative", i, (long long)min_voxels[i]);
    a.min_voxels[i] = (unsigned long long)min_voxels[i];
    if (keep_largest[i]) a.keep_largest |= 1ull << i;
  }
  hipStream_t s = (hipStream_t)stream;
  const long long M = (long long)n * r;
  a.mask_in = mask_in; a.mask_out = mask_out;
  if (label != nullptr) a.lab = tv(label);
  else a.lab = TV{};
  a.M = (int)M; a.R = r; a.D = d; a.H = h; a.W = w; a.V = V;
  a.maxn = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3;
  a.tz = (d + CC_TZ - 1) / CC_TZ; a.ty = (h + CC_TY - 1) / CC_TY; a.tx = (w + CC_TX - 1) / CC_TX;
  const long long tiles = (long long)a.tz * a.ty * a.tx;
  a.tiles = tiles;
  const long long vblocks = (V + 255) / 256;
  MMTTA_CHECK(M * vblocks <= CC_MAX_BLOCKS, MMTTA_ERR_UNSUPPORTED,
              "components: %lld masks of %lld voxels in one call, at most 2^32 - 256 voxels (rounded up to 256 per mask): split the batch",
              M, V);
  const size_t mv = (size_t)M * (size_t)V;
  char* base = (char*)scratch;
  const size_t head = cc_align((size_t)M * 16);
  a.best = (unsigned long long*)base;
  a.ncomp = (unsigned int*)(base + (size_t)M * 8);
  a.nkept = (unsigned int*)(base + (size_t)M * 12);
  a.size = (unsigned int*)(base + head);
  a.L = (int*)(base + head + cc_align(mv * 4));
  a.counts = (unsigned long long*)counts;
  a.stats = (unsigned long long*)stats;
  a.labels_out = labels;
  hipError_t e = hipMemsetAsync(base, 0, head + mv * 4, s);      // per-mask header and the sizes
  MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "components: memset failed: %s", hipGetErrorString(e));
  if (counts != nullptr) {
    e = hipMemsetAsync(counts, 0, (size_t)M * 3 * sizeof(int64_t), s);
    MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "components: memset failed: %s", hipGetErrorString(e));
  }
  if (stats != nullptr) {
    e = hipMemsetAsync(stats, 0, (size_t)M * 3 * sizeof(int64_t), s);
    MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "components: memset failed: %s", hipGetErrorString(e));
  }
  const dim3 vox((unsigned)((V + 255) / 256), (unsigned)M);
  int st = cc_label(a, s);
  if (st) return st;
  hipLaunchKernelGGL(cc_select_kernel, vox, dim3(256), 0, s, a);
  st = launch_status("components select");
  if (st) return st;
  hipLaunchKernelGGL(cc_final_kernel, vox, dim3(256), 0, s, a);
  return launch_status("components final");
}
