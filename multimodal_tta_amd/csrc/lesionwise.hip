// Lesion-wise scores of the evaluation tail (the BraTS-2023 scheme): every ground-truth lesion is scored on its own against
// the predicted components that touch it, every unmatched predicted component counts as a false positive.  Replaces two
// scipy.ndimage.label calls and a binary_dilation per (volume, region) over masks copied off the device.
//
//   K1 dilate   threshold the label (> 0.5) and dilate it `iterations` times with the 6 / 18 / 26 neighbourhood, all iterations
//               in LDS on a LW_TZ x LW_TY x LW_TX tile plus a halo of `iterations` voxels.  A row of the tile along x is one
//               64-bit word (a wave's ballot of label > 0.5), so an iteration is nine word reads, shifts and ORs per row, two
//               planes ping-pong.  Cells outside the volume are background in every iteration; a tile with no ground truth
//               within reach skips the iterations.  One byte per voxel goes out: bit 0 = in the dilated ground truth Gd,
//               bit 1 = in the ground truth G itself, so no later pass reads the label again.
//   K2 - K4     the labeller of components.hip (tile, merge, flatten) at connectivity 26 over Gd: lesions
//   K5 - K7     the same over the predicted mask P: predicted components, with their sizes
//   K8 pair     per voxel: own voxels and intersections per lesion (one atomic per distinct lesion of a wave), and the set
//               of distinct (predicted component, lesion) pairs: an open-addressing table of 64-bit keys per mask, linear
//               probing, atomicCAS insert, one insert per distinct pair of a wave.  The thread whose CAS finds the slot
//               empty adds the component's size to the lesion's |P_g| and marks the component matched.  Optional lesion
//               labels (1 + root of the Gd component on the voxels of G).
//   K9 finish   per lesion root: kept?, found?, q_g = round(2 inter / (|P_g| + |own|) * 2^30); per component root: matched or
//               false positive; wave popcounts / LDS atomics -> one integer atomic per block and column.
//
// Size of the pair table.  Two 26-adjacent voxels that both lie in P and in Gd belong to the same component and the same
// lesion, hence to the same pair; so one witness voxel per distinct pair gives a set of pairwise non-adjacent voxels, and
// a D x H x W box holds at most ceil(D/2) ceil(H/2) ceil(W/2) of those.  The table has the next power of two >= twice that
// many slots: it is never more than half full, so a probe always ends on the key or on an empty slot.
//
// The launch sequence depends on the shape alone; every sum is an integer and a root is the smallest index of its
// component, so the results do not depend on scheduling or on the order of the inserts.
#include "lesionwise.h"

namespace mmtta {

constexpr int LW_TZ = 8, LW_TY = 8, LW_TX = 32;
constexpr int LW_MAX_IT = 8;
constexpr int LW_ROWS = (LW_TZ + 2 * LW_MAX_IT) * (LW_TY + 2 * LW_MAX_IT);      // 576 words per plane
static_assert(LW_TX + 2 * LW_MAX_IT <= 64, "a row of the tile plus halo is one 64-bit word");

struct LwArgs {
  TV lab;
  const unsigned char* pred;      // [M][V]
  unsigned char* gd;              // [M][V] bit 0: Gd, bit 1: G
  int M, R, D, H, W, it, maxn;
  int tz, ty, tx;                 // dilation tiles per axis
  long long tiles, V;
  const int* LG;                  // [M][V] root of the Gd component, -1 background
  const int* LP;                  // [M][V] root of the predicted component, -1 background
  const unsigned int* sizeP;      // [M][V] voxels of a predicted component, at its root
  unsigned int* pg;               // [M][V] at a lesion root: voxels of the components matched to it
  unsigned int* own;              // [M][V] at a lesion root: voxels of G in it
  unsigned int* inter;            // [M][V] at a lesion root: voxels of G and P in it
  unsigned char* matched;         // [M][V] at a component root
  unsigned long long* table;      // [M][cap] pair keys, 0 = empty
  unsigned long long cap;         // slots per mask, a power of two >= 2
  int logcap;
  int* labels_out;                // [M][V] or nullptr
  unsigned long long* stats;      // [M][7]
  unsigned long long min_voxels[CC_MAX_R];
};

__global__ __launch_bounds__(256) void lw_dilate_kernel(LwArgs a) {
  __shared__ unsigned long long pl[3][LW_ROWS];      // G, ping, pong: one 64-bit word per (z, y) row of the tile plus halo
  const int m = blockIdx.y, n = m / a.R, r = m % a.R;
  const int it = a.it;
  const int ez = LW_TZ + 2 * it, ey = LW_TY + 2 * it, ex = LW_TX + 2 * it;      // ex <= 48: a row is one word, bit = local x
  const int rows = ez * ey;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* lp = a.lab.p + (long long)n * a.lab.sn + (long long)r * a.lab.sc;
  unsigned char* out = a.gd + (long long)m * a.V;
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    long long t = tile;
    const int x0 = (int)(t % a.tx) * LW_TX - it; t /= a.tx;
    const int y0 = (int)(t % a.ty) * LW_TY - it;
    const int z0 = (int)(t / a.ty) * LW_TZ - it;
    // bits of a row that lie in the volume (and in the halo): everything else stays background in every iteration
    const int lo = x0 < 0 ? -x0 : 0, hi = a.W - x0 < ex ? a.W - x0 : ex;
    const unsigned long long xmask = hi > lo ? (((1ull << (hi - lo)) - 1ull) << lo) : 0ull;
    bool any = false;
    for (int row = wave; row < rows; row += 4) {      // a wave reads a row of the label: one ballot is the row's word
      const int z = z0 + row / ey, y = y0 + row % ey, x = x0 + lane;
      const bool in = lane < ex && z >= 0 && z < a.D && y >= 0 && y < a.H && x >= 0 && x < a.W;
      const long long off = in ? (long long)z * a.lab.sd + (long long)y * a.lab.sh + (long long)x * a.lab.sw : 0;
      const unsigned long long bal = __ballot(in && lp[off] > 0.5f);
      if (lane == 0) { pl[0][row] = bal; pl[1][row] = bal; }
      any = any || bal != 0ull;
    }
    const int some = __syncthreads_or(any ? 1 : 0);      // no ground truth within reach of the tile: nothing to dilate
    if (some) {
      for (int k = 0; k < it; ++k) {
        const unsigned long long* src = pl[1 + (k & 1)];
        unsigned long long* dst = pl[1 + ((k + 1) & 1)];
        for (int row = threadIdx.x; row < rows; row += 256) {
          const int lz = row / ey, ly = row % ey;
          const int z = z0 + lz, y = y0 + ly;
          unsigned long long acc = 0ull;
#pragma unroll
          for (int j = 0; j < 9; ++j) {
            const int dz = j / 3 - 1, dy = j % 3 - 1;
            const int nd = (dz != 0) + (dy != 0);
            const int nz = lz + dz, ny = ly + dy;
            if (nd > a.maxn || nz < 0 || nz >= ez || ny < 0 || ny >= ey) continue;      // beyond the halo: cannot reach the core
            const unsigned long long w = src[nz * ey + ny];
            acc |= nd + 1 <= a.maxn ? (w | (w << 1) | (w >> 1)) : w;      // the x neighbours of that row, where the element has them
          }
          dst[row] = (z >= 0 && z < a.D && y >= 0 && y < a.H) ? (acc & xmask) : 0ull;
        }
        __syncthreads();
      }
    }
    const unsigned long long* fin = pl[some ? 1 + (it & 1) : 1];
    for (int i = threadIdx.x; i < LW_TZ * LW_TY * LW_TX; i += 256) {
      const int cz = i / (LW_TY * LW_TX), cy = (i / LW_TX) % LW_TY, cx = i % LW_TX;
      const int z = z0 + it + cz, y = y0 + it + cy, x = x0 + it + cx;
      const int row = (cz + it) * ey + cy + it, bit = cx + it;
      if (z < a.D && y < a.H && x < a.W)
        out[((long long)z * a.H + y) * a.W + x] = (unsigned char)(((fin[row] >> bit) & 1ull) | (((pl[0][row] >> bit) & 1ull) << 1));
    }
    __syncthreads();      // the planes are reused by the next round
  }
}

__global__ __launch_bounds__(256) void lw_pair_kernel(LwArgs a) {
  const int m = blockIdx.y;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool in = v < a.V;
  const long long at = (long long)m * a.V + (in ? v : 0);
  const unsigned int gd = in ? a.gd[at] : 0u;
  const int lg = (gd & 1u) ? a.LG[at] : -1;
  const int lp = in ? a.LP[at] : -1;
  const bool own = (gd & 2u) != 0u;
  if (in && a.labels_out != nullptr) a.labels_out[at] = own ? lg + 1 : 0;
  const int lane = threadIdx.x & 63;
  const long long mv = (long long)m * a.V;
  // own voxels and intersections: one atomic per distinct lesion of the wave (a wave covers a run of 64 voxels)
  unsigned long long todo = __ballot(own);
  while (todo != 0ull) {
    const int lead = __ffsll((long long)todo) - 1;
    const int lr = __shfl(lg, lead);
    const unsigned long long same = __ballot(own && lg == lr);
    const unsigned long long hit = __ballot(own && lg == lr && lp >= 0);
    if (lane == lead) {
      atomicAdd(a.own + mv + lr, (unsigned int)__popcll(same));
      if (hit != 0ull) atomicAdd(a.inter + mv + lr, (unsigned int)__popcll(hit));
    }
    todo &= ~same;
  }
  // distinct (component, lesion) pairs: one insert per distinct pair of the wave
  const bool pair = lp >= 0 && lg >= 0;
  todo = __ballot(pair);
  while (todo != 0ull) {
    const int lead = __ffsll((long long)todo) - 1;
    const int kp = __shfl(lp, lead), kg = __shfl(lg, lead);
    const unsigned long long same = __ballot(pair && lp == kp && lg == kg);
    if (lane == lead) {
      const unsigned long long key = ((unsigned long long)(unsigned int)(kp + 1) << 32) | (unsigned long long)(unsigned int)(kg + 1);
      unsigned long long* tab = a.table + (unsigned long long)m * a.cap;
      unsigned long long idx = (key * 0x9E3779B97F4A7C15ull) >> (64 - a.logcap);
      bool first = false;
      for (unsigned long long probe = 0; probe < a.cap; ++probe) {      // at most half full: ends on the key or an empty slot
        const unsigned long long old = atomicCAS(tab + idx, 0ull, key);
        if (old == 0ull) { first = true; break; }
        if (old == key) break;
        idx = (idx + 1) & (a.cap - 1);
      }
      if (first) {
        atomicAdd(a.pg + mv + kg, a.sizeP[mv + kp]);
        a.matched[mv + kp] = 1;
      }
    }
    todo &= ~same;
  }
}

__global__ __launch_bounds__(256) void lw_finish_kernel(LwArgs a) {
  __shared__ unsigned int s_cnt[5];             // lesions, kept, found, components, matched components
  __shared__ unsigned long long s_sum[2];       // dice_q, false-positive voxels
  const int m = blockIdx.y, r = m % a.R;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x < 5) s_cnt[threadIdx.x] = 0u;
  if (threadIdx.x < 2) s_sum[threadIdx.x] = 0ull;
  __syncthreads();
  const bool in = v < a.V;
  const long long at = (long long)m * a.V + (in ? v : 0);
  const bool isg = in && (a.gd[at] & 1u) && a.LG[at] == (int)v;
  const bool isp = in && a.LP[at] == (int)v;
  bool kept = false, found = false, hit = false;
  if (isg) {
    const unsigned long long own = a.own[at], pg = a.pg[at];
    kept = own >= a.min_voxels[r];
    found = kept && pg != 0ull;
    if (found) {
      const unsigned long long den = pg + own;      // >= 2
      const unsigned long long q = (((unsigned long long)a.inter[at] << 31) + den / 2) / den;      // 2 inter 2^30, rounded once
      if (q != 0ull) atomicAdd(&s_sum[0], q);
    }
  }
  if (isp) {
    hit = a.matched[at] != 0;
    if (!hit) atomicAdd(&s_sum[1], (unsigned long long)a.sizeP[at]);
  }
  const bool conds[5] = {isg, kept, found, isp, hit};
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const unsigned long long bal = __ballot(conds[k]);
    if ((threadIdx.x & 63) == 0 && bal != 0ull) atomicAdd(&s_cnt[k], (unsigned int)__popcll(bal));
  }
  __syncthreads();
  unsigned long long* st = a.stats + (long long)m * 7;
  if (threadIdx.x < 5 && s_cnt[threadIdx.x] != 0u) atomicAdd(st + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
  if (threadIdx.x >= 5 && threadIdx.x < 7 && s_sum[threadIdx.x - 5] != 0ull) atomicAdd(st + threadIdx.x, s_sum[threadIdx.x - 5]);
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int64_t mmtta_lesionwise_scratch_bytes(int64_t n_masks, int64_t d, int64_t h, int64_t w) {
  if (!lw_extent_ok(n_masks, d, h, w)) return -1;
  int logcap;
  const unsigned long long cap = lw_table_slots(d, h, w, logcap);
  return (int64_t)lw_layout(n_masks, d * h * w, cap).total;
}

extern "C" int mmtta_lesionwise_scores(const uint8_t* mask, const mmtta_tensor* label, int n, int r, int d, int h, int w,
                                       int iterations, int dilation_connectivity, const int64_t* min_lesion_voxels,
                                       int64_t* stats, int32_t* labels, void* scratch, void* stream) {
  MMTTA_CHECK(mask && label && min_lesion_voxels && stats && scratch, MMTTA_ERR_INVALID, "lesionwise: null argument");
  MMTTA_CHECK(iterations >= 0 && iterations <= LW_MAX_IT, MMTTA_ERR_INVALID, "lesionwise: iterations %d (0 ... %d)", iterations,
              LW_MAX_IT);
  MMTTA_CHECK(dilation_connectivity == 6 || dilation_connectivity == 18 || dilation_connectivity == 26, MMTTA_ERR_INVALID,
              "lesionwise: dilation connectivity %d (6, 18 or 26)", dilation_connectivity);
  MMTTA_CHECK(n >= 1 && r >= 1 && d >= 1 && h >= 1 && w >= 1, MMTTA_ERR_INVALID,
              "lesionwise: every extent must be >= 1, got %d %d %d %d %d", n, r, d, h, w);
  MMTTA_CHECK(r <= CC_MAX_R, MMTTA_ERR_UNSUPPORTED, "lesionwise: r = %d regions, at most %d", r, CC_MAX_R);
  MMTTA_CHECK((long long)n * r <= 65535, MMTTA_ERR_UNSUPPORTED, "lesionwise: more than 65535 masks per call");
  const long long dh = (long long)d * h;      // each factor below 2^31: no overflow before the checks
  MMTTA_CHECK(dh <= CC_MAX_V && dh * w <= CC_MAX_V, MMTTA_ERR_UNSUPPORTED,
              "lesionwise: d*h*w = %d*%d*%d voxels, at most 2^31 - 2", d, h, w);
  const long long V = dh * w, M = (long long)n * r;
  MMTTA_CHECK(M * ((V + 255) / 256) <= CC_MAX_BLOCKS, MMTTA_ERR_UNSUPPORTED,
              "lesionwise: %lld masks of %lld voxels in one call, at most 2^32 - 256 voxels (rounded up to 256 per mask): split the batch",
              M, V);
  MMTTA_CHECK(label->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "mmtta_lesionwise_scores: `label` must be fp32-stored");
  MMTTA_CHECK(label->ptr != nullptr, MMTTA_ERR_INVALID, "lesionwise: null label data");
  MMTTA_CHECK(label->n == n && label->c == r && label->d == d && label->h == h && label->w == w, MMTTA_ERR_INVALID,
              "lesionwise: label shape differs from the mask's");
  LwArgs a;
  for (int i = 0; i < CC_MAX_R; ++i) a.min_voxels[i] = 0ull;
  for (int i = 0; i < r; ++i) {
    MMTTA_CHECK(min_lesion_voxels[i] >= 0, MMTTA_ERR_INVALID, "lesionwise: min_lesion_voxels[%d] = %lld is negative", i,
                (long long)min_lesion_voxels[i]);
    a.min_voxels[i] = (unsigned long long)min_lesion_voxels[i];
  }
  hipStream_t s = (hipStream_t)stream;
  a.cap = lw_table_slots(d, h, w, a.logcap);
  const LwLayout l = lw_layout(M, V, a.cap);
  char* base = (char*)scratch;
  a.lab = tv(label);
  a.pred = mask;
  a.gd = (unsigned char*)(base + l.gd);
  a.M = (int)M; a.R = r; a.D = d; a.H = h; a.W = w; a.V = V;
  a.it = iterations;
  a.maxn = dilation_connectivity == 6 ? 1 : dilation_connectivity == 18 ? 2 : 3;
  a.tz = (d + LW_TZ - 1) / LW_TZ; a.ty = (h + LW_TY - 1) / LW_TY; a.tx = (w + LW_TX - 1) / LW_TX;
  a.tiles = (long long)a.tz * a.ty * a.tx;
  a.LG = (const int*)(base + l.LG);
  a.LP = (const int*)(base + l.LP);
  a.sizeP = (const unsigned int*)(base + l.sizeP);
  a.pg = (unsigned int*)(base + l.pg);
  a.own = (unsigned int*)(base + l.own);
  a.inter = (unsigned int*)(base + l.inter);
  a.matched = (unsigned char*)(base + l.matched);
  a.table = (unsigned long long*)(base + l.table);
  a.labels_out = labels;
  a.stats = (unsigned long long*)stats;

  // the labeller's arguments: connectivity 26, once over Gd (sizes into `pg`, zeroed again below) and once over P
  CcArgs c;
  c.mask_out = nullptr; c.lab = TV{};
  c.M = (int)M; c.R = r; c.D = d; c.H = h; c.W = w; c.V = V; c.maxn = 3;
  c.tz = (d + CC_TZ - 1) / CC_TZ; c.ty = (h + CC_TY - 1) / CC_TY; c.tx = (w + CC_TX - 1) / CC_TX;
  c.tiles = (long long)c.tz * c.ty * c.tx;
  c.best = (unsigned long long*)base;
  c.nkept = (unsigned int*)(base + (size_t)M * 8);
  c.counts = nullptr; c.stats = nullptr; c.labels_out = nullptr;
  c.keep_largest = 0ull;
  for (int i = 0; i < CC_MAX_R; ++i) c.min_voxels[i] = 0ull;

  hipError_t e = hipMemsetAsync(base, 0, l.zero_bytes, s);
  MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "lesionwise: memset failed: %s", hipGetErrorString(e));
  e = hipMemsetAsync(base + l.table, 0, (size_t)M * (size_t)a.cap * 8, s);
  MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "lesionwise: memset failed: %s", hipGetErrorString(e));
  e = hipMemsetAsync(stats, 0, (size_t)M * 7 * sizeof(int64_t), s);
  MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "lesionwise: memset failed: %s", hipGetErrorString(e));

  const long long dblocks = a.tiles < CC_MAX_BLOCKS / M ? a.tiles : CC_MAX_BLOCKS / M;      // >= 1; further tiles loop
  hipLaunchKernelGGL(lw_dilate_kernel, dim3((unsigned)dblocks, (unsigned)M), dim3(256), 0, s, a);
  int st = launch_status("lesionwise dilate");
  if (st) return st;
  c.mask_in = a.gd; c.L = (int*)(base + l.LG); c.size = a.pg; c.ncomp = (unsigned int*)(base + (size_t)M * 16);
  st = cc_label(c, s);
  if (st) return st;
  e = hipMemsetAsync(a.pg, 0, (size_t)M * (size_t)V * 4, s);      // held the sizes of the Gd components
  MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "lesionwise: memset failed: %s", hipGetErrorString(e));
  c.mask_in = mask; c.L = (int*)(base + l.LP); c.size = (unsigned int*)(base + l.sizeP); c.ncomp = (unsigned int*)(base + (size_t)M * 20);
  st = cc_label(c, s);
  if (st) return st;
  const dim3 vox((unsigned)((V + 255) / 256), (unsigned)M);
  hipLaunchKernelGGL(lw_pair_kernel, vox, dim3(256), 0, s, a);
  st = launch_status("lesionwise pair");
  if (st) return st;
  hipLaunchKernelGGL(lw_finish_kernel, vox, dim3(256), 0, s, a);
  return launch_status("lesionwise finish");
}
