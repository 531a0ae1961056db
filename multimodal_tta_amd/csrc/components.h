// What the component filter (components.hip), the lesion-wise scores (lesionwise.hip) and the hole filling (fill_holes.hip) share: the launch arguments of the
// block-based union-find labeller and its host entry.  The kernels themselves live in components.hip.
#pragma once
#include "common.h"

namespace mmtta {

constexpr int CC_TZ = 4, CC_TY = 8, CC_TX = 32;
constexpr int CC_TILE = CC_TZ * CC_TY * CC_TX;      // 1024 voxels, 4 per thread, 4 KB of LDS
constexpr int CC_MAX_R = 64;
constexpr long long CC_MAX_V = 2147483646ll;        // label = index + 1 stays an int32
constexpr long long CC_MAX_BLOCKS = 16777215ll;     // workgroups of 256 threads in one launch: fewer than 2^32 threads

struct CcArgs {
  const unsigned char* mask_in;   // [M][V]
  unsigned char* mask_out;        // [M][V] or the same buffer (read in K1 only, written in K5 only)
  TV lab;                         // ground truth, used when counts != nullptr
  int M, R, D, H, W, maxn;        // maxn: largest |dz| + |dy| + |dx| of a neighbour (1, 2, 3)
  int tz, ty, tx;                 // tiles per axis
  long long tiles;                // tz * ty * tx
  long long V;
  int* L;                         // [M][V] parent / label, 0-based, -1 background
  unsigned int* size;             // [M][V] voxels of the component, at its root
  unsigned long long* best;       // [M] (size << 32) | ~label of the largest surviving component, 0 = none
  unsigned int* ncomp;            // [M]
  unsigned int* nkept;            // [M]
  unsigned long long* counts;     // [M][3] or nullptr
  unsigned long long* stats;      // [M][3] or nullptr
  int* labels_out;                // [M][V] or nullptr
  unsigned long long keep_largest;          // bit r
  unsigned long long min_voxels[CC_MAX_R];  // per region
};

// components.hip: labelling passes K1 - K3 (tile, merge, flatten) queued on `s`
int cc_label(const CcArgs& a, hipStream_t s);

// components.hip: K2 and K3 on their own, for a caller that brings its own tile pass (fill_holes.hip labels the complement of
// a mask).  One thread per voxel, grid ((V + 255) / 256, M); they read L, size, ncomp, the geometry and maxn.
__global__ __launch_bounds__(256) void cc_merge_kernel(CcArgs a);
__global__ __launch_bounds__(256) void cc_flatten_kernel(CcArgs a);

}  // namespace mmtta
