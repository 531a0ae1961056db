// The float32 quantile of a list of non-negative distances, shared by the region surface pass (surface.hip) and the
// lesion-wise HD95 pass (lesionwise_hd95.hip): a radix select on the float bit patterns, 8 bits per round, then
// torch.quantile's linear interpolation.  The result does not depend on the order of the list.
#pragma once
#include "common.h"

namespace mmtta {

// Called by every thread of the workgroup (any size).  `hist`: 256 words of LDS, `sh`: 2 words of LDS.  n >= 1.
__device__ inline float surf_quantile(const float* list, unsigned int n, float q, unsigned int* hist, unsigned int* sh) {
  // torch.quantile(linear) in float32: rank = q * (n - 1); lerp(v[floor], v[ceil], rank - floor)
  const float rank = q * (float)(n - 1);
  const unsigned int lo = (unsigned int)rank;
  const float wgt = rank - (float)lo;
  const bool need_hi = ceilf(rank) != (float)lo;
  unsigned int prefix = 0, maskbits = 0, k = lo;
  for (int pass = 3; pass >= 0; --pass) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (unsigned int i = threadIdx.x; i < n; i += blockDim.x) {
      const unsigned int b = __float_as_uint(list[i]);
      if ((b & maskbits) == prefix) atomicAdd(&hist[(b >> (8 * pass)) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned int cum = 0, bsel = 255;
      for (unsigned int bkt = 0; bkt < 256; ++bkt) {
        if (cum + hist[bkt] > k) { bsel = bkt; break; }
        cum += hist[bkt];
      }
      sh[0] = bsel; sh[1] = k - cum;
    }
    __syncthreads();
    prefix |= sh[0] << (8 * pass);
    k = sh[1];
    maskbits |= 255u << (8 * pass);
    __syncthreads();
  }
  const float vlo = __uint_as_float(prefix);
  if (!need_hi) return vlo;
  // v[lo + 1]: vlo again when enough copies of it exist, else the smallest larger value
  if (threadIdx.x == 0) { sh[0] = 0; sh[1] = 0xffffffffu; }
  __syncthreads();
  unsigned int cle = 0, nmin = 0xffffffffu;
  for (unsigned int i = threadIdx.x; i < n; i += blockDim.x) {
    const unsigned int b = __float_as_uint(list[i]);
    if (b <= prefix) ++cle;
    else nmin = b < nmin ? b : nmin;
  }
  atomicAdd(&sh[0], cle);
  atomicMin(&sh[1], nmin);
  __syncthreads();
  const float vhi = (lo + 1 < sh[0]) ? vlo : __uint_as_float(sh[1]);
  __syncthreads();
  const float diff = vhi - vlo;
  return wgt < 0.5f ? fmaf(wgt, diff, vlo) : fmaf(wgt - 1.0f, diff, vhi);
}

}  // namespace mmtta
