// The do-no-harm guard on gfx950: compare the hard prediction of the adapted model with the one taken before the first step,
// per (item, region), and put the earlier logits back where the adapted mask collapsed or exploded.  Two launches:
//   guard_counts   one streaming pass over both logit tensors -> int64 (s, a, i) = |reference mask|, |adapted mask|, |both|
//   guard_select   every workgroup evaluates the integer rule on its item's counts; a failing item's workgroups copy the
//                  reference rows over the logits in place, a passing item's exit at once
// The hard prediction is the evaluator's (dice_counts_kernel): 1 / (1 + expf(-z)) >= threshold in fp32.
// See include/mmtta.h for the contract.
#include "common.h"

namespace mmtta {

constexpr int GUARD_MAX_R = 16;            // regions of the generic route
constexpr int GUARD_MAX_GRID_Y = 65535;    // gridDim.y carries the item
constexpr int GUARD_VOX = 8;               // voxels per thread: a workgroup covers 2048 consecutive voxels of one item
constexpr int GUARD_CHUNK = 256 * GUARD_VOX;
constexpr unsigned long long GUARD_Q = 1ull << 16;

__device__ __forceinline__ bool guard_hard(float z, float thr) { return 1.f / (1.f + expf(-z)) >= thr; }

// ------------------------------------------------------------------ counts
// DENSE: 16-byte voxel rows (R <= 4) addressed by the voxel index, one 16-byte load per voxel and tensor.  Otherwise any
// channels-last rows of R <= 16 elements.  A wave reduces each of the three bits of a (voxel, region) with a ballot and a
// population count into wave-uniform counters; the four waves meet in 3 R LDS words and 3 R threads add them to `counts`.
template <int RMAX, bool DENSE>
__global__ __launch_bounds__(256) void guard_counts_kernel(TV ref, TV ada, float thr, unsigned long long* counts) {
  __shared__ unsigned int sh[4][3 * RMAX];
  const int R = ref.c;
  const unsigned total = (unsigned)ref.d * ref.h * ref.w;      // < 2^31: checked on the host
  const float* rp = ref.p + (long long)blockIdx.y * ref.sn;
  const float* ap = ada.p + (long long)blockIdx.y * ada.sn;
  unsigned int cs[RMAX], ca[RMAX], ci[RMAX];
#pragma unroll
  for (int r = 0; r < RMAX; ++r) cs[r] = ca[r] = ci[r] = 0u;
  const unsigned base = blockIdx.x * (unsigned)GUARD_CHUNK + threadIdx.x;
#pragma unroll 2
  for (int k = 0; k < GUARD_VOX; ++k) {
    const unsigned v = base + (unsigned)k * 256u;
    const bool in = v < total;
    float zr[RMAX], za[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) zr[r] = za[r] = -INFINITY;      // (outside the volume: no bit)
    if (in) {
      if (DENSE) {
        const float4 q = *reinterpret_cast<const float4*>(rp + (size_t)v * 4u);
        const float4 p = *reinterpret_cast<const float4*>(ap + (size_t)v * 4u);
        zr[0] = q.x; za[0] = p.x;
        if (RMAX > 1) { zr[1] = q.y; za[1] = p.y; }
        if (RMAX > 2) { zr[2] = q.z; za[2] = p.z; }
        if (RMAX > 3) { zr[3] = q.w; za[3] = p.w; }
      } else {
        const int x = (int)(v % (unsigned)ref.w), rr = (int)(v / (unsigned)ref.w);
        const int y = rr % ref.h, z = rr / ref.h;
        const float* rv = rp + z * ref.sd + y * ref.sh + x * ref.sw;
        const float* av = ap + z * ada.sd + y * ada.sh + x * ada.sw;
#pragma unroll
        for (int r = 0; r < RMAX; ++r)
          if (r < R) {
            zr[r] = rv[r];
            za[r] = av[r];
          }
      }
    }
#pragma unroll
    for (int r = 0; r < RMAX; ++r)
      if (r < R) {      // (wave-uniform: every lane takes part in the ballots)
        const bool s = in && guard_hard(zr[r], thr), a = in && guard_hard(za[r], thr);
        cs[r] += (unsigned)__popcll(__ballot(s));
        ca[r] += (unsigned)__popcll(__ballot(a));
        ci[r] += (unsigned)__popcll(__ballot(s && a));
      }
  }
  if ((threadIdx.x & 63) == 0) {
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      sh[wv][r * 3 + 0] = cs[r];
      sh[wv][r * 3 + 1] = ca[r];
      sh[wv][r * 3 + 2] = ci[r];
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < 3 * R) {
    // integer sums and ONE integer atomic per workgroup and count: the result is the same in every run
    const unsigned int t = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
    if (t > 0u) atomicAdd(counts + (size_t)blockIdx.y * (3 * R) + threadIdx.x, (unsigned long long)t);
  }
}

// ------------------------------------------------------------------ select
struct GuardRule {
  unsigned long long A, G, H, m;      // round(min_agreement Q), round(max_growth Q), round(max_shrink Q), min_voxels
  int region;                         // scope: 0 the whole volume returns, 1 only the failing channels
};

// the rule of include/mmtta.h on one region's counts, in unsigned 64-bit arithmetic (no product reaches 2^58)
__device__ __forceinline__ bool guard_fails(unsigned long long s, unsigned long long a, unsigned long long i, const GuardRule& g) {
  const unsigned long long big = s > a ? s : a, m1 = g.m > 1ull ? g.m : 1ull;
  const bool agree = g.A > 0ull && big >= m1 && 2ull * i * GUARD_Q < g.A * (s + a);
  const bool grew = g.G > 0ull && a * GUARD_Q > g.G * (s > g.m ? s : g.m);
  const bool shrank = g.H > 0ull && s * GUARD_Q > g.H * (a > g.m ? a : g.m);
  return agree || grew || shrank;
}

// FULL: failing rows are one 16-byte load and store (scope volume on dense rows whose pad lanes the view owns, or R == 4).
template <bool DENSE, bool FULL>
__global__ __launch_bounds__(256) void guard_select_kernel(const long long* counts, GuardRule g, TV ref, TV lg, int* fallback) {
  const int R = ref.c;
  const long long* c = counts + (size_t)blockIdx.y * (3 * R);
  unsigned fail = 0u;
  for (int r = 0; r < R; ++r)      // (uniform: every workgroup of the item decides for itself, from 3 R counts in L2)
    if (guard_fails((unsigned long long)c[r * 3], (unsigned long long)c[r * 3 + 1], (unsigned long long)c[r * 3 + 2], g))
      fail |= 1u << r;
  if (!g.region && fail != 0u) fail = (1u << R) - 1u;
  if (blockIdx.x == 0 && (int)threadIdx.x < R) fallback[(size_t)blockIdx.y * R + threadIdx.x] = (int)((fail >> threadIdx.x) & 1u);
  if (fail == 0u) return;      // a passing item: its logits are not touched
  const unsigned total = (unsigned)ref.d * ref.h * ref.w;
  const float* rp = ref.p + (long long)blockIdx.y * ref.sn;
  float* lp = lg.p + (long long)blockIdx.y * lg.sn;
  const unsigned base = blockIdx.x * (unsigned)GUARD_CHUNK + threadIdx.x;
#pragma unroll 2
  for (int k = 0; k < GUARD_VOX; ++k) {
    const unsigned v = base + (unsigned)k * 256u;
    if (v >= total) break;
    if (DENSE) {
      const float4 q = *reinterpret_cast<const float4*>(rp + (size_t)v * 4u);
      float* o = lp + (size_t)v * 4u;
      if (FULL) {
        *reinterpret_cast<float4*>(o) = q;      // the pad lanes take the reference's
      } else {      // pad lanes and passing channels are left as they are
        if (fail & 1u) o[0] = q.x;
        if (fail & 2u) o[1] = q.y;
        if (fail & 4u) o[2] = q.z;
        if (fail & 8u) o[3] = q.w;
      }
    } else {
      const int x = (int)(v % (unsigned)ref.w), rr = (int)(v / (unsigned)ref.w);
      const int y = rr % ref.h, z = rr / ref.h;
      const float* rv = rp + z * ref.sd + y * ref.sh + x * ref.sw;
      float* o = lp + z * lg.sd + y * lg.sh + x * lg.sw;
      for (int r = 0; r < R; ++r)
        if ((fail >> r) & 1u) o[r] = rv[r];
    }
  }
}

// 16-byte voxel rows with nothing between them: what the dense kernels address with the voxel index
static bool guard_dense4(const mmtta_tensor* t) {
  return t->sc == 1 && t->sw == 4 && t->sh == (int64_t)t->w * 4 && t->sd == (int64_t)t->h * t->sh && t->sn % 4 == 0 &&
         ((uintptr_t)t->ptr) % 16 == 0;
}

static bool guard_overlap(const mmtta_tensor* a, const mmtta_tensor* b) {
  auto span = [](const mmtta_tensor* t, uintptr_t& lo, uintptr_t& hi) {
    const long long last = (long long)(t->n - 1) * t->sn + (long long)(t->d - 1) * t->sd + (long long)(t->h - 1) * t->sh +
                           (long long)(t->w - 1) * t->sw + t->c;
    lo = (uintptr_t)t->ptr;
    hi = lo + (uintptr_t)(last * 4);
  };
  uintptr_t alo, ahi, blo, bhi;
  span(a, alo, ahi);
  span(b, blo, bhi);
  return !(ahi <= blo || bhi <= alo);
}

// what both entries ask of their two logit tensors; `what` names the entry, `na` / `nb` the operands
static int guard_check_pair(const char* what, const mmtta_tensor* a, const char* na, const mmtta_tensor* b, const char* nb) {
  MMTTA_CHECK(a && a->ptr, MMTTA_ERR_INVALID, "%s: null `%s`", what, na);
  MMTTA_CHECK(b && b->ptr, MMTTA_ERR_INVALID, "%s: null `%s`", what, nb);
  MMTTA_CHECK(a->n >= 1 && a->c >= 1 && a->d >= 1 && a->h >= 1 && a->w >= 1, MMTTA_ERR_INVALID, "%s: empty `%s`", what, na);
  MMTTA_CHECK(same_shape(a, b), MMTTA_ERR_INVALID, "%s: shape mismatch between `%s` and `%s`", what, na, nb);
  MMTTA_CHECK(a->sw == b->sw, MMTTA_ERR_INVALID, "%s: row width mismatch between `%s` and `%s`", what, na, nb);
  MMTTA_CHECK(a->c <= GUARD_MAX_R, MMTTA_ERR_UNSUPPORTED, "%s: more than %d regions", what, GUARD_MAX_R);
  MMTTA_CHECK(is_f32(a) && is_f32(b), MMTTA_ERR_UNSUPPORTED, "%s: `%s` and `%s` must be fp32-stored", what, na, nb);
  auto cl = [](const mmtta_tensor* t) { return t->sc == 1 && t->sw >= t->c && t->sh >= 0 && t->sd >= 0 && t->sn >= 0; };
  MMTTA_CHECK(cl(a) && cl(b), MMTTA_ERR_UNSUPPORTED, "%s: channels-last only", what);
  MMTTA_CHECK((long long)a->d * a->h * a->w < (1ll << 31), MMTTA_ERR_UNSUPPORTED, "%s: an item of 2^31 voxels or more", what);
  MMTTA_CHECK(a->n <= GUARD_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "%s: more than %d items in one call", what, GUARD_MAX_GRID_Y);
  return MMTTA_OK;
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int mmtta_guard_counts(const mmtta_tensor* reference, const mmtta_tensor* adapted, float threshold, int64_t* counts,
                                  void* stream) {
  const int st = guard_check_pair("guard counts", reference, "reference", adapted, "adapted");
  if (st) return st;
  MMTTA_CHECK(counts != nullptr, MMTTA_ERR_INVALID, "guard counts: null `counts`");
  MMTTA_CHECK(__builtin_isfinite(threshold) && threshold > 0.f && threshold < 1.f, MMTTA_ERR_INVALID,
              "guard counts: threshold must be finite and in (0, 1), got %g", (double)threshold);
  hipStream_t s = (hipStream_t)stream;
  const int items = reference->n, R = reference->c;
  const long long vox = (long long)reference->d * reference->h * reference->w;
  const dim3 grid((unsigned)((vox + GUARD_CHUNK - 1) / GUARD_CHUNK), items);
  if (hipMemsetAsync(counts, 0, sizeof(int64_t) * 3 * (size_t)R * (size_t)items, s) != hipSuccess)
    return launch_status("guard counts clear");
  unsigned long long* cnt = (unsigned long long*)counts;
  if (R <= 4 && guard_dense4(reference) && guard_dense4(adapted)) {
#define GUARD_COUNTS(RM) hipLaunchKernelGGL((guard_counts_kernel<RM, true>), grid, dim3(256), 0, s, tv(reference), tv(adapted), threshold, cnt)
    if (R == 1) GUARD_COUNTS(1);
    else if (R == 2) GUARD_COUNTS(2);
    else if (R == 3) GUARD_COUNTS(3);
    else GUARD_COUNTS(4);
#undef GUARD_COUNTS
  } else {
    hipLaunchKernelGGL((guard_counts_kernel<GUARD_MAX_R, false>), grid, dim3(256), 0, s, tv(reference), tv(adapted), threshold, cnt);
  }
  return launch_status("guard counts");
}

extern "C" int mmtta_guard_select(const int64_t* counts, const mmtta_guard_rule* rule, const mmtta_tensor* reference,
                                  const mmtta_tensor* logits, int32_t* fallback, void* stream) {
  const int st = guard_check_pair("guard select", reference, "reference", logits, "logits");
  if (st) return st;
  MMTTA_CHECK(counts != nullptr, MMTTA_ERR_INVALID, "guard select: null `counts`");
  MMTTA_CHECK(rule != nullptr, MMTTA_ERR_INVALID, "guard select: null `rule`");
  MMTTA_CHECK(fallback != nullptr, MMTTA_ERR_INVALID, "guard select: null `fallback`");
  MMTTA_CHECK(rule->min_agreement_q16 <= (1u << 16), MMTTA_ERR_INVALID,
              "guard select: min_agreement_q16 must be 0 .. 65536, got %u", rule->min_agreement_q16);
  for (int k = 0; k < 2; ++k) {
    const uint32_t v = k == 0 ? rule->max_growth_q16 : rule->max_shrink_q16;
    MMTTA_CHECK(v == 0u || (v >= (1u << 16) && v <= (1024u << 16)), MMTTA_ERR_INVALID,
                "guard select: %s must be 0 (off) or 65536 .. 1024 * 65536, got %u", k == 0 ? "max_growth_q16" : "max_shrink_q16", v);
  }
  MMTTA_CHECK(rule->min_voxels >= 0, MMTTA_ERR_INVALID, "guard select: min_voxels must be 0 .. 2^31 - 1, got %d", rule->min_voxels);
  MMTTA_CHECK(rule->scope == MMTTA_GUARD_SCOPE_VOLUME || rule->scope == MMTTA_GUARD_SCOPE_REGION, MMTTA_ERR_INVALID,
              "guard select: scope must be MMTTA_GUARD_SCOPE_VOLUME or _REGION, got %d", rule->scope);
  MMTTA_CHECK(!guard_overlap(reference, logits), MMTTA_ERR_INVALID, "guard select: `reference` and `logits` are aliased");
  hipStream_t s = (hipStream_t)stream;
  const int items = reference->n, R = reference->c;
  const long long vox = (long long)reference->d * reference->h * reference->w;
  const dim3 grid((unsigned)((vox + GUARD_CHUNK - 1) / GUARD_CHUNK), items);
  GuardRule g;
  g.A = rule->min_agreement_q16; g.G = rule->max_growth_q16; g.H = rule->max_shrink_q16; g.m = (unsigned long long)rule->min_voxels;
  g.region = rule->scope == MMTTA_GUARD_SCOPE_REGION ? 1 : 0;
  const long long* c = (const long long*)counts;
  if (R <= 4 && guard_dense4(reference) && guard_dense4(logits)) {
    const bool full = !g.region && (R == 4 || (logits->flags & MMTTA_TENSOR_OWNS_PAD));
    if (full) hipLaunchKernelGGL((guard_select_kernel<true, true>), grid, dim3(256), 0, s, c, g, tv(reference), tv(logits), fallback);
    else hipLaunchKernelGGL((guard_select_kernel<true, false>), grid, dim3(256), 0, s, c, g, tv(reference), tv(logits), fallback);
  } else {
    hipLaunchKernelGGL((guard_select_kernel<false, false>), grid, dim3(256), 0, s, c, g, tv(reference), tv(logits), fallback);
  }
  return launch_status("guard select");
}
