// Calibration of the evaluation tail: a streaming reliability histogram with Brier and NLL sums, from the logits the
// plugins return (gfx950).  One pass over the logits and the label, the bytes dice_counts_kernel moves minus the mask.
//
// Reproducible by construction: everything that is summed is an INTEGER.  Counts are counts; a confidence, a Brier term
// and an NLL term enter as fixed-point numbers (scales below), so the adds commute and the table does not depend on how
// lanes, waves and workgroups are scheduled (the pattern of the surface kernel's distance sum).  The integers are summed
// in `out` itself, viewed as uint64, and calibration_finish_kernel turns every entry into its double in place: no scratch.
//
// Contention: after adaptation almost every element sits in the top bin.  A lane therefore keeps a RUN per region in
// registers - (bin, count, correct, sum of confidence) - and touches the workgroup's LDS table only when its bin changes
// and once at the end; the Brier and NLL sums have no bin and stay in registers for the whole loop.  One row per workgroup
// then leaves the CU as 64-bit integer atomics on the entries that are not zero.
#include "common.h"

namespace mmtta {

constexpr int CAL_MAX_BINS = 64;
constexpr int CAL_MAX_COLS = 3 * CAL_MAX_BINS + 2;
constexpr int CAL_SOFTMAX_MAX_R = 16;
constexpr int CAL_CHUNK = 4;                       // regions one lane carries on the sigmoid head
// fixed-point scales.  A confidence is >= 1/16 (>= 1/2 on the sigmoid head), an fp32 multiple of 2^-28: exact.  A Brier
// term is <= 2: rounding 2^-31 per element.  An NLL term saturates at CAL_NLL_MAX nats (p < 1e-110): rounding 2^-25.
// The largest sum, (2^31 - 1) elements: 2^59, 2^62, 2^63 - inside 64 bits.
constexpr float CAL_CONF_SCALE = 268435456.f;      // 2^28
constexpr float CAL_BRIER_SCALE = 1073741824.f;    // 2^30
constexpr float CAL_NLL_SCALE = 16777216.f;        // 2^24
constexpr float CAL_NLL_MAX = 255.f;

struct CalRun {
  int bin;
  unsigned int cnt, cor;
  unsigned long long conf;
};

__device__ __forceinline__ void cal_flush(const CalRun& r, unsigned long long* row) {
  if (r.cnt == 0u) return;
  atomicAdd(row + r.bin * 3 + 0, (unsigned long long)r.cnt);
  atomicAdd(row + r.bin * 3 + 1, r.conf);
  if (r.cor) atomicAdd(row + r.bin * 3 + 2, (unsigned long long)r.cor);
}

// one element into the lane's run; the LDS row is touched only when the bin changes
__device__ __forceinline__ void cal_add(CalRun& r, float conf, bool correct, int bins, unsigned long long* row) {
  int k = (int)ceilf(conf * (float)bins) - 1;       // (k/B, (k+1)/B], fp32
  k = min(bins - 1, max(0, k));
  if (k != r.bin) {
    cal_flush(r, row);
    r.bin = k; r.cnt = 0u; r.cor = 0u; r.conf = 0ull;
  }
  r.cnt += 1u;
  r.cor += correct ? 1u : 0u;
  r.conf += (unsigned long long)__float2uint_rn(conf * CAL_CONF_SCALE);
}

struct CalArgs {
  TV z, lab;
  unsigned long long* out;      // [N][Rout][3 * bins + 2], zeroed
  int bins, scope, blocks_per_n;
  int lab_dense;                // the label's voxels of one (item, region) are one dense run: offset = voxel index
};

// element offsets of voxel v in the logits and in the label (without the item and channel terms)
template <bool VEC>
__device__ __forceinline__ void cal_offsets(const CalArgs& a, unsigned int v, long long& zo, long long& lo) {
  if (VEC && a.lab_dense) {     // uniform: no division
    zo = (long long)v * 4;
    lo = v;
    return;
  }
  const unsigned int x = v % (unsigned)a.z.w, t = v / (unsigned)a.z.w;
  const unsigned int y = t % (unsigned)a.z.h, zz = t / (unsigned)a.z.h;
  zo = VEC ? (long long)v * 4 : zz * a.z.sd + y * a.z.sh + x * a.z.sw;
  lo = a.lab_dense ? (long long)v : zz * a.lab.sd + y * a.lab.sh + x * a.lab.sw;
}

// CAL_CHUNK consecutive channels from c0 of one voxel.  VEC: the 16-byte row of a voxel (<= 4 channels, dense rows of
// 4 floats).  The pad lanes travel with the load and are never used; the last voxel of an item is read lane by lane,
// because nothing says that a view owns the pad behind its last element.
template <bool VEC>
__device__ __forceinline__ void cal_load4(const float* zp, long long sc, int c0, int C, bool last, float (&t)[CAL_CHUNK]) {
  if (VEC && !last) {
    const float4 q = *reinterpret_cast<const float4*>(zp);
    t[0] = q.x; t[1] = q.y; t[2] = q.z; t[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < CAL_CHUNK; ++j) t[j] = zp[(long long)min(c0 + j, C - 1) * sc];    // clamped: straight-line loads
  }
}

// rows of the workgroup's table -> the item's rows in `out`
__device__ __forceinline__ void cal_publish(const unsigned long long* sh, int words, unsigned long long* dst) {
  __syncthreads();
  for (int i = threadIdx.x; i < words; i += blockDim.x)
    if (sh[i] != 0ull) atomicAdd(dst + i, sh[i]);
}

// ------------------------------------------------------------------ sigmoid head
// Every (voxel, region) is a Bernoulli element.  A lane owns a voxel and the CAL_CHUNK regions from blockIdx.y * CAL_CHUNK.
template <bool VEC>
__global__ __launch_bounds__(256) void calibration_sigmoid_kernel(CalArgs a) {
  __shared__ unsigned long long sh[CAL_CHUNK * CAL_MAX_COLS];
  const int R = a.z.c, B = a.bins, cols = 3 * B + 2;
  const int n = blockIdx.z, r0 = blockIdx.y * CAL_CHUNK;
  const int rc = min(CAL_CHUNK, R - r0);
  for (int i = threadIdx.x; i < CAL_CHUNK * cols; i += 256) sh[i] = 0ull;
  __syncthreads();
  const unsigned int dhw = (unsigned)a.z.d * a.z.h * a.z.w;
  const float* zb = a.z.p + n * a.z.sn + (VEC ? 0 : (long long)r0 * a.z.sc);
  const float* lb = a.lab.p + n * a.lab.sn;
  CalRun run[CAL_CHUNK];
  unsigned long long brier[CAL_CHUNK], nll[CAL_CHUNK];
#pragma unroll
  for (int j = 0; j < CAL_CHUNK; ++j) {
    run[j].bin = -1; run[j].cnt = 0u; run[j].cor = 0u; run[j].conf = 0ull;
    brier[j] = 0ull; nll[j] = 0ull;
  }
  for (unsigned int v = blockIdx.x * 256u + threadIdx.x; v < dhw; v += (unsigned)a.blocks_per_n * 256u) {
    long long zo, lo;
    cal_offsets<VEC>(a, v, zo, lo);
    float t[CAL_CHUNK], yv[CAL_CHUNK];
    cal_load4<VEC>(zb + zo, a.z.sc, 0, rc, v + 1u == dhw, t);        // zb starts at channel r0
#pragma unroll
    for (int j = 0; j < CAL_CHUNK; ++j) yv[j] = lb[lo + (long long)min(r0 + j, R - 1) * a.lab.sc];
#pragma unroll
    for (int j = 0; j < CAL_CHUNK; ++j) {
      if (j < rc) {                                  // uniform
        const float zl = t[j];
        const bool pred = zl >= 0.f, gt = yv[j] > 0.5f;
        if (a.scope == 0 || pred || gt) {
          const float mag = fabsf(zl);
          const float e = expf(-mag);
          const float conf = 1.f / (1.f + e);        // sigmoid(|z|): the probability of the predicted side
          const bool correct = pred == gt;
          const float d = correct ? e / (1.f + e) : conf;              // |sigmoid(z) - y| without the cancellation
          const float ce = (correct ? 0.f : mag) + log1pf(e);          // max(z,0) - z y + log1p(exp(-|z|)), y in {0,1}
          cal_add(run[j], conf, correct, B, sh + j * cols);
          brier[j] += (unsigned long long)__float2uint_rn(d * d * CAL_BRIER_SCALE);
          nll[j] += (unsigned long long)__float2uint_rn(fminf(ce, CAL_NLL_MAX) * CAL_NLL_SCALE);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < CAL_CHUNK; ++j) {
    if (j < rc) {
      cal_flush(run[j], sh + j * cols);
      if (brier[j]) atomicAdd(sh + j * cols + 3 * B, brier[j]);
      if (nll[j]) atomicAdd(sh + j * cols + 3 * B + 1, nll[j]);
    }
  }
  cal_publish(sh, rc * cols, a.out + ((long long)n * R + r0) * cols);
}

// ------------------------------------------------------------------ softmax head
// Every voxel is one element: prediction = argmax z, label class = argmax of the label channels (lowest index on ties).
template <bool VEC, int MAXR>
__global__ __launch_bounds__(256) void calibration_softmax_kernel(CalArgs a) {
  __shared__ unsigned long long sh[CAL_MAX_COLS];
  const int R = a.z.c, B = a.bins, cols = 3 * B + 2;
  const int n = blockIdx.z;
  for (int i = threadIdx.x; i < cols; i += 256) sh[i] = 0ull;
  __syncthreads();
  const unsigned int dhw = (unsigned)a.z.d * a.z.h * a.z.w;
  const float* zb = a.z.p + n * a.z.sn;
  const float* lb = a.lab.p + n * a.lab.sn;
  CalRun run;
  run.bin = -1; run.cnt = 0u; run.cor = 0u; run.conf = 0ull;
  unsigned long long brier = 0ull, nll = 0ull;
  for (unsigned int v = blockIdx.x * 256u + threadIdx.x; v < dhw; v += (unsigned)a.blocks_per_n * 256u) {
    long long zo, lo;
    cal_offsets<VEC>(a, v, zo, lo);
    float t[MAXR], yv[MAXR];
    if constexpr (MAXR == CAL_CHUNK) {
      float q[CAL_CHUNK];
      cal_load4<VEC>(zb + zo, a.z.sc, 0, R, v + 1u == dhw, q);
#pragma unroll
      for (int k = 0; k < MAXR; ++k) t[k] = q[k % CAL_CHUNK];
    } else {
#pragma unroll
      for (int k = 0; k < MAXR; ++k) t[k] = zb[zo + (long long)min(k, R - 1) * a.z.sc];
    }
#pragma unroll
    for (int k = 0; k < MAXR; ++k) yv[k] = lb[lo + (long long)min(k, R - 1) * a.lab.sc];
    float m = -INFINITY, best = -INFINITY, zlab = t[0];
    int pred = 0, cls = 0;
#pragma unroll
    for (int k = 0; k < MAXR; ++k) {
      if (k >= R) { t[k] = -INFINITY; yv[k] = -INFINITY; }       // a pad lane or a clamped repeat: never the maximum
      if (t[k] > m) { m = t[k]; pred = k; }
      if (yv[k] > best) { best = yv[k]; cls = k; zlab = t[k]; }
    }
    if (a.scope != 0 && pred == 0 && cls == 0) continue;
    float ex[MAXR], others = 0.f;
#pragma unroll
    for (int k = 0; k < MAXR; ++k) {
      ex[k] = expf(t[k] - m);
      others += k == pred ? 0.f : ex[k];             // sum exp(z_k - z_max) = 1 + others, the 1 kept apart
    }
    const float conf = 1.f / (1.f + others);
    float bs = 0.f;
#pragma unroll
    for (int k = 0; k < MAXR; ++k) {
      const float d = ex[k] * conf - (k == cls ? 1.f : 0.f);
      bs += d * d;
    }
    const float ce = (m - zlab) + log1pf(others);    // log-sum-exp minus the label's logit
    cal_add(run, conf, pred == cls, B, sh);
    brier += (unsigned long long)__float2uint_rn(fminf(bs, 2.f) * CAL_BRIER_SCALE);
    nll += (unsigned long long)__float2uint_rn(fminf(ce, CAL_NLL_MAX) * CAL_NLL_SCALE);
  }
  cal_flush(run, sh);
  if (brier) atomicAdd(sh + 3 * B, brier);
  if (nll) atomicAdd(sh + 3 * B + 1, nll);
  cal_publish(sh, cols, a.out + (long long)n * cols);
}

// the integer table -> doubles, in place (counts exact, fixed-point sums scaled back)
__global__ __launch_bounds__(256) void calibration_finish_kernel(unsigned long long* table, long long total, int bins) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= total) return;
  const int cols = 3 * bins + 2, j = (int)(i % cols);
  const double scale = j == 3 * bins ? 1.0 / (double)CAL_BRIER_SCALE
                       : j == 3 * bins + 1 ? 1.0 / (double)CAL_NLL_SCALE
                       : j % 3 == 1 ? 1.0 / (double)CAL_CONF_SCALE : 1.0;
  const double v = (double)table[i] * scale;
  reinterpret_cast<double*>(table)[i] = v;
}

static int calibration_check_logits(const mmtta_tensor* logits, int bins) {
  MMTTA_CHECK(logits != nullptr, MMTTA_ERR_INVALID, "calibration: null argument");
  MMTTA_CHECK(bins >= 1 && bins <= CAL_MAX_BINS, MMTTA_ERR_INVALID, "calibration: bins %d (1 ... %d)", bins, CAL_MAX_BINS);
  MMTTA_CHECK(logits->n >= 1 && logits->c >= 1 && logits->d >= 1 && logits->h >= 1 && logits->w >= 1, MMTTA_ERR_INVALID,
              "calibration: empty logits");
  MMTTA_CHECK(logits->c <= 256, MMTTA_ERR_UNSUPPORTED, "calibration: more than 256 regions");
  MMTTA_CHECK((long long)logits->d * logits->h * logits->w < (1ll << 31), MMTTA_ERR_UNSUPPORTED,
              "calibration: more than 2^31 - 1 voxels per volume");
  return MMTTA_OK;
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int64_t mmtta_calibration_scratch_bytes(const mmtta_tensor* logits, int bins) {
  return calibration_check_logits(logits, bins) == MMTTA_OK ? 0 : -1;      // the sums are integers in `out`: no scratch
}

extern "C" int mmtta_calibration_bins(const mmtta_tensor* logits, const mmtta_tensor* label, int softmax, int bins, int scope,
                                      double* out, void* scratch, void* stream) {
  (void)scratch;
  MMTTA_CHECK(logits && label && out && logits->ptr && label->ptr, MMTTA_ERR_INVALID, "calibration: null argument");
  MMTTA_CHECK(logits->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "mmtta_calibration_bins: `logits` must be fp32-stored");
  MMTTA_CHECK(label->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "mmtta_calibration_bins: `label` must be fp32-stored");
  int st = calibration_check_logits(logits, bins);
  if (st) return st;
  MMTTA_CHECK(scope == 0 || scope == 1, MMTTA_ERR_INVALID, "calibration: scope %d (0: volume, 1: union)", scope);
  MMTTA_CHECK(same_shape(logits, label), MMTTA_ERR_INVALID, "calibration: logits/label shape mismatch");
  const int R = logits->c;
  MMTTA_CHECK(!softmax || R >= 2, MMTTA_ERR_INVALID, "calibration: the softmax head needs at least 2 classes");
  MMTTA_CHECK(!softmax || R <= CAL_SOFTMAX_MAX_R, MMTTA_ERR_UNSUPPORTED, "calibration: more than %d classes on the softmax head",
              CAL_SOFTMAX_MAX_R);
  MMTTA_CHECK(logits->n <= 65535, MMTTA_ERR_UNSUPPORTED, "calibration: more than 65535 volumes in one call");
  hipStream_t s = (hipStream_t)stream;
  const int rout = softmax ? 1 : R, cols = 3 * bins + 2;
  const long long total = (long long)logits->n * rout * cols;
  hipError_t e = hipMemsetAsync(out, 0, (size_t)total * sizeof(double), s);
  MMTTA_CHECK(e == hipSuccess, MMTTA_ERR_LAUNCH, "calibration: memset failed: %s", hipGetErrorString(e));
  const long long dhw = (long long)logits->d * logits->h * logits->w;
  long long bpn = (dhw + 256 * 16 - 1) / (256 * 16);     // ~16 voxels per lane: runs long enough to stay in registers
  if (bpn > 1024) bpn = 1024;
  CalArgs a;
  a.z = tv(logits); a.lab = tv(label);
  a.out = reinterpret_cast<unsigned long long*>(out);
  a.bins = bins; a.scope = scope; a.blocks_per_n = (int)bpn;
  a.lab_dense = label->sw == 1 && label->sh == label->w && label->sd == (int64_t)label->h * label->w;
  // 16-byte voxel rows: <= 4 channels in dense rows of 4 floats (the channels-last view the plugins return)
  const bool vec = R <= 4 && logits->sc == 1 && logits->sw == 4 && logits->sh == (int64_t)logits->w * 4 &&
                   logits->sd == (int64_t)logits->h * logits->sh && logits->sn % 4 == 0 && ((uintptr_t)logits->ptr) % 16 == 0;
  const dim3 blk(256);
  if (!softmax) {
    const dim3 grid((unsigned)bpn, (unsigned)((R + CAL_CHUNK - 1) / CAL_CHUNK), (unsigned)logits->n);
    if (vec) hipLaunchKernelGGL(calibration_sigmoid_kernel<true>, grid, blk, 0, s, a);
    else hipLaunchKernelGGL(calibration_sigmoid_kernel<false>, grid, blk, 0, s, a);
  } else {
    const dim3 grid((unsigned)bpn, 1u, (unsigned)logits->n);
    if (vec) hipLaunchKernelGGL((calibration_softmax_kernel<true, CAL_CHUNK>), grid, blk, 0, s, a);
    else if (R <= CAL_CHUNK) hipLaunchKernelGGL((calibration_softmax_kernel<false, CAL_CHUNK>), grid, blk, 0, s, a);
    else hipLaunchKernelGGL((calibration_softmax_kernel<false, CAL_SOFTMAX_MAX_R>), grid, blk, 0, s, a);
  }
  st = launch_status("calibration bins");
  if (st) return st;
  hipLaunchKernelGGL(calibration_finish_kernel, dim3((unsigned)((total + 255) / 256)), blk, 0, s, a.out, total, bins);
  return launch_status("calibration finish");
}
