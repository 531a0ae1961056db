// Implicit-GEMM convolution on the CDNA4 matrix cores (gfx950), channels-last activations.
//
// One kernel family serves Conv3d forward, its input gradient, ConvTranspose3d forward and its
// input gradient (reference call sites: src/models/unet.py:68-69 via monai UNet,
// src/models/unet_multimodal_midfusion.py:204-267; backward from
// src/core/trainers/seg_trainer.py:142).  All four are the same "gather GEMM":
//
//     out[g*so + o][n] = sum_{tap} sum_{k} T(in[g*si + d_tap][k]) * Wp[slab_tap][k][n]
//
// g runs over an output sub-grid.  Conv: so=1, si=stride, d = k-pad.  Input gradient of a stride-1
// conv: d = pad-k.  The stride-2 transposed forms are split into 8 output parity classes (so=2),
// each a small dense conv over 1..8 taps - no zero-stuffing, no atomics, no wasted MACs.
//
// Work decomposition (wave = 64 lanes, 4 waves per workgroup, one workgroup = one spatial box):
//   * the input box of the tile (tile + halo, KCI channels at a time) is staged ONCE in LDS and
//     re-used by every tap (27x re-use for k=3) - global reads are ~1.5-2.4x the input instead
//     of 27x; norm+ReLU of the producer is applied while staging (norm on load), padding voxels
//     are written as exact zeros;
//   * each wave owns MB 32-row blocks x one 32-column block: v_mfma_f32_32x32x2_f32 (exact fp32,
//     one operand element per lane, so the LDS image needs no fragment layout) with the
//     weight fragment fetched straight from the packed image (L1/L2 resident) one tap ahead;
//   * LDS voxel stride KCI+1 words: the 32 rows of an A fragment fall on distinct banks;
//   * epilogue: bias, optional fused residual add, store (128-B segments), per-tile
//     sum / sum-of-squares for the following InstanceNorm (deterministic partial slab, no atomics);
//   * small spatial extents (8^3 bottleneck) get split-K over channel blocks through a workspace
//     so that >= 256 workgroups exist.
#include "common.h"

namespace mmtta {
MMTTA_ACT_NS_OPEN

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned int pack_bf16x2(float lo, float hi) {
  bf16x2 v;
  v[0] = (__bf16)lo;   // plain casts: hipcc emits v_cvt_pk_bf16_f32 (round to nearest even, NaN preserved)
  v[1] = (__bf16)hi;
  return __builtin_bit_cast(unsigned int, v);
}

struct Taps {      // host-side description of one tap set
  int n;
  int slab[27];
  signed char dz[27], dy[27], dx[27];
  int zmin, ymin, xmin;
  int zext, yext, xext;
};

// One output parity class of a launch (a plain conv is a single class with all its taps).  The stride-2
// transposed forms run their 8 classes in ONE launch, interleaved with the tile index (class_of_tile below).
struct ClassInfo {
  int tap0, ntaps;
  int oz, oy, ox;
  int zmin, ymin, xmin;
  int zext, yext, xext;
  int Dg, Hg, Wg;
  // box extents of this class for the launch's tile, with reciprocals for exact division of a box index < 2^16:
  // q = __umulhi(v, ceil(2^32 / d))
  int BX, BXY;
  unsigned mBX, mBXY;
};

struct GArgs {
  const float* in; long long isn, isd, ish, isw; int Ci, Di, Hi, Wi;
  NL tin;
  float* out; long long osn, osd, osh, osw; int Co, Do, Ho, Wo;
  int so;
  int si;
  const float* wp; int Kp, Np;
  const float* bias;
  PSets ps;        // per-item parameter sets: wp / bias are set 0's (common.h)
  const float* add; long long asn, asd, ash, asw; NL tadd;
  int accumulate;
  float* stats; int stats_rows_per_n;
  float* ws; int ksplit, stages_per_split, nstages;
  int tz, ty, tx;
  int in_bf, out_bf, add_bf;   // storage of the three activation operands: 1 = bf16 elements (common.h storage helpers)
  int vec4;
  int ovec;        // 16-byte epilogue stores (out / add rows 16-byte aligned, Co % 4 == 0)
  int coef_off;    // word offset of the coefficient table behind the LDS box image
  int rowload;     // the input admits the row-structured loader (alignment, 24-bit strides, < 2^31 elements)
  int flip27;      // canonical 27-tap stride-1 stage (rowload): tap t reads weight slab 26 - t (stride-1 input gradient) instead of t
  int ncls;
  ClassInfo cls[8];
  int toff[27];   // box-relative voxel offset of each tap (int32 tables: read with SCALAR loads)
  int slab[27];   // weight slab of each tap
};

// Launch tile index -> (parity class, tile inside the class).  The classes of one tile are NEIGHBOURS in the index, the
// 8-tap class first: the 8 XCDs each run one contiguous eighth of the index (xcd_contiguous_id), and with the classes laid
// out one after the other XCD c ran class c alone - 1 tap's work on XCD 0 against 8 taps' on XCD 7, the launch as slow as
// its heaviest eighth (2.4x the mean of 27/8 taps).  Interleaved, every XCD carries the same mix and the 8 classes of a tile
// read their shared input box from one L2.
__device__ __forceinline__ void class_of_tile(const GArgs& a, int tile, int& cidx, int& t) {
  if (a.ncls == 8) { cidx = 7 - (tile & 7); t = tile >> 3; }
  else { cidx = 0; t = tile; }
}

// MFMA row index v of a tile -> local voxel.  PERM (bf16 images): inside every 32-row block (4 y-rows x 8 x) the
// rows are permuted so that the 16 lanes ds_read_b128 services together ({0-3,12-15,20-27} and {4-11,16-19,28-31})
// hold the voxels of y-rows {0,2} and {1,3}: with an LDS x-row pitch of LP = 12 voxels of 48 bytes their
// 16-byte slots are all distinct modulo 16 - the A-fragment reads are bank-conflict free (3-way before).
template <int TZ, int TY, int TX, bool PERM>
__device__ __forceinline__ void row_to_local(int v, int& zl, int& yl, int& xl) {
  if (PERM) {
    static_assert(TX == 8 && TY % 4 == 0, "the permutation assumes 4 x 8 row blocks");
    const int r = v & 31, q = r >> 2;
    const int y = (0xEB14 >> (2 * q)) & 3;           // q: 0 1 2 3 4 5 6 7 -> y: 0 1 1 0 3 2 2 3
    const int xh = (q >> 1) & 1;
    v = (v & ~31) + y * 8 + xh * 4 + (r & 3);
  }
  xl = v % TX;
  yl = (v / TX) % TY;
  zl = v / (TX * TY);
}

constexpr int LDS_PITCH_BF16 = 12;   // x-row pitch (voxels) of the bf16 LDS image of stride-1 gathers

// Box-relative voxel offset of tap t of the canonical 3x3x3 stride-1 stage (taps in ascending (z, y, x) box order, RBY box
// rows per z plane): a compile-time constant once the tap loops are unrolled, i.e. an immediate of the ds_read.
__host__ __device__ constexpr int tap27_off(int t, int rby) { return ((t / 9) * rby + (t / 3) % 3) * LDS_PITCH_BF16 + t % 3; }

// Fragment reuse along x (igemm_reuse_kernel, the lean 4 x 8 x 8 tile).  The two row blocks of a wave (one z slice: 8 y x 8 x)
// are the voxels of even and of odd x: MFMA row r of block b is the voxel y = (r >> 3) + 4 (r >> 2 & 1), x = 2 (r & 3) + b.
// Block 0 at tap kx + 1 then reads exactly the 32 voxels block 1 reads at tap kx, and block 1 at kx + 1 those of block 0 at
// kx + 2: a box row (kz, ky) takes the four fragments m = b + kx = 0..3 (voxels x = 2 (r & 3) + m) instead of six.  The
// staged image keeps the even box columns in x slots 0-4 of a row and the odd ones in slots 5-9 (reuse_xslot), so the four
// x of a fragment are neighbours and the 16 lanes ds_read_b128 services together - 4 x of 4 rows y that differ modulo 4 -
// fall on 16 distinct 16-byte slots modulo 256 bytes (slot = 4 y + 3 x + const mod 16) as in the plain image.
__host__ __device__ constexpr int reuse_xslot(int bx) { return (bx & 1) * 5 + (bx >> 1); }
// accumulator register i (lane half h) of parity block b -> row index, inside the wave's 64 rows, that row_to_local's
// permuted mapping gives the same voxel, less 32 h: y = (i >> 2) + 4 h is plain block h, row y & 3 = i >> 2 of it
__host__ __device__ constexpr int reuse_row(int i, int b) {
  const int yl = i >> 2, x = 2 * (i & 3) + b, xh = x >> 2;
  int q = 0;
  for (int c = 0; c < 8; ++c)
    if (((0xEB14 >> (2 * c)) & 3) == yl && ((c >> 1) & 1) == xh) q = c;
  return q * 4 + (x & 3);
}

// Epilogue with 16-byte stores.  An MFMA accumulator block holds ONE output channel per lane (32 lanes = a 128-byte
// voxel row) and 16 voxels in its registers, so storing straight from it takes 16 four-byte-per-lane stores per block -
// measured in the producer/consumer kernel (s_memtime): 42k cycles per 512-voxel tile, more than its four MFMA stages
// together; the store path is issue-bound at ~1.6 bytes per cycle and CU that way.  Here every 32 x 32 block goes
// through a wave-private LDS tile and comes back as float4 = 4 channels of one voxel per lane: 4 stores of 1 KiB per
// block (8 lanes cover a voxel row), and the fused add / accumulate operands are fetched 16 bytes per lane too.
// `tr`: 32 x 36 floats of this wave.  Per-lane sums for the following norm: channels colbase + 4*(lane&7) + 0..3,
// already added up over the 8 row lanes (valid in lanes 0-7).
// XPAR (igemm_reuse_kernel): the accumulator blocks hold the x-parity row mapping (reuse_row); both go into a 64-row tile at
// the row index the plain mapping gives their voxels, and everything behind the tile is the plain epilogue - the same
// voxels per lane in the same order, so the statistics rows sum as they always did.
template <int TZ, int TY, int TX, int MB, bool PERM, bool ABF, bool XPAR = false>
__device__ __forceinline__ void epilogue_vec16(const GArgs& a, const float* biasp, const ClassInfo& ci, f32x16 (&acc)[MB], float* tr,
                                               int lane, int rowblock0, int colbase, bool colact, int n, int gz0, int gy0, int gx0,
                                               float (&ssum)[4], float (&ssq)[4]) {
  // kernel-argument fields used per row: opaque scalar copies (see the tap tables of the producer/consumer kernel)
  int osd = (int)a.osd, osh = (int)a.osh, osw = (int)a.osw, asd = (int)a.asd, ash_ = (int)a.ash, asw = (int)a.asw;
  int so = a.so, Do = a.Do, Ho = a.Ho, Wo = a.Wo, coz = ci.oz, coy = ci.oy, cox = ci.ox, cDg = ci.Dg, cHg = ci.Hg, cWg = ci.Wg;
  asm volatile("" : "+s"(osd), "+s"(osh), "+s"(osw), "+s"(asd), "+s"(ash_), "+s"(asw), "+s"(so), "+s"(Do), "+s"(Ho), "+s"(Wo));
  asm volatile("" : "+s"(coz), "+s"(coy), "+s"(cox), "+s"(cDg), "+s"(cHg), "+s"(cWg));
  const int h = lane >> 5, r = lane & 31;
  const int rsub = lane >> 3, c4 = (lane & 7) * 4;
  const int colv = colbase + c4;
  const bool cvok = colact && colv < a.Co;                 // Co % 4 == 0 on this path: all four channels or none
  const int colc = min(colv, a.Co - 4);
  float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float asc[4] = {1.f, 1.f, 1.f, 1.f}, ash[4] = {0.f, 0.f, 0.f, 0.f};
  if (biasp) bias4 = *reinterpret_cast<const float4*>(biasp + colc);
  if (a.add) nl_coeff_vec<4>(a.tadd, n, a.Co, colc, asc, ash);
#pragma unroll
  for (int j = 0; j < 4; ++j) { ssum[j] = 0.f; ssq[j] = 0.f; }
  const float* addb = a.add;
  float* outb = a.out;
  const long long abase = (long long)n * a.asn + colc, obase = (long long)n * a.osn + colc;
  // value path of one (block, row slot): bias, fused add, accumulate, store, statistics - shared by both address paths
  auto finish = [&](const float4& val, const float4& addq, const float4& oldq, bool okk, int oo) {
    float v[4] = {val.x + bias4.x, val.y + bias4.y, val.z + bias4.z, val.w + bias4.w};
    if (a.add) {
      const float av[4] = {addq.x, addq.y, addq.z, addq.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += nl_apply(av[j], asc[j], ash[j], a.tadd.relu);
    }
    if (a.accumulate) { v[0] += oldq.x; v[1] += oldq.y; v[2] += oldq.z; v[3] += oldq.w; }
    if (okk) {
      st4_t<ABF>(outb, obase + oo, make_float4(v[0], v[1], v[2], v[3]));
#pragma unroll
      for (int j = 0; j < 4; ++j) { ssum[j] += v[j]; ssq[j] += v[j] * v[j]; }
    }
  };
  // Interior tiles of the un-decomposed ops (every row inside the tensor, output voxel = grid voxel): the offsets of the
  // 4 row slots of a block are wave-uniform terms plus two per-lane constants (the row permutation keeps x = 4 (k & 1) +
  // (lane >> 3 & 3) and picks y from one of two compile-time values by lane bit 5), ~2 vector instructions per row
  // instead of ~35 (decode, bounds, clamps, six 32-bit multiplies); and because nothing depends on the accumulators, the
  // fused-add (or accumulate) operand of ALL blocks is requested up front - one exposed round trip per tile, not one per
  // block (the weight-fragment registers are free by now).
  if constexpr (XPAR) {
    static_assert(MB == 2, "two parity blocks");
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) tr[(reuse_row(i, b) + 32 * h) * 36 + r] = acc[b][i];
  }
  const bool interior = PERM && so == 1 && coz == 0 && coy == 0 && cox == 0 && gz0 + TZ <= min(cDg, Do) && gy0 + TY <= min(cHg, Ho) &&
                        gx0 + TX <= min(cWg, Wo);
  if (interior) {
    const bool lb = (rsub >> 2) != 0;
    const int lxo = (rsub & 3) * osw, lxa = (rsub & 3) * asw;
    constexpr int T = 0xEB14;                         // row_to_local's y table
    auto row_off = [&](int mb, int k, int sd_, int sh_, int sw_, int lx) {     // (block, row slot) -> element offset
      const int rb = rowblock0 + mb;
      const int zl = TY == 4 ? rb : (rb >> 1), yb = TY == 4 ? 0 : (rb & 1) * 4;
      const int u = (gz0 + zl) * sd_ + (gy0 + yb) * sh_ + (gx0 + 4 * (k & 1)) * sw_;              // wave-uniform
      const int y0 = (T >> (2 * (2 * k))) & 3, y1 = (T >> (2 * (2 * k + 1))) & 3;
      return (lb ? u + y1 * sh_ : u + y0 * sh_) + lx;
    };
    const bool one_operand = (a.add != nullptr) != (a.accumulate != 0);
    float4 pre[MB][4];
    if (one_operand) {
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int k = 0; k < 4; ++k)
          pre[mb][k] = a.add ? ld4_t<ABF>(addb, abase + row_off(mb, k, asd, ash_, asw, lxa))
                             : ld4_t<ABF>(outb, obase + row_off(mb, k, osd, osh, osw, lxo));
    }
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      if constexpr (!XPAR) {
#pragma unroll
        for (int i = 0; i < 16; ++i) tr[((i & 3) + 8 * (i >> 2) + 4 * h) * 36 + r] = acc[mb][i];
      }
      const float* trb = tr + (XPAR ? mb * 32 * 36 : 0);
      float4 val[4], addv[4], oldv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) val[k] = *reinterpret_cast<const float4*>(trb + (rsub + 8 * k) * 36 + c4);
      if (!one_operand) {
        if (a.add) {
#pragma unroll
          for (int k = 0; k < 4; ++k) addv[k] = ld4_t<ABF>(addb, abase + row_off(mb, k, asd, ash_, asw, lxa));
        }
        if (a.accumulate) {
#pragma unroll
          for (int k = 0; k < 4; ++k) oldv[k] = ld4_t<ABF>(outb, obase + row_off(mb, k, osd, osh, osw, lxo));
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int oo = row_off(mb, k, osd, osh, osw, lxo);
        if (one_operand) finish(val[k], pre[mb][k], pre[mb][k], cvok, oo);
        else finish(val[k], addv[k], oldv[k], cvok, oo);
      }
    }
  } else {
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    if constexpr (!XPAR) {
#pragma unroll
      for (int i = 0; i < 16; ++i) tr[((i & 3) + 8 * (i >> 2) + 4 * h) * 36 + r] = acc[mb][i];
    }
    const float* trb = tr + (XPAR ? mb * 32 * 36 : 0);
    int ooff[4], aoff[4];
    bool ok[4];
    float4 val[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int row = rsub + 8 * k;
      val[k] = *reinterpret_cast<const float4*>(trb + row * 36 + c4);
      int zl, yl, xl;
      row_to_local<TZ, TY, TX, PERM>((rowblock0 + mb) * 32 + row, zl, yl, xl);
      const int gz = gz0 + zl, gy = gy0 + yl, gx = gx0 + xl;
      const int oz = gz * so + coz, oy = gy * so + coy, ox = gx * so + cox;
      ok[k] = cvok && gz < cDg && gy < cHg && gx < cWg && oz < Do && oy < Ho && ox < Wo;
      const int cz = min(oz, Do - 1), cy = min(oy, Ho - 1), cx = min(ox, Wo - 1);
      ooff[k] = cz * osd + cy * osh + cx * osw;
      aoff[k] = cz * asd + cy * ash_ + cx * asw;
    }
    float4 addv[4], oldv[4];
    if (a.add) {
#pragma unroll
      for (int k = 0; k < 4; ++k) addv[k] = ld4_t<ABF>(addb, abase + aoff[k]);
    }
    if (a.accumulate) {
#pragma unroll
      for (int k = 0; k < 4; ++k) oldv[k] = ld4_t<ABF>(outb, obase + ooff[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) finish(val[k], addv[k], oldv[k], ok[k], ooff[k]);
  }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) { ssum[j] += __shfl_xor(ssum[j], o, 64); ssq[j] += __shfl_xor(ssq[j], o, 64); }
  }
}

constexpr int EPI_TILE_FLOATS = 32 * 36;     // LDS words of one wave's transposition tile

// BF == false: fp32 operands, v_mfma_f32_32x32x2_f32 (bit-exact fp32 products, the parity path).
// BF == true : activations are rounded to bf16 while they are staged, weights come from a bf16 image,
//              v_mfma_f32_32x32x16_bf16 with fp32 accumulation (16x the matrix rate: these layers turn
//              HBM/LDS bound).  Storage, statistics, epilogue stay fp32 in both modes.
// OCC = workgroups the register budget admits per CU (launch bound in waves per SIMD): 2 for the four-block tiles
// (<= 256 registers), 4 for the lean two-block tile <1,2,4,8,8,16> of the 32-channel 64^3 layers (<= 128 registers,
// smaller weight-fragment groups, no box prefetch): twice the resident waves to cover each other's load, LDS and
// store latencies (MMTTA_OPT_IGEMM_LEAN).
// ABF: the three activation operands (input, output, fused add) are bf16-STORED (forward convolutions of bf16 precision);
// false: all fp32 (every input-gradient launch, fp32 precision).  Compile-time: see MMTTA_BF_DISPATCH in common.h.
// REUSE: the x-parity row mapping with shared activation fragments (reuse_xslot / reuse_row above; igemm_reuse_kernel).  The
// host launches it for the canonical 27-tap stage only (row loader, full 16-channel stages, 16-byte epilogue), so every
// other path of the body is compiled out of it.
template <int NB, int MB, int TZ, int TY, int TX, int KCI, bool BF, int OCC = 2, bool ABF = false>
__global__ __launch_bounds__(256, OCC) void igemm_kernel(GArgs a) {
  constexpr bool REUSE = false, RAW = false;
#include "conv_igemm_body.h"
}

// The stride-1 3x3x3 32 -> 32 layers of bf16 precision (the 64^3 level; forward and mirrored input gradient): the lean tile
// with two thirds of the activation-fragment reads.  Bit for bit igemm_kernel<1, 2, 4, 8, 8, 16, true, 3, ABF>.
template <bool ABF>
__global__ __launch_bounds__(256, 3) void igemm_reuse_kernel(GArgs a) {
  constexpr int NB = 1, MB = 2, TZ = 4, TY = 8, TX = 8, KCI = 16, OCC = 3;
  constexpr bool BF = true, REUSE = true, RAW = false;
#include "conv_igemm_body.h"
}

// Raw staging (MMTTA_OPT_RAW_STAGING bit 0; host: raw_staging): the bf16 tiles of igemm_kernel and igemm_reuse_kernel for a
// bf16-stored input without norm-on-load and with whole 8-channel chunks.  For such an input the staging chain - unpack,
// x * 1 + 0, max with -inf, round back to bf16 - returns the bits it was given (but -0.0 -> +0.0, which no sum that starts
// at +0 can tell), and it is most of a stage's vector-ALU work (profiles/igemm64_reuse_ab.md: 177 of 207 instructions
// of a K-loop trip).  These kernels store the loaded item under its mask.  The same body text with one more constant, so
// the kernels above keep theirs; launched from the plain translation unit only (the form has no activation to vary).
template <int NB, int MB, int TZ, int TY, int TX, int KCI, int OCC>
__global__ __launch_bounds__(256, OCC) void igemm_raw_kernel(GArgs a) {
  constexpr bool BF = true, ABF = true, REUSE = false, RAW = true;
#include "conv_igemm_body.h"
}

template <bool ABF>      // (always true: a template, so that the body's discarded branches stay uninstantiated)
__global__ __launch_bounds__(256, 3) void igemm_reuse_raw_kernel(GArgs a) {
  constexpr int NB = 1, MB = 2, TZ = 4, TY = 8, TX = 8, KCI = 16, OCC = 3;
  constexpr bool BF = true, REUSE = true, RAW = true;
#include "conv_igemm_body.h"
}

// ---------------------------------------------------------------- class-fused stride-2 transposed forms (bf16 operands)
// ConvTranspose3d forward and the input gradient of a stride-2 Conv3d are 8 output parity classes, each a dense
// convolution over 1 / 2 / 4 / 8 taps of the coarse input grid (27 taps in all).  igemm_kernel runs them as 8 x tiles
// independent workgroups that each stage their own halo box for 1-8 taps: per 16-channel stage 4-32 MFMAs per wave
// against a full staging pass and two barriers (measured: convT 128->32 at 64^3 out = 70 us at 105 TFLOP/s, the slowest
// implicit-GEMM launches of the network).  Here ONE workgroup produces all 8 classes of a coarse 4 x 4 x 8 tile (= an
// 8 x 8 x 16 block of the output): the box (tile + 1 on the high side of every axis: all tap offsets are 0 or 1) is staged
// once, the 27 taps' weight fragments of the stage go through LDS too (every wave needs all of them), and wave w owns
// row block w (z slice w of the tile) of EVERY class - 27 MFMAs per k step and wave, perfectly balanced, fed by 8
// activation fragments (one per offset, shared by the classes) and 27 weight fragments from LDS.
struct ClsTap { int cls, d, slab; };
__host__ __device__ constexpr ClsTap cls_tap(int f) {        // f-th (class, tap) in class order; d = (dz*2 + dy)*2 + dx
  int idx = 0;
  for (int cls = 0; cls < 8; ++cls) {
    const int pz = (cls >> 2) & 1, py = (cls >> 1) & 1, px = cls & 1;
    for (int a = 0; a <= pz; ++a)
      for (int b = 0; b <= py; ++b)
        for (int c = 0; c <= px; ++c) {
          // parity 0: k = 1 reads g (d = 0); parity 1: k = 0 reads g + 1, k = 2 reads g   (build_taps)
          const int kz = pz ? (a == 0 ? 0 : 2) : 1, dz = pz ? (a == 0 ? 1 : 0) : 0;
          const int ky = py ? (b == 0 ? 0 : 2) : 1, dy = py ? (b == 0 ? 1 : 0) : 0;
          const int kx = px ? (c == 0 ? 0 : 2) : 1, dx = px ? (c == 0 ? 1 : 0) : 0;
          if (idx == f) return ClsTap{cls, (dz * 2 + dy) * 2 + dx, (kz * 3 + ky) * 3 + kx};
          ++idx;
        }
  }
  return ClsTap{0, 0, 0};
}

// A 16-byte operand read from LDS.  TYPED (igemm_cls8_pipe_kernel): as ONE load of a vector type.  The copy of a uint4 is a
// struct copy, which reaches the back end as a load without type information, and hipcc makes every such LDS read wait for all
// direct global-to-LDS loads in flight (vmcnt(0) at the head of the MFMA phase, i.e. for the image just requested); the typed
// load waits only for a load it may alias.  The reads of a stage never touch the image in flight: the barriers order them.
typedef unsigned cls8_u32x4 __attribute__((ext_vector_type(4)));
template <bool TYPED>
__device__ __forceinline__ uint4 cls8_lds_q(const void* p) {
  if constexpr (TYPED) {
    const cls8_u32x4 v = *reinterpret_cast<const cls8_u32x4*>(p);
    return make_uint4(v.x, v.y, v.z, v.w);
  } else {
    return *reinterpret_cast<const uint4*>(p);
  }
}

// The epilogue of a tile of igemm_cls8_lean_kernel whose 8 x 8 x 16 output block lies wholly inside the tensor (the body tests
// that once per tile): bf16 rows, Co and the add's channels multiples of 8 (host: cls8_lean).  The value path is
// epilogue_vec16's - accumulator block -> the wave's transposition tile -> float4 of 4 channels x 4 row slots per lane -> bias
// -> nl_apply of the add -> accumulate, on the same lanes - and so are the statistics sums: k = 0 ... 3 per lane, the xor
// tree over 8, 16, 32, per class, then tsum += over the classes.  What differs:
//   * the lane's four row-slot offsets are worked out once per tile: class (pz, py, px) moves a wave-uniform base by
//     pz osd + py osh + px osw, and the lane term is the interior row_off of epilogue_vec16 at TY = 4 with doubled strides
//     (x = 4 (k & 1) + (lane >> 3 & 3), y one of two compile-time values by lane bit 5); a second set from the add's strides,
//     which may be a slice of a wider tensor.  No decode, bound or clamp: every row of every class is inside;
//   * the fused-add / accumulate operands of class c + AHEAD are requested before class c is finished, raw (converted when
//     used: a conversion behind the load would wait for it), ADD and ACC compile-time so that a slot holds what the call reads;
//   * 16-byte stores: each lane rounds its 4 channels x 4 row slots as st4_t<true> does, then lanes l and l ^ 1 - channels
//     8 m ... 8 m + 3 and 8 m + 4 ... 8 m + 7 of the same rows - swap halves: the even lane ends with all 8 channels of row
//     slots 0 and 2, the odd one with those of slots 1 and 3.  Two stores per class and lane instead of four.  The column
//     mask is per 4 channels; with Co % 8 == 0 both lanes of a pair agree, which the host gate guarantees;
//   * no statistics arithmetic or shuffles when the call asks for no statistics rows (every input gradient).
// The squares are spelled as the fused multiply-add hipcc's contraction makes of `ssq += v * v` in epilogue_vec16, with
// implicit contraction off, as in chan_mfma_body.h (tests/test_hip_cls8_lean_epilogue.py compares the rows bit for bit).
template <bool ADD, bool ACC>
__device__ __forceinline__ void epilogue_cls8_lean_t(const GArgs& a, const float* biasp, f32x16 (&acc)[8], float* tr, int lane, int wave,
                                                     int colbase, bool colact, int n, int gz0, int gy0, int gx0, float (&tsum)[4],
                                                     float (&tsq)[4]) {
  constexpr int AHEAD = (ADD && ACC) ? 1 : 3;      // classes whose operands are in flight ahead of the one being finished
  const int osd = (int)a.osd, osh = (int)a.osh, osw = (int)a.osw, asd = (int)a.asd, ash_ = (int)a.ash, asw = (int)a.asw;
  const int h = lane >> 5, r = lane & 31;
  const int rsub = lane >> 3, c4 = (lane & 7) * 4;
  const int colv = colbase + c4;
  const bool cvok = colact && colv < a.Co;                 // Co % 8 == 0: lanes l and l ^ 1 agree
  const int colc = min(colv, a.Co - 4);
  float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float asc[4] = {1.f, 1.f, 1.f, 1.f}, ash[4] = {0.f, 0.f, 0.f, 0.f};
  if (biasp) bias4 = *reinterpret_cast<const float4*>(biasp + colc);
  if constexpr (ADD) nl_coeff_vec<4>(a.tadd, n, a.Co, colc, asc, ash);
  // ---- addresses, once per tile: 32-bit lane offsets in BYTES (an item has < 2^31 elements) beside 64-bit wave-uniform bases:
  // the loads and stores take the scalar-base + 32-bit-offset form, no 64-bit vector arithmetic
  const bool lb = (rsub >> 2) != 0, odd = (lane & 1) != 0;
  constexpr int T = 0xEB14;                                // row_to_local's y table
  unsigned lo[4], la[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y0 = (T >> (2 * (2 * k))) & 3, y1 = (T >> (2 * (2 * k + 1))) & 3, x2 = 2 * (4 * (k & 1) + (rsub & 3));
    lo[k] = (unsigned)((lb ? 2 * y1 : 2 * y0) * osh + x2 * osw + colc) * 2u;
    la[k] = (unsigned)((lb ? 2 * y1 : 2 * y0) * ash_ + x2 * asw + colc) * 2u;
  }
  // the even lane stores row slots 0 and 2 from its own first channel, the odd lane slots 1 and 3 from its neighbour's
  const unsigned lst[2] = {odd ? lo[1] - 8u : lo[0], odd ? lo[3] - 8u : lo[2]};
  char* const outh = reinterpret_cast<char*>(reinterpret_cast<unsigned short*>(a.out) + ((long long)n * a.osn + (long long)(2 * (gz0 + wave)) * osd +
                                                                               (long long)(2 * gy0) * osh + (long long)(2 * gx0) * osw));
  const char* const addh = reinterpret_cast<const char*>(reinterpret_cast<const unsigned short*>(a.add) + ((long long)n * a.asn + (long long)(2 * (gz0 + wave)) * asd +
                                                                                           (long long)(2 * gy0) * ash_ + (long long)(2 * gx0) * asw));
  uint2 qa[AHEAD + 1][4], qo[AHEAD + 1][4];
  auto request = [&](auto cc) {
    constexpr int c = decltype(cc)::value, s = c % (AHEAD + 1), pz = (c >> 2) & 1, py = (c >> 1) & 1, px = c & 1;
    if constexpr (ADD) {
      const char* const p = addh + 2 * (pz * asd + py * ash_ + px * asw);
#pragma unroll
      for (int k = 0; k < 4; ++k) qa[s][k] = *reinterpret_cast<const uint2*>(p + la[k]);
    }
    if constexpr (ACC) {
      const char* const p = outh + 2 * (pz * osd + py * osh + px * osw);
#pragma unroll
      for (int k = 0; k < 4; ++k) qo[s][k] = *reinterpret_cast<const uint2*>(p + lo[k]);
    }
  };
  static_for<0, AHEAD>([&](auto cc) { request(cc); });
  static_for<0, 8>([&](auto cc) {
    constexpr int c = decltype(cc)::value, s = c % (AHEAD + 1), pz = (c >> 2) & 1, py = (c >> 1) & 1, px = c & 1;
    if constexpr (c + AHEAD < 8) request(std::integral_constant<int, c + AHEAD>{});
#pragma unroll
    for (int i = 0; i < 16; ++i) tr[((i & 3) + 8 * (i >> 2) + 4 * h) * 36 + r] = acc[c][i];
    float v[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4 val = *reinterpret_cast<const float4*>(tr + (rsub + 8 * k) * 36 + c4);
      v[k][0] = val.x + bias4.x; v[k][1] = val.y + bias4.y; v[k][2] = val.z + bias4.z; v[k][3] = val.w + bias4.w;
    }
    unsigned pk[4][2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if constexpr (ADD) {
        const uint2 u = qa[s][k];
        const float av[4] = {bf16_bits_to_f32(u.x & 0xffffu), bf16_bits_to_f32(u.x >> 16), bf16_bits_to_f32(u.y & 0xffffu),
                             bf16_bits_to_f32(u.y >> 16)};
#pragma unroll
        for (int j = 0; j < 4; ++j) v[k][j] += nl_apply(av[j], asc[j], ash[j], a.tadd.relu);
      }
      if constexpr (ACC) {
        const uint2 u = qo[s][k];
        v[k][0] += bf16_bits_to_f32(u.x & 0xffffu); v[k][1] += bf16_bits_to_f32(u.x >> 16);
        v[k][2] += bf16_bits_to_f32(u.y & 0xffffu); v[k][3] += bf16_bits_to_f32(u.y >> 16);
      }
      pk[k][0] = f32x2_to_bf16x2(v[k][0], v[k][1]);
      pk[k][1] = f32x2_to_bf16x2(v[k][2], v[k][3]);
    }
    // rows (k, k + 1): the even lane gives its half of row k + 1 for the odd lane's half of row k
    char* const po = outh + 2 * (pz * osd + py * osh + px * osw);
    uint4 q[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const unsigned s0 = odd ? pk[2 * p][0] : pk[2 * p + 1][0], s1 = odd ? pk[2 * p][1] : pk[2 * p + 1][1];
      const unsigned n0 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)s0, 0xb1, 0xf, 0xf, true);      // lane ^ 1
      const unsigned n1 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)s1, 0xb1, 0xf, 0xf, true);
      q[p] = odd ? make_uint4(n0, n1, pk[2 * p + 1][0], pk[2 * p + 1][1]) : make_uint4(pk[2 * p][0], pk[2 * p][1], n0, n1);
    }
    if (cvok) {
      *reinterpret_cast<uint4*>(po + lst[0]) = q[0];
      *reinterpret_cast<uint4*>(po + lst[1]) = q[1];
    }
    if (a.stats != nullptr) {
#pragma clang fp contract(off)
      float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
      if (cvok) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int j = 0; j < 4; ++j) { ssum[j] += v[k][j]; ssq[j] = fmaf(v[k][j], v[k][j], ssq[j]); }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int o = 8; o < 64; o <<= 1) { ssum[j] += __shfl_xor(ssum[j], o, 64); ssq[j] += __shfl_xor(ssq[j], o, 64); }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) { tsum[j] += ssum[j]; tsq[j] += ssq[j]; }
    }
  });
}

template <bool ABF>
__device__ __forceinline__ void epilogue_cls8_lean(const GArgs& a, const float* biasp, f32x16 (&acc)[8], float* tr, int lane, int wave,
                                                   int colbase, bool colact, int n, int gz0, int gy0, int gx0, float (&tsum)[4],
                                                   float (&tsq)[4]) {
  static_assert(ABF, "bf16 rows: a lane pair holds 16 bytes of one");
  // one wave-uniform choice per tile: a slot of operands in flight holds what the call reads and nothing else
  if (a.add != nullptr) {
    if (a.accumulate) epilogue_cls8_lean_t<true, true>(a, biasp, acc, tr, lane, wave, colbase, colact, n, gz0, gy0, gx0, tsum, tsq);
    else epilogue_cls8_lean_t<true, false>(a, biasp, acc, tr, lane, wave, colbase, colact, n, gz0, gy0, gx0, tsum, tsq);
  } else {
    if (a.accumulate) epilogue_cls8_lean_t<false, true>(a, biasp, acc, tr, lane, wave, colbase, colact, n, gz0, gy0, gx0, tsum, tsq);
    else epilogue_cls8_lean_t<false, false>(a, biasp, acc, tr, lane, wave, colbase, colact, n, gz0, gy0, gx0, tsum, tsq);
  }
}

template <int KCI, bool ABF>
__global__ __launch_bounds__(256, 2) void igemm_cls8_kernel(GArgs a) {
  constexpr bool RAW = false, PIPE = false, LEAN = false;
#include "conv_igemm_cls8_body.h"
}

// ... for a bf16-stored input that takes no norm-on-load (raw staging, igemm_raw_kernel above): no sc / sh[AIT][8] live
// across the requests of a stage
template <int KCI, bool ABF>      // (ABF always true: see igemm_reuse_raw_kernel)
__global__ __launch_bounds__(256, 2) void igemm_cls8_raw_kernel(GArgs a) {
  constexpr bool RAW = true, PIPE = false, LEAN = false;
#include "conv_igemm_cls8_body.h"
}

// ... and with the K loop pipelined (MMTTA_OPT_CLS8_PIPELINE; host: cls8_pipelined): two weight images in LDS, the image of
// stage k + 1 fetched by direct global-to-LDS loads while stage k multiplies, the box items of stage k + 1 requested a stage
// ahead.  No register holds the weights on their way, so the prefetch costs none across the MFMA phase - what the register
// pipeline of round 3 could not afford beside 8 accumulator blocks.  Same products in the same order, same epilogue.
template <int KCI, bool ABF>      // (ABF always true)
__global__ __launch_bounds__(256, 2) void igemm_cls8_pipe_kernel(GArgs a) {
  constexpr bool RAW = true, PIPE = true, LEAN = false;
#include "conv_igemm_cls8_body.h"
}

// ... and with an epilogue of its own for the tiles inside the tensor (MMTTA_OPT_CLS8_LEAN_EPILOGUE; host: cls8_lean;
// epilogue_cls8_lean above).  The K loop is the pipelined kernel's, and so is the epilogue of a tile on the border.
template <int KCI, bool ABF>      // (ABF always true)
__global__ __launch_bounds__(256, 2) void igemm_cls8_lean_kernel(GArgs a) {
  constexpr bool RAW = true, PIPE = true, LEAN = true;
#include "conv_igemm_cls8_body.h"
}

template <int KCI, bool ABF, bool RAW = false, bool PIPE = false, bool LEAN = false>
static int launch_cls8_t(const GArgs& a, int tiles, hipStream_t s) {
  static_assert(!LEAN || PIPE, "the lean epilogue belongs to the pipelined kernel");
  constexpr int VS = KCI + 8;
  // the box image and the stage's weight image (PIPE: two of them; 69 696 bytes at KCI = 16, two workgroups per CU still)
  size_t lds = ((size_t)(5 * 5 * LDS_PITCH_BF16 * VS + 7) / 8 * 8) * 2 + (size_t)(PIPE ? 2 : 1) * 27 * (KCI / 8) * 32 * 16;
  const size_t epi = (4 * EPI_TILE_FLOATS + 4 * 2 * 32) * sizeof(float);
  if (lds < epi) lds = epi;
  void (*kern)(GArgs) = igemm_cls8_kernel<KCI, ABF>;
  if constexpr (RAW && !PIPE) kern = igemm_cls8_raw_kernel<KCI, ABF>;
  if constexpr (PIPE && !LEAN) kern = igemm_cls8_pipe_kernel<KCI, ABF>;
  if constexpr (LEAN) kern = igemm_cls8_lean_kernel<KCI, ABF>;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set = true;
  }
  hipLaunchKernelGGL(kern, dim3(tiles, a.Np / 32), dim3(256), lds, s, a);
  return launch_status("conv igemm (class-fused stride-2 form)");
}

// Reduce split-K slabs: sum over splits, then the same epilogue as above.
// grid (tiles * MT/32, ceil(Np/32)); 256 threads = 8 row lanes x 32 columns, 4 rows per thread, i.e. one
// block per 32 rows x 32 columns; each block writes ONE statistics row (rows per tile = MT/32).
template <int TZ, int TY, int TX, bool PERM, bool ABF = false>
__global__ __launch_bounds__(256) void splitk_finalize_kernel(GArgs a, int tiles) {
  __shared__ float red[2][8][32];
  constexpr int MT = TZ * TY * TX;
  constexpr int RB = MT / 32;
  const int tid = threadIdx.x, r = tid & 31, rg = tid >> 5;
  const int tile = blockIdx.x / RB, rb = blockIdx.x % RB;
  int cidx, t;
  class_of_tile(a, tile, cidx, t);
  const ClassInfo ci = a.cls[cidx];
  const int tile_in_n = t % (a.tz * a.ty * a.tx);
  const int txi = t % a.tx; t /= a.tx;
  const int tyi = t % a.ty; t /= a.ty;
  const int tzi = t % a.tz;
  const int n = t / a.tz;
  const int col = blockIdx.y * 32 + r;
  const bool colok = col < a.Co;
  float bias = 0.f, asc = 1.f, ash = 0.f;
  if (colok) {
    const float* biasn = pset_bias(a.ps, a.bias, n);
    if (biasn) bias = biasn[col];
    if (a.add) nl_coeff(a.tadd, n, a.Co, col, asc, ash);
  }
  float s_sum = 0.f, s_sq = 0.f;
  // the thread's 4 rows advance together: every load is unconditional (clamped address) and independent
  const int colc = min(col, a.Co - 1);
  const long long kstride = (long long)tiles * MT * a.Np;
  const float* wsp[4];
  long long ooff[4], aoff[4];
  bool ok[4];
  float s4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int v = rb * 32 + rg * 4 + q;
    int zl, yl, xl;
    row_to_local<TZ, TY, TX, PERM>(v, zl, yl, xl);
    const int gz = tzi * TZ + zl, gy = tyi * TY + yl, gx = txi * TX + xl;
    const int oz = gz * a.so + ci.oz, oy = gy * a.so + ci.oy, ox = gx * a.so + ci.ox;
    ok[q] = colok && gz < ci.Dg && gy < ci.Hg && gx < ci.Wg && oz < a.Do && oy < a.Ho && ox < a.Wo;
    const int cz = min(oz, a.Do - 1), cy = min(oy, a.Ho - 1), cx = min(ox, a.Wo - 1);
    ooff[q] = (long long)n * a.osn + cz * a.osd + cy * a.osh + cx * a.osw + colc;
    aoff[q] = (long long)n * a.asn + cz * a.asd + cy * a.ash + cx * a.asw + colc;
    wsp[q] = a.ws + ((long long)tile * MT + v) * a.Np + min(col, a.Np - 1);
  }
  for (int kz = 0; kz < a.ksplit; kz += 4) {        // 4 splits x 4 rows = 16 independent loads per trip
    float v[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q][u] = wsp[q][(long long)min(kz + u, a.ksplit - 1) * kstride];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) s4[q] += kz + u < a.ksplit ? v[q][u] : 0.f;
  }
  float addv[4] = {0.f, 0.f, 0.f, 0.f}, oldv[4] = {0.f, 0.f, 0.f, 0.f};
  if (a.add) {
#pragma unroll
    for (int q = 0; q < 4; ++q) addv[q] = ld1_t<ABF>(a.add, aoff[q]);
  }
  if (a.accumulate) {
#pragma unroll
    for (int q = 0; q < 4; ++q) oldv[q] = ld1_t<ABF>(a.out, ooff[q]);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float val = s4[q] + bias;
    if (a.add) val += nl_apply(addv[q], asc, ash, a.tadd.relu);
    if (a.accumulate) val += oldv[q];
    if (ok[q]) {
      st1_t<ABF>(a.out, ooff[q], val);
      s_sum += val;
      s_sq += val * val;
    }
  }
  if (a.stats != nullptr) {
    red[0][rg][r] = s_sum;
    red[1][rg][r] = s_sq;
    __syncthreads();
    if (rg == 0 && colok) {
      float ts = 0.f, tq = 0.f;
#pragma unroll
      for (int g = 0; g < 8; ++g) { ts += red[0][g][r]; tq += red[1][g][r]; }
      const long long row = (long long)n * a.stats_rows_per_n + (cidx * (a.tz * a.ty * a.tx) + tile_in_n) * RB + rb;
      a.stats[(row * 2 + 0) * a.Co + col] = ts;
      a.stats[(row * 2 + 1) * a.Co + col] = tq;
    }
  }
}

// ---------------------------------------------------------------- weight packing
// torch layout W[A][B][T] (A = dim0, B = dim1, T = k^3 taps) -> P[T][Kp][Np]
// kn_is_ba: K = B, N = A (Conv3d forward, ConvTranspose3d input gradient)
// else    : K = A, N = B (Conv3d input gradient, ConvTranspose3d forward)
// W'[d][k][(p, co)] of the 2x2x2 gather-GEMM up-convolution (conv_direct.hip): tap (kz, ky, kx) of a k3 s2 transposed
// convolution belongs to exactly one (coarse offset d, output parity p) pair - per axis k = 1: (p 0, d 0); k = 0: (p 1, d 1);
// k = 2: (p 1, d 0) - the image is in MFMA B-fragment order (lane = 32 * ((k >> 3) & 1) + column, 8 k per lane), bf16; the
// 37 slots no tap owns are written as zeros.  One call writes the 64 (d, p) entries of one (input channel k, output channel
// co) pair; `src` = that pair's 27 taps (null: a padded output channel, all zeros).
__device__ __forceinline__ void upconv8_put_pair(unsigned short* img, int K, int k, int co, const float* src) {
  for (int dp = 0; dp < 64; ++dp) {
    const int d = dp >> 3, p = dp & 7;
    int tap = 0;
    bool owned = true;
#pragma unroll
    for (int ax = 2; ax >= 0; --ax) {                       // z, y, x: (p 0, d 0) -> k 1; (p 1, d 1) -> k 0; (p 1, d 0) -> k 2
      const int pa = (p >> ax) & 1, da = (d >> ax) & 1;
      owned = owned && !(pa == 0 && da == 1);
      tap = tap * 3 + (pa == 0 ? 1 : (da == 1 ? 0 : 2));
    }
    const float v = (owned && src != nullptr) ? src[tap] : 0.f;
    img[(((d * (K >> 4) + (k >> 4)) * 64 + ((k >> 3) & 1) * 32 + p * 4 + co) << 3) + (k & 7)] =
        (unsigned short)(f32x2_to_bf16x2(v, 0.f) & 0xffffu);
  }
}

// the whole W' image of one ConvTranspose3d weight [K][N][27] (single-layer pack path)
__global__ void pack_upconv8_kernel(const float* __restrict__ w, unsigned short* __restrict__ img, int K, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K * 4) return;
  const int k = i >> 2, co = i & 3;
  upconv8_put_pair(img, K, k, co, co < N ? w + ((long long)k * N + co) * 27 : nullptr);
}

__global__ void pack_weights_kernel(const float* __restrict__ w, float* __restrict__ p, int A, int B, int T,
                                    int Kp, int Np, int kn_is_ba) {
  const long long total = (long long)T * Kp * Np;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int nn = (int)(i % Np);
    const int k = (int)((i / Np) % Kp);
    const int tp = (int)(i / ((long long)Np * Kp));
    const int K = kn_is_ba ? B : A, N = kn_is_ba ? A : B;
    float v = 0.f;
    if (k < K && nn < N) {
      const int ai = kn_is_ba ? nn : k, bi = kn_is_ba ? k : nn;
      v = w[((long long)ai * B + bi) * T + tp];
    }
    p[i] = v;
  }
}

// bf16 image [T][Kp/8][Np][8]: a lane's MFMA B fragment (8 consecutive k for one column) is one 16-byte load
__global__ void pack_weights_bf16_kernel(const float* __restrict__ w, unsigned short* __restrict__ p, int A, int B, int T,
                                         int Kp, int Np, int kn_is_ba) {
  const long long total = (long long)T * Kp * Np;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(i & 7);
    const int nn = (int)((i >> 3) % Np);
    const int k8 = (int)((i / (8LL * Np)) % (Kp / 8));
    const int tp = (int)(i / ((long long)Kp * Np));
    const int k = k8 * 8 + j;
    const int K = kn_is_ba ? B : A, N = kn_is_ba ? A : B;
    float v = 0.f;
    if (k < K && nn < N) {
      const int ai = kn_is_ba ? nn : k, bi = kn_is_ba ? k : nn;
      v = w[((long long)ai * B + bi) * T + tp];
    }
    p[i] = __builtin_bit_cast(unsigned short, (__bf16)v);
  }
}

// All packed images of a model in ONE launch: a device table of entries; a workgroup finds its entry by
// binary search over the prefix sums of the entries' workgroup counts (uniform, scalar).
//
// A packed image is a transpose of the torch weight (taps innermost there, outermost here), so a workgroup
// moves one 8 (k) x 32 (n) x T tile through LDS: coalesced runs of the master in, 128-byte (fp32: one n row)
// or 512-byte (bf16: 32 n x 8 k) runs of the image out.  ~155 MB per U-Net repack: HBM-bound.
struct PackEntry {
  const float* w; void* p;
  unsigned short* up8;      // fragment-ordered bf16 image of the gather-GEMM up-convolution (or null)
  uint4* chfr; int KI, NO;  // B-fragment image of the thin-K matrix-core convolution (or null), its actual K and N
  int A, B, T, Kp, Np, kn_is_ba, bf16, direct;
  long long start;   // first workgroup of this entry
};

constexpr int PK = 8, PN = 32;

template <int T>
__device__ __forceinline__ void pack_tile(const PackEntry& e, int lb, float* tile) {
  const int tiles_n = e.Np / PN;
  const int k0 = (lb / tiles_n) * PK, n0 = (lb % tiles_n) * PN;
  const int K = e.kn_is_ba ? e.B : e.A, N = e.kn_is_ba ? e.A : e.B;
  constexpr int RS = PK * T + 1;                 // row stride of the [n][k*T+tap] staging (odd: no bank conflicts)
  // PN*PK*T is a multiple of 256 (6912 = 27 * 256, 256): U loads are issued before the first one is stored (one load per
  // trip left the workgroup waiting 27 memory latencies in a row)
  constexpr int IT = PN * PK * T / 256, U = IT % 9 == 0 ? 9 : 1;
  static_assert(PN * PK * T % 256 == 0, "pack tile: whole trips");
  // full 27-tap tiles whose runs start on 16 bytes (B a multiple of 4: every wide layer): the runs are read as float4,
  // 7 loads per thread instead of 27 and a quarter of the index arithmetic (the kernel was vector-ALU bound on it)
  constexpr int RUN4 = (T == 27) ? PK * T / 4 : 1;            // float4 per n-run (kn_is_ba) = 54
  const bool full = T == 27 && k0 + PK <= K && n0 + PN <= N && e.B % 4 == 0 && ((uintptr_t)e.w) % 16 == 0;
  if (T == 27 && full) {
    constexpr int N4 = PN * PK * T / 4, IT4 = (N4 + 255) / 256;      // 1728 float4, 7 trips (the last one partial)
    float4 v[IT4];
    if (e.kn_is_ba) {
#pragma unroll
      for (int u = 0; u < IT4; ++u) {
        const int i4 = min(u * 256 + (int)threadIdx.x, N4 - 1);
        const int nn = i4 / RUN4, r4 = i4 % RUN4;
        v[u] = *reinterpret_cast<const float4*>(e.w + ((long long)(n0 + nn) * e.B + k0) * T + r4 * 4);
      }
#pragma unroll
      for (int u = 0; u < IT4; ++u) {
        const int i4 = u * 256 + (int)threadIdx.x;
        if (i4 < N4) {
          const int nn = i4 / RUN4, r4 = i4 % RUN4;
          float* d = tile + nn * RS + r4 * 4;                 // RS is odd: four 4-byte stores
          d[0] = v[u].x; d[1] = v[u].y; d[2] = v[u].z; d[3] = v[u].w;
        }
      }
    } else {
      constexpr int KRUN4 = PN * T / 4;                       // float4 per k-run = 216
#pragma unroll
      for (int u = 0; u < IT4; ++u) {
        const int i4 = min(u * 256 + (int)threadIdx.x, N4 - 1);
        const int kk = i4 / KRUN4, r4 = i4 % KRUN4;
        v[u] = *reinterpret_cast<const float4*>(e.w + ((long long)(k0 + kk) * e.B + n0) * T + r4 * 4);
      }
#pragma unroll
      for (int u = 0; u < IT4; ++u) {
        const int i4 = u * 256 + (int)threadIdx.x;
        if (i4 < N4) *reinterpret_cast<float4*>(tile + i4 * 4) = v[u];
      }
    }
  } else
  if (e.kn_is_ba) {                              // a = n, b = k: per n a run of PK*T contiguous floats
    for (int it = 0; it < IT; it += U) {
      float v[U]; int dst[U]; bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = (it + u) * 256 + threadIdx.x;
        const int nn = idx / (PK * T), r = idx % (PK * T);
        const int kk = r / T;
        // unconditional load from a clamped address, masked afterwards (a load behind a branch is waited for at once)
        ok[u] = n0 + nn < N && k0 + kk < K;
        v[u] = e.w[((long long)min(n0 + nn, N - 1) * e.B + min(k0 + kk, K - 1)) * T + (r - kk * T)];
        dst[u] = nn * RS + r;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) tile[dst[u]] = ok[u] ? v[u] : 0.f;
    }
  } else {                                       // a = k, b = n: per k a run of PN*T contiguous floats
    for (int it = 0; it < IT; it += U) {
      float v[U]; bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = (it + u) * 256 + threadIdx.x;
        const int kk = idx / (PN * T), r = idx % (PN * T);
        const int nn = r / T;
        ok[u] = k0 + kk < K && n0 + nn < N;
        v[u] = e.w[((long long)min(k0 + kk, K - 1) * e.B + min(n0 + nn, N - 1)) * T + (r - nn * T)];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) tile[(it + u) * 256 + threadIdx.x] = ok[u] ? v[u] : 0.f;
    }
  }
  __syncthreads();
  const long long slab = (long long)e.Kp * e.Np;
  if (e.bf16) {
    for (int o = threadIdx.x; o < T * PN; o += 256) {
      const int nn = o % PN, tp = o / PN;
      unsigned short h[8];
#pragma unroll
      for (int kk = 0; kk < PK; ++kk) {
        const float v = e.kn_is_ba ? tile[nn * RS + kk * T + tp] : tile[kk * (PN * T) + nn * T + tp];
        h[kk] = f32_to_bf16_bits(v);
      }
      *reinterpret_cast<uint4*>((unsigned short*)e.p + tp * slab + ((long long)(k0 >> 3) * e.Np + n0 + nn) * 8) = bf16x8_pack(h);
    }
  } else {
    for (int o = threadIdx.x; o < T * PK * PN; o += 256) {
      const int nn = o % PN, kk = (o / PN) % PK, tp = o / (PN * PK);
      const float v = e.kn_is_ba ? tile[nn * RS + kk * T + tp] : tile[kk * (PN * T) + nn * T + tp];
      ((float*)e.p)[tp * slab + (long long)(k0 + kk) * e.Np + n0 + nn] = v;
    }
  }
}

// B fragments of the thin-K matrix-core convolution from the layer's fp32 tap image [27][Kp][Np] (conv_direct.hip:
// chan_frag_bytes has the layout).  Runs behind the kernel that wrote the tap image.
__device__ __forceinline__ void chan_frags_write(const float* img, uint4* fr, int Kp, int Np, int KI, int N) {
  const int NB = N / 32;
  for (int i = threadIdx.x; i < 7 * NB * 64; i += blockDim.x) {
    const int lane = i & 63, frn = i >> 6, s2 = frn / NB, nb = frn % NB;
    const int h = lane >> 5, col = nb * 32 + (lane & 31);
    float wv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int tap = s2 * 4 + h * 2 + (e >> 2), c = e & 3;
      wv[e] = (tap < 27 && c < KI && col < N) ? img[((long long)tap * Kp + c) * Np + col] : 0.f;
    }
    uint4 pk;
    pk.x = f32x2_to_bf16x2(wv[0], wv[1]); pk.y = f32x2_to_bf16x2(wv[2], wv[3]);
    pk.z = f32x2_to_bf16x2(wv[4], wv[5]); pk.w = f32x2_to_bf16x2(wv[6], wv[7]);
    fr[i] = pk;
  }
}
__global__ __launch_bounds__(256) void pack_chan_frags_kernel(const float* img, uint4* fr, int Kp, int Np, int KI, int N) {
  chan_frags_write(img, fr, Kp, Np, KI, N);
}
__global__ __launch_bounds__(256) void pack_chan_frags_batched_kernel(const PackEntry* __restrict__ tab) {
  const PackEntry e = tab[blockIdx.x];
  if (e.chfr != nullptr) chan_frags_write((const float*)e.p, e.chfr, e.Kp, e.Np, e.KI, e.NO);
}

__global__ __launch_bounds__(256) void pack_batched_kernel(const PackEntry* __restrict__ tab, int count) {
  __shared__ __attribute__((aligned(16))) float tile[PN * (PK * 27 + 1)];
  int lo = 0, hi = count - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].start <= (long long)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const PackEntry e = tab[lo];
  const int lb = (int)(blockIdx.x - e.start);
  if (e.direct) {
    // [T][K][4] fp32 image of a direct-convolution layer: a few KB, one position per thread
    const int li = lb * 256 + threadIdx.x;
    if (li >= e.Kp * e.Np) return;
    const int nn = li % e.Np, k = li / e.Np;
    const int N = e.kn_is_ba ? e.A : e.B;
    const int ai = e.kn_is_ba ? nn : k, bi = e.kn_is_ba ? k : nn;
    const float* src = e.w + ((long long)ai * e.B + bi) * e.T;
    for (int tp = 0; tp < e.T; ++tp)
      ((float*)e.p)[(long long)tp * e.Kp * e.Np + li] = nn < N ? src[tp] : 0.f;
    if (e.up8 != nullptr) upconv8_put_pair(e.up8, e.Kp, k, nn, nn < N ? src : nullptr);      // + the gather-GEMM image W'
    return;
  }
  if (e.T == 27) pack_tile<27>(e, lb, tile);
  else pack_tile<1>(e, lb, tile);
}


// ------------------------------------------------------------------ streaming 1x1x1 convolution (bf16 operands, round 3)
// The 1x1x1 layers of the deep-fusion decoder at full resolution (33 -> 32 shortcut convolutions and their input gradients at
// 128^3, 96 -> 64 at 64^3) ran on the gather GEMM above: LDS box, barriers and a 27-tap tile shape for what is a [voxels x K] x
// [K x N] product - 3.3 to 9 times their HBM time.  Without taps there is nothing to share between voxels, so nothing goes
// through LDS: lane (r, h) of a wave loads the 8 channels k16 * 16 + 8 h .. + 7 of voxel r STRAIGHT into its A fragment (one
// 16-byte load of bf16, two of fp32), the B fragments of all k steps sit in registers for the whole launch (K <= 128, N <=
// 64), and a wave owns 32 voxels per trip.  Epilogue as in chan_mfma_kernel: bias, fused add (with its norm-on-load),
// accumulate, bf16 rows stored as channel-pair dwords.  No statistics, no norm-on-load of the input: those calls stay above.
struct PWArgs {
  const float* in; long long isn; unsigned isw; int Ci;       // voxel-dense tensors: element offset of voxel v = v * sw
  float* out; long long osn; unsigned osw; int Co;
  const float* add; long long asn; unsigned asw; NL tadd;
  const float* wp; const float* bias; int Np; PSets ps;
  int accumulate; long long dhw;
};

template <int KB, int NB, bool BF>
__global__ __launch_bounds__(256) void pointwise_mfma_kernel(PWArgs a) {
  constexpr int TP = NB * 32 + 4;                     // tile row pitch (floats): 16-byte rows, conflict-free column writes
  __shared__ __attribute__((aligned(16))) float tile[4][32][TP];
  __shared__ float coef[3][NB * 32];                  // bias | scale, shift of the fused add, per output column
  const int n = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, r = lane & 31;
  const float* wpn = pset_packed(a.ps, a.wp, n);
  const float* biasn = pset_bias(a.ps, a.bias, n);
  uint4 bfr[KB][NB];
  {
    const uint4* wq = reinterpret_cast<const uint4*>(wpn);            // [Kp / 8][Np] entries of 8 bf16
#pragma unroll
    for (int ks = 0; ks < KB; ++ks)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) bfr[ks][nb] = wq[(long long)(ks * 2 + h) * a.Np + nb * 32 + r];
  }
  if (tid < NB * 32) {
    const int col = min(tid, a.Co - 1);
    float sc = 1.f, sh = 0.f;
    if (a.add) nl_coeff(a.tadd, n, a.Co, col, sc, sh);
    coef[0][tid] = (biasn && tid < a.Co) ? biasn[col] : 0.f;
    coef[1][tid] = sc; coef[2][tid] = sh;
  }
  __syncthreads();
  const float* inn = item_base<BF>(a.in, n, a.isn);
  float* outn = const_cast<float*>(item_base<BF>(a.out, n, a.osn));
  const float* addn = a.add == nullptr ? nullptr : item_base<BF>(a.add, n, a.asn);
  const float relu_lo = act_lo(a.tadd.relu);
  // every wave makes the same number of trips (a wave past the end works on clamped voxels and stores nothing): the tile
  // hand-over below needs no more than the wave's own program order
  for (long long base = (long long)blockIdx.x * 128; base < a.dhw; base += (long long)gridDim.x * 128) {
    const long long v0 = base + wave * 32;
    const unsigned vo = (unsigned)min(v0 + r, a.dhw - 1) * a.isw;
    uint4 af[KB];
#pragma unroll
    for (int ks = 0; ks < KB; ++ks) {
      const unsigned c0 = ks * 16 + h * 8;
      if (c0 + 8 <= a.isw) {          // (rows are padded to 8 channels; what lies behind the row is not read)
        if constexpr (BF) {
          af[ks] = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(inn) + vo + c0);
        } else {
          const float4 lo = *reinterpret_cast<const float4*>(inn + vo + c0), hi = *reinterpret_cast<const float4*>(inn + vo + c0 + 4);
          af[ks] = make_uint4(f32x2_to_bf16x2(lo.x, lo.y), f32x2_to_bf16x2(lo.z, lo.w), f32x2_to_bf16x2(hi.x, hi.y), f32x2_to_bf16x2(hi.z, hi.w));
        }
      } else if (!BF && c0 + 4 <= a.isw) {          // fp32 rows are padded to 4 channels
        const float4 lo = *reinterpret_cast<const float4*>(inn + vo + c0);
        af[ks] = make_uint4(f32x2_to_bf16x2(lo.x, lo.y), f32x2_to_bf16x2(lo.z, lo.w), 0u, 0u);
      } else {
        af[ks] = make_uint4(0u, 0u, 0u, 0u);
      }
      if ((int)c0 + 8 > a.Ci) {          // channels past the tensor's last one (a slice of a wider row, pad lanes): exact zeros
        auto pm = [&](int c) { return (c < a.Ci ? 0xffffu : 0u) | (c + 1 < a.Ci ? 0xffff0000u : 0u); };
        af[ks].x &= pm(c0); af[ks].y &= pm(c0 + 2); af[ks].z &= pm(c0 + 4); af[ks].w &= pm(c0 + 6);
      }
    }
    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KB; ++ks)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[ks]), __builtin_bit_cast(bf16x8, bfr[ks][nb]), acc[nb], 0, 0, 0);
    // ---- epilogue through the wave's LDS tile: accumulator i of lane (h, r) = voxel (i & 3) + 8 (i >> 2) + 4 h, column
    // nb * 32 + r goes in column-wise (conflict-free), comes back as 8 consecutive channels of one voxel per lane: the fused
    // add and the accumulate operand are one 16-byte load each, the result one 16-byte store
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) tile[wave][(i & 3) + 8 * (i >> 2) + 4 * h][nb * 32 + r] = acc[nb][i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int q = 0; q < 2 * NB; ++q) {
      const int item = lane + 64 * q, vl = item / (4 * NB), c8 = item % (4 * NB), c0 = c8 * 8;
      const long long vv = v0 + vl;
      if (vv < a.dhw && c0 < a.Co) {
        const float4 t0 = *reinterpret_cast<const float4*>(&tile[wave][vl][c0]), t1 = *reinterpret_cast<const float4*>(&tile[wave][vl][c0 + 4]);
        float v[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
        const bool full = c0 + 8 <= a.Co;
        const unsigned oo = (unsigned)vv * a.osw + c0;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += coef[0][c0 + e];
        if (a.add) {
          float ad[8];
          if (full || c0 + 8 <= (int)a.asw) {
            oct8_f8(oct8_ld<BF>(addn, (unsigned)vv * a.asw + c0, (unsigned)vv * a.asw + c0 + 4), ad);
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) ad[e] = c0 + e < a.Co ? ld1_t<BF>(addn, (unsigned)vv * a.asw + c0 + e) : 0.f;
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += act_max(fmaf(ad[e], coef[1][c0 + e], coef[2][c0 + e]), relu_lo);
        }
        if (full) {
          if (a.accumulate) {
            float old[8];
            oct8_f8(oct8_ld<BF>(outn, oo, oo + 4), old);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += old[e];
          }
          oct8_st<BF>(outn, oo, v);
        } else {                           // ragged last chunk: element stores, nothing behind the last channel is touched
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (c0 + e < a.Co) st1_t<BF>(outn, oo + e, a.accumulate ? v[e] + ld1_t<BF>(outn, oo + e) : v[e]);
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

template <int KB, bool BF>
static void launch_pointwise_mfma_nb(const PWArgs& a, int nb, dim3 grid, hipStream_t s) {
  if (nb == 1) hipLaunchKernelGGL((pointwise_mfma_kernel<KB, 1, BF>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((pointwise_mfma_kernel<KB, 2, BF>), grid, dim3(256), 0, s, a);
}
template <bool BF>
static void launch_pointwise_mfma(const PWArgs& a, int kb, int nb, dim3 grid, hipStream_t s) {
  switch (kb) {
    case 1: launch_pointwise_mfma_nb<1, BF>(a, nb, grid, s); break;
    case 2: launch_pointwise_mfma_nb<2, BF>(a, nb, grid, s); break;
    case 3: launch_pointwise_mfma_nb<3, BF>(a, nb, grid, s); break;
    case 4: launch_pointwise_mfma_nb<4, BF>(a, nb, grid, s); break;
    case 6: launch_pointwise_mfma_nb<6, BF>(a, nb, grid, s); break;
    default: launch_pointwise_mfma_nb<8, BF>(a, nb, grid, s); break;
  }
}

// ---------------------------------------------------------------- host side
struct Config { int NB, MB, TZ, TY, TX, KCI; bool bf; };

static inline int roundup(int v, int m) { return (v + m - 1) / m * m; }

static void op_dims(const mmtta_conv_desc* d, int& K, int& N, int& si, bool& classes) {
  switch (d->op) {
    case MMTTA_CONV_FWD: K = d->cin; N = d->cout; si = d->stride; classes = false; break;
    case MMTTA_CONV_DGRAD: K = d->cout; N = d->cin; si = 1; classes = d->stride == 2; break;
    case MMTTA_CONVT_FWD: K = d->cin; N = d->cout; si = 1; classes = true; break;
    default: K = d->cout; N = d->cin; si = 2; classes = false; break;  // CONVT_DGRAD
  }
}

static Config pick_config(int Np, int si, long long voxels, int K, bool bf) {
  // fp32 stage depth / bf16 stage depth (bf16 stages are multiples of the MFMA K = 16)
  if (si == 1) {
    if (Np == 32 && bf && g_igemm_lean) return {1, 2, 4, 8, 8, 16, bf};      // lean tile, four workgroups per CU
    if (Np == 32) return {1, 4, 8, 8, 8, bf ? 16 : 8, bf};
    // (128-voxel tiles for the 64-channel stride-1 layers as well - {2,2,4,4,8,16} - measured 64.6 against 65.2 volumes/s)
    if (Np == 64) return {2, 4, 4, 8, 8, bf ? 32 : 16, bf};
    // wide layers on a small grid (the 8^3 / 16^3 levels): shallow stages so that split-K can reach
    // >= 256 workgroups; otherwise 32-channel stages (fewer barriers, fewer weight fetches)
    const long long tiles = (voxels + 127) / 128, colgroups = (Np + 127) / 128;
    if (tiles * colgroups * ((K + 31) / 32) < 384) return {4, 4, 4, 4, 8, bf ? 16 : 8, bf};
    return {4, 4, 4, 4, 8, 32, bf};
  }
  if (Np == 32) return {1, 1, 4, 4, 8, bf ? 16 : 8, bf};
  // (the stride-2 64-column layers as two 32-column groups - twice the workgroups, the halo staged twice - measured 65.0
  // against 65.5 volumes/s)
  // (round 3: the 32 -> 64 layer at 64^3 fetches 3.6x its algorithmic bytes by the PMC count - two 16-channel stages each
  // touch half of every 64-byte voxel row of a 9 x 9 x 17 box that the L2 does not hold in between.  One 32-channel stage
  // on the same tile (110 KB of LDS: one workgroup per CU) 200 us against 124 per group of 8; on a 2 x 4 x 8 tile 146: the
  // launch is bound by its latency chain, not by the fabric)
  if (Np == 64) return {2, 2, 4, 4, 8, bf ? 16 : 8, bf};
  return {4, 4, 4, 4, 8, bf ? 16 : 8, bf};
}

// bf16 operands only where the reduction is deep enough for the K=16 MFMA and the layer is not on the
// direct (<= 4 produced channels) path; everything else computes in fp32 whatever desc.dtype says.
static bool use_bf16(const mmtta_conv_desc* d, int K) {
  return d->dtype == MMTTA_BF16 && K >= 16 && !direct_applicable(d);
}

static int validate_desc(const mmtta_conv_desc* d) {
  MMTTA_CHECK(d != nullptr, MMTTA_ERR_INVALID, "conv: null desc");
  MMTTA_CHECK(d->op >= 0 && d->op <= 3, MMTTA_ERR_INVALID, "conv: bad op %d", d->op);
  MMTTA_CHECK(d->ksize == 1 || d->ksize == 3, MMTTA_ERR_UNSUPPORTED, "conv: ksize %d (1 or 3)", d->ksize);
  MMTTA_CHECK(d->stride == 1 || d->stride == 2, MMTTA_ERR_UNSUPPORTED, "conv: stride %d (1 or 2)", d->stride);
  MMTTA_CHECK(!(d->ksize == 1 && d->stride != 1), MMTTA_ERR_UNSUPPORTED, "conv: 1x1x1 with stride 2");
  MMTTA_CHECK(d->cin > 0 && d->cout > 0, MMTTA_ERR_INVALID, "conv: channels must be positive");
  MMTTA_CHECK(d->dtype == MMTTA_F32 || d->dtype == MMTTA_BF16, MMTTA_ERR_UNSUPPORTED, "conv: dtype %d", d->dtype);
  if (d->op == MMTTA_CONVT_FWD || d->op == MMTTA_CONVT_DGRAD)
    MMTTA_CHECK(d->ksize == 3 && d->stride == 2, MMTTA_ERR_UNSUPPORTED,
                "conv_transpose: only k3 s2 p1 op1 (the monai UNet up layer)");
  return MMTTA_OK;
}

static int config_id(const Config& c) {
  int id;
  if (c.bf && c.NB == 1 && c.MB == 2) return 14;     // lean bf16 tile <1,2,4,8,8,16>
  if (c.NB == 1) id = c.MB == 4 ? 0 : 3;
  else if (c.NB == 2) id = c.MB == 4 ? 1 : 4;
  else id = c.KCI == 32 ? 2 : 5;
  return c.bf ? id + 7 : id;      // 7..12 = bf16 variants
}

// Which kernel a call runs: the values are the public ids (mmtta_conv_plan_t.config, mmtta_conv_route).  Every other value
// 0..14 is an implicit GEMM, config_id of its tile.
enum CRoute : int {
  C_DIRECT = 6,      // conv_direct.hip: <= 4 produced channels (direct_kernel names the variant, direct_conv_run launches it)
  C_THIN = 13,       // conv_direct.hip: thin-K kernels, <= 4 gathered channels into 32 / 64 (chan_kernel, chan_conv_run)
  C_CLS_FUSED = 15,  // igemm_cls8_kernel: the 8 parity classes of a stride-2 transposed form in one workgroup
  C_PW_SMALL = 16,   // pointwise_small_k_kernel: fp32 1x1x1 from <= 4 channels, nothing fused
  C_PW_MFMA = 17,    // pointwise_mfma_kernel: bf16 1x1x1 streamed over voxel-dense tensors
  C_IGEMM_REUSE = 18,  // igemm_reuse_kernel: config 14's tile for 3x3x3 stride-1 32 -> 32, activation fragments shared along x
};

// What a run knows beyond the shapes.  mmtta_conv_plan has none of it and plans the route of the shape (geometry: rt = null).
struct RunFacts {
  const float* stats; const mmtta_tensor* add; const mmtta_norm_on_load* x_norm;      // add: epi->add
  int accumulate;                      // (no route gate reads it today: the streaming kernels accumulate themselves)
  const float* bias;                   // the run's bias (mmtta_conv_route has none to show: null)
};

// The class-fused kernel of a call of route 15: each form is a special case of the one before it
enum Cls8Form : int {
  CLS8_TRANSFORM = 0,      // igemm_cls8_kernel: the norm-on-load applied while staging
  CLS8_RAW = 1,            // igemm_cls8_raw_kernel (raw_staging)
  CLS8_PIPELINED = 2,      // igemm_cls8_pipe_kernel (cls8_pipelined)
  CLS8_LEAN = 3,           // igemm_cls8_lean_kernel (cls8_lean)
};

struct Geometry {
  int route;      // CRoute
  int K, N, Kp, Np, si;
  bool classes;
  Config cfg;
  int tz, ty, tx, tiles_per_n, tiles, ncls;      // (class-fused: its own tiling, coarse 4 x 4 x 8, one statistics row per tile)
  int nstages, ksplit, sps;
  int stats_rows;              // rows of the partial-statistics slab the call writes
  int64_t workspace_bytes;     // split-K partial sums
  // ---- the variant of the route: what picks the kernel of a run.  plan_run fills these and the launchers read them; a plan
  // of the shapes alone (geometry with rt = null) leaves them cleared.
  bool leaky;                  // a LeakyReLU on x or on the fused add: the call runs in the leaky:: instantiation, which has
                               // none of the raw, pipelined, lean or head-loss kernels
  bool raw;                    // raw_staging
  int cls8;                    // Cls8Form (route 15)
  int thin_kernel;             // routes 6 and 13: the THIN_* id, or the negative status the launcher returns; 0 elsewhere
  int thin_lean;               // what mmtta_conv_thin_lean reports: 1 the thin-K convolution (route 13), 2 the up-convolution (6)
};

// Raw staging of the implicit-GEMM family (MMTTA_OPT_RAW_STAGING bit 0; igemm_raw_kernel, igemm_reuse_raw_kernel,
// igemm_cls8_raw_kernel): a bf16-stored x whose norm-on-load is the identity - none, or neither mean nor scale and no
// activation - in whole 8-channel chunks (no lane of a 16-byte item holds row padding or a neighbour's channel) that the
// kernels can read 16 bytes at a time, on a bf16-operand tile with y and the fused add bf16-stored like x.  plan_run asks
// it for the calls of the plain instantiation.
static bool raw_operand(const mmtta_tensor* x, const mmtta_norm_on_load* x_norm) {
  return is_bf16(x) && x->c % 8 == 0 && quad_aligned(x, 16, 8) &&
         (x_norm == nullptr || (x_norm->mean == nullptr && x_norm->scale == nullptr && x_norm->relu == MMTTA_ACT_NONE));
}
static bool raw_staging(const Geometry& g, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm, const mmtta_tensor* y,
                        const mmtta_tensor* add) {
  const bool igemm = g.route != C_DIRECT && g.route != C_THIN && g.route != C_PW_SMALL && g.route != C_PW_MFMA;
  return (g_raw_staging & 1) && igemm && g.cfg.bf && raw_operand(x, x_norm) && is_bf16(y) && (add == nullptr || is_bf16(add));
}

// The pipelined class-fused kernel (MMTTA_OPT_CLS8_PIPELINE; igemm_cls8_pipe_kernel): route 15 on a call that stages raw.
static bool cls8_pipelined(const Geometry& g) { return g_cls8_pipeline && g.route == C_CLS_FUSED && g.raw; }

// ... with the lean interior epilogue (MMTTA_OPT_CLS8_LEAN_EPILOGUE bit 0; igemm_cls8_lean_kernel): a pipelined call - so x, y
// and the add are bf16-stored - whose y and add have whole 8-channel groups: a lane pair stores 16 bytes of a row, and both
// lanes of a pair are live or dead together.  (cls_fused_operand has put y's rows and strides on 16 bytes.)
static bool cls8_lean(const mmtta_tensor* y, const mmtta_tensor* add) {
  return (g_cls8_lean_epilogue & 1) && y->c % 8 == 0 && (add == nullptr || add->c % 8 == 0);
}

static int expected_out_dim(const mmtta_conv_desc* d, int in) {
  switch (d->op) {
    case MMTTA_CONV_FWD: return d->stride == 1 ? in : (in + 1) / 2;
    case MMTTA_CONVT_FWD: return in * 2;
    case MMTTA_CONVT_DGRAD: return in / 2;
    default: return -1;  // CONV_DGRAD: caller gives dx shape (in*1 or in*2 or in*2-1)
  }
}

// ---- the gates of the routes (6, 16 and 13: direct_applicable, pointwise_small_applicable, chan_applicable of conv_direct.hip)
// 17: 1x1x1 over many voxels with bf16 operands, nothing but bias / add / accumulate around it
static bool pointwise_mfma_applicable(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_tensor* y, const Geometry& g,
                                      const RunFacts& rt) {
  static const bool pw_on = !(getenv("MMTTA_POINTWISE_MFMA") && atoi(getenv("MMTTA_POINTWISE_MFMA")) == 0);      // (A/B switch)
  const int kb = (g.K + 15) / 16;
  auto rows_ok = [&](const mmtta_tensor* t) { return dense_rows16(t) && is_bf16(t) == is_bf16(x); };
  return pw_on && d->ksize == 1 && (d->op == MMTTA_CONV_FWD || d->op == MMTTA_CONV_DGRAD) && use_bf16(d, g.K) &&
         (kb <= 4 || kb == 6 || kb == 8) && g.Np <= 64 && rt.stats == nullptr && !(rt.x_norm && (rt.x_norm->mean || rt.x_norm->scale)) &&
         (long long)y->d * y->h * y->w >= 4096 && rows_ok(x) && rows_ok(y) && (rt.add == nullptr || (rows_ok(rt.add) && same_shape(rt.add, y)));
}

// the operands admit the row-structured loader of the bf16 3x3x3 stride-1 stages: 8-channel items, 32-bit element offsets
// from 24-bit multiply-adds
static bool rowload_operand(const mmtta_tensor* x) {
  const int64_t lim24 = (int64_t)1 << 24;
  return quad_aligned(x, 16, is_bf16(x) ? 8 : 4) && strides_fit_24(x) && x->d < lim24 && x->h < lim24 && x->w < lim24 &&
         item_fits_31(x, x->c + 16);
}

// 18 (MMTTA_OPT_IGEMM_FRAGMENT_REUSE): exactly the 32 -> 32 3x3x3 stride-1 layers of bf16 precision on the lean tile, forward
// and input gradient, with the whole K loop in one workgroup (the 64^3 level never splits; small grids that do stay on
// 14), when the run takes the canonical stage (row loader) and the 16-byte epilogue.  The kernel has no other path, so
// everything those depend on is asked here, the alignment of the run's bias included: a bias off its 16 bytes sends route
// 14 to its 4-byte epilogue, whose statistics rows sum in another order, and stays there.
static bool igemm_reuse_applicable(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_tensor* y, const Geometry& g,
                                   const RunFacts& rt) {
  const mmtta_tensor* ad = rt.add;
  return g_igemm_reuse && g_igemm_pipeline && g_epilogue_vec && g.route == 14 && !g.classes && d->ksize == 3 && g.si == 1 &&
         g.K == 32 && g.N == 32 && g.ksplit == 1 && rowload_operand(x) && quad_aligned(y, quad_bytes(y)) && (!ad || quad_aligned(ad, quad_bytes(ad))) &&
         is_bf16(x) == is_bf16(y) && (!ad || is_bf16(ad) == is_bf16(y)) && ((uintptr_t)rt.bias) % 16 == 0;
}

// 15: the tensors admit the class-fused kernel's 16-byte accesses behind 32-bit offsets from 24-bit multiply-adds
static bool cls_fused_operand(const mmtta_tensor* t) {
  return quad_aligned(t, 16, is_bf16(t) ? 8 : 4) && strides_fit_24(t) && item_fits_31(t, t->c + 16);
}

// statistics rows written per tile: 1 by the conv epilogue, MT/32 by the split-K finalize
static int stats_rows_per_tile(const Geometry& g) {
  if (g.route == C_CLS_FUSED) return 1;
  return g.ksplit > 1 ? g.cfg.TZ * g.cfg.TY * g.cfg.TX / 32 : 1;
}

// The planner of a whole call: argument checks, the route, and the numbers mmtta_conv_plan reports for it.
static int geometry(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_tensor* y, const RunFacts* rt, Geometry& g) {
  int st = validate_desc(d);
  if (st) return st;
  g.leaky = g.raw = false; g.cls8 = CLS8_TRANSFORM; g.thin_kernel = g.thin_lean = 0;
  MMTTA_CHECK(x && y && x->ptr && y->ptr, MMTTA_ERR_INVALID, "conv: null tensor");
  MMTTA_CHECK(is_cl(x) && is_cl(y), MMTTA_ERR_UNSUPPORTED, "conv: tensors must be channels-last (sc == 1)");
  op_dims(d, g.K, g.N, g.si, g.classes);
  MMTTA_CHECK(x->c == g.K && y->c == g.N, MMTTA_ERR_INVALID, "conv: channel mismatch (x.c=%d want %d, y.c=%d want %d)",
              x->c, g.K, y->c, g.N);
  MMTTA_CHECK(x->n == y->n, MMTTA_ERR_INVALID, "conv: batch mismatch");
  const int xd[3] = {x->d, x->h, x->w}, yd[3] = {y->d, y->h, y->w};
  for (int i = 0; i < 3; ++i) {
    int e = expected_out_dim(d, xd[i]);
    if (e >= 0) {
      MMTTA_CHECK(yd[i] == e, MMTTA_ERR_INVALID, "conv: spatial mismatch axis %d: in %d -> out %d, expected %d", i, xd[i],
                  yd[i], e);
      if (d->op == MMTTA_CONVT_DGRAD)
        MMTTA_CHECK(xd[i] % 2 == 0, MMTTA_ERR_INVALID, "conv_transpose dgrad: dy extent must be even");
    } else {
      // CONV_DGRAD: x = dy (conv output extent), y = dx (conv input extent)
      int want = d->stride == 1 ? yd[i] : (yd[i] + 1) / 2;
      MMTTA_CHECK(xd[i] == want, MMTTA_ERR_INVALID, "conv dgrad: dy extent %d does not match dx extent %d", xd[i], yd[i]);
    }
  }
  g.Kp = roundup(g.K, 32);
  g.Np = roundup(g.N, 32);
  int Dg = y->d, Hg = y->h, Wg = y->w;
  if (g.classes) { Dg = (y->d + 1) / 2; Hg = (y->h + 1) / 2; Wg = (y->w + 1) / 2; }
  // launch geometry is a function of ONE batch item's extent: every item is computed as if launched alone (the contract of
  // the per-item parameter sets, include/mmtta.h), the batch only multiplies the workgroups
  g.cfg = pick_config(g.Np, g.si, (long long)Dg * Hg * Wg * (g.classes ? 8 : 1), g.K, use_bf16(d, g.K));
  g.tz = (Dg + g.cfg.TZ - 1) / g.cfg.TZ;
  g.ty = (Hg + g.cfg.TY - 1) / g.cfg.TY;
  g.tx = (Wg + g.cfg.TX - 1) / g.cfg.TX;
  g.tiles_per_n = g.tz * g.ty * g.tx;
  g.ncls = g.classes ? 8 : 1;
  g.tiles = g.tiles_per_n * x->n * g.ncls;     // the parity classes share one launch
  g.nstages = (g.K + g.cfg.KCI - 1) / g.cfg.KCI;
  const int ncolgroups = (g.Np + 32 * g.cfg.NB - 1) / (32 * g.cfg.NB);
  const int wgs = g.tiles_per_n * g.ncls * ncolgroups;      // per batch item
  g.ksplit = 1;
  g.sps = g.nstages;
  // Split the reduction when a launch has fewer than 192 workgroups, up to ~256.  Measured on the U-Net: with ONE volume
  // in flight 384/512 is the optimum (1024: +6 %, 256: +2 %, no split-K: +80 % of a step's conv time); with TWO in flight
  // (method.lanes: 2, the default) the other lane fills idle CUs and less splitting wins: 384/512, 192/256, 96/128 ->
  // 41.5, 42.9, 42.2 volumes/s (one lane at 192/256: 28.9 vs 29.6).
  if (wgs < g_tune[0] && g.nstages > 1) {
    int want = (g_tune[1] + wgs - 1) / wgs;
    if (want > g.nstages) want = g.nstages;
    g.sps = (g.nstages + want - 1) / want;
    g.ksplit = (g.nstages + g.sps - 1) / g.sps;
  }
  // Class-fused kernel (MMTTA_OPT_CLASS_FUSED_MIN_WORKGROUPS): all 8 parity classes of a coarse 4 x 4 x 8 tile in one
  // workgroup, when that still makes enough workgroups (no split-K there) and the tensors admit its 16-byte accesses
  g.route = config_id(g.cfg);
  if (g.classes && g.cfg.bf && g_cls_fused_min > 0) {
    const int ftz = (Dg + 3) / 4, fty = (Hg + 3) / 4, ftx = (Wg + 7) / 8;
    const long long fw = (long long)ftz * fty * ftx * (g.Np / 32);      // per batch item
    if (fw >= g_cls_fused_min && cls_fused_operand(x) && cls_fused_operand(y) && y->c % 4 == 0 && is_bf16(x) == is_bf16(y) &&
        g_epilogue_vec) {
      g.route = C_CLS_FUSED;
      g.tz = ftz; g.ty = fty; g.tx = ftx;
      g.tiles_per_n = ftz * fty * ftx;
      g.ncls = 1;                                  // one statistics row per fused tile
      g.tiles = g.tiles_per_n * x->n;
      g.nstages = (g.K + 15) / 16;
      g.ksplit = 1; g.sps = g.nstages;
    }
  }
  // the kernels outside this file come first; the direct and thin-K plans are one workgroup and one statistics row per tile
  const bool f32_operands = !use_bf16(d, g.K);
  if (direct_applicable(d)) {
    g.route = C_DIRECT; g.ksplit = 1;
    g.tiles = direct_blocks_per_n(d, x, y) * y->n;
  } else if (rt && f32_operands && is_f32(x) && pointwise_small_applicable(d, x, y, rt->stats, rt->add, rt->x_norm)) {      // (y: fp32- or bf16-stored)
    g.route = C_PW_SMALL;
  } else if (f32_operands && chan_applicable(d, x, y)) {
    g.route = C_THIN; g.ksplit = 1;
    g.tiles = chan_tiles_per_n(y) * y->n;
  } else if (rt && pointwise_mfma_applicable(d, x, y, g, *rt)) {
    g.route = C_PW_MFMA;
  } else if (rt && igemm_reuse_applicable(d, x, y, g, *rt)) {
    g.route = C_IGEMM_REUSE;
  }
  g.stats_rows = g.tiles * stats_rows_per_tile(g);
  g.workspace_bytes = g.ksplit > 1 ? (int64_t)g.ksplit * g.tiles * g.cfg.TZ * g.cfg.TY * g.cfg.TX * g.Np * (int64_t)sizeof(float) : 0;
  return MMTTA_OK;
}

static void build_taps(const mmtta_conv_desc* d, int pz, int py, int px, Taps& t) {
  // pz/py/px: output parity class for the transposed forms, ignored otherwise
  int n = 0;
  const bool classes = (d->op == MMTTA_CONVT_FWD) || (d->op == MMTTA_CONV_DGRAD && d->stride == 2);
  if (d->ksize == 1) {
    t.dz[0] = t.dy[0] = t.dx[0] = 0; t.slab[0] = 0; n = 1;
  } else if (!classes) {
    // stride-1 input gradient mirrors the taps; they are enumerated in ascending (z, y, x) order of the voxel they READ in
    // both forms (kernel tap 26 - m for the mirrored one), the order the canonical stage of igemm_kernel assumes (tap27_off)
    const int sgn = (d->op == MMTTA_CONV_DGRAD) ? -1 : 1;
    for (int m = 0; m < 27; ++m) {
      const int q = sgn < 0 ? 26 - m : m, kz = q / 9, ky = q / 3 % 3, kx = q % 3;
      t.dz[n] = (signed char)(sgn * (kz - 1)); t.dy[n] = (signed char)(sgn * (ky - 1));
      t.dx[n] = (signed char)(sgn * (kx - 1)); t.slab[n] = q; ++n;
    }
  } else {
    // out index i = 2*o - 1 + k.  parity 0: k=1 reads o=g (d=0); parity 1: k=0 reads g+1, k=2 reads g.
    int kzs[2], dzs[2], nz, kys[2], dys[2], ny, kxs[2], dxs[2], nx;
    auto axis = [](int p, int* ks, int* ds) { if (p == 0) { ks[0] = 1; ds[0] = 0; return 1; }
                                              ks[0] = 0; ds[0] = 1; ks[1] = 2; ds[1] = 0; return 2; };
    nz = axis(pz, kzs, dzs); ny = axis(py, kys, dys); nx = axis(px, kxs, dxs);
    for (int a = 0; a < nz; ++a) for (int b = 0; b < ny; ++b) for (int c = 0; c < nx; ++c) {
      t.dz[n] = (signed char)dzs[a]; t.dy[n] = (signed char)dys[b]; t.dx[n] = (signed char)dxs[c];
      t.slab[n] = (kzs[a] * 3 + kys[b]) * 3 + kxs[c]; ++n;
    }
  }
  t.n = n;
  int zmn = 9, zmx = -9, ymn = 9, ymx = -9, xmn = 9, xmx = -9;
  for (int i = 0; i < n; ++i) {
    zmn = t.dz[i] < zmn ? t.dz[i] : zmn; zmx = t.dz[i] > zmx ? t.dz[i] : zmx;
    ymn = t.dy[i] < ymn ? t.dy[i] : ymn; ymx = t.dy[i] > ymx ? t.dy[i] : ymx;
    xmn = t.dx[i] < xmn ? t.dx[i] : xmn; xmx = t.dx[i] > xmx ? t.dx[i] : xmx;
  }
  t.zmin = zmn; t.ymin = ymn; t.xmin = xmn;
  t.zext = zmx - zmn; t.yext = ymx - ymn; t.xext = xmx - xmn;
}

template <int NB, int MB, int TZ, int TY, int TX, int KCI, bool BF, int OCC, bool ABF, bool REUSE = false, bool RAW = false>
static int launch_cfg_t(const GArgs& a_in, const Taps* ht, int tiles, hipStream_t s) {
  GArgs a = a_in;
  size_t lds = 0;
  for (int c = 0; c < a.ncls; ++c) {
    const Taps& tp = ht[c];
    const int BZ = (TZ - 1) * a.si + tp.zext + 1, BY = (TY - 1) * a.si + tp.yext + 1, BX = (TX - 1) * a.si + tp.xext + 1;
    const int LP = (BF && a.si == 1) ? LDS_PITCH_BF16 : BX;
    for (int t = 0; t < tp.n; ++t) {
      a.toff[a.cls[c].tap0 + t] = ((tp.dz[t] - tp.zmin) * BY + (tp.dy[t] - tp.ymin)) * LP + (tp.dx[t] - tp.xmin);
      a.slab[a.cls[c].tap0 + t] = tp.slab[t];
    }
    a.cls[c].BX = BX; a.cls[c].BXY = BX * BY;
    a.cls[c].mBX = (unsigned)(((1ULL << 32) + BX - 1) / BX);
    a.cls[c].mBXY = (unsigned)(((1ULL << 32) + (unsigned long long)BX * BY - 1) / ((unsigned long long)BX * BY));
    const size_t need = BF ? (size_t)BZ * BY * LP * (KCI + 8) * 2 : (size_t)BZ * BY * BX * (KCI + 1) * sizeof(float);
    if (need > lds) lds = need;
  }
  if (BF && a.rowload && a.si == 1 && a.ncls == 1 && a.cls[0].ntaps == 27) {
    // the canonical stage addresses taps by formula: the tables must agree with it, or the generic loader runs
    a.flip27 = a.slab[0] == 26 ? 1 : 0;
    for (int t = 0; t < 27; ++t)
      if (a.toff[t] != tap27_off(t, TY + 2) || a.slab[t] != (a.flip27 ? 26 - t : t)) a.rowload = 0;
  }
  constexpr size_t epi = (4 * (REUSE ? 2 : 1) * EPI_TILE_FLOATS + 4 * 2 * 32) * sizeof(float);
  if (lds < epi) lds = epi;
  if constexpr (REUSE) {
    // the planner asked for everything the kernel needs but the tap tables, which exist only here: should they ever not be
    // the canonical ones, the plain kernel of the tile computes the same values
    if (!(a.rowload && a.ovec && a.ksplit == 1 && a.Ci == KCI * a.nstages))
      return launch_cfg_t<NB, MB, TZ, TY, TX, KCI, BF, OCC, ABF, false, RAW>(a_in, ht, tiles, s);
  }
  lds = (lds + 15) / 16 * 16;
  a.coef_off = (int)(lds / sizeof(float));
  if (BF && !RAW) lds += (size_t)2 * a.stages_per_split * KCI * sizeof(float);     // scale | shift of the staged channels
  MMTTA_CHECK(lds <= 160 * 1024, MMTTA_ERR_UNSUPPORTED, "conv: LDS box of %zu bytes exceeds 160 KiB", lds);
  int st;
  void (*kern)(GArgs);
  if constexpr (RAW) {
    static_assert(BF && ABF, "raw staging copies bf16-stored items");
    if constexpr (REUSE) kern = igemm_reuse_raw_kernel<ABF>;
    else kern = igemm_raw_kernel<NB, MB, TZ, TY, TX, KCI, OCC>;
  } else if constexpr (REUSE) {
    kern = igemm_reuse_kernel<ABF>;
  } else {
    kern = igemm_kernel<NB, MB, TZ, TY, TX, KCI, BF, OCC, ABF>;
  }
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set = true;
  }
  dim3 grid(tiles, (a.Np + 32 * NB - 1) / (32 * NB), a.ksplit);
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a);
  st = launch_status("conv igemm");
  if (st) return st;
  if (a.ksplit > 1 && !g_profile_main_only) {
    dim3 g2(tiles * (TZ * TY * TX / 32), (a.Np + 31) / 32);
    hipLaunchKernelGGL((splitk_finalize_kernel<TZ, TY, TX, BF, ABF>), g2, dim3(256), 0, s, a, tiles);
    st = launch_status("conv split-K finalize");
  }
  return st;
}

// The raw, pipelined and lean kernels are instantiated in the plain translation unit only (their form has no activation to
// vary).  The guard keeps the LeakyReLU one from instantiating them; which call takes them is the plan's word (Geometry::raw,
// ::cls8), and the plan of a call that runs there says none.
#ifdef MMTTA_ACT_LEAKY_TU
constexpr bool RAW_KERNELS = false;
#else
constexpr bool RAW_KERNELS = true;
#endif

// storage dispatch: bf16-stored activations exist for bf16-operand layers only (forward: input, output and fused add all
// bf16; everything else all fp32)
template <int NB, int MB, int TZ, int TY, int TX, int KCI, bool BF, int OCC = 2, bool REUSE = false>
static int launch_cfg(const GArgs& a, const Taps* ht, int tiles, bool raw, hipStream_t s) {
  if constexpr (BF) {
    if (a.in_bf || a.out_bf || a.add_bf) {
      MMTTA_CHECK(a.in_bf && a.out_bf && (a.add == nullptr || a.add_bf), MMTTA_ERR_UNSUPPORTED,
                  "conv: input, output and fused add must share one storage type (in %d out %d add %d)", a.in_bf, a.out_bf,
                  a.add_bf);
      if constexpr (RAW_KERNELS) {
        if (raw) return launch_cfg_t<NB, MB, TZ, TY, TX, KCI, BF, OCC, true, REUSE, true>(a, ht, tiles, s);
      }
      return launch_cfg_t<NB, MB, TZ, TY, TX, KCI, BF, OCC, true, REUSE>(a, ht, tiles, s);
    }
  }
  return launch_cfg_t<NB, MB, TZ, TY, TX, KCI, BF, OCC, false, REUSE>(a, ht, tiles, s);
}

static int launch_any(int route, const GArgs& a, const Taps* ht, int tiles, bool raw, hipStream_t s) {
  switch (route) {
    case 0: return launch_cfg<1, 4, 8, 8, 8, 8, false>(a, ht, tiles, raw, s);
    case 1: return launch_cfg<2, 4, 4, 8, 8, 16, false>(a, ht, tiles, raw, s);
    case 2: return launch_cfg<4, 4, 4, 4, 8, 32, false>(a, ht, tiles, raw, s);
    case 3: return launch_cfg<1, 1, 4, 4, 8, 8, false>(a, ht, tiles, raw, s);
    case 4: return launch_cfg<2, 2, 4, 4, 8, 8, false>(a, ht, tiles, raw, s);
    case 5: return launch_cfg<4, 4, 4, 4, 8, 8, false>(a, ht, tiles, raw, s);
    case 14: return launch_cfg<1, 2, 4, 8, 8, 16, true, 3>(a, ht, tiles, raw, s);
    case C_IGEMM_REUSE: return launch_cfg<1, 2, 4, 8, 8, 16, true, 3, true>(a, ht, tiles, raw, s);
    case 7: return launch_cfg<1, 4, 8, 8, 8, 16, true>(a, ht, tiles, raw, s);
    case 8: return launch_cfg<2, 4, 4, 8, 8, 32, true>(a, ht, tiles, raw, s);
    case 9: return launch_cfg<4, 4, 4, 4, 8, 32, true>(a, ht, tiles, raw, s);
    case 10: return launch_cfg<1, 1, 4, 4, 8, 16, true>(a, ht, tiles, raw, s);
    case 11: return launch_cfg<2, 2, 4, 4, 8, 16, true>(a, ht, tiles, raw, s);
    default: return launch_cfg<4, 4, 4, 4, 8, 16, true>(a, ht, tiles, raw, s);
  }
}

struct ConvCall {      // the operands of a call, as conv_run_body received them
  const mmtta_conv_desc* d; const mmtta_tensor* x; const mmtta_norm_on_load* x_norm; const void* packed; const float* bias;
  const mmtta_conv_epilogue* epi; const mmtta_tensor* y; int accumulate; float* stats; void* workspace; int64_t workspace_bytes;
  PSets ps; hipStream_t stream;
};

// ---- one launcher per family of this file (direct_conv_run, chan_conv_run, pointwise_small_run: conv_direct.hip)
// GArgs and the tap tables of a call: what igemm_kernel and igemm_cls8_kernel share
static int fill_gargs(const ConvCall& c, const Geometry& g, GArgs& a, Taps* ht) {
  const mmtta_tensor *x = c.x, *y = c.y, *ad = (c.epi && c.epi->add) ? c.epi->add : nullptr;
  a.in = (const float*)x->ptr; a.isn = x->sn; a.isd = x->sd; a.ish = x->sh; a.isw = x->sw;
  a.Ci = x->c; a.Di = x->d; a.Hi = x->h; a.Wi = x->w; a.tin = nl(c.x_norm);
  a.out = (float*)y->ptr; a.osn = y->sn; a.osd = y->sd; a.osh = y->sh; a.osw = y->sw;
  a.Co = y->c; a.Do = y->d; a.Ho = y->h; a.Wo = y->w;
  a.si = g.si; a.bias = c.bias; a.ps = c.ps; a.accumulate = c.accumulate;
  a.wp = (const float*)c.packed; a.Kp = g.Kp; a.Np = g.Np;
  const int st = epilogue_add(c.epi, y, a);
  if (st) return st;
  a.in_bf = is_bf16(x) ? 1 : 0; a.out_bf = is_bf16(y) ? 1 : 0; a.add_bf = (ad && is_bf16(ad)) ? 1 : 0;
  const bool oal = quad_aligned(y, quad_bytes(y)) && y->c % 4 == 0 &&                                    // 4-channel accesses
                   (!ad || quad_aligned(ad, quad_bytes(ad))) && (c.bias == nullptr || ((uintptr_t)c.bias) % 16 == 0);
  a.ovec = (oal && g_epilogue_vec) ? 1 : 0;
  a.stats = c.stats; a.stats_rows_per_n = g.ncls * g.tiles_per_n * stats_rows_per_tile(g);
  a.ws = (float*)c.workspace; a.ksplit = g.ksplit; a.stages_per_split = g.sps; a.nstages = g.nstages;
  a.tz = g.tz; a.ty = g.ty; a.tx = g.tx;
  MMTTA_CHECK(g.cfg.bf || (!a.in_bf && !a.out_bf && !a.add_bf), MMTTA_ERR_UNSUPPORTED,
              "conv: bf16-stored tensors need a bf16-operand layer (K >= 16 in bf16 precision)");
  // 8-channel items: 32 bytes of fp32 (two 16-byte loads) or 16 bytes of bf16 (one): strides must keep them aligned
  const bool al = quad_aligned(x, 16, a.in_bf ? 8 : 4);
  a.vec4 = al ? 1 : 0; a.flip27 = 0;
  // row-structured loader of the 3x3x3 stride-1 stages: 32-bit element offsets from 24-bit multiply-adds
  a.rowload = (rowload_operand(x) && g_igemm_pipeline) ? 1 : 0;
  a.ncls = g.classes ? 8 : 1; a.so = g.classes ? 2 : 1;
  int tap0 = 0;
  for (int cls = 0; cls < a.ncls; ++cls) {
    const int pz = (cls >> 2) & 1, py = (cls >> 1) & 1, px = cls & 1;
    build_taps(c.d, pz, py, px, ht[cls]);
    ClassInfo& ci = a.cls[cls];
    ci.tap0 = tap0; ci.ntaps = ht[cls].n; tap0 += ht[cls].n;
    ci.zmin = ht[cls].zmin; ci.ymin = ht[cls].ymin; ci.xmin = ht[cls].xmin;
    ci.zext = ht[cls].zext; ci.yext = ht[cls].yext; ci.xext = ht[cls].xext;
    if (g.classes) {
      ci.oz = pz; ci.oy = py; ci.ox = px;
      ci.Dg = (y->d - pz + 1) / 2; ci.Hg = (y->h - py + 1) / 2; ci.Wg = (y->w - px + 1) / 2;
    } else {
      ci.oz = ci.oy = ci.ox = 0;
      ci.Dg = y->d; ci.Hg = y->h; ci.Wg = y->w;
    }
  }
  return MMTTA_OK;
}

static int igemm_run(const ConvCall& c, const Geometry& g) {
  MMTTA_CHECK(g.workspace_bytes == 0 || (c.workspace != nullptr && c.workspace_bytes >= g.workspace_bytes), MMTTA_ERR_WORKSPACE,
              "conv: workspace %lld bytes, need %lld", (long long)c.workspace_bytes, (long long)g.workspace_bytes);
  GArgs a; Taps ht[8];
  const int st = fill_gargs(c, g, a, ht);
  if (st) return st;
  return launch_any(g.route, a, ht, g.tiles, g.raw, c.stream);
}

static int cls_fused_run(const ConvCall& c, const Geometry& g) {
  GArgs a; Taps ht[8];
  const int st = fill_gargs(c, g, a, ht);
  if (st) return st;
  MMTTA_CHECK(a.ovec && a.vec4, MMTTA_ERR_UNSUPPORTED,
              "conv (class-fused stride-2 form): the epilogue operands must admit 16-byte accesses");
  MMTTA_CHECK(a.in_bf == a.out_bf && (a.add == nullptr || a.add_bf == a.out_bf), MMTTA_ERR_UNSUPPORTED,
              "conv: input, output and fused add must share one storage type (in %d out %d add %d)", a.in_bf, a.out_bf, a.add_bf);
  if constexpr (RAW_KERNELS) {
    switch (g.cls8) {
      case CLS8_LEAN: return launch_cls8_t<16, true, true, true, true>(a, g.tiles, c.stream);
      case CLS8_PIPELINED: return launch_cls8_t<16, true, true, true>(a, g.tiles, c.stream);
      case CLS8_RAW: return launch_cls8_t<16, true, true>(a, g.tiles, c.stream);
      default: break;
    }
  }
  return a.in_bf ? launch_cls8_t<16, true>(a, g.tiles, c.stream) : launch_cls8_t<16, false>(a, g.tiles, c.stream);
}

static int pointwise_mfma_run(const ConvCall& c, const Geometry& g) {
  const mmtta_tensor *x = c.x, *y = c.y, *ad = (c.epi && c.epi->add) ? c.epi->add : nullptr;
  PWArgs q;
  q.in = (const float*)x->ptr; q.isn = x->sn; q.isw = (unsigned)x->sw; q.Ci = x->c;
  q.out = (float*)y->ptr; q.osn = y->sn; q.osw = (unsigned)y->sw; q.Co = y->c;
  q.add = ad ? (const float*)ad->ptr : nullptr; q.asn = ad ? ad->sn : 0; q.asw = ad ? (unsigned)ad->sw : 0u;
  q.tadd = ad ? nl(&c.epi->add_norm) : nl(nullptr);
  q.wp = (const float*)c.packed; q.bias = c.bias; q.Np = g.Np; q.ps = c.ps; q.accumulate = c.accumulate;
  q.dhw = (long long)y->d * y->h * y->w;
  long long blocks = (q.dhw + 127) / 128;
  if (blocks > 2048) blocks = 2048;
  const dim3 grid((unsigned)blocks, y->n);
  if (is_bf16(x)) launch_pointwise_mfma<true>(q, (g.K + 15) / 16, g.Np / 32, grid, c.stream);
  else launch_pointwise_mfma<false>(q, (g.K + 15) / 16, g.Np / 32, grid, c.stream);
  return launch_status("1x1 conv (streaming MFMA)");
}

// The plan of a run - the route and its variant: the one function behind conv_run_body and every query of a run
// (mmtta_conv_route ... mmtta_conv_thin_kernel, mmtta_conv_head_loss_eligible).  A thin kernel's refusal is part of the plan
// (Geometry::thin_kernel < 0), not an error of planning: the launcher returns it from its place in the run.
static int plan_run(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm, const mmtta_conv_epilogue* epi,
                    const mmtta_tensor* y, int accumulate, const float* stats, const float* bias, Geometry& g) {
  const mmtta_tensor* add = epi ? epi->add : nullptr;
  const RunFacts rt{stats, add, x_norm, accumulate, bias};
  const int st = geometry(d, x, y, &rt, g);
  if (st) return st;
  g.leaky = nl_leaky(x_norm) || (add && nl_leaky(&epi->add_norm));
  g.raw = !g.leaky && raw_staging(g, x, x_norm, y, add);
  if (cls8_pipelined(g)) g.cls8 = cls8_lean(y, add) ? CLS8_LEAN : CLS8_PIPELINED;
  else if (g.route == C_CLS_FUSED && g.raw) g.cls8 = CLS8_RAW;
  if (g.route == C_THIN) {
    g.thin_lean = chan_lean_applicable(d, x, x_norm, epi, y, accumulate) ? 1 : 0;
    g.thin_kernel = chan_kernel(d, x, epi, y, g.thin_lean != 0);
  } else if (g.route == C_DIRECT) {
    g.thin_lean = direct_upconv8_lean(d, x, x_norm, epi, y) ? 2 : 0;
    g.thin_kernel = direct_kernel(d, x, x_norm, epi, y, accumulate, stats, g.thin_lean != 0);
  }
  return MMTTA_OK;
}

// mmtta_conv_run_sets past the checks of its norm-on-load descriptors: plan, check, switch
int conv_run_body(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm, const void* packed,
                  const float* bias, const mmtta_conv_epilogue* epi, const mmtta_tensor* y, int accumulate, float* stats,
                  void* workspace, int64_t workspace_bytes, const mmtta_param_sets* sets, void* stream) {
  Geometry g;
  int st = plan_run(d, x, x_norm, epi, y, accumulate, stats, bias, g);
  if (st) return st;
  MMTTA_CHECK(packed != nullptr, MMTTA_ERR_INVALID, "conv: null packed weights");
  st = psets_validate(sets, x->n);
  if (st) return st;
  const ConvCall c{d, x, x_norm, packed, bias, epi, y, accumulate, stats, workspace, workspace_bytes, psets(sets), (hipStream_t)stream};
  switch (g.route) {
    case C_DIRECT: return direct_conv_run(g.thin_kernel, d, x, x_norm, packed, bias, epi, y, accumulate, stats, c.ps, c.stream);
    case C_PW_SMALL: return pointwise_small_run(x, packed, g.Kp, g.Np, bias, y, accumulate, c.ps, c.stream);
    case C_THIN: return chan_conv_run(g.thin_kernel, d, x, x_norm, packed, g.Kp, g.Np, bias, epi, y, accumulate, stats, c.ps, c.stream);
    case C_PW_MFMA: return pointwise_mfma_run(c, g);
    case C_CLS_FUSED: return cls_fused_run(c, g);
    default: return igemm_run(c, g);
  }
}

MMTTA_ACT_NS_CLOSE
}  // namespace mmtta

#ifndef MMTTA_ACT_LEAKY_TU
using namespace mmtta;

// the geometry of an entry (every field but the pointers); up8 / chfr: whether those images follow the tap image
static int pack_entry_geometry(const mmtta_conv_desc* d, PackEntry& e, bool& up8, bool& chfr) {
  int st = validate_desc(d);
  if (st) return st;
  int K, N, si; bool cl;
  op_dims(d, K, N, si, cl);
  const bool convt = d->op == MMTTA_CONVT_FWD || d->op == MMTTA_CONVT_DGRAD;
  const bool direct = direct_applicable(d);
  e.w = nullptr; e.p = nullptr; e.up8 = nullptr; e.chfr = nullptr;
  e.A = convt ? d->cin : d->cout; e.B = convt ? d->cout : d->cin;
  e.T = d->ksize * d->ksize * d->ksize;
  e.Kp = direct ? K : roundup(K, 32); e.Np = direct ? 4 : roundup(N, 32);
  // K,N in terms of (A,B): CONV_FWD K=cin=B ; CONV_DGRAD K=cout=A ; CONVT_FWD K=cin=A ; CONVT_DGRAD K=cout=B
  e.kn_is_ba = (d->op == MMTTA_CONV_FWD || d->op == MMTTA_CONVT_DGRAD) ? 1 : 0;
  e.bf16 = use_bf16(d, K) ? 1 : 0; e.direct = direct ? 1 : 0;
  up8 = direct && upconv8_image_bytes(d) > 0;       // ConvTranspose3d K -> R: + the gather-GEMM image behind the tap image
  chfr = !direct && chan_frag_bytes(d) > 0;         // thin-K convolution: + its B fragments behind the fp32 tap image
  e.KI = K; e.NO = N;
  MMTTA_CHECK(e.T == 1 || e.T == 27, MMTTA_ERR_UNSUPPORTED, "pack: ksize %d", d->ksize);
  e.start = 0;
  return MMTTA_OK;
}

static int fill_pack_entry(const mmtta_conv_desc* d, const float* w, void* packed, PackEntry& e) {
  bool up8, chfr;
  int st = pack_entry_geometry(d, e, up8, chfr);
  if (st) return st;
  MMTTA_CHECK(w && packed, MMTTA_ERR_INVALID, "pack: null pointer");
  e.w = w; e.p = packed;
  e.up8 = up8 ? (unsigned short*)((char*)packed + (size_t)e.T * e.Kp * e.Np * 4) : nullptr;
  e.chfr = chfr ? (uint4*)((char*)packed + (size_t)e.T * e.Kp * e.Np * 4) : nullptr;
  return MMTTA_OK;
}

extern "C" int64_t mmtta_conv_packed_bytes(const mmtta_conv_desc* d) {
  PackEntry e;
  bool up8, chfr;
  if (pack_entry_geometry(d, e, up8, chfr)) return -1;
  return (int64_t)e.T * e.Kp * e.Np * (int64_t)(e.bf16 ? 2 : sizeof(float)) + (e.direct ? upconv8_image_bytes(d) : chan_frag_bytes(d));
}

extern "C" int mmtta_conv_pack_weights(const mmtta_conv_desc* d, const float* w, void* packed, void* stream) {
  PackEntry e;
  int st = fill_pack_entry(d, w, packed, e);
  if (st) return st;
  const long long total = (long long)e.T * e.Kp * e.Np;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  if (e.bf16)
    hipLaunchKernelGGL(pack_weights_bf16_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, (unsigned short*)packed,
                       e.A, e.B, e.T, e.Kp, e.Np, e.kn_is_ba);
  else
    hipLaunchKernelGGL(pack_weights_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, (float*)packed, e.A, e.B, e.T,
                       e.Kp, e.Np, e.kn_is_ba);
  if (e.up8)
    hipLaunchKernelGGL(pack_upconv8_kernel, dim3((e.KI * 4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, e.up8, e.KI, e.NO);
  if (e.chfr)
    hipLaunchKernelGGL(pack_chan_frags_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)packed, e.chfr, e.Kp,
                       e.Np, e.KI, e.NO);
  return launch_status("pack weights");
}

namespace mmtta {
int pack_image_geometry(const mmtta_conv_desc* d, PackImageGeo& g) {
  PackEntry e;
  bool up8, chfr;
  const int st = pack_entry_geometry(d, e, up8, chfr);
  if (st) return st;
  g.A = e.A; g.B = e.B; g.T = e.T; g.Kp = e.Kp; g.Np = e.Np; g.kn_is_ba = e.kn_is_ba;
  g.plain_bf16 = (e.bf16 && !e.direct && !up8 && !chfr) ? 1 : 0;
  return MMTTA_OK;
}
}  // namespace mmtta

extern "C" int64_t mmtta_conv_pack_table_bytes(int count) { return count < 0 ? -1 : (int64_t)count * (int64_t)sizeof(PackEntry); }

extern "C" int mmtta_conv_pack_table_build(const mmtta_pack_item* items, int count, void* table_host, int64_t* total) {
  MMTTA_CHECK(items && table_host && total && count > 0, MMTTA_ERR_INVALID, "pack table: bad argument");
  PackEntry* tab = (PackEntry*)table_host;
  long long run = 0;
  for (int i = 0; i < count; ++i) {
    int st = fill_pack_entry(&items[i].desc, items[i].w_master, items[i].packed, tab[i]);
    if (st) return st;
    tab[i].start = run;
    run += tab[i].direct ? ((long long)tab[i].Kp * tab[i].Np + 255) / 256
                         : (long long)(tab[i].Kp / PK) * (tab[i].Np / PN);
  }
  *total = run;
  return MMTTA_OK;
}

extern "C" int mmtta_conv_pack_batched(const void* table_dev, int count, int64_t total, void* stream) {
  MMTTA_CHECK(table_dev && count > 0 && total > 0, MMTTA_ERR_INVALID, "pack batched: bad argument");
  MMTTA_CHECK(total < (1LL << 31), MMTTA_ERR_UNSUPPORTED, "pack batched: %lld workgroups", (long long)total);
  hipLaunchKernelGGL(pack_batched_kernel, dim3((unsigned)total), dim3(256), 0, (hipStream_t)stream, (const PackEntry*)table_dev,
                     count);
  int st = launch_status("pack batched");
  if (st) return st;
  // the thin-K layers' B fragments, from the tap images the launch above wrote (a block per table entry; most return at once)
  hipLaunchKernelGGL(pack_chan_frags_batched_kernel, dim3((unsigned)count), dim3(256), 0, (hipStream_t)stream, (const PackEntry*)table_dev);
  return launch_status("pack batched (thin-K fragments)");
}

extern "C" int mmtta_conv_plan(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_tensor* y,
                               mmtta_conv_plan_t* plan) {
  MMTTA_CHECK(plan != nullptr, MMTTA_ERR_INVALID, "conv plan: null plan");
  Geometry g;
  int st = geometry(d, x, y, nullptr, g);
  if (st) return st;
  *plan = mmtta_conv_plan_t{g.tiles, /*launches*/ 1, g.ksplit, g.stats_rows, g.route, 0, g.workspace_bytes};
  return MMTTA_OK;
}

// ---- the queries of a run: each reads one field of the plan mmtta_conv_run would make for these operands (it has no bias
// to show: null), or reports the plan's error as a negative status
static int query_plan(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm, const mmtta_conv_epilogue* epi,
                      const mmtta_tensor* y, int accumulate, const float* stats, Geometry& g) {
  const int st = plan_run(d, x, x_norm, epi, y, accumulate, stats, nullptr, g);
  return st < 0 ? st : -st;
}
#define MMTTA_CONV_QUERY(name, field)                                                                                      \
  extern "C" int name(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,                  \
                      const mmtta_conv_epilogue* epi, const mmtta_tensor* y, int accumulate, const float* stats) {         \
    Geometry g;                                                                                                            \
    const int st = query_plan(d, x, x_norm, epi, y, accumulate, stats, g);                                                 \
    return st ? st : (field);                                                                                              \
  }
MMTTA_CONV_QUERY(mmtta_conv_route, g.route)
MMTTA_CONV_QUERY(mmtta_conv_stages_raw, g.raw ? 1 : 0)
MMTTA_CONV_QUERY(mmtta_conv_cls8_pipelined, g.cls8 >= CLS8_PIPELINED ? 1 : 0)
MMTTA_CONV_QUERY(mmtta_conv_cls8_lean_epilogue, g.cls8 == CLS8_LEAN ? 1 : 0)
MMTTA_CONV_QUERY(mmtta_conv_thin_lean, g.thin_lean)
MMTTA_CONV_QUERY(mmtta_conv_thin_kernel, g.thin_kernel)
#undef MMTTA_CONV_QUERY

// ---- the head convolution with the entropy objective in its epilogue (MMTTA_OPT_HEAD_LOSS_PAIR bit 0)
static int head_loss_plan(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                          const mmtta_conv_epilogue* epi, const mmtta_tensor* y, const mmtta_tensor* dz, int softmax, int per_item,
                          bool& eligible) {
  Geometry g;
  const int st = query_plan(d, x, x_norm, epi, y, 0, nullptr, g);
  if (st) return st;
  eligible = g.route == C_DIRECT && direct_head_loss_eligible(d, x, x_norm, epi, y, dz, softmax, per_item);
  return MMTTA_OK;
}

extern "C" int mmtta_conv_head_loss_eligible(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                                             const mmtta_conv_epilogue* epi, const mmtta_tensor* y, const mmtta_tensor* dlogits,
                                             int softmax, int per_item) {
  bool ok = false;
  const int st = head_loss_plan(d, x, x_norm, epi, y, dlogits, softmax, per_item, ok);
  return st ? st : (ok ? 1 : 0);
}

extern "C" int64_t mmtta_conv_head_loss_partials(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_tensor* y) {
  Geometry g;
  if (geometry(d, x, y, nullptr, g) || g.route != C_DIRECT) return -1;
  return (int64_t)direct_blocks_per_n(d, x, y) * y->n;
}

extern "C" int mmtta_conv_head_loss_run_sets(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                                             const void* packed, const float* bias, const mmtta_conv_epilogue* epi,
                                             const mmtta_tensor* y, const mmtta_tensor* dlogits, int softmax, int per_item,
                                             double* partial, float* loss, const mmtta_param_sets* sets, void* stream) {
  int st = nl_act_check(x_norm, "conv_head_loss_run (x_norm)");
  if (st) return st;
  st = nl_act_check((epi && epi->add) ? &epi->add_norm : nullptr, "conv_head_loss_run (epilogue add_norm)");
  if (st) return st;
  st = nl_per_item_check(x_norm, "conv_head_loss_run (x_norm)");
  if (st) return st;
  st = nl_per_item_check(epi ? &epi->add_norm : nullptr, "conv_head_loss_run (epilogue add_norm)");
  if (st) return st;
  bool ok = false;
  st = head_loss_plan(d, x, x_norm, epi, y, dlogits, softmax, per_item, ok);
  if (st) return st;
  MMTTA_CHECK(ok, MMTTA_ERR_UNSUPPORTED,
              "conv_head_loss_run: not a sigmoid head on the 4x4x4 matrix tiles with a dense 4-lane `dlogits` (ask "
              "mmtta_conv_head_loss_eligible; run mmtta_conv_run and mmtta_entropy_loss_items instead)");
  MMTTA_CHECK(packed != nullptr && partial != nullptr && loss != nullptr, MMTTA_ERR_INVALID, "conv_head_loss_run: null argument");
  st = psets_validate(sets, x->n);
  if (st) return st;
  return direct_head_loss_run(d, x, x_norm, packed, bias, epi, y, dlogits, partial, loss, psets(sets), (hipStream_t)stream);
}

extern "C" int mmtta_conv_run(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                              const void* packed, const float* bias, const mmtta_conv_epilogue* epi,
                              const mmtta_tensor* y, int accumulate, float* stats, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  return mmtta_conv_run_sets(d, x, x_norm, packed, bias, epi, y, accumulate, stats, workspace, workspace_bytes, nullptr, stream);
}

extern "C" int mmtta_conv_run_sets(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                                   const void* packed, const float* bias, const mmtta_conv_epilogue* epi,
                                   const mmtta_tensor* y, int accumulate, float* stats, void* workspace,
                                   int64_t workspace_bytes, const mmtta_param_sets* sets, void* stream) {
  const mmtta_norm_on_load* add_norm = (epi && epi->add) ? &epi->add_norm : nullptr;
  {
    int st = nl_act_check(x_norm, "conv_run (x_norm)");
    if (st) return st;
    st = nl_act_check(add_norm, "conv_run (epilogue add_norm)");
    if (st) return st;
    st = nl_per_item_check(x_norm, "conv_run (x_norm)");
    if (st) return st;
    st = nl_per_item_check(epi ? &epi->add_norm : nullptr, "conv_run (epilogue add_norm)");
    if (st) return st;
  }
  if (nl_leaky(x_norm) || nl_leaky(add_norm))
    return leaky::conv_run_body(d, x, x_norm, packed, bias, epi, y, accumulate, stats, workspace, workspace_bytes, sets, stream);
  return conv_run_body(d, x, x_norm, packed, bias, epi, y, accumulate, stats, workspace, workspace_bytes, sets, stream);
}
#endif  // MMTTA_ACT_LEAKY_TU
