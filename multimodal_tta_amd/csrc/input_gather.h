// What the two input-adaptation translation units share (input_norm.hip: theta = (s, b, g) per modality; bias_field.hip: a
// smooth log-field per modality): the streaming pass over the raw fp32 voxel rows, the gather of the first level's input
// gradient per input voxel, Adam's step on one coefficient and the host checks of the row layout.  One copy of each.
#pragma once
#include "common.h"

// products and sums round on their own, as torch's do; the gather spells its fused multiply-adds out (see eata.hip)
#pragma clang fp contract(off)

namespace mmtta {

constexpr int IN_ROW = 4;                  // channels of an input voxel row: one 16-byte (fp32) or 8-byte (bf16) access
constexpr int IN_MAX_BLOCKS = 2048;        // workgroups per volume of the streaming pass
constexpr int IN_MAX_GRID_Y = 65535;       // gridDim.y carries the volume
constexpr int IN_MAX_C0 = 64;              // output channels of the first level's convolutions
constexpr int IN_TZ = 4, IN_TY = 8, IN_TX = 64;      // input voxels of a workgroup's tile: 8 parity classes x 256 threads
constexpr int IN_PZ = IN_TZ / 2 + 1, IN_PY = IN_TY / 2 + 1, IN_PX = IN_TX / 2 + 1;      // output positions behind a tile
constexpr int IN_POS = IN_PZ * IN_PY * IN_PX;
constexpr int IN_OC = 8;                   // output channels of a staged dy chunk

// ------------------------------------------------------------------ the streaming pass
// y[v, c] = row(x[v]) over the `dhw` voxels of one item, 256 threads x gridDim.x: one 16-byte load per voxel; fp32 out one
// 16-byte store per voxel, bf16 out one 16-byte store per PAIR of voxels (the pairs start where the item's rows are 16-byte
// aligned: `lead` = 1 shifts them by one voxel, and the voxel without a partner at either end takes an 8-byte store).
// `row(raw, voxel, out)` fills the four fp32 lanes of a voxel as bits.
template <bool BF, class Row>
__device__ __forceinline__ void in_stream_rows(const uint4* __restrict__ xb, void* __restrict__ y, long long n, long long ysn, unsigned dhw,
                                               Row&& row) {
  if constexpr (!BF) {
    uint4* yb = reinterpret_cast<uint4*>(y) + n * (ysn / IN_ROW);
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < dhw; i += gridDim.x * 256u) {
      unsigned o[4];
      row(xb[i], i, o);
      yb[i] = make_uint4(o[0], o[1], o[2], o[3]);
    }
  } else {
    char* yb = reinterpret_cast<char*>(y) + n * ysn * 2;
    const unsigned lead = (unsigned)((reinterpret_cast<uintptr_t>(yb) >> 3) & 1u);
    const unsigned pairs = (dhw + lead + 1u) / 2u;
    for (unsigned j = blockIdx.x * 256u + threadIdx.x; j < pairs; j += gridDim.x * 256u) {
      const long long v0 = 2ll * j - lead, v1 = v0 + 1;
      const bool h0 = v0 >= 0, h1 = v1 < (long long)dhw;
      unsigned o0[4] = {0u, 0u, 0u, 0u}, o1[4] = {0u, 0u, 0u, 0u};
      if (h0) row(xb[v0], (unsigned)v0, o0);
      if (h1) row(xb[v1], (unsigned)v1, o1);
      const uint2 a = make_uint2(f32x2_to_bf16x2(__uint_as_float(o0[0]), __uint_as_float(o0[1])),
                                 f32x2_to_bf16x2(__uint_as_float(o0[2]), __uint_as_float(o0[3])));
      const uint2 b = make_uint2(f32x2_to_bf16x2(__uint_as_float(o1[0]), __uint_as_float(o1[1])),
                                 f32x2_to_bf16x2(__uint_as_float(o1[2]), __uint_as_float(o1[3])));
      if (h0 && h1) *reinterpret_cast<uint4*>(yb + v0 * 8) = make_uint4(a.x, a.y, b.x, b.y);
      else if (h0) *reinterpret_cast<uint2*>(yb + v0 * 8) = a;
      else if (h1) *reinterpret_cast<uint2*>(yb + v1 * 8) = b;
    }
  }
}

// ------------------------------------------------------------------ the gather
struct InBranch {
  const float* dy;       // [N, Do, Ho, Wo, c0], fp32 or bf16 elements
  long long sn;          // strides in ELEMENTS (a channel slice of a wider tensor keeps the wide row stride)
  unsigned sd, sh, sw;
  const float* w;        // fp32 [c0, C, 27], set 0
  long long wset;        // elements between the sets of consecutive items (0: one set)
};
// the raw volume, its extents and the branches that read it: what a gradient kernel's tile needs to find its voxels
struct InGather {
  const uint4* x;
  long long xsn;         // rows between items
  int C, D, H, W, Do, Ho, Wo, c0, nbr;
  unsigned keep;
  int tiles_y, tiles_x;
  InBranch br[2];
};
// where a thread stands in its workgroup's tile (blockIdx.x: the tile, threadIdx.x: one voxel of each parity class)
struct InTile {
  int bx, by, bz, lx, ly, lz;
  __device__ __forceinline__ InTile(const InGather& a) {
    const int tid = threadIdx.x;
    bx = blockIdx.x % a.tiles_x; by = (blockIdx.x / a.tiles_x) % a.tiles_y; bz = blockIdx.x / (a.tiles_x * a.tiles_y);
    lx = tid & 31; ly = (tid >> 5) & 3; lz = tid >> 7;
  }
};

// A workgroup owns a tile of IN_TZ x IN_TY x IN_TX input voxels of volume n: 8 parity classes with one voxel per thread
// each.  Stride 2, pad 1: an even coordinate i meets tap 1 at output i / 2, an odd one taps 0 and 2 at outputs (i + 1) / 2
// and (i - 1) / 2, so the tile needs the IN_PZ x IN_PY x IN_PX output positions behind it and all threads of a class see
// the same taps.  Per branch the weights go to LDS as [tap][o][4 channels] (`in_w`, 27 * c0 float4; absent channels and pad
// lanes zero: read at wavefront-uniform addresses), and per chunk of IN_OC output channels the dy values of those positions
// as [half][position][4] fp32 (`dys`; coalesced rows in, zeros outside the output; neighbouring lanes read neighbouring 16
// bytes).  acc[class][channel] = dX' of the thread's 8 voxels, fp32 in a fixed order.  Starts with a barrier: what the
// caller wrote to LDS before the call is visible after it.
template <bool BF>
__device__ __forceinline__ void in_gather(const InGather& a, const InTile& t, int n, float4* __restrict__ in_w, float4 (&dys)[2][IN_POS],
                                          float (&acc)[8][4]) {
  const int tid = threadIdx.x, c0 = a.c0, C = a.C;
  const int oz0 = t.bz * (IN_TZ / 2), oy0 = t.by * (IN_TY / 2), ox0 = t.bx * (IN_TX / 2);
  const int p0 = (t.lz * IN_PY + t.ly) * IN_PX + t.lx;
#pragma unroll
  for (int v = 0; v < 8; ++v) { acc[v][0] = 0.f; acc[v][1] = 0.f; acc[v][2] = 0.f; acc[v][3] = 0.f; }

  for (int r = 0; r < a.nbr; ++r) {
    const InBranch& b = a.br[r];
    const float* wsrc = b.w + (long long)n * b.wset;
    const float* db = item_base<BF>(b.dy, n, b.sn);
    __syncthreads();                                     // (the previous branch's weights are no longer read)
    for (int i = tid; i < 27 * c0; i += 256) {
      const int tp = i / c0, o = i - tp * c0;
      float wv[4];
#pragma unroll
      for (int c = 0; c < IN_ROW; ++c) {
        const float v = wsrc[(o * C + (c < C ? c : 0)) * 27 + tp];
        wv[c] = (c < C && ((a.keep >> c) & 1u)) ? v : 0.f;
      }
      in_w[i] = make_float4(wv[0], wv[1], wv[2], wv[3]);
    }
    for (int oc = 0; oc < c0; oc += IN_OC) {
      const bool two = oc + 4 < c0;                      // (c0 is a multiple of 4: the chunk's second half may not exist)
      __syncthreads();                                   // (the previous chunk's tile is no longer read; the weights are in)
      for (int p = tid; p < IN_POS; p += 256) {
        const int qx = p % IN_PX, q = p / IN_PX, qy = q % IN_PY, qz = q / IN_PY;
        const int oz = oz0 + qz, oy = oy0 + qy, ox = ox0 + qx;
        float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0;
        if (oz < a.Do && oy < a.Ho && ox < a.Wo) {
          const unsigned off = (unsigned)oz * b.sd + (unsigned)oy * b.sh + (unsigned)ox * b.sw + (unsigned)oc;
          g0 = ld4_t<BF>(db, (long long)off);
          if (two) g1 = ld4_t<BF>(db, (long long)(off + 4u));
        }
        dys[0][p] = g0;
        dys[1][p] = g1;
      }
      __syncthreads();
      const float4* wc = in_w + oc;
      static_for<0, 8>([&](auto cls_) {
        constexpr int cls = decltype(cls_)::value, pz = cls >> 2, py = (cls >> 1) & 1, px = cls & 1;
        static_for<0, pz + 1>([&](auto jz_) {
          constexpr int jz = decltype(jz_)::value, tz = pz ? 2 * jz : 1, dz = (pz && jz == 0) ? 1 : 0;
          static_for<0, py + 1>([&](auto jy_) {
            constexpr int jy = decltype(jy_)::value, ty = py ? 2 * jy : 1, dy = (py && jy == 0) ? 1 : 0;
            static_for<0, px + 1>([&](auto jx_) {
              constexpr int jx = decltype(jx_)::value, tx = px ? 2 * jx : 1, dx = (px && jx == 0) ? 1 : 0;
              constexpr int tap = (tz * 3 + ty) * 3 + tx, dp = (dz * IN_PY + dy) * IN_PX + dx;
              const float4* wl = wc + tap * c0;
              const float4 g0 = dys[0][p0 + dp];
              const float4 w0 = wl[0], w1 = wl[1], w2 = wl[2], w3 = wl[3];
              float* q = acc[cls];
              q[0] = fmaf(g0.x, w0.x, q[0]); q[1] = fmaf(g0.x, w0.y, q[1]); q[2] = fmaf(g0.x, w0.z, q[2]); q[3] = fmaf(g0.x, w0.w, q[3]);
              q[0] = fmaf(g0.y, w1.x, q[0]); q[1] = fmaf(g0.y, w1.y, q[1]); q[2] = fmaf(g0.y, w1.z, q[2]); q[3] = fmaf(g0.y, w1.w, q[3]);
              q[0] = fmaf(g0.z, w2.x, q[0]); q[1] = fmaf(g0.z, w2.y, q[1]); q[2] = fmaf(g0.z, w2.z, q[2]); q[3] = fmaf(g0.z, w2.w, q[3]);
              q[0] = fmaf(g0.w, w3.x, q[0]); q[1] = fmaf(g0.w, w3.y, q[1]); q[2] = fmaf(g0.w, w3.z, q[2]); q[3] = fmaf(g0.w, w3.w, q[3]);
              if (two) {
                const float4 g1 = dys[1][p0 + dp];
                const float4 w4 = wl[4], w5 = wl[5], w6 = wl[6], w7 = wl[7];
                q[0] = fmaf(g1.x, w4.x, q[0]); q[1] = fmaf(g1.x, w4.y, q[1]); q[2] = fmaf(g1.x, w4.z, q[2]); q[3] = fmaf(g1.x, w4.w, q[3]);
                q[0] = fmaf(g1.y, w5.x, q[0]); q[1] = fmaf(g1.y, w5.y, q[1]); q[2] = fmaf(g1.y, w5.z, q[2]); q[3] = fmaf(g1.y, w5.w, q[3]);
                q[0] = fmaf(g1.z, w6.x, q[0]); q[1] = fmaf(g1.z, w6.y, q[1]); q[2] = fmaf(g1.z, w6.z, q[2]); q[3] = fmaf(g1.z, w6.w, q[3]);
                q[0] = fmaf(g1.w, w7.x, q[0]); q[1] = fmaf(g1.w, w7.y, q[1]); q[2] = fmaf(g1.w, w7.z, q[2]); q[3] = fmaf(g1.w, w7.w, q[3]);
              }
            });
          });
        });
      });
    }
  }
}

// the raw row of the thread's voxel of parity class `cls`, and whether the voxel is inside the volume (a voxel past it saw
// zeros or its neighbours' outputs: its dX' is dropped, and the row read in its place is the item's first)
template <int cls>
__device__ __forceinline__ bool in_voxel(const InGather& a, const InTile& t, int& iz, int& iy, int& ix) {
  constexpr int pz = cls >> 2, py = (cls >> 1) & 1, px = cls & 1;
  iz = t.bz * IN_TZ + 2 * t.lz + pz; iy = t.by * IN_TY + 2 * t.ly + py; ix = t.bx * IN_TX + 2 * t.lx + px;
  return iz < a.D && iy < a.H && ix < a.W;
}

// ------------------------------------------------------------------ Adam on one coefficient
// torch.optim.Adam's step (betas 0.9 / 0.999, eps 1e-8, no decay) on one fp32 coefficient `p` with gradient `g`, in fp64 on
// fp32 state; `t0` steps were taken before (0: the moments start from zero whatever the buffers hold); then the clamp to
// +- `bound`.
__device__ __forceinline__ float in_adam(float p, float g, int t0, double lr, double bound, float* __restrict__ m, float* __restrict__ v) {
  const double t = (double)(t0 + 1);
  const double b1 = 0.9, b2 = 0.999, eps = 1e-8;
  const double step_size = lr / (1.0 - pow(b1, t)), bc2_sqrt = sqrt(1.0 - pow(b2, t));
  const double gi = (double)g;
  const double m0 = t0 == 0 ? 0.0 : (double)*m, v0 = t0 == 0 ? 0.0 : (double)*v;
  const double m1 = b1 * m0 + (1.0 - b1) * gi, v1 = b2 * v0 + (1.0 - b2) * gi * gi;
  double q = (double)p - step_size * (m1 / (sqrt(v1) / bc2_sqrt + eps));
  q = fmin(fmax(q, -bound), bound);
  *m = (float)m1;
  *v = (float)v1;
  return (float)q;
}

// ------------------------------------------------------------------ host checks
// dense channels-last voxel rows of 4 lanes (<= 4 channels), aligned to a row; every row index of an item fits 31 bits
static inline int in_rows_check(const char* what, const char* name, const mmtta_tensor* t) {
  MMTTA_CHECK(t->n > 0 && t->c > 0 && t->d > 0 && t->h > 0 && t->w > 0, MMTTA_ERR_INVALID, "%s: empty `%s`", what, name);
  MMTTA_CHECK(t->c <= IN_ROW, MMTTA_ERR_UNSUPPORTED, "%s: `%s` has %d channels, more than %d", what, name, t->c, IN_ROW);
  MMTTA_CHECK(t->sc == 1 && t->sw == IN_ROW && t->sh == (int64_t)t->w * IN_ROW && t->sd == (int64_t)t->h * t->sh &&
                  t->sn % IN_ROW == 0 && t->sn >= (int64_t)t->d * t->sd,
              MMTTA_ERR_UNSUPPORTED, "%s: `%s` must be dense channels-last voxel rows of 4 lanes", what, name);
  MMTTA_CHECK(((uintptr_t)t->ptr) % (t->dtype == MMTTA_BF16 ? 8 : 16) == 0, MMTTA_ERR_UNSUPPORTED, "%s: misaligned `%s`", what, name);
  MMTTA_CHECK((long long)t->d * t->h * t->w * IN_ROW < (1ll << 31), MMTTA_ERR_UNSUPPORTED, "%s: an item of 2^31 elements or more", what);
  MMTTA_CHECK(t->n <= IN_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "%s: more than %d volumes in one call", what, IN_MAX_GRID_Y);
  return MMTTA_OK;
}

// x and y of a streaming pass (`what` names the entry point in the messages): the raw fp32 volume, never written, and rows
// of the same shape in fp32 or bf16 that own their pad lanes
static inline int in_apply_check(const char* what, const mmtta_tensor* x, const mmtta_tensor* y) {
  MMTTA_CHECK(x && x->ptr, MMTTA_ERR_INVALID, "%s: null `x`", what);
  MMTTA_CHECK(y && y->ptr, MMTTA_ERR_INVALID, "%s: null `y`", what);
  MMTTA_CHECK(same_shape(x, y), MMTTA_ERR_INVALID, "%s: shape mismatch between `x` and `y`", what);
  MMTTA_CHECK(x->ptr != y->ptr, MMTTA_ERR_INVALID, "%s: `y` must not be `x` (the raw volume is kept)", what);
  MMTTA_CHECK(is_f32(x), MMTTA_ERR_UNSUPPORTED, "%s: `x` must be fp32-stored (the raw volume)", what);
  MMTTA_CHECK(is_f32(y) || is_bf16(y), MMTTA_ERR_UNSUPPORTED, "%s: `y` must be fp32 or bf16", what);
  int st = in_rows_check(what, "x", x);
  if (st) return st;
  st = in_rows_check(what, "y", y);
  if (st) return st;
  MMTTA_CHECK(y->c == IN_ROW || (y->flags & MMTTA_TENSOR_OWNS_PAD), MMTTA_ERR_UNSUPPORTED, "%s: `y` must own the pad lanes of its rows",
              what);
  return MMTTA_OK;
}

static inline long long in_tiles(const mmtta_tensor* x, int& ty, int& tx) {
  const long long tz = (x->d + IN_TZ - 1) / IN_TZ;
  ty = (x->h + IN_TY - 1) / IN_TY;
  tx = (x->w + IN_TX - 1) / IN_TX;
  return tz * ty * tx;
}

// The branch checks of a reduced input gradient (k = 3, stride 2, pad 1, C -> c0 with c0 a multiple of 4 up to IN_MAX_C0; dy
// against the output extents of x) and the fill of the gather's description.  Nothing touches the device.
static inline int in_gather_fill(const char* what, const mmtta_tensor* x, const mmtta_input_norm_branch* branches, int n_branches,
                                 uint32_t keep_mask, InGather& a, long long& tiles) {
  const int Do = (x->d + 1) / 2, Ho = (x->h + 1) / 2, Wo = (x->w + 1) / 2;
  for (int r = 0; r < n_branches; ++r) {
    const mmtta_input_norm_branch& b = branches[r];
    MMTTA_CHECK(b.dy && b.dy->ptr, MMTTA_ERR_INVALID, "%s: null `dy` of branch %d", what, r);
    MMTTA_CHECK(b.weight != nullptr, MMTTA_ERR_INVALID, "%s: null `weight` of branch %d", what, r);
    MMTTA_CHECK(b.ksize == 3 && b.stride == 2, MMTTA_ERR_UNSUPPORTED,
                "%s: branch %d is a convolution k = %d, stride %d; the kernel gathers k = 3, stride 2, pad 1", what, r, b.ksize, b.stride);
    const mmtta_tensor* d = b.dy;
    MMTTA_CHECK(d->n == x->n && d->d == Do && d->h == Ho && d->w == Wo, MMTTA_ERR_INVALID,
                "%s: shape mismatch: `dy` of branch %d is [%d, %d, %d, %d], the input's outputs are [%d, %d, %d, %d]", what, r,
                d->n, d->d, d->h, d->w, x->n, Do, Ho, Wo);
    MMTTA_CHECK(d->c >= 4 && d->c % 4 == 0 && d->c <= IN_MAX_C0, MMTTA_ERR_UNSUPPORTED,
                "%s: branch %d has %d output channels (a multiple of 4 up to %d)", what, r, d->c, IN_MAX_C0);
    MMTTA_CHECK(d->c == branches[0].dy->c, MMTTA_ERR_INVALID, "%s: the branches differ in output channels (%d, %d)", what,
                branches[0].dy->c, d->c);
    MMTTA_CHECK(is_f32(d) || is_bf16(d), MMTTA_ERR_UNSUPPORTED, "%s: `dy` must be fp32 or bf16", what);
    MMTTA_CHECK(d->dtype == branches[0].dy->dtype, MMTTA_ERR_INVALID, "%s: storage mismatch between the branches' `dy`", what);
    MMTTA_CHECK(d->sc == 1, MMTTA_ERR_UNSUPPORTED, "%s: `dy` must be channels-last", what);
    MMTTA_CHECK(quad_aligned(d, quad_bytes(d)) && d->sw >= d->c && d->sh > 0 && d->sd > 0, MMTTA_ERR_UNSUPPORTED,
                "%s: misaligned `dy` of branch %d", what, r);
    MMTTA_CHECK(item_fits_31(d, d->c), MMTTA_ERR_UNSUPPORTED, "%s: an item of 2^31 elements or more", what);
    MMTTA_CHECK(b.set_stride >= 0, MMTTA_ERR_INVALID, "%s: negative set stride of branch %d", what, r);
    a.br[r].dy = (const float*)d->ptr;
    a.br[r].sn = d->sn; a.br[r].sd = (unsigned)d->sd; a.br[r].sh = (unsigned)d->sh; a.br[r].sw = (unsigned)d->sw;
    a.br[r].w = b.weight; a.br[r].wset = b.set_stride;
  }
  if (n_branches == 1) a.br[1] = a.br[0];
  a.x = (const uint4*)x->ptr;
  a.xsn = x->sn / IN_ROW;
  a.C = x->c; a.D = x->d; a.H = x->h; a.W = x->w; a.Do = Do; a.Ho = Ho; a.Wo = Wo;
  a.c0 = branches[0].dy->c; a.nbr = n_branches; a.keep = keep_mask;
  tiles = in_tiles(x, a.tiles_y, a.tiles_x);
  MMTTA_CHECK(tiles < (1ll << 31), MMTTA_ERR_UNSUPPORTED, "%s: 2^31 tiles or more", what);
  return MMTTA_OK;
}

}  // namespace mmtta
