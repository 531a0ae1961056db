// MEMO objective (Zhang, Levine, Finn, NeurIPS 2022) over the mirrored views of a volume (gfx950): the entropy of the
// MARGINAL prediction of V views, its gradient for every view, the view layout of the staged input and the ensemble of
// the views' predictions.  See include/mmtta.h for the contract of the four entry points.
//
// Batch layout everywhere: [G * V, D, H, W, R], item g * V + v = view v of volume g.  View v is the volume mirrored along
// the axes of mask view_axes[v] (bit 0 = W, 1 = H, 2 = D); mirroring is an involution on the voxel grid, so voxel
// (z, y, x) of the volume's own frame is voxel (z', y', x') of view v with x' = W-1-x where the mask says so.  A thread owns
// a voxel of the volume's frame and visits its V images.  Inside a row of W the order of voxels reverses, but the 64 voxels
// of a wavefront still cover one contiguous segment of every view: the accesses stay coalesced.
//
// Bit 4 (value 16) of a view's code transposes H and W BEFORE the mirrors of bits 0-2 (H == W is required; bit 4 stays
// unused and invalid, so the codes are 0..7 and 16..23): a quarter turn in the (H, W) plane is code 18 (k = 1), 3 (k = 2)
// or 17 (k = 3).  Voxel (z, y, x) of the volume's frame then sits at view voxel
// (fd(z), fh(x), fw(y)), f* = the mirror of that VIEW axis where its bit is set; bringing a view back to the frame is flip,
// then transpose - a view is no longer its own inverse.  A call without such a code launches the kernels of the mirror
// group (the <false> instantiations below and memo_bernoulli_vec_kernel, untouched).  With one, 64 consecutive frame voxels
// land W rows apart in the view, so the per-step kernels of the fast path take a tiled form (memo_bernoulli_tiled_kernel,
// memo_ensemble_tiled_kernel: the view's tile is loaded along the VIEW's W and turned through LDS); the generic Bernoulli,
// categorical, generic ensemble and mirror kernels follow the coordinate map alone and are UNCOALESCED for transposed views.
#include "voxel_loss.h"

namespace mmtta {

constexpr int MEMO_MAX_V = 8;
constexpr int MEMO_TURN = 16;              // bit 4 of a view's code: H and W transposed before the mirrors of bits 0-2
constexpr float MEMO_TINY = 1.17549435e-38f;   // smallest normal fp32: v_log_f32 and x log x stay finite from here up

struct MemoViews {
  int v;
  int axes[MEMO_MAX_V];
};

// coordinates of linear voxel i (32-bit: the host checks D*H*W*ldc < 2^31) and of its mirror image
struct MemoVox {
  unsigned x, y, z, xm, ym, zm;
};
__device__ __forceinline__ MemoVox memo_vox(unsigned i, unsigned D, unsigned H, unsigned W) {
  MemoVox p;
  const unsigned t = i / W;
  p.x = i - t * W;
  p.z = t / H;
  p.y = t - p.z * H;
  p.xm = W - 1 - p.x; p.ym = H - 1 - p.y; p.zm = D - 1 - p.z;
  return p;
}
// linear voxel index of the image of `p` in a view with mirror mask `m` (wave-uniform selects)
__device__ __forceinline__ unsigned memo_image(const MemoVox& p, int m, unsigned H, unsigned W) {
  const unsigned xx = (m & 1) ? p.xm : p.x, yy = (m & 2) ? p.ym : p.y, zz = (m & 4) ? p.zm : p.z;
  return (zz * H + yy) * W + xx;
}

// coordinates (z, y, x) of the image of frame voxel `p` in a view with code `m`; TR = false: the mirror group's own
// expressions (bit 4 is never set there), TR = true: bit 4 swaps the roles of y and x (H == W, so ym / xm mirror either axis)
template <bool TR>
__device__ __forceinline__ void memo_view_zyx(const MemoVox& p, int m, unsigned& zz, unsigned& yy, unsigned& xx) {
  zz = (m & 4) ? p.zm : p.z;
  if (TR && (m & MEMO_TURN)) {
    yy = (m & 2) ? p.xm : p.x;
    xx = (m & 1) ? p.ym : p.y;
  } else {
    yy = (m & 2) ? p.ym : p.y;
    xx = (m & 1) ? p.xm : p.x;
  }
}
template <bool TR>
__device__ __forceinline__ long long memo_addr(const TV& t, long long item, const MemoVox& p, int m) {
  if (!TR) return vox_addr(t, (int)item, (m & 4) ? p.zm : p.z, (m & 2) ? p.ym : p.y, (m & 1) ? p.xm : p.x);
  unsigned zz, yy, xx;
  memo_view_zyx<true>(p, m, zz, yy, xx);
  return vox_addr(t, (int)item, zz, yy, xx);
}

// sigmoid(t), sigmoid(-t) and their product, none formed by subtraction: v_exp_f32 / v_rcp_f32 as the entropy fast path
__device__ __forceinline__ void memo_sigmoid_terms(float t, float& p, float& q, float& pq) {
  const SigmoidPair s = sigmoid_pair(t, exp_neg_abs(t));
  p = s.p;
  q = s.q;
  pq = s.er * s.r;
}
__device__ __forceinline__ float memo_ln(float x) { return __builtin_amdgcn_logf(x) * 0.6931471805599453f; }   // x normal
// log p and log q of a complementary pair (p + q = 1 up to rounding), finite for p or q = 0: the log of the smaller one is
// taken at max(s, smallest normal) - s log s is below 1e-35 there - and the log of the larger one is log1p(-s), the 4-term
// series below 2^-6 (relative error < 2e-8) and log(1 - s) above, as the entropy fast path takes its log1p
__device__ __forceinline__ void memo_pair_logs(float p, float q, float& lp, float& lq) {
  const float s = fminf(p, q);
  const float ls = memo_ln(fmaxf(s, MEMO_TINY));
  const float series = -s * fmaf(s, fmaf(s, fmaf(s, 0.25f, 0.33333334f), 0.5f), 1.f);
  const float lb = s < 0.015625f ? series : memo_ln(1.f - s);
  const bool pbig = p >= q;
  lp = pbig ? lb : ls;
  lq = pbig ? ls : lb;
}

// ------------------------------------------------------------------ marginal entropy, Bernoulli head
// Fast path: <= 4 regions in dense 16-byte voxel rows.  Per view and voxel one 16-byte load and one 16- / 8-byte store
// (the gradient tensor owns its pad lane), two 32-bit divisions per voxel, ~2 logs per (voxel, region) and one exp per
// view.  gridDim.y = volume; the block partials and the scale of a volume are those of a call on that volume alone.
template <int V, bool OBF>
__global__ __launch_bounds__(256) void memo_bernoulli_vec_kernel(const float* __restrict__ z, float* __restrict__ dz,
                                                                 long long zsn, long long dzsn, int C, unsigned D, unsigned H,
                                                                 unsigned W, MemoViews mv, double* partial, float inv_count) {
  __shared__ double sh[4];
  const long long item0 = (long long)blockIdx.y * V;
  partial += (long long)blockIdx.y * gridDim.x;
  const unsigned dhw = D * H * W;
  const float inv_v = 1.f / (float)V;
  double acc = 0.0;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < dhw; i += gridDim.x * 256u) {
    const MemoVox pos = memo_vox(i, D, H, W);
    unsigned off[V];
    float4 t4[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      off[v] = memo_image(pos, mv.axes[v], H, W) * 4u;
      t4[v] = *reinterpret_cast<const float4*>(z + (item0 + v) * zsn + off[v]);
    }
    float pq[V][4];
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    float h = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < C) {
        float ps = 0.f, qs = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const float t = c == 0 ? t4[v].x : (c == 1 ? t4[v].y : (c == 2 ? t4[v].z : t4[v].w));
          float p, q;
          memo_sigmoid_terms(t, p, q, pq[v][c]);
          ps += p; qs += q;
        }
        const float pbar = ps * inv_v, qbar = qs * inv_v;
        float lp, lq;
        memo_pair_logs(pbar, qbar, lp, lq);
        h -= fmaf(pbar, lp, qbar * lq);
        f[c] = (lq - lp) * inv_count;
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) pq[v][c] = 0.f;
      }
    }
    acc += (double)h;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      float* gb = OBF ? reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(dz) + (item0 + v) * dzsn)
                      : dz + (item0 + v) * dzsn;
      st4_any(gb, off[v], make_float4(f[0] * pq[v][0], f[1] * pq[v][1], f[2] * pq[v][2], f[3] * pq[v][3]), OBF);
    }
  }
  const double t = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// Tiled fast path, taken when a view of the call is transposed (bit 4).  A workgroup owns a 16 x 16 tile of one z-plane of
// the volume's frame, thread (th, tw) = (threadIdx.x / 16, threadIdx.x % 16) owns frame voxel (h0 + th, w0 + tw).  A direct
// view is read and written at the mirror kernel's addresses (16 voxels = 256 contiguous bytes per row of the tile).  The
// image of the tile in a transposed view is again a 16 x 16 square of the view, whose rows run along the frame's H: thread
// (th, tw) MOVES the row of frame voxel (h0 + tw, w0 + th) - consecutive lanes, consecutive voxels of the view's W - and
// hands it through LDS to the thread that owns it; the gradient goes back the same way.  A 16-byte element of row r, column
// c of the square sits at slot r * 16 + (c ^ r): the mover's ds_write_b128 (r fixed, 8 consecutive c per lane group) and the
// owner's ds_read_b128 (c ^ r over the 16 lanes of a group takes 16 distinct values: 64 distinct banks) are conflict-free,
// which a padded pitch of 17 is not (lanes 12 and 27 of the first group meet).  Loads are unconditional, from clamped
// coordinates, and masked afterwards; tiles are walked in a grid-stride loop under memo_blocks' block count, so the partials
// of a volume are sized as before (a workgroup without a tile writes a zero).  The arithmetic per voxel is
// memo_bernoulli_vec_kernel's, expression by expression: equal rows give equal gradient bits.
constexpr unsigned MEMO_TILE = 16;
__device__ __forceinline__ unsigned memo_tile_offset(int m, unsigned D, unsigned H, unsigned W, unsigned z, unsigned h, unsigned w) {
  // element offset (4 per voxel) of the image of frame voxel (z, h, w) under code m (wave-uniform selects)
  const unsigned a = (m & MEMO_TURN) ? w : h, b = (m & MEMO_TURN) ? h : w;
  const unsigned zz = (m & 4) ? D - 1 - z : z, yy = (m & 2) ? H - 1 - a : a, xx = (m & 1) ? W - 1 - b : b;
  return ((zz * H + yy) * W + xx) * 4u;
}
struct MemoTile {
  unsigned z, h, w, hm, wm;      // own frame voxel (h, w) and the one moved for transposed views (hm, wm), both clamped
  bool live, livem;              // ... and whether they lie inside the volume
};
__device__ __forceinline__ MemoTile memo_tile(unsigned tile, unsigned tiles_h, unsigned tiles_w, unsigned H, unsigned W) {
  const unsigned th = threadIdx.x >> 4, tw = threadIdx.x & 15u;
  const unsigned per = tiles_h * tiles_w;
  MemoTile t;
  t.z = tile / per;
  const unsigned r = tile - t.z * per, ty = r / tiles_w, tx = r - ty * tiles_w;
  const unsigned h = ty * MEMO_TILE + th, w = tx * MEMO_TILE + tw, hm = ty * MEMO_TILE + tw, wm = tx * MEMO_TILE + th;
  t.live = h < H && w < W;
  t.livem = hm < H && wm < W;
  t.h = min(h, H - 1); t.w = min(w, W - 1); t.hm = min(hm, H - 1); t.wm = min(wm, W - 1);
  return t;
}

template <int V, bool OBF>
__global__ __launch_bounds__(256) void memo_bernoulli_tiled_kernel(const float* __restrict__ z, float* __restrict__ dz,
                                                                   long long zsn, long long dzsn, int C, unsigned D, unsigned H,
                                                                   unsigned W, MemoViews mv, double* partial, float inv_count) {
  __shared__ double sh[4];
  __shared__ float4 turn[V][MEMO_TILE * MEMO_TILE];
  const long long item0 = (long long)blockIdx.y * V;
  partial += (long long)blockIdx.y * gridDim.x;
  const unsigned tiles_h = (H + MEMO_TILE - 1) / MEMO_TILE, tiles_w = (W + MEMO_TILE - 1) / MEMO_TILE;
  const unsigned tiles = D * tiles_h * tiles_w;
  const unsigned th = threadIdx.x >> 4, tw = threadIdx.x & 15u;
  const unsigned mine = th * MEMO_TILE + (tw ^ th);        // slot this thread fills (rows it moves in, gradients it hands out)
  const unsigned theirs = tw * MEMO_TILE + (th ^ tw);      // slot filled for it by thread (tw, th)
  const float inv_v = 1.f / (float)V;
  double acc = 0.0;
  for (unsigned tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const MemoTile pos = memo_tile(tile, tiles_h, tiles_w, H, W);
    unsigned off[V];
    float4 t4[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int m = mv.axes[v];
      off[v] = (m & MEMO_TURN) ? memo_tile_offset(m, D, H, W, pos.z, pos.hm, pos.wm) : memo_tile_offset(m, D, H, W, pos.z, pos.h, pos.w);
      t4[v] = *reinterpret_cast<const float4*>(z + (item0 + v) * zsn + off[v]);
    }
#pragma unroll
    for (int v = 0; v < V; ++v)
      if (mv.axes[v] & MEMO_TURN) turn[v][mine] = t4[v];
    __syncthreads();
#pragma unroll
    for (int v = 0; v < V; ++v)
      if (mv.axes[v] & MEMO_TURN) t4[v] = turn[v][theirs];
    float pq[V][4];
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    float h = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < C) {
        float ps = 0.f, qs = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const float t = c == 0 ? t4[v].x : (c == 1 ? t4[v].y : (c == 2 ? t4[v].z : t4[v].w));
          float p, q;
          memo_sigmoid_terms(t, p, q, pq[v][c]);
          ps += p; qs += q;
        }
        const float pbar = ps * inv_v, qbar = qs * inv_v;
        float lp, lq;
        memo_pair_logs(pbar, qbar, lp, lq);
        h -= fmaf(pbar, lp, qbar * lq);
        f[c] = (lq - lp) * inv_count;
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) pq[v][c] = 0.f;
      }
    }
    acc += pos.live ? (double)h : 0.0;
    // a slot is touched by two threads only - its mover (row in, gradient out) and its owner (row out, gradient in), each
    // in program order: the two barriers of a tile are all the ordering there is to keep
    float4 g4[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      g4[v] = make_float4(f[0] * pq[v][0], f[1] * pq[v][1], f[2] * pq[v][2], f[3] * pq[v][3]);
      if (mv.axes[v] & MEMO_TURN) turn[v][theirs] = g4[v];
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const bool tr = (mv.axes[v] & MEMO_TURN) != 0;
      if (tr) g4[v] = turn[v][mine];
      float* gb = OBF ? reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(dz) + (item0 + v) * dzsn)
                      : dz + (item0 + v) * dzsn;
      if (tr ? pos.livem : pos.live) st4_any(gb, off[v], g4[v], OBF);
    }
  }
  const double t = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// Generic path: any R, any row stride, fp32 gradients; a thread owns a (voxel, region) pair.
template <bool TR>
__global__ __launch_bounds__(256) void memo_bernoulli_kernel(TV z, TV dz, MemoViews mv, double* partial, float inv_count) {
  __shared__ double sh[4];
  const int V = mv.v;
  const long long item0 = (long long)blockIdx.y * V;
  partial += (long long)blockIdx.y * gridDim.x;
  const unsigned C = z.c, D = z.d, H = z.h, W = z.w;
  const unsigned total = D * H * W * C;
  const float inv_v = 1.f / (float)V;
  double acc = 0.0;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned vox = i / C, c = i - vox * C;
    const MemoVox pos = memo_vox(vox, D, H, W);
    float pq[MEMO_MAX_V];
    float ps = 0.f, qs = 0.f;
#pragma unroll
    for (int v = 0; v < MEMO_MAX_V; ++v) {
      if (v < V) {
        const int m = mv.axes[v];
        const long long a = memo_addr<TR>(z, item0 + v, pos, m);
        float p, q;
        memo_sigmoid_terms(z.p[a + c], p, q, pq[v]);
        ps += p; qs += q;
      }
    }
    const float pbar = ps * inv_v, qbar = qs * inv_v;
    float lp, lq;
    memo_pair_logs(pbar, qbar, lp, lq);
    acc += (double)(-fmaf(pbar, lp, qbar * lq));
    const float f = (lq - lp) * inv_count;
#pragma unroll
    for (int v = 0; v < MEMO_MAX_V; ++v) {
      if (v < V) {
        const int m = mv.axes[v];
        const long long a = memo_addr<TR>(dz, item0 + v, pos, m);
        dz.p[a + c] = f * pq[v];
      }
    }
  }
  const double t = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// ------------------------------------------------------------------ marginal entropy, categorical head
// log softmax of one voxel row into lp[0..R), finite for every finite row (a difference that overflows is held at -3e38)
__device__ __forceinline__ void memo_log_softmax_row(const float* zp, int R, float (&lp)[LOSS_MAX_R]) {
  float m = -INFINITY;
#pragma unroll
  for (int r = 0; r < LOSS_MAX_R; ++r)
    if (r < R) { lp[r] = zp[r]; m = fmaxf(m, lp[r]); }
  float se = 0.f;
#pragma unroll
  for (int r = 0; r < LOSS_MAX_R; ++r)
    if (r < R) se += expf(lp[r] - m);
  // (t - m) - log(se), not t - (m + log(se)): at logits of 1e4 the sum m + log(se) would round log(se) to 1e-3
  const float lg = logf(se);             // se >= 1: the maximum contributes exp(0)
#pragma unroll
  for (int r = 0; r < LOSS_MAX_R; ++r)
    if (r < R) lp[r] = fmaxf((lp[r] - m) - lg, -3e38f);
}
// log pbar_r = logsumexp_v(log softmax_r(u_v)) - log V, accumulated view by view (running maximum mx, scaled sum sm):
// the log-domain form keeps the relative accuracy of small probabilities, and one view gives its log softmax back exactly
__device__ __forceinline__ void memo_lse_add(float lp, bool first, float& mx, float& sm) {
  if (first) { mx = lp; sm = 1.f; return; }
  const float nm = fmaxf(mx, lp);
  sm = sm * expf(mx - nm) + expf(lp - nm);
  mx = nm;
}
template <bool TR>
__device__ __forceinline__ const float* memo_row(const TV& z, long long item, const MemoVox& pos, int m) {
  return z.p + memo_addr<TR>(z, item, pos, m);
}

// A thread owns a voxel.  Two sweeps over the views (the second one re-reads the rows through the cache): the marginal
// needs every view before any gradient can be written, and V x R probabilities do not fit the register file.
template <bool TR>
__global__ __launch_bounds__(256) void memo_categorical_kernel(TV z, TV dz, MemoViews mv, double* partial, float inv_count) {
  __shared__ double sh[4];
  const int V = mv.v, R = z.c;
  const long long item0 = (long long)blockIdx.y * V;
  partial += (long long)blockIdx.y * gridDim.x;
  const unsigned D = z.d, H = z.h, W = z.w;
  const unsigned total = D * H * W;
  const float log_v = logf((float)V);
  double acc = 0.0;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const MemoVox pos = memo_vox(i, D, H, W);
    float lpb[LOSS_MAX_R], sm[LOSS_MAX_R], lp[LOSS_MAX_R];
    for (int v = 0; v < V; ++v) {
      memo_log_softmax_row(memo_row<TR>(z, item0 + v, pos, mv.axes[v]), R, lp);
#pragma unroll
      for (int r = 0; r < LOSS_MAX_R; ++r)
        if (r < R) memo_lse_add(lp[r], v == 0, lpb[r], sm[r]);
    }
    float h = 0.f;
#pragma unroll
    for (int r = 0; r < LOSS_MAX_R; ++r)
      if (r < R) {
        lpb[r] = lpb[r] + logf(sm[r]) - log_v;
        h -= expf(lpb[r]) * lpb[r];
      }
    acc += (double)h;
    for (int v = 0; v < V; ++v) {
      memo_log_softmax_row(memo_row<TR>(z, item0 + v, pos, mv.axes[v]), R, lp);
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < LOSS_MAX_R; ++r)
        if (r < R) { lp[r] = expf(lp[r]); s = fmaf(lp[r], lpb[r], s); }
      float* gp = const_cast<float*>(memo_row<TR>(dz, item0 + v, pos, mv.axes[v]));
#pragma unroll
      for (int r = 0; r < LOSS_MAX_R; ++r)
        if (r < R) gp[r] = lp[r] * (s - lpb[r]) * inv_count;
    }
  }
  const double t = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// ------------------------------------------------------------------ ensemble of the views' predictions
// out[g] = logit(pbar) (Bernoulli; a thread per (voxel, region)) or log pbar (categorical; a thread per voxel; log-sum-exp over the views) in the
// volume's frame.  Where pbar or qbar underflows the logit is +-87.3365 (-ln of the smallest normal: as far as the fp32
// sigmoid inverts).  V = 1: the Bernoulli ensemble is the logits themselves.
template <bool TR>
__global__ __launch_bounds__(256) void memo_ensemble_bernoulli_kernel(TV z, TV out, MemoViews mv) {
  const int V = mv.v;
  const long long item0 = (long long)blockIdx.y * V;
  const unsigned C = z.c, D = z.d, H = z.h, W = z.w;
  const unsigned total = D * H * W * C;
  const float inv_v = 1.f / (float)V;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned vox = i / C, c = i - vox * C;
    const MemoVox pos = memo_vox(vox, D, H, W);
    float ps = 0.f, qs = 0.f, t0 = 0.f;
#pragma unroll
    for (int v = 0; v < MEMO_MAX_V; ++v) {
      if (v < V) {
        const int m = mv.axes[v];
        const float t = z.p[memo_addr<TR>(z, item0 + v, pos, m) + c];
        if (v == 0) t0 = t;
        float p, q, pq;
        memo_sigmoid_terms(t, p, q, pq);
        ps += p; qs += q;
      }
    }
    float lp, lq;
    memo_pair_logs(ps * inv_v, qs * inv_v, lp, lq);
    out.p[vox_addr(out, (int)blockIdx.y, pos.z, pos.y, pos.x) + c] = V == 1 ? t0 : lp - lq;
  }
}

// The Bernoulli ensemble over dense 16-byte rows with a transposed view in the call: memo_bernoulli_tiled_kernel's gather
// (same tiles, same slots), memo_ensemble_bernoulli_kernel's arithmetic; a thread writes its voxel's
// whole row of `out` (the pad lanes, which `out` owns, take 0).
template <int V>
__global__ __launch_bounds__(256) void memo_ensemble_tiled_kernel(const float* __restrict__ z, float* __restrict__ out, long long zsn,
                                                                  long long osn, int C, unsigned D, unsigned H, unsigned W,
                                                                  MemoViews mv) {
  __shared__ float4 turn[V][MEMO_TILE * MEMO_TILE];
  const long long item0 = (long long)blockIdx.y * V;
  const unsigned tiles_h = (H + MEMO_TILE - 1) / MEMO_TILE, tiles_w = (W + MEMO_TILE - 1) / MEMO_TILE;
  const unsigned tiles = D * tiles_h * tiles_w;
  const unsigned th = threadIdx.x >> 4, tw = threadIdx.x & 15u;
  const unsigned mine = th * MEMO_TILE + (tw ^ th), theirs = tw * MEMO_TILE + (th ^ tw);
  const float inv_v = 1.f / (float)V;
  float* ob = out + (long long)blockIdx.y * osn;
  for (unsigned tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const MemoTile pos = memo_tile(tile, tiles_h, tiles_w, H, W);
    float4 t4[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int m = mv.axes[v];
      const unsigned off = (m & MEMO_TURN) ? memo_tile_offset(m, D, H, W, pos.z, pos.hm, pos.wm) : memo_tile_offset(m, D, H, W, pos.z, pos.h, pos.w);
      t4[v] = *reinterpret_cast<const float4*>(z + (item0 + v) * zsn + off);
    }
#pragma unroll
    for (int v = 0; v < V; ++v)
      if (mv.axes[v] & MEMO_TURN) turn[v][mine] = t4[v];
    __syncthreads();
#pragma unroll
    for (int v = 0; v < V; ++v)
      if (mv.axes[v] & MEMO_TURN) t4[v] = turn[v][theirs];
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < C) {
        float ps = 0.f, qs = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const float t = c == 0 ? t4[v].x : (c == 1 ? t4[v].y : (c == 2 ? t4[v].z : t4[v].w));
          float p, q, pq;
          memo_sigmoid_terms(t, p, q, pq);
          ps += p; qs += q;
        }
        float lp, lq;
        memo_pair_logs(ps * inv_v, qs * inv_v, lp, lq);
        o[c] = lp - lq;
      }
    }
    if (pos.live) *reinterpret_cast<float4*>(ob + memo_tile_offset(0, D, H, W, pos.z, pos.h, pos.w)) = make_float4(o[0], o[1], o[2], o[3]);
    __syncthreads();      // the owners have read their slots: the movers may fill them for the next tile
  }
}

template <bool TR>
__global__ __launch_bounds__(256) void memo_ensemble_categorical_kernel(TV z, TV out, MemoViews mv) {
  const int V = mv.v, R = z.c;
  const long long item0 = (long long)blockIdx.y * V;
  const unsigned D = z.d, H = z.h, W = z.w;
  const unsigned total = D * H * W;
  const float log_v = logf((float)V);
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const MemoVox pos = memo_vox(i, D, H, W);
    float lpb[LOSS_MAX_R], sm[LOSS_MAX_R], lp[LOSS_MAX_R];
    for (int v = 0; v < V; ++v) {
      memo_log_softmax_row(memo_row<TR>(z, item0 + v, pos, mv.axes[v]), R, lp);
#pragma unroll
      for (int r = 0; r < LOSS_MAX_R; ++r)
        if (r < R) memo_lse_add(lp[r], v == 0, lpb[r], sm[r]);
    }
    float* op = out.p + vox_addr(out, (int)blockIdx.y, pos.z, pos.y, pos.x);
#pragma unroll
    for (int r = 0; r < LOSS_MAX_R; ++r)
      if (r < R) op[r] = lpb[r] + logf(sm[r]) - log_v;
  }
}

// ------------------------------------------------------------------ the mirrored views of the staged input
// y[g * V + v] = x[g] mirrored along the axes of view v; a voxel's whole row (pad lanes included) moves as `upr` units of
// type T.  A thread owns a unit of the OUTPUT; gridDim.y = output item.  Once per volume: index arithmetic is not tuned.
// A mirror is its own inverse, a transposed view is not: voxel (z', y', x') of a view with bit 4 holds frame voxel
// (fd(z'), fw(x'), fh(y')) (TR = true; the gather runs W rows apart there: uncoalesced, once per volume).
template <class T, bool TR>
__global__ __launch_bounds__(256) void memo_mirror_kernel(const T* __restrict__ x, T* __restrict__ y, long long xsn, long long ysn,
                                                          unsigned upr, unsigned D, unsigned H, unsigned W, MemoViews mv) {
  const int item = blockIdx.y, g = item / mv.v, m = mv.axes[item - g * mv.v];
  const unsigned total = D * H * W * upr;
  const T* xb = x + (long long)g * xsn;
  T* yb = y + (long long)item * ysn;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned vox = i / upr, u = i - vox * upr;
    const MemoVox pos = memo_vox(vox, D, H, W);
    unsigned src;
    if (TR && (m & MEMO_TURN)) src = ((((m & 4) ? pos.zm : pos.z) * H + ((m & 1) ? pos.xm : pos.x)) * W + ((m & 2) ? pos.ym : pos.y));
    else src = memo_image(pos, m, H, W);
    yb[i] = xb[src * upr + u];
  }
}

// `turned`: a view of the call transposes H and W (bit 4), which needs square (H, W) planes
static int memo_views_check(const char* what, int views, const int32_t* view_axes, const mmtta_tensor* t, MemoViews& mv, bool& turned) {
  const int n = t->n;
  MMTTA_CHECK(views == 1 || views == 2 || views == 4 || views == 8, MMTTA_ERR_INVALID, "%s: views = %d (1, 2, 4 or 8)", what, views);
  MMTTA_CHECK(view_axes != nullptr, MMTTA_ERR_INVALID, "%s: null argument (view_axes)", what);
  MMTTA_CHECK(view_axes[0] == 0, MMTTA_ERR_INVALID, "%s: view_axes[0] = %d, view 0 is the unmirrored volume", what, view_axes[0]);
  mv.v = views;
  for (int v = 0; v < MEMO_MAX_V; ++v) {
    mv.axes[v] = v < views ? view_axes[v] : 0;
    MMTTA_CHECK((mv.axes[v] & ~(7 | MEMO_TURN)) == 0, MMTTA_ERR_INVALID,
                "%s: view_axes[%d] = %d (bit 0 = W, 1 = H, 2 = D mirrored, bit 4 = H and W transposed first)", what, v, mv.axes[v]);
  }
  MMTTA_CHECK(n >= views && n % views == 0, MMTTA_ERR_INVALID, "%s: batch %d is no multiple of views %d", what, n, views);
  turned = false;
  for (int v = 0; v < views; ++v)
    if (mv.axes[v] & MEMO_TURN) {
      turned = true;
      MMTTA_CHECK(t->h == t->w, MMTTA_ERR_INVALID, "%s: view_axes[%d] = %d transposes H and W, which needs h == w: h = %d, w = %d",
                  what, v, mv.axes[v], t->h, t->w);
    }
  return MMTTA_OK;
}

}  // namespace mmtta

using namespace mmtta;

extern "C" int64_t mmtta_memo_partials(const mmtta_tensor* logits, int views) {
  if (logits == nullptr || !(views == 1 || views == 2 || views == 4 || views == 8) || logits->n < views || logits->n % views) return -1;
  return (int64_t)loss_blocks(logits) * (logits->n / views);
}

extern "C" int mmtta_memo_loss_items(const mmtta_tensor* logits, int softmax, int views, const int32_t* view_axes,
                                     const mmtta_tensor* dlogits, double* partial, float* loss, void* stream) {
  MMTTA_CHECK(logits && dlogits && partial && loss && logits->ptr && dlogits->ptr, MMTTA_ERR_INVALID, "memo loss: null argument");
  MemoViews mv;
  bool turned;
  int st = memo_views_check("memo loss", views, view_axes, logits, mv, turned);
  if (st) return st;
  MMTTA_CHECK(logits->n == dlogits->n && logits->c == dlogits->c && logits->d == dlogits->d && logits->h == dlogits->h &&
                  logits->w == dlogits->w, MMTTA_ERR_INVALID, "memo loss: shape mismatch");
  // one view: nothing is mirrored and the marginal is that view's prediction - the entropy objective itself, same kernels
  // and same bits (mmtta_memo_partials(logits, 1) is mmtta_entropy_partials_items(logits))
  if (views == 1) return mmtta_entropy_loss_items(logits, softmax, dlogits, partial, loss, stream);
  MMTTA_CHECK(logits->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "memo loss: `logits` must be fp32-stored");
  MMTTA_CHECK(is_cl(logits) && is_cl(dlogits), MMTTA_ERR_UNSUPPORTED, "memo loss: channels-last only");
  MMTTA_CHECK(loss_small_item(logits) && loss_small_item(dlogits), MMTTA_ERR_UNSUPPORTED, "memo loss: an item of 2^31 elements or more");
  hipStream_t s = (hipStream_t)stream;
  const int volumes = logits->n / views;
  MMTTA_CHECK(volumes <= LOSS_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "memo loss: more than %d volumes in one call", LOSS_MAX_GRID_Y);
  const int blocks = loss_blocks(logits);
  const long long nvox = (long long)logits->d * logits->h * logits->w;
  const dim3 grid(blocks, volumes);
  const double cnt = softmax ? (double)nvox : (double)nvox * logits->c;
  const float inv = (float)(1.0 / (cnt * views));
  if (!softmax) {
    const bool vec = logits->c <= 4 && loss_dense16(logits) && loss_dense16(dlogits) &&
                     ((dlogits->flags & MMTTA_TENSOR_OWNS_PAD) || dlogits->c == 4);
    MMTTA_CHECK(is_f32(dlogits) || vec, MMTTA_ERR_UNSUPPORTED, "memo loss: a bf16-stored `dlogits` needs dense 4-channel voxel rows that own their pad");
    if (vec) {
      const float* zp = (const float*)logits->ptr;
      float* gp = (float*)dlogits->ptr;
#define MEMO_VEC(VV)                                                                                                          \
  do {                                                                                                                        \
    if (is_bf16(dlogits))                                                                                                     \
      hipLaunchKernelGGL((memo_bernoulli_vec_kernel<VV, true>), grid, dim3(256), 0, s, zp, gp, (long long)logits->sn,          \
                         (long long)dlogits->sn, (int)logits->c, (unsigned)logits->d, (unsigned)logits->h, (unsigned)logits->w, \
                         mv, partial, inv);                                                                                   \
    else                                                                                                                      \
      hipLaunchKernelGGL((memo_bernoulli_vec_kernel<VV, false>), grid, dim3(256), 0, s, zp, gp, (long long)logits->sn,         \
                         (long long)dlogits->sn, (int)logits->c, (unsigned)logits->d, (unsigned)logits->h, (unsigned)logits->w, \
                         mv, partial, inv);                                                                                   \
  } while (0)
#define MEMO_TILED(VV)                                                                                                        \
  do {                                                                                                                        \
    if (is_bf16(dlogits))                                                                                                     \
      hipLaunchKernelGGL((memo_bernoulli_tiled_kernel<VV, true>), grid, dim3(256), 0, s, zp, gp, (long long)logits->sn,        \
                         (long long)dlogits->sn, (int)logits->c, (unsigned)logits->d, (unsigned)logits->h, (unsigned)logits->w, \
                         mv, partial, inv);                                                                                   \
    else                                                                                                                      \
      hipLaunchKernelGGL((memo_bernoulli_tiled_kernel<VV, false>), grid, dim3(256), 0, s, zp, gp, (long long)logits->sn,       \
                         (long long)dlogits->sn, (int)logits->c, (unsigned)logits->d, (unsigned)logits->h, (unsigned)logits->w, \
                         mv, partial, inv);                                                                                   \
  } while (0)
      if (!turned) {
        if (views == 2) MEMO_VEC(2);
        else if (views == 4) MEMO_VEC(4);
        else MEMO_VEC(8);
      } else {
        if (views == 2) MEMO_TILED(2);
        else if (views == 4) MEMO_TILED(4);
        else MEMO_TILED(8);
      }
#undef MEMO_TILED
#undef MEMO_VEC
    } else if (!turned) {
      hipLaunchKernelGGL(memo_bernoulli_kernel<false>, grid, dim3(256), 0, s, tv(logits), tv(dlogits), mv, partial, inv);
    } else {
      hipLaunchKernelGGL(memo_bernoulli_kernel<true>, grid, dim3(256), 0, s, tv(logits), tv(dlogits), mv, partial, inv);
    }
    st = launch_status("memo bernoulli");
  } else {
    MMTTA_CHECK(logits->c <= LOSS_MAX_R, MMTTA_ERR_UNSUPPORTED, "memo loss softmax: more than %d classes", LOSS_MAX_R);
    MMTTA_CHECK(is_f32(dlogits), MMTTA_ERR_UNSUPPORTED, "memo loss softmax: `dlogits` must be fp32-stored");
    if (!turned)
      hipLaunchKernelGGL(memo_categorical_kernel<false>, grid, dim3(256), 0, s, tv(logits), tv(dlogits), mv, partial, inv);
    else
      hipLaunchKernelGGL(memo_categorical_kernel<true>, grid, dim3(256), 0, s, tv(logits), tv(dlogits), mv, partial, inv);
    st = launch_status("memo categorical");
  }
  if (st) return st;
  hipLaunchKernelGGL(mean_finish_kernel, dim3(volumes), dim3(64), 0, s, partial, blocks, 1.0 / cnt, loss);
  return launch_status("memo finish");
}

extern "C" int mmtta_memo_ensemble(const mmtta_tensor* logits, int softmax, int views, const int32_t* view_axes,
                                   const mmtta_tensor* out, void* stream) {
  MMTTA_CHECK(logits && out && logits->ptr && out->ptr, MMTTA_ERR_INVALID, "memo ensemble: null argument");
  MemoViews mv;
  bool turned;
  int st = memo_views_check("memo ensemble", views, view_axes, logits, mv, turned);
  if (st) return st;
  MMTTA_CHECK(logits->n == out->n * views && logits->c == out->c && logits->d == out->d && logits->h == out->h &&
                  logits->w == out->w, MMTTA_ERR_INVALID, "memo ensemble: shape mismatch");
  MMTTA_CHECK(logits->dtype == MMTTA_F32 && out->dtype == MMTTA_F32, MMTTA_ERR_UNSUPPORTED, "memo ensemble: fp32-stored tensors only");
  MMTTA_CHECK(is_cl(logits) && is_cl(out), MMTTA_ERR_UNSUPPORTED, "memo ensemble: channels-last only");
  MMTTA_CHECK(loss_small_item(logits) && loss_small_item(out), MMTTA_ERR_UNSUPPORTED, "memo ensemble: an item of 2^31 elements or more");
  MMTTA_CHECK(!softmax || logits->c <= LOSS_MAX_R, MMTTA_ERR_UNSUPPORTED, "memo ensemble softmax: more than %d classes", LOSS_MAX_R);
  MMTTA_CHECK(out->n <= LOSS_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "memo ensemble: more than %d volumes in one call", LOSS_MAX_GRID_Y);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(loss_blocks(logits), out->n);
  if (!turned) {
    if (softmax)
      hipLaunchKernelGGL(memo_ensemble_categorical_kernel<false>, grid, dim3(256), 0, s, tv(logits), tv(out), mv);
    else
      hipLaunchKernelGGL(memo_ensemble_bernoulli_kernel<false>, grid, dim3(256), 0, s, tv(logits), tv(out), mv);
  } else if (softmax) {
    hipLaunchKernelGGL(memo_ensemble_categorical_kernel<true>, grid, dim3(256), 0, s, tv(logits), tv(out), mv);
  } else if (logits->c <= 4 && loss_dense16(logits) && loss_dense16(out) && ((out->flags & MMTTA_TENSOR_OWNS_PAD) || out->c == 4)) {
    // the tiled gather (views >= 2 here: view 0 is never transposed)
    const float* zp = (const float*)logits->ptr;
    float* op = (float*)out->ptr;
#define MEMO_ENS_TILED(VV)                                                                                             \
  hipLaunchKernelGGL(memo_ensemble_tiled_kernel<VV>, grid, dim3(256), 0, s, zp, op, (long long)logits->sn, (long long)out->sn, \
                     (int)logits->c, (unsigned)logits->d, (unsigned)logits->h, (unsigned)logits->w, mv)
    if (views == 2) MEMO_ENS_TILED(2);
    else if (views == 4) MEMO_ENS_TILED(4);
    else MEMO_ENS_TILED(8);
#undef MEMO_ENS_TILED
  } else {
    hipLaunchKernelGGL(memo_ensemble_bernoulli_kernel<true>, grid, dim3(256), 0, s, tv(logits), tv(out), mv);
  }
  return launch_status("memo ensemble");
}

extern "C" int mmtta_mirror_views(const mmtta_tensor* x, const mmtta_tensor* y, int views, const int32_t* view_axes, void* stream) {
  MMTTA_CHECK(x && y && x->ptr && y->ptr, MMTTA_ERR_INVALID, "mirror views: null argument");
  MemoViews mv;
  bool turned;
  int st = memo_views_check("mirror views", views, view_axes, y, mv, turned);
  if (st) return st;
  MMTTA_CHECK(y->n == x->n * views && x->c == y->c && x->d == y->d && x->h == y->h && x->w == y->w && x->dtype == y->dtype,
              MMTTA_ERR_INVALID, "mirror views: shape mismatch");
  MMTTA_CHECK(x->dtype == MMTTA_F32 || x->dtype == MMTTA_BF16, MMTTA_ERR_UNSUPPORTED, "mirror views: fp32 or bf16 rows");
  auto dense = [](const mmtta_tensor* t) {
    return t->sc == 1 && t->sw >= t->c && t->sh == (int64_t)t->w * t->sw && t->sd == (int64_t)t->h * t->sh;
  };
  MMTTA_CHECK(dense(x) && dense(y) && x->sw == y->sw, MMTTA_ERR_UNSUPPORTED, "mirror views: dense channels-last rows of one width");
  MMTTA_CHECK(y->sw == y->c || (y->flags & MMTTA_TENSOR_OWNS_PAD), MMTTA_ERR_UNSUPPORTED, "mirror views: `y` must own the pad lanes of its rows");
  MMTTA_CHECK(loss_small_item(x), MMTTA_ERR_UNSUPPORTED, "mirror views: an item of 2^31 elements or more");
  MMTTA_CHECK(y->n <= LOSS_MAX_GRID_Y, MMTTA_ERR_UNSUPPORTED, "mirror views: more than %d output items in one call", LOSS_MAX_GRID_Y);
  const long long esz = x->dtype == MMTTA_BF16 ? 2 : 4;
  const long long row = x->sw * esz;
  const uintptr_t both = (uintptr_t)x->ptr | (uintptr_t)y->ptr | (uintptr_t)(x->sn * esz) | (uintptr_t)(y->sn * esz) | (uintptr_t)row;
  const int unit = both % 16 == 0 ? 16 : (both % 8 == 0 ? 8 : (both % 4 == 0 ? 4 : 2));
  MMTTA_CHECK(unit >= esz && both % esz == 0, MMTTA_ERR_UNSUPPORTED, "mirror views: misaligned tensor");
  hipStream_t s = (hipStream_t)stream;
  const unsigned upr = (unsigned)(row / unit);
  const long long units = (long long)x->d * x->h * x->w * upr;
  long long b = (units + 255) / 256;
  if (b > 4096) b = 4096;
  const dim3 grid((unsigned)b, y->n);
  const long long xsn = x->sn * esz / unit, ysn = y->sn * esz / unit;
  const unsigned D = x->d, H = x->h, W = x->w;
#define MEMO_MIRROR(T, TR) \
  hipLaunchKernelGGL((memo_mirror_kernel<T, TR>), grid, dim3(256), 0, s, (const T*)x->ptr, (T*)y->ptr, xsn, ysn, upr, D, H, W, mv)
  if (!turned) {
    if (unit == 16) MEMO_MIRROR(uint4, false);
    else if (unit == 8) MEMO_MIRROR(uint2, false);
    else if (unit == 4) MEMO_MIRROR(unsigned, false);
    else MEMO_MIRROR(unsigned short, false);
  } else {
    if (unit == 16) MEMO_MIRROR(uint4, true);
    else if (unit == 8) MEMO_MIRROR(uint2, true);
    else if (unit == 4) MEMO_MIRROR(unsigned, true);
    else MEMO_MIRROR(unsigned short, true);
  }
#undef MEMO_MIRROR
  return launch_status("mirror views");
}
