// Weight / bias gradient of Conv3d and ConvTranspose3d on the CDNA4 matrix cores (gfx950).
//
// Replaces autograd's weight-gradient kernels reached from reference
// src/core/trainers/seg_trainer.py:142 (loss.backward()) for every conv of
// src/models/unet.py / src/models/unet_multimodal_midfusion.py.
//
// Both modules reduce to one form.  With a DENSE tensor on the coarse grid (Conv3d: dy,
// ConvTranspose3d: x) and a GATHERED tensor on the fine grid (Conv3d: x, ConvTranspose3d: dy):
//
//     R[tap][cg][cd] = sum_{n,o} T(G[n][o*s + tap - 1][cg]) * Td(D[n][o][cd])
//
// and the torch weight layout is [cd][cg][tap] for both (Conv3d [Cout,Cin,k], ConvT [Cin,Cout,k]).
// The reduction index is the voxel, so this is a GEMM with K = voxels:  A[row=cg][k=voxel],
// B[k=voxel][col=cd] on v_mfma_f32_32x32x2_f32.  One workgroup: one (32 cg x 32 cd) block, a run
// of spatial tiles; G's halo box and D's tile are staged in LDS once per tile and shared by all
// 27 taps; the four waves split the taps (7/7/7/6), i.e. 7 accumulators x 16 registers per lane.
// Partial results of the spatial splits go to a slab and are summed by a deterministic reduce
// kernel (no float atomics) that also emits the torch layout.
#include "common.h"

namespace mmtta {
MMTTA_ACT_NS_OPEN

typedef float f32x16 __attribute__((ext_vector_type(16)));
static inline int roundup(int v, int m) { return (v + m - 1) / m * m; }

struct WArgs {
  const float* g; long long gsn, gsd, gsh, gsw; int Cg, Dgg, Hgg, Wgg; NL tg;
  const float* dn; long long dsn, dsd, dsh, dsw; int Cd, Dd, Hd, Wd; NL td;
  int N;
  int si, ntaps;
  float* slab;     // [nsl][ntaps][CGp][CDp]
  float* dbpart;   // [nsl][CDp] or null
  int tz, ty, tx, tiles, tiles_per_split;
  int S, tiles_set;   // slabs and tiles per parameter set (one set: S = launch slabs, tiles_set = tiles)
  int CGp, CDp;
  int gvec4, dvec4;
  int g_bf, d_bf;   // storage of the gathered / dense tensor: 1 = bf16 elements (the forward activation of bf16 precision)
  int convt;        // transposed module: the dense operand is the module input (carries the norm-on-load)
};
// An entry of a launch table (a form that is not built: null).  The tables list bf16- before fp32-stored, paired before single
// and ConvTranspose3d before Conv3d, and are indexed to match: the order the kernels have in the code object.
using WLaunch = int (*)(const WArgs& a, int S, hipStream_t s);

// NTW = accumulators per wave: 7 for the 27-tap kernel (taps wave, wave+4, ...; slot 27 is a dummy that is
// never flushed), 1 for a single tap (the four waves then split the voxel pairs instead).
template <int TZ, int TY, int TX, int NTW, bool GBF = false, bool DBF = false>
__global__ __launch_bounds__(256) void wgrad_f32_kernel(WArgs a) {
  extern __shared__ float lds[];
  constexpr int MT = TZ * TY * TX;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: keeps every tap branch uniform
  const int h = lane >> 5, r = lane & 31;
  const int ext = NTW == 1 ? 0 : 2;
  const int BZ = (TZ - 1) * a.si + ext + 1, BY = (TY - 1) * a.si + ext + 1, BX = (TX - 1) * a.si + ext + 1;
  const int boxvox = BZ * BY * BX;
  const int dmin = NTW == 1 ? 0 : -1;
  float* gl = lds;                 // [boxvox][32]
  float* dl = lds + boxvox * 32;   // [MT][32]
  const int cg0 = blockIdx.y * 32, cd0 = blockIdx.z * 32;

  int toff[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int tap = NTW == 1 ? 0 : min(wave + 4 * j, 26);
    toff[j] = NTW == 1 ? 0 : (((tap / 9) * BY + ((tap / 3) % 3)) * BX + (tap % 3)) * 32;
  }
  const int kstep0 = NTW == 1 ? wave : 0, kstride = NTW == 1 ? 4 : 1;

  f32x16 acc[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
  float dbacc = 0.f;

  // slab index = blockIdx.x; the TILE RANGE of a slab follows the XCD-contiguous order, so the workgroups of one XCD
  // sweep one contiguous part of the volume and re-read each other's halo rows from their own L2
  // slab sx = slab (sx % S) of parameter set (sx / S): a set's slabs cover ITS batch items only, in the order a launch of
  // those items alone would use (the reduce kernels then sum a set's rows in that same order)
  const int sx = (int)xcd_contiguous_id(blockIdx.x, gridDim.x);
  const int qset = sx / a.S, sls = sx - qset * a.S;
  const int t0 = qset * a.tiles_set + sls * a.tiles_per_split;
  const int t1 = min((qset + 1) * a.tiles_set, t0 + a.tiles_per_split);
  const int tpn = a.tz * a.ty * a.tx;
  for (int tile = t0; tile < t1; ++tile) {
    const int n = tile / tpn;
    int t = tile % tpn;
    const int txi = t % a.tx; t /= a.tx;
    const int tyi = t % a.ty;
    const int tzi = t / a.ty;
    const int oz0 = tzi * TZ, oy0 = tyi * TY, ox0 = txi * TX;
    const int iz0 = oz0 * a.si + dmin, iy0 = oy0 * a.si + dmin, ix0 = ox0 * a.si + dmin;
    // ---- stage G box: [boxvox][32 channels cg0..cg0+31]
    {
      const float* gb = a.g;
      const long long gbo = (long long)n * a.gsn;
      if (a.gvec4) {
        const int cv = tid & 7;
        const int c = cg0 + cv * 4;
        float sc[4], sh[4];
        nl_coeff_vec<4>(a.tg, n, a.Cg, c, sc, sh);
        constexpr int U = 4;       // 4 box voxels per trip: loads first, then transform + LDS store
        for (int bv0 = tid >> 3; bv0 < boxvox; bv0 += 32 * U) {
          float4 xin[U];
          bool ok[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int bv = bv0 + 32 * u;
            const int bx = bv % BX, by = (bv / BX) % BY, bz = bv / (BX * BY);
            const int iz = iz0 + bz, iy = iy0 + by, ix = ix0 + bx;
            ok[u] = bv < boxvox && (unsigned)iz < (unsigned)a.Dgg && (unsigned)iy < (unsigned)a.Hgg &&
                    (unsigned)ix < (unsigned)a.Wgg && c < a.Cg;
            xin[u] = ld4_t<GBF>(gb, gbo + (long long)min(max(iz, 0), a.Dgg - 1) * a.gsd + (long long)min(max(iy, 0), a.Hgg - 1) * a.gsh +
                                      (long long)min(max(ix, 0), a.Wgg - 1) * a.gsw + min(c, (a.Cg - 1) & ~3));
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int bv = bv0 + 32 * u;
            if (bv < boxvox) {
              float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
              if (ok[u]) {
                v.x = nl_apply(xin[u].x, sc[0], sh[0], a.tg.relu);
                v.y = (c + 1 < a.Cg) ? nl_apply(xin[u].y, sc[1], sh[1], a.tg.relu) : 0.f;
                v.z = (c + 2 < a.Cg) ? nl_apply(xin[u].z, sc[2], sh[2], a.tg.relu) : 0.f;
                v.w = (c + 3 < a.Cg) ? nl_apply(xin[u].w, sc[3], sh[3], a.tg.relu) : 0.f;
              }
              *reinterpret_cast<float4*>(gl + bv * 32 + cv * 4) = v;
            }
          }
        }
      } else {
        const int cc = tid & 31;
        const int c = cg0 + cc;
        float sc = 0.f, sh = 0.f;
        nl_coeff_vec<1>(a.tg, n, a.Cg, c, &sc, &sh);
        for (int bv = tid >> 5; bv < boxvox; bv += 8) {
          const int bx = bv % BX, by = (bv / BX) % BY, bz = bv / (BX * BY);
          const int iz = iz0 + bz, iy = iy0 + by, ix = ix0 + bx;
          float v = 0.f;
          if ((unsigned)iz < (unsigned)a.Dgg && (unsigned)iy < (unsigned)a.Hgg && (unsigned)ix < (unsigned)a.Wgg &&
              c < a.Cg)
            v = nl_apply(ld1_t<GBF>(gb, gbo + (long long)iz * a.gsd + (long long)iy * a.gsh + (long long)ix * a.gsw + c), sc, sh, a.tg.relu);
          gl[bv * 32 + cc] = v;
        }
      }
    }
    // ---- stage D tile: [MT][32 channels cd0..cd0+31]; every load unconditional from a clamped address, all of a
    // thread's loads in flight together (a load behind a per-item branch is waited for at once: 16 exposed round
    // trips per tile before)
    {
      const float* db = a.dn;
      const long long dbo = (long long)n * a.dsn;
      if (a.dvec4) {
        const int cv = tid & 7;
        const int c = cd0 + cv * 4;
        float sc[4], sh[4];
        nl_coeff_vec<4>(a.td, n, a.Cd, c, sc, sh);
        const int cl4 = min(c, (a.Cd - 1) & ~3);
        constexpr int NQ = MT / 32;
        float4 raw[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int v = (tid >> 3) + 32 * q;
          const int xl = v % TX, yl = (v / TX) % TY, zl = v / (TX * TY);
          raw[q] = ld4_t<DBF>(db, dbo + (long long)min(oz0 + zl, a.Dd - 1) * a.dsd + (long long)min(oy0 + yl, a.Hd - 1) * a.dsh +
                                    (long long)min(ox0 + xl, a.Wd - 1) * a.dsw + cl4);
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int v = (tid >> 3) + 32 * q;
          const int xl = v % TX, yl = (v / TX) % TY, zl = v / (TX * TY);
          const bool ok = oz0 + zl < a.Dd && oy0 + yl < a.Hd && ox0 + xl < a.Wd;
          float4 o;
          o.x = (ok && c < a.Cd) ? nl_apply(raw[q].x, sc[0], sh[0], a.td.relu) : 0.f;
          o.y = (ok && c + 1 < a.Cd) ? nl_apply(raw[q].y, sc[1], sh[1], a.td.relu) : 0.f;
          o.z = (ok && c + 2 < a.Cd) ? nl_apply(raw[q].z, sc[2], sh[2], a.td.relu) : 0.f;
          o.w = (ok && c + 3 < a.Cd) ? nl_apply(raw[q].w, sc[3], sh[3], a.td.relu) : 0.f;
          *reinterpret_cast<float4*>(dl + v * 32 + cv * 4) = o;
        }
      } else {
        const int cc = tid & 31;
        const int c = cd0 + cc;
        float sc = 0.f, sh = 0.f;
        nl_coeff_vec<1>(a.td, n, a.Cd, c, &sc, &sh);
        const int cl = min(c, a.Cd - 1);
        constexpr int NQ = MT / 8;
        float raw[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int v = (tid >> 5) + 8 * q;
          const int xl = v % TX, yl = (v / TX) % TY, zl = v / (TX * TY);
          raw[q] = ld1_t<DBF>(db, dbo + (long long)min(oz0 + zl, a.Dd - 1) * a.dsd + (long long)min(oy0 + yl, a.Hd - 1) * a.dsh +
                                    (long long)min(ox0 + xl, a.Wd - 1) * a.dsw + cl);
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int v = (tid >> 5) + 8 * q;
          const int xl = v % TX, yl = (v / TX) % TY, zl = v / (TX * TY);
          const bool ok = oz0 + zl < a.Dd && oy0 + yl < a.Hd && ox0 + xl < a.Wd && c < a.Cd;
          dl[v * 32 + cc] = ok ? nl_apply(raw[q], sc, sh, a.td.relu) : 0.f;
        }
      }
    }
    __syncthreads();
    // ---- MFMA: k = voxel pairs; straight-line body (reads of a step are independent of its MFMAs)
#pragma unroll 2
    for (int kk = kstep0; kk < MT / 2; kk += kstride) {
      const int v = 2 * kk + h;
      const int xl = v % TX, yl = (v / TX) % TY, zl = v / (TX * TY);
      const int gaddr = (((zl * a.si) * BY + yl * a.si) * BX + xl * a.si) * 32 + r;
      const float b = dl[v * 32 + r];
      float av[NTW];
#pragma unroll
      for (int j = 0; j < NTW; ++j) av[j] = gl[gaddr + toff[j]];
      dbacc += b;
#pragma unroll
      for (int j = 0; j < NTW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], b, acc[j], 0, 0, 0);
    }
    __syncthreads();
  }

  // ---- flush partials
  const int sl = NTW == 1 ? (sx * 4 + wave) : sx;
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int tap = NTW == 1 ? 0 : wave + 4 * j;
    if (tap < a.ntaps) {
      float* sb = a.slab + (((long long)sl * a.ntaps + tap) * a.CGp + cg0) * a.CDp + cd0 + r;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
        sb[(long long)row * a.CDp] = acc[j][i];
      }
    }
  }
  if (a.dbpart != nullptr && blockIdx.y == 0 && (NTW == 1 || wave == 0)) {
    dbacc += __shfl_xor(dbacc, 32, 64);
    if (h == 0) a.dbpart[(long long)sl * a.CDp + cd0 + r] = dbacc;
  }
}

// The sums of the 27-tap reduction, shared by wgrad_reduce27_kernel and wgrad_update27_kernel (the two must agree bit for
// bit).  slab_sums: NI elements per thread, element it = sum over sl of pit[it][sl * st] in slab order, 4 slabs per trip.
template <int NI>
__device__ __forceinline__ void slab_sums(const float* const* pit, int nsl, long long st, float* acc) {
#pragma unroll
  for (int it = 0; it < NI; ++it) acc[it] = 0.f;
  for (int sl = 0; sl < nsl; sl += 4) {
    float v[NI][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int it = 0; it < NI; ++it) v[it][u] = pit[it][(long long)min(sl + u, nsl - 1) * st];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int it = 0; it < NI; ++it) acc[it] += sl + u < nsl ? v[it][u] : 0.f;
  }
}
// bias_rows_sum: db[cd0 + t] for thread t < 32 = sum_sl dbpart[sl][cd] (8 threads per channel, then 8 partials in order);
// every thread of the block calls it (one barrier), `red` holds 256 floats of LDS
__device__ __forceinline__ float bias_rows_sum(const float* __restrict__ dbpart, int db_nsl, int Cd, int CDp, int cd0, float* red) {
  const int cdl = threadIdx.x & 31, part = threadIdx.x >> 5;
  const int cd = min(cd0 + cdl, Cd - 1);
  float s4[4] = {0.f, 0.f, 0.f, 0.f};
  for (int sl = part; sl < db_nsl; sl += 32) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = sl + 8 * u;
      const float v = dbpart[(long long)min(q, db_nsl - 1) * CDp + cd];
      s4[u] += q < db_nsl ? v : 0.f;
    }
  }
  red[threadIdx.x] = (s4[0] + s4[1]) + (s4[2] + s4[3]);
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x < 32) {
#pragma unroll
    for (int q = 0; q < 8; ++q) t += red[q * 32 + threadIdx.x];
  }
  return t;
}

// dw[cd][cg][tap] (+)= sum_sl slab[sl][tap][cg][cd]   (torch weight layout out of the [tap][cg][cd] slabs)
// The transpose goes through LDS so that both sides stay coalesced: reads run along cd, writes are runs of
// `ntaps` consecutive floats per (cd, cg).  27 taps: one block = one cg x 64 cd;  1 tap: 32 cg x 32 cd.
__global__ __launch_bounds__(256) void wgrad_reduce27_kernel(const float* __restrict__ slab, float* __restrict__ dw,
                                                             int nsl, int Cg, int Cd, int CGp, int CDp, int accumulate,
                                                             const float* __restrict__ dbpart, float* __restrict__ db,
                                                             int db_nsl, PSets ps) {
  __shared__ float tile[32][28];
  {  // parameter set blockIdx.z: its rows of the slab / bias partials, its dw / db
    const int q = blockIdx.z;
    slab += (long long)q * nsl * 27 * CGp * CDp;
    dw += pset_weight_elems(ps, q);
    if (db != nullptr) { dbpart += (long long)q * db_nsl * CDp; db += pset_bias_elems(ps, q); }
  }
  const int cd0 = blockIdx.y * 32;
  if ((int)blockIdx.x == Cg) {
    // bias gradient rows ride in the same launch: db[cd] (+)= sum_sl dbpart[sl][cd]; 8 threads per channel
    const float t = bias_rows_sum(dbpart, db_nsl, Cd, CDp, cd0, &tile[0][0]);
    if (threadIdx.x < 32 && cd0 + (int)threadIdx.x < Cd) {
      float* o = db + cd0 + threadIdx.x;
      *o = accumulate ? (*o + t) : t;
    }
    return;
  }
  // one block = one cg x 32 cd x 27 taps = 864 sums: up to 4 per thread, all advancing together through the slabs
  // (4 slabs x 4 items = 16 independent loads per trip, unconditional from clamped addresses)
  const int cg = blockIdx.x;
  const long long st = (long long)27 * CGp * CDp;
  const float* pit[4];
  bool live[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int i = threadIdx.x + 256 * it;
    const int cdl = i & 31, tap = min(i >> 5, 26);
    live[it] = i < 27 * 32 && cd0 + cdl < Cd;
    pit[it] = slab + ((long long)tap * CGp + cg) * CDp + min(cd0 + cdl, CDp - 1);
  }
  float acc[4];
  slab_sums<4>(pit, nsl, st, acc);
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int i = threadIdx.x + 256 * it;
    if (i < 27 * 32) tile[i & 31][i >> 5] = live[it] ? acc[it] : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 27 * 32; i += 256) {
    const int cdl = i / 27, tap = i % 27;
    const int cd = cd0 + cdl;
    if (cd < Cd) {
      const long long idx = ((long long)cd * Cg + cg) * 27 + tap;
      const float v = tile[cdl][tap];
      dw[idx] = accumulate ? (dw[idx] + v) : v;
    }
  }
}

// ------------------------------------------------------------------ fused weight update (27 taps)
// wgrad_reduce27_kernel + the arena optimizer + the repack of both bf16 images in one pass over a layer's weights.  One
// block = one parameter set (blockIdx.z) x 8 cg x 32 cd x 27 taps of the layer: the tile pack_tile<27> moves (PK x PN), so
// both images are written as whole 16-byte runs.  Per element: the slab sum of wgrad_reduce27_kernel (slab_sums), then
// optim_update on the torch-layout p / m / v of the set, then fp32 -> bf16 into the images.  The extra column of blocks
// (blockIdx.x == cg tiles) reduces and updates the bias rows.  Nothing else reads the gradient: it never reaches memory.
struct UpdImage {
  unsigned short* p;                  // set 0's image (null: none)
  long long outer, inner;             // bytes between the images of sets
  int Kp, Np, kn_is_ba;
};
struct UpdArgs {
  OptimArgs a;
  float *wp, *wm, *wv, *bp, *bm, *bv;
  UpdImage img[2];
  const int* step;
  int w_decay, b_decay;
};

constexpr int UPD_CG = 8, UPD_CD = 32, UPD_RS = UPD_CG * 27 + 1;      // LDS row = one cd: [cg][tap] (odd stride)
constexpr int UPD_NV = 27 * UPD_CG * UPD_CD / 4;                      // float4 items of a tile: 1728 = 6.75 per thread

__device__ __forceinline__ void add4(float4& a, const float4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }

// slab_sums for a thread that owns 4 consecutive cd of a (tap, cg) row: each lane of the float4 is slab_sums' value, the
// sum over the slabs in slab order.  (The tail trip loads only the slabs that exist instead of clamped copies plus 0: the
// accumulator starts at +0 and can never become -0, so the dropped `+ 0.f` terms change no bit.)
template <int NI>
__device__ __forceinline__ void slab_sums4(const float4* const* pit, int nsl, long long st4, float4* acc) {
#pragma unroll
  for (int it = 0; it < NI; ++it) acc[it] = make_float4(0.f, 0.f, 0.f, 0.f);
  int sl = 0;
  for (; sl + 4 <= nsl; sl += 4) {
    float4 v[NI][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int it = 0; it < NI; ++it) v[it][u] = pit[it][(long long)(sl + u) * st4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int it = 0; it < NI; ++it) add4(acc[it], v[it][u]);
  }
  const int rem = nsl - sl;                                           // 0 .. 3, the same for the whole launch
  if (rem > 0) {
    float4 v[NI][3];
#pragma unroll
    for (int u = 0; u < 3; ++u)
      if (u < rem) {
#pragma unroll
        for (int it = 0; it < NI; ++it) v[it][u] = pit[it][(long long)(sl + u) * st4];
      }
#pragma unroll
    for (int u = 0; u < 3; ++u)
      if (u < rem) {
#pragma unroll
        for (int it = 0; it < NI; ++it) add4(acc[it], v[it][u]);
      }
  }
}

// reduce phase, 16-byte form: item f = tid + 256 j (j < 7) is row f / 8 = cgl * 27 + tap of the tile and cd 4 (f % 8) ..+3
template <int NI>
__device__ __forceinline__ void upd_reduce4(const float* __restrict__ slab, int nsl, long long st, int j0, int cg0, int cd0, int Cg,
                                            int Cd, int CGp, int CDp, float* tile) {
  const float4* pit[NI];
#pragma unroll
  for (int it = 0; it < NI; ++it) {
    const int f = min((int)threadIdx.x + 256 * (j0 + it), UPD_NV - 1);
    const int row = f >> 3, c4 = f & 7, cgl = row / 27, tap = row % 27;
    pit[it] = reinterpret_cast<const float4*>(slab + ((long long)tap * CGp + min(cg0 + cgl, Cg - 1)) * CDp + cd0 + 4 * c4);
  }
  float4 acc[NI];
  slab_sums4<NI>(pit, nsl, st / 4, acc);
#pragma unroll
  for (int it = 0; it < NI; ++it) {
    const int f = threadIdx.x + 256 * (j0 + it);
    if (f < UPD_NV) {
      const int row = f >> 3, c4 = f & 7, cgl = row / 27;              // row = cgl * 27 + tap: the offset inside an LDS row
      const bool lg = cg0 + cgl < Cg;
      const int cd = cd0 + 4 * c4;
      float* t = tile + (4 * c4) * UPD_RS + row;
      t[0] = lg && cd < Cd ? acc[it].x : 0.f;
      t[UPD_RS] = lg && cd + 1 < Cd ? acc[it].y : 0.f;
      t[2 * UPD_RS] = lg && cd + 2 < Cd ? acc[it].z : 0.f;
      t[3 * UPD_RS] = lg && cd + 3 < Cd ? acc[it].w : 0.f;
    }
  }
}

// optimizer phase, 16-byte form: a cd's run of 8 cg x 27 taps is 54 float4; item g = tid + 256 k is (cdl, r4) = (g / 54,
// g % 54).  All of a batch's p / m / v loads are issued before the first use (clamped addresses, stores predicated).
template <int KIND, int NB>
__device__ __forceinline__ void upd_optim4(const UpdArgs& u, long long ob, long long rowst, int k0, int cd0, int Cd, bool first,
                                           bool keep_m, bool decay, float step_size, float bc2_sqrt, float* tile) {
  float4 p[NB], m[NB], v[NB];
  long long off[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    const int g = min((int)threadIdx.x + 256 * (k0 + k), UPD_NV - 1);
    const int cdl = min(g / 54, Cd - 1 - cd0), r4 = g % 54;
    off[k] = ob + cdl * rowst + 4 * r4;
    p[k] = *reinterpret_cast<const float4*>(u.wp + off[k]);
    m[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!first) {
      if (keep_m) m[k] = *reinterpret_cast<const float4*>(u.wm + off[k]);
      if (KIND != 2) v[k] = *reinterpret_cast<const float4*>(u.wv + off[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    const int g = threadIdx.x + 256 * (k0 + k);
    const int cdl = g / 54, r4 = g % 54;
    if (g < UPD_NV && cd0 + cdl < Cd) {
      float* t = tile + cdl * UPD_RS + 4 * r4;
      optim_update<KIND>(p[k].x, t[0], m[k].x, v[k].x, decay, u.a, step_size, bc2_sqrt, first);
      optim_update<KIND>(p[k].y, t[1], m[k].y, v[k].y, decay, u.a, step_size, bc2_sqrt, first);
      optim_update<KIND>(p[k].z, t[2], m[k].z, v[k].z, decay, u.a, step_size, bc2_sqrt, first);
      optim_update<KIND>(p[k].w, t[3], m[k].w, v[k].w, decay, u.a, step_size, bc2_sqrt, first);
      *reinterpret_cast<float4*>(u.wp + off[k]) = p[k];
      if (keep_m) *reinterpret_cast<float4*>(u.wm + off[k]) = m[k];
      if (KIND != 2) *reinterpret_cast<float4*>(u.wv + off[k]) = v[k];
      t[0] = p[k].x; t[1] = p[k].y; t[2] = p[k].z; t[3] = p[k].w;
    }
  }
}

// repack phase: one image from the updated tile, pack_tile's index map and rounding (positions outside the weight hold 0,
// as there).  One text for wgrad_update27_kernel and the transposed-read kernels that update in their epilogue.  (The image
// by value and the loop over the two at the call site: wgrad_update27_kernel keeps its registers that way.)
__device__ __forceinline__ void upd_repack(const UpdImage im, const PSets& ps, int q, int cg0, int cd0, const float* tile) {
  if (im.p == nullptr) return;
  unsigned short* img = reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(im.p) + (ps.inner == 1
      ? q * im.outer : (q / ps.inner) * im.outer + (q % ps.inner) * im.inner));
  const long long tslab = (long long)im.Kp * im.Np;
  if (im.kn_is_ba) {
    // k = cg (one group of 8), n = cd (32 columns): 27 x 32 runs of 16 bytes
    for (int o = threadIdx.x; o < 27 * UPD_CD; o += 256) {
      const int nn = o % UPD_CD, tp = o / UPD_CD;
      unsigned short h[8];
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) h[kk] = f32_to_bf16_bits(tile[nn * UPD_RS + kk * 27 + tp]);
      *reinterpret_cast<uint4*>(img + tp * tslab + ((long long)(cg0 >> 3) * im.Np + cd0 + nn) * 8) = bf16x8_pack(h);
    }
  } else {
    // k = cd (four groups of 8), n = cg (8 columns)
    for (int o = threadIdx.x; o < 27 * 4 * UPD_CG; o += 256) {
      const int c = o % UPD_CG, k8 = (o / UPD_CG) % 4, tp = o / (UPD_CG * 4);
      unsigned short h[8];
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) h[kk] = f32_to_bf16_bits(tile[(k8 * 8 + kk) * UPD_RS + c * 27 + tp]);
      *reinterpret_cast<uint4*>(img + tp * tslab + ((long long)((cd0 >> 3) + k8) * im.Np + cg0 + c) * 8) = bf16x8_pack(h);
    }
  }
}

__device__ __forceinline__ bool ptr16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int KIND>
__global__ __launch_bounds__(256) void wgrad_update27_kernel(const float* __restrict__ slab, int nsl, int Cg, int Cd, int CGp,
                                                             int CDp, const float* __restrict__ dbpart, int db_nsl, PSets ps,
                                                             UpdArgs u) {
  __shared__ float tile[UPD_CD * UPD_RS];
  __shared__ float s_step_size, s_bc2_sqrt;
  const int q = blockIdx.z;
  slab += (long long)q * nsl * 27 * CGp * CDp;
  const int t0 = *u.step;
  if (threadIdx.x == 0) optim_scalars(KIND, u.a, t0, s_step_size, s_bc2_sqrt);
  const bool first = t0 == 0;
  const bool wd_on = u.a.wd != 0.f;
  const bool keep_m = KIND != 2 || u.a.momentum != 0.f;
  const int cd0 = blockIdx.y * UPD_CD;
  const int cg_tiles = (Cg + UPD_CG - 1) / UPD_CG;
  if ((int)blockIdx.x == cg_tiles) {
    // bias rows: the reduction of wgrad_reduce27_kernel's extra column, then the optimizer
    const float t = bias_rows_sum(dbpart + (long long)q * db_nsl * CDp, db_nsl, Cd, CDp, cd0, tile);
    const float step_size = s_step_size, bc2_sqrt = s_bc2_sqrt;       // (written before bias_rows_sum's barrier)
    const int cd = cd0 + (int)threadIdx.x;
    if (threadIdx.x < 32 && cd < Cd) {
      const long long o = pset_bias_elems(ps, q) + cd;
      float pi = u.bp[o], mi = 0.f, vi = 0.f;
      if (!first) {
        if (keep_m) mi = u.bm[o];
        if (KIND != 2) vi = u.bv[o];
      }
      optim_update<KIND>(pi, t, mi, vi, wd_on && u.b_decay, u.a, step_size, bc2_sqrt, first);
      u.bp[o] = pi;
      if (keep_m) u.bm[o] = mi;
      if (KIND != 2) u.bv[o] = vi;
    }
    return;
  }
  const int cg0 = blockIdx.x * UPD_CG;
  const long long st = (long long)27 * CGp * CDp;
  // ---- reduce.  16-byte form when the slab rows allow it (the padded [tap][CGp][CDp] slabs of the planner always do): a
  // thread owns 4 consecutive cd of a row, 4 + 3 rows in two chunks, 4 slabs in flight per row
  if (ptr16(slab) && CDp % 4 == 0) {
    upd_reduce4<4>(slab, nsl, st, 0, cg0, cd0, Cg, Cd, CGp, CDp, tile);
    upd_reduce4<3>(slab, nsl, st, 4, cg0, cd0, Cg, Cd, CGp, CDp, tile);
  } else {
    // 4-byte form: element e = tid + 256 j (j < 27) is (cgl, tap, cdl) = (e / 864, (e % 864) >> 5, e & 31), as in reduce27
    constexpr int NI = 9;
#pragma unroll 1
    for (int j0 = 0; j0 < 27; j0 += NI) {
      const float* pit[NI];
      bool live[NI];
#pragma unroll
      for (int it = 0; it < NI; ++it) {
        const int e = threadIdx.x + 256 * (j0 + it);
        const int cgl = e / 864, i = e % 864, cdl = i & 31, tap = i >> 5;
        const int cg = cg0 + cgl, cd = cd0 + cdl;
        live[it] = cg < Cg && cd < Cd;
        pit[it] = slab + ((long long)tap * CGp + min(cg, Cg - 1)) * CDp + min(cd, CDp - 1);
      }
      float acc[NI];
      slab_sums<NI>(pit, nsl, st, acc);
#pragma unroll
      for (int it = 0; it < NI; ++it) {
        const int e = threadIdx.x + 256 * (j0 + it);
        const int cgl = e / 864, i = e % 864, cdl = i & 31, tap = i >> 5;
        tile[cdl * UPD_RS + cgl * 27 + tap] = live[it] ? acc[it] : 0.f;
      }
    }
  }
  __syncthreads();
  // ---- optimizer on the torch-layout rows: per cd a run of 8 cg x 27 taps = 216 consecutive floats
  {
    const float step_size = s_step_size, bc2_sqrt = s_bc2_sqrt;
    const bool decay = wd_on && u.w_decay;
    const long long wo = pset_weight_elems(ps, q);
    const int ncg = min(UPD_CG, Cg - cg0);
    const long long ob = wo + ((long long)cd0 * Cg + cg0) * 27, rowst = (long long)Cg * 27;
    // 16-byte form: whole runs (a full cg tile) that start on 16 bytes in every row, for every array the step touches
    bool vec = ncg == UPD_CG && rowst % 4 == 0 && ptr16(u.wp + ob);
    if (keep_m) vec = vec && ptr16(u.wm + ob);
    if (KIND != 2) vec = vec && ptr16(u.wv + ob);
    if (vec) {
      upd_optim4<KIND, 4>(u, ob, rowst, 0, cd0, Cd, first, keep_m, decay, step_size, bc2_sqrt, tile);
      upd_optim4<KIND, 3>(u, ob, rowst, 4, cd0, Cd, first, keep_m, decay, step_size, bc2_sqrt, tile);
    } else {
      for (int e = threadIdx.x; e < UPD_CD * UPD_CG * 27; e += 256) {
        const int cdl = e / (UPD_CG * 27), r = e % (UPD_CG * 27);
        const int cd = cd0 + cdl;
        if (cd < Cd && r < ncg * 27) {
          const long long o = ob + cdl * rowst + r;
          float pi = u.wp[o], mi = 0.f, vi = 0.f;
          if (!first) {
            if (keep_m) mi = u.wm[o];
            if (KIND != 2) vi = u.wv[o];
          }
          optim_update<KIND>(pi, tile[cdl * UPD_RS + r], mi, vi, decay, u.a, step_size, bc2_sqrt, first);
          u.wp[o] = pi;
          if (keep_m) u.wm[o] = mi;
          if (KIND != 2) u.wv[o] = vi;
          tile[cdl * UPD_RS + r] = pi;
        }
      }
    }
  }
  __syncthreads();
  // ---- repack: both images
#pragma unroll
  for (int m = 0; m < 2; ++m) upd_repack(u.img[m], ps, q, cg0, cd0, tile);
}

__global__ __launch_bounds__(256) void wgrad_reduce1_kernel(const float* __restrict__ slab, float* __restrict__ dw,
                                                            int nsl, int Cg, int Cd, int CGp, int CDp, int accumulate, PSets ps) {
  __shared__ float tile[32][33];
  slab += (long long)blockIdx.z * nsl * CGp * CDp;       // parameter set blockIdx.z
  dw += pset_weight_elems(ps, blockIdx.z);
  const int cg0 = blockIdx.x * 32, cd0 = blockIdx.y * 32;
  for (int i = threadIdx.x; i < 32 * 32; i += 256) {
    const int cdl = i & 31, cgl = i >> 5;
    float s = 0.f;
    if (cg0 + cgl < Cg && cd0 + cdl < Cd)
      for (int sl = 0; sl < nsl; ++sl) s += slab[((long long)sl * CGp + cg0 + cgl) * CDp + cd0 + cdl];
    tile[cdl][cgl] = s;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 32 * 32; i += 256) {
    const int cgl = i & 31, cdl = i >> 5;
    if (cg0 + cgl < Cg && cd0 + cdl < Cd) {
      const long long idx = (long long)(cd0 + cdl) * Cg + cg0 + cgl;
      const float v = tile[cdl][cgl];
      dw[idx] = accumulate ? (dw[idx] + v) : v;
    }
  }
}

// first reduction stage when many spatial splits exist: out[chunk][e] = sum of 32 consecutive slabs (coalesced)
__global__ __launch_bounds__(256) void slab_prereduce_kernel(const float* __restrict__ slab, float* __restrict__ out,
                                                             int nsl, long long elems) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= elems) return;
  slab += (long long)blockIdx.z * nsl * elems;           // parameter set blockIdx.z: its slabs, its chunks
  out += (long long)blockIdx.z * gridDim.y * elems;
  const int s0 = blockIdx.y * 32, s1 = min(nsl, s0 + 32);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int sl = s0; sl < s1; sl += 8) {          // 8 independent loads per trip (clamped, masked)
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = slab[(long long)min(sl + u, s1 - 1) * elems + e];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] += sl + u < s1 ? v[u] : 0.f;
  }
  out[(long long)blockIdx.y * elems + e] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}

// db[c] (+)= sum_sl part[sl*ld + c]: one wave per channel, lanes stride the partial rows
__global__ __launch_bounds__(64) void db_reduce_kernel(const float* __restrict__ part, float* __restrict__ db, int nsl,
                                                       int C, int ld, int accumulate, PSets ps, int is_weight) {
  const int c = blockIdx.x;
  part += (long long)blockIdx.y * nsl * ld;              // parameter set blockIdx.y
  db += is_weight ? pset_weight_elems(ps, blockIdx.y) : pset_bias_elems(ps, blockIdx.y);
  float s = 0.f;
  for (int sl = threadIdx.x; sl < nsl; sl += 64) s += part[(long long)sl * ld + c];
  s = wave_sum(s);
  if (threadIdx.x == 0) db[c] = accumulate ? db[c] + s : s;
}

// ------------------------------------------------------------------ bf16 helpers of the matrix-core weight gradients
typedef __bf16 wbf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 wbf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned int wpack2(float lo, float hi) {
  wbf16x2 v; v[0] = (__bf16)lo; v[1] = (__bf16)hi;
  return __builtin_bit_cast(unsigned int, v);
}


// ------------------------------------------------------------------ transposed-read weight gradient (bf16 operands)
// The kernels above keep the contraction index (voxels) contiguous per lane by transposing while staging: a thread owns
// channels, walks x with element (or 4-channel) loads and writes three x-shifted [channel][voxel] copies.  gfx950 can do
// that transpose in the LDS read instead (ds_read_b64_tr_b16: a 16-lane group reads 4 rows x 16 columns of 16-bit
// elements and each lane receives one column), so here both operands sit in LDS exactly as they sit in HBM -
// [voxel][32 channels] bf16, 64-byte rows - staged with 16-byte (bf16 storage: 8-byte) coalesced loads, ONE copy of the
// gathered box, and a tap is a constant byte offset.  Lane l of the MFMA operand (column l & 31, k = 8 (l >> 5) + j)
// receives, from two transposed reads, channel l & 31 of the 8 voxels x = 0..7 of tile row 2 ks + (l >> 5): the k order
// is the same for A and B, which is all the contraction needs.  Every address in the k loop is lane base + immediate.
// Stride 2: the box's x positions are stored even-first so that the stride-2 walk of a tap is contiguous (4 rows of a
// transposed read 64 bytes apart: conflict-free), the same as stride 1.
template <int TZ, int TY, int SI>
struct WTGeo {
  static constexpr int BZ = (TZ - 1) * SI + 3, BY = (TY - 1) * SI + 3, BX = 7 * SI + 3;
  static constexpr int XH = (BX + 1) / 2;
  static constexpr int NG = BZ * BY * BX, ND = TZ * TY * 8;
  static constexpr int G_BYTES = NG * 64, D_BYTES = ND * 64;
  static constexpr int LDS_BYTES = G_BYTES + D_BYTES + 256;       // + scale / shift of the 32 module-input channels
  __host__ __device__ static constexpr int lds_bytes(int nb) { return G_BYTES + nb * (D_BYTES + 256); }   // nb dense column blocks
  static constexpr int NK = ND / 16;                  // k steps: two tile rows of 8 voxels each
  // staging: an item = 8 channels (16 bytes of the bf16 image) of one voxel; a thread keeps ONE (x, channel chunk) of the
  // box and walks the box rows RPP at a time, so x, the channel offset and the LDS column are per-thread constants
  static constexpr int IPR = BX * 4;                  // items per box row
  static constexpr int RPP = 256 / IPR;               // box rows per pass (threads >= RPP * IPR repeat row RPP - 1)
  static constexpr int NROW = BZ * BY;
  static constexpr int GP = NROW / RPP;               // passes over the box
  static constexpr int DP = ND * 4 / 256;             // dense-tile items per thread
  static_assert(NROW % RPP == 0 && (ND * 4) % 256 == 0 && RPP <= BY, "whole passes; at most one y wrap inside a pass");
  __host__ __device__ static constexpr int xmap(int x) { return SI == 1 ? x : (x & 1) * XH + (x >> 1); }
  __host__ __device__ static constexpr int tap_off(int tap) {        // bytes; tap = (kz*3 + ky)*3 + kx
    return (((tap / 9) * BY + (tap / 3) % 3) * BX + xmap(tap % 3)) * 64;
  }
  __host__ __device__ static constexpr int row_off(int ks) {         // bytes; tile row 2 ks (the lane adds its half)
    return ((((2 * ks) / TY) * SI * BY + ((2 * ks) % TY) * SI) * BX) * 64;
  }
};

typedef short wshort4 __attribute__((ext_vector_type(4)));
typedef short wshort8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) wshort4* wlds4_t;

// 8 k values of one operand column: two transposed reads 4 voxels (256 bytes) apart
#define MMTTA_TR_FRAG(ptr, off)                                                                          \
  __builtin_bit_cast(wbf16x8, __builtin_shufflevector(__builtin_amdgcn_ds_read_tr16_b64_v4i16((wlds4_t)((ptr) + (off))),       \
                                                      __builtin_amdgcn_ds_read_tr16_b64_v4i16((wlds4_t)((ptr) + (off) + 256)), \
                                                      0, 1, 2, 3, 4, 5, 6, 7))

// Staging is the vector-ALU cost of this kernel, and with several volumes in flight vector-ALU issue is what bounds the
// chip (profiles/r02c_sq_counters.md), so the loader is built for few instructions per element:
//  * an item is 8 channels; a thread owns one (x, chunk) column of the box: x bounds, x / channel offsets, the x
//    de-interleave of stride 2 and the LDS column are computed once per tile, the LDS row is an immediate offset;
//  * a pass covers RPP whole box rows: z is wave-uniform up to one wrap (two scalar candidates, one select), y is one add;
//  * element offsets are 32-bit, products are 24-bit multiply-adds (strides < 2^24, tensor < 2^31 elements: host check);
//  * the norm-on-load exists on the module-input side only (template TD: the dense operand of a transposed module, else
//    the gathered one): the gradient side is a plain fp32 -> bf16 pack;  ReLU is max(x, lo) with lo = 0 or -inf.
// Software pipeline over the tiles of a workgroup: the dense tile and the first PG box passes of tile i+1 are requested
// right before tile i's MFMA loop (which reads LDS only) and land under it; the remaining passes are requested first
// thing in tile i+1 and land under the commit of the prefetched ones.
// NB = 2: ONE workgroup multiplies the gathered box with two 32-channel blocks of the dense operand (14 accumulator blocks:
// one workgroup per CU).  The stride-2 layers stage a box of 12x the tile's voxels for 28 MFMAs a wave - the staging (vector
// ALU, L2) is their cost, and every dense column block used to repeat it (conv 32->64 at 64^3: 2x, convT 128->32: 4x).
// (the kernels that write slabs: the body's one UPD site is discarded, and names these only)
#define MMTTA_TR_NO_UPDATE    \
  constexpr bool UPD = false; \
  constexpr int KIND = 0;     \
  constexpr UpdArgs u{};      \
  constexpr PSets ps{};
template <int TZ, int TY, int SI, bool GBF, bool DBF, bool TD, int NB = 1>
__global__ __launch_bounds__(256, (NB == 1 && SI == 1) ? 2 : 1) void wgrad_tr_kernel(WArgs a) {
  constexpr bool RG = false, RD = false;
  MMTTA_TR_NO_UPDATE
#include "conv_wgrad_tr_body.h"
}

// Raw staging (MMTTA_OPT_RAW_STAGING bit 1; host: wgrad_raw_bits) of the all-bf16 forms: an operand that takes no transform -
// the gradient side always (it was unpacked and repacked), the module-input side when its norm-on-load is the identity - goes
// to LDS as loaded.  RG / RD: the gathered / the dense operand.  The same body text with two more constants; launched from
// the plain translation unit only.
template <int TZ, int TY, int SI, bool TD, int NB, bool RG, bool RD>
__global__ __launch_bounds__(256, (NB == 1 && SI == 1) ? 2 : 1) void wgrad_tr_raw_kernel(WArgs a) {
  constexpr bool GBF = true, DBF = true;
  MMTTA_TR_NO_UPDATE
#include "conv_wgrad_tr_body.h"
}

// The update in the epilogue (MMTTA_OPT_WGRAD_EPILOGUE_UPDATE; host: wgrad_updates_in_epilogue) of the all-bf16 forms: a
// launch that plans ONE slab per parameter set has the complete gradient of a 27 x 32 cg x 32 NB cd block in the registers
// of one workgroup, so the kernel steps the optimizer on p / m / v and writes both bf16 images itself (upd_optim4 and
// upd_repack on wgrad_update27_kernel's LDS tile, 8 cg at a time) - no slab write, no read-back, no second launch, and the
// optimizer's streaming of a finished workgroup runs under the MFMA phases of the others.  RG / RD as in wgrad_tr_raw_kernel
// (both false: the transform form).  The same body text with UPD set; launched from the plain translation unit only, and
// only as the stride-1 one-block transform form (wgrad_updates_in_epilogue says why).
template <int TZ, int TY, int SI, bool TD, int NB, bool RG, bool RD, int KIND>
__global__ __launch_bounds__(256, (NB == 1 && SI == 1) ? 2 : 1) void wgrad_tr_upd_kernel(WArgs a, UpdArgs u, PSets ps) {
  constexpr bool GBF = true, DBF = true, UPD = true;
#include "conv_wgrad_tr_body.h"
}

template <int TZ, int TY, int SI, bool GBF, bool DBF, bool TD, int NB = 1, bool RG = false, bool RD = false>
static int launch_wgrad_tr_t(const WArgs& a, int S, hipStream_t s) {
  using G = WTGeo<TZ, TY, SI>;
  void (*kern)(WArgs);
  if constexpr (RG || RD) kern = wgrad_tr_raw_kernel<TZ, TY, SI, TD, NB, RG, RD>;
  else kern = wgrad_tr_kernel<TZ, TY, SI, GBF, DBF, TD, NB>;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set = true;
  }
  MMTTA_CHECK((a.CDp / 32) % NB == 0, MMTTA_ERR_INVALID, "wgrad: %d dense column blocks in groups of %d", a.CDp / 32, NB);
  dim3 grid(S, a.CGp / 32, a.CDp / 32 / NB);
  hipLaunchKernelGGL(kern, grid, dim3(256), G::lds_bytes(NB), s, a);
  return launch_status("conv wgrad bf16 (transposed reads)");
}

// ------------------------------------------------------------------ 1x1x1 weight gradient on transposed reads (bf16 operands)
// dw[cg][cd] = sum over voxels of x[v][cg] dy[v][cd]: no taps, no halo - a streaming kernel.  The fp32 form above walks
// 128-voxel tiles through load -> barrier -> 64 fp32 MFMAs -> barrier with a handful of workgroups (measured on the
// deep-fusion decoder: 33 -> 32 at 128^3 = 1.2 ms for 545 MB, 3.6 TFLOP/s).  Here both operands of a 4 x 8 x 8 tile sit in
// LDS as they sit in HBM ([voxel][32 channels] bf16), ds_read_b64_tr_b16 feeds v_mfma_f32_32x32x16_bf16, the four waves
// split the 16 k steps of a tile (one accumulator block each: registers are free for a full tile of prefetch) and write
// one slab each, as the fp32 kernel does; the loads of tile i+1 are requested before tile i's barrier.
template <bool GBF, bool DBF>
__global__ __launch_bounds__(256, 2) void wgrad_tr1_kernel(WArgs a) {
  constexpr int TZ = 4, TY = 8, NV = TZ * TY * 8, NP = NV * 4 / 256;      // 256 voxels, 4 items per thread and operand
  extern __shared__ float lds[];
  unsigned char* gl = reinterpret_cast<unsigned char*>(lds);
  unsigned char* dl = gl + NV * 64;
  float* coefl = reinterpret_cast<float*>(dl + NV * 64);                // [2][32] scale, shift of the module-input channels
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, r = lane & 31;
  const int cg0 = blockIdx.y * 32, cd0 = blockIdx.z * 32;
  const int lq = (lane & 15) >> 2, lp = lane & 3, lc = (lane >> 4) & 1;
  const unsigned char* gread = gl + (h * 8 + lq) * 64 + lc * 32 + lp * 8;
  const unsigned char* dread = dl + (h * 8 + lq) * 64 + lc * 32 + lp * 8;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  float dbs[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) dbs[c] = 0.f;
  const bool want_db = a.dbpart != nullptr && blockIdx.y == 0;
  const bool td = a.convt != 0;                                         // the dense operand carries the norm-on-load

  const int vox0 = tid >> 2, c8 = tid & 3;                              // item p: voxel vox0 + 64 p (z = p), chunk c8
  unsigned char* gst = gl + vox0 * 64 + c8 * 16;
  unsigned char* dst = dl + vox0 * 64 + c8 * 16;
  const int yl = vox0 >> 3, xl = vox0 & 7;
  const int gcb = cg0 + 8 * c8, dcb = cd0 + 8 * c8;
  const unsigned gc_lo = GBF ? min(gcb, (a.Cg - 1) & ~7) : min(gcb, (a.Cg - 1) & ~3), gc_hi = min(gcb + 4, (a.Cg - 1) & ~3);
  const unsigned dc_lo = DBF ? min(dcb, (a.Cd - 1) & ~7) : min(dcb, (a.Cd - 1) & ~3), dc_hi = min(dcb + 4, (a.Cd - 1) & ~3);
  const bool gtail = (a.Cg & 7) != 0, dtail = (a.Cd & 7) != 0;
  auto pair_mask = [](int c, int C) { return (c < C ? 0xffffu : 0u) | (c + 1 < C ? 0xffff0000u : 0u); };
  const unsigned gsd = (unsigned)a.gsd, gsh = (unsigned)a.gsh, gsw = (unsigned)a.gsw;
  const unsigned dsd = (unsigned)a.dsd, dsh = (unsigned)a.dsh, dsw = (unsigned)a.dsw;

  // slab sx = slab (sx % S) of parameter set (sx / S): a set's slabs cover ITS batch items only, in the order a launch of
  // those items alone would use (the reduce kernels then sum a set's rows in that same order)
  const int sx = (int)xcd_contiguous_id(blockIdx.x, gridDim.x);
  const int qset = sx / a.S, sls = sx - qset * a.S;
  const int t0 = qset * a.tiles_set + sls * a.tiles_per_split;
  const int t1 = min((qset + 1) * a.tiles_set, t0 + a.tiles_per_split);
  const int tpn = a.tz * a.ty * a.tx;
  Oct8<GBF> gv[NP];
  Oct8<DBF> dq[NP];
  unsigned okbits = 0u;
  int pn = -1, cn = -1;
  auto issue = [&](int tile) {
    pn = tile / tpn;
    int t = tile % tpn;
    const int txi = t % a.tx; t /= a.tx;
    const int tyi = t % a.ty;
    const int tzi = t / a.ty;
    const int oz0 = tzi * TZ, oy = tyi * TY + yl, ox = txi * 8 + xl;
    const float* gbase = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.g) + (long long)pn * a.gsn * (GBF ? 2 : 4));
    const float* dbase = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.dn) + (long long)pn * a.dsn * (DBF ? 2 : 4));
    const bool yxok = oy < a.Hd && ox < a.Wd;
    const unsigned gyx = __umul24((unsigned)min(oy, a.Hd - 1), gsh) + __umul24((unsigned)min(ox, a.Wd - 1), gsw);
    const unsigned dyx = __umul24((unsigned)min(oy, a.Hd - 1), dsh) + __umul24((unsigned)min(ox, a.Wd - 1), dsw);
    okbits = 0u;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int oz = oz0 + p;
      okbits |= ((yxok && oz < a.Dd) ? 1u : 0u) << p;
      const unsigned go = __umul24((unsigned)min(oz, a.Dd - 1), gsd) + gyx, dof = __umul24((unsigned)min(oz, a.Dd - 1), dsd) + dyx;
      gv[p] = oct8_ld<GBF>(gbase, go + gc_lo, go + gc_hi);
      dq[p] = oct8_ld<DBF>(dbase, dof + dc_lo, dof + dc_hi);
    }
  };
  if (t0 < t1) issue(t0);
  for (int tile = t0; tile < t1; ++tile) {
    const int n = pn;
    if (n != cn) {
      float s8[8], h8[8];
      if (td) nl_coeff_vec<8>(a.td, n, a.Cd, dcb, s8, h8);
      else nl_coeff_vec<8>(a.tg, n, a.Cg, gcb, s8, h8);
#pragma unroll
      for (int j = 0; j < 8; ++j) { coefl[8 * c8 + j] = s8[j]; coefl[32 + 8 * c8 + j] = h8[j]; }
      cn = n;
      __syncthreads();
    }
    float sc[8], sh[8];
    {
      const float4* cq = reinterpret_cast<const float4*>(coefl + 8 * c8);
      const float4 s0 = cq[0], s1 = cq[1], h0 = cq[8], h1 = cq[9];
      sc[0] = s0.x; sc[1] = s0.y; sc[2] = s0.z; sc[3] = s0.w; sc[4] = s1.x; sc[5] = s1.y; sc[6] = s1.z; sc[7] = s1.w;
      sh[0] = h0.x; sh[1] = h0.y; sh[2] = h0.z; sh[3] = h0.w; sh[4] = h1.x; sh[5] = h1.y; sh[6] = h1.z; sh[7] = h1.w;
    }
    const float relu_lo = act_lo(td ? a.td.relu : a.tg.relu);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const unsigned okm = ((okbits >> p) & 1u) ? 0xffffffffu : 0u;
      float v[8], u[8];
      oct8_f8(gv[p], v);
      oct8_f8(dq[p], u);
      if (td) {
#pragma unroll
        for (int j = 0; j < 8; ++j) u[j] = act_max(fmaf(u[j], sc[j], sh[j]), relu_lo);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = act_max(fmaf(v[j], sc[j], sh[j]), relu_lo);
      }
      if (want_db) {
#pragma unroll
        for (int j = 0; j < 8; ++j) dbs[j] += __uint_as_float(__float_as_uint(u[j]) & ((dcb + j < a.Cd) ? okm : 0u));
      }
      uint4 pk, pd;
      pk.x = wpack2(v[0], v[1]) & okm; pk.y = wpack2(v[2], v[3]) & okm; pk.z = wpack2(v[4], v[5]) & okm; pk.w = wpack2(v[6], v[7]) & okm;
      pd.x = wpack2(u[0], u[1]) & okm; pd.y = wpack2(u[2], u[3]) & okm; pd.z = wpack2(u[4], u[5]) & okm; pd.w = wpack2(u[6], u[7]) & okm;
      if (gtail) { pk.x &= pair_mask(gcb, a.Cg); pk.y &= pair_mask(gcb + 2, a.Cg); pk.z &= pair_mask(gcb + 4, a.Cg); pk.w &= pair_mask(gcb + 6, a.Cg); }
      if (dtail) { pd.x &= pair_mask(dcb, a.Cd); pd.y &= pair_mask(dcb + 2, a.Cd); pd.z &= pair_mask(dcb + 4, a.Cd); pd.w &= pair_mask(dcb + 6, a.Cd); }
      *reinterpret_cast<uint4*>(gst + p * 4096) = pk;
      *reinterpret_cast<uint4*>(dst + p * 4096) = pd;
    }
    __syncthreads();
    if (tile + 1 < t1) issue(tile + 1);                               // lands during the reads / MFMAs below and the next commit
    wbf16x8 fa[4], fb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      fa[i] = MMTTA_TR_FRAG(gread, (wave + 4 * i) * 1024);
      fb[i] = MMTTA_TR_FRAG(dread, (wave + 4 * i) * 1024);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[i], acc, 0, 0, 0);
    __syncthreads();
  }
  const int sl = sx * 4 + wave;                                       // one slab per wave (the reduce kernels sum them)
  {
    float* sb = a.slab + ((long long)sl * a.CGp + cg0) * a.CDp + cd0 + r;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
      sb[(long long)row * a.CDp] = acc[i];
    }
  }
  if (want_db) {                                    // the workgroup's bias sums go to wave 0's slab row, zeros to the others
    float* red8 = lds;
#pragma unroll
    for (int c = 0; c < 8; ++c) red8[tid * 8 + c] = dbs[c];
    __syncthreads();
    if (tid < 32) {
      float sacc = 0.f;
#pragma unroll 8
      for (int q = 0; q < 64; ++q) sacc += red8[((q << 2) | (tid >> 3)) * 8 + (tid & 7)];
      a.dbpart[(long long)(sx * 4) * a.CDp + cd0 + tid] = sacc;
#pragma unroll
      for (int w2 = 1; w2 < 4; ++w2) a.dbpart[(long long)(sx * 4 + w2) * a.CDp + cd0 + tid] = 0.f;
    }
  }
}

template <bool GBF, bool DBF>
static int launch_wgrad_tr1_t(const WArgs& a, int S, hipStream_t s) {
  auto kern = wgrad_tr1_kernel<GBF, DBF>;
  dim3 grid(S, a.CGp / 32, a.CDp / 32);
  hipLaunchKernelGGL(kern, grid, dim3(256), 2 * 256 * 64 + 256, s, a);
  return launch_status("conv wgrad 1x1x1 bf16 (transposed reads)");
}

static int launch_wgrad_tr1(const WArgs& a, int S, hipStream_t s) {
  static constexpr WLaunch by_storage[2][2] = {      // [g fp32-stored][d fp32-stored] (bf16-stored gradients: method.grad_storage)
      {launch_wgrad_tr1_t<true, true>, launch_wgrad_tr1_t<true, false>},
      {launch_wgrad_tr1_t<false, true>, launch_wgrad_tr1_t<false, false>}};
  return by_storage[!a.g_bf][!a.d_bf](a, S, s);
}

// the module input (norm-on-load, possibly bf16-stored) is the gathered operand of a convolution and the dense one of a
// transposed convolution (stride 2 only); the other operand is a gradient: read as is, fp32- or (method.grad_storage: bf16,
// then next to a bf16-stored module input only) bf16-stored
#ifdef MMTTA_ACT_LEAKY_TU
constexpr bool WGRAD_RAW_KERNELS = false;
#else
constexpr bool WGRAD_RAW_KERNELS = true;
#endif
// launch_wgrad_tr_t as a table entry; a form that is not built is null, and not instantiated
template <bool BUILT, int TZ, int TY, int SI, bool GBF, bool DBF, bool TD, int NB = 1, bool RG = false, bool RD = false>
static constexpr WLaunch wgrad_tr_form() {
  if constexpr (BUILT) return launch_wgrad_tr_t<TZ, TY, SI, GBF, DBF, TD, NB, RG, RD>;
  else return nullptr;
}

// The forms of one tile: a bf16-stored gradient next to a bf16-stored module input only, paired column blocks for the all-bf16
// forms only, transposed convolutions at stride 2 only - the planner (wgeometry) produces no other index.  raw (the plan's:
// all-bf16 forms, stride 2, plain translation unit): bit 1 the gradient goes to LDS as loaded, bit 0 the module input too.
template <int TZ, int TY, int SI>
static int launch_wgrad_tr(const WArgs& a, int S, int ncb, int raw, hipStream_t s) {
  constexpr bool T = SI == 2, R = WGRAD_RAW_KERNELS && SI == 2;
#define MMTTA_TR_FORM(built, ...) wgrad_tr_form<built, TZ, TY, SI, __VA_ARGS__>()
  static constexpr WLaunch staged_raw[2][2][2] = {      // [Conv3d][one column block][the gradient only]
      {{MMTTA_TR_FORM(R, true, true, true, 2, true, true), MMTTA_TR_FORM(R, true, true, true, 2, true, false)},
       {MMTTA_TR_FORM(R, true, true, true, 1, true, true), MMTTA_TR_FORM(R, true, true, true, 1, true, false)}},
      {{MMTTA_TR_FORM(R, true, true, false, 2, true, true), MMTTA_TR_FORM(R, true, true, false, 2, false, true)},
       {MMTTA_TR_FORM(R, true, true, false, 1, true, true), MMTTA_TR_FORM(R, true, true, false, 1, false, true)}}};
  static constexpr WLaunch plain[2][2][2][2] = {      // [one column block][Conv3d][g fp32-stored][d fp32-stored]
      {{{MMTTA_TR_FORM(T, true, true, true, 2), nullptr}, {nullptr, nullptr}},
       {{MMTTA_TR_FORM(true, true, true, false, 2), nullptr}, {nullptr, nullptr}}},
      {{{MMTTA_TR_FORM(T, true, true, true), nullptr}, {MMTTA_TR_FORM(T, false, true, true), MMTTA_TR_FORM(T, false, false, true)}},
       {{MMTTA_TR_FORM(true, true, true, false), MMTTA_TR_FORM(true, true, false, false)}, {nullptr, MMTTA_TR_FORM(true, false, false, false)}}}};
#undef MMTTA_TR_FORM
  const WLaunch form = (raw & 2) ? staged_raw[!a.convt][ncb == 1][!(raw & 1)] : plain[ncb == 1][!a.convt][!a.g_bf][!a.d_bf];
  MMTTA_CHECK(form != nullptr, MMTTA_ERR_UNSUPPORTED, "wgrad: no transposed-read kernel of stride %d for conv_transpose %d, storage %d / %d, "
              "%d column blocks, raw %d", SI, a.convt, a.g_bf, a.d_bf, ncb, raw);
  return form(a, S, s);
}

// The kernel that updates in its epilogue (wgrad_tr_upd_kernel): only the form wgrad_updates_in_epilogue admits is built -
// stride 1, one column block, transform staging - for Adam, AdamW and SGD; none in the LeakyReLU translation unit.
#ifdef MMTTA_ACT_LEAKY_TU
constexpr bool WGRAD_UPD_KERNELS = false;
#else
constexpr bool WGRAD_UPD_KERNELS = true;
#endif
template <int TZ, int TY, int SI, bool TD, int NB, bool RG, bool RD>
static int launch_wgrad_tr_upd_t(const WArgs& a, const UpdArgs& u, const PSets& ps, int kind, int S, hipStream_t s) {
  using G = WTGeo<TZ, TY, SI>;
  static_assert(G::lds_bytes(NB) >= (int)((UPD_CD * UPD_RS + 2) * sizeof(float)), "the update tile and its two scalars fit the images");
  static constexpr void (*kinds[3])(WArgs, UpdArgs, PSets) = {      // KIND = mmtta_optim_desc.kind (checked)
      wgrad_tr_upd_kernel<TZ, TY, SI, TD, NB, RG, RD, MMTTA_OPTIM_ADAM>, wgrad_tr_upd_kernel<TZ, TY, SI, TD, NB, RG, RD, MMTTA_OPTIM_ADAMW>,
      wgrad_tr_upd_kernel<TZ, TY, SI, TD, NB, RG, RD, MMTTA_OPTIM_SGD>};
  static bool attr_set = false;
  if (!attr_set) {
    for (int k = 0; k < 3; ++k) (void)hipFuncSetAttribute((const void*)kinds[k], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set = true;
  }
  dim3 grid(S, a.CGp / 32, a.CDp / 32 / NB);
  hipLaunchKernelGGL(kinds[kind], grid, dim3(256), G::lds_bytes(NB), s, a, u, ps);
  return launch_status("conv wgrad bf16 (transposed reads, update in the epilogue)");
}

template <int TZ, int TY>
static int launch_wgrad_tr_upd_s1(const WArgs& a, const UpdArgs& u, const PSets& ps, int kind, int S, hipStream_t s) {
  if constexpr (WGRAD_UPD_KERNELS) return launch_wgrad_tr_upd_t<TZ, TY, 1, false, 1, false, false>(a, u, ps, kind, S, s);
  set_error("wgrad: no kernel updates in its epilogue in this translation unit");
  return MMTTA_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------------ small-channel weight gradient
// When one side of the layer has <= 4 channels (first layers: Cin = 1..4; last layers: Cout = 1..3) the
// 32x32 (cg x cd) blocking above would pad it 8-32x.  Here the small tensor Q is the GATHERED one and its
// (tap, channel) pairs are flattened into the MFMA row index (27*4 = 108 <= 128 rows = 4 waves x 32), the
// big tensor P is dense:      S[row=(tap,cs)][col=cb] = sum_o T(Q[o*si + tap - 1][cs]) * T(P[o][cb])
// One MFMA per voxel pair and wave instead of seven, and no padded channels.
struct W2Args {
  const float* q; long long qsn, qsd, qsh, qsw; int Cs, Dq, Hq, Wq; NL tq;
  const float* p; long long psn, psd, psh, psw; int Cb, Dp, Hp, Wp; NL tp;
  int si, ntaps;
  float* slab;     // [nsl][128][CBp]
  float* dbpart;   // [nsl][CBp] or null: per-channel sums of P (bias gradient when cb is the output channel)
  int tz, ty, tx, tiles, tiles_per_split, CBp;
  int S, tiles_set;   // slabs and tiles per parameter set
  int qvec4, pvec4;
  int p_bf;        // the dense tensor P is bf16-stored (forward activation of bf16 precision)
  int p_thin;      // wgrad_thin_tr_kernel: P has <= 4 channels too (fp32 voxels of 16 bytes)
  int q_bf;        // wgrad_thin_tr_kernel: the thin gathered tensor Q is bf16-stored (8 bytes a voxel)
  int bf;          // bf16 precision mode: operands rounded to bf16, 16 voxels per v_mfma_f32_32x32x16_bf16
};

// SI (gather stride) and T27 (27 taps / 1 tap) are template parameters: the box extents divide every staged voxel's index,
// and a run-time divisor is a ~30-instruction division (36 of them per tile and thread before)
template <bool PBF, int SI, bool T27>
__global__ __launch_bounds__(256) void wgrad_small_kernel(W2Args a) {
  extern __shared__ float lds[];
  constexpr int TZ = 4, TY = 4, TX = 8, MT = 128;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, r = lane & 31;
  constexpr int NT = T27 ? 27 : 1;
  constexpr int ext = T27 ? 2 : 0;
  constexpr int BZ = (TZ - 1) * SI + ext + 1, BY = (TY - 1) * SI + ext + 1, BX = (TX - 1) * SI + ext + 1;
  constexpr int boxvox = BZ * BY * BX;
  constexpr int dmin = T27 ? -1 : 0;
  float* ql = lds;                  // [boxvox][4]
  float* pl = lds + boxvox * 4;     // [MT][32]
  const int cb0 = blockIdx.y * 32;
  const int nrows = NT * a.Cs;
  const int rowid = wave * 32 + r;
  int toffl = 0;
  if (rowid < nrows) {
    const int tap = rowid / a.Cs, cs = rowid % a.Cs;
    toffl = (!T27 ? 0 : (((tap / 9) * BY + ((tap / 3) % 3)) * BX + (tap % 3))) * 4 + cs;
  }
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  float dbacc = 0.f;
  const int sx = (int)xcd_contiguous_id(blockIdx.x, gridDim.x);                       // one part of the volume per XCD
  const int qset = sx / a.S, sls = sx - qset * a.S;                                   // (parameter set, slab of the set)
  const int t0 = qset * a.tiles_set + sls * a.tiles_per_split;
  const int t1 = min((qset + 1) * a.tiles_set, t0 + a.tiles_per_split);
  const int tpn = a.tz * a.ty * a.tx;
  // Both operands 16-byte addressable (every layer of the shipped networks): the NEXT tile's global loads are issued
  // before this tile's MFMAs and land while they run (a workgroup walked load -> barrier -> MFMA -> barrier with one
  // workgroup per CU: every tile paid a full memory latency).  Otherwise the loads sit in the staging step itself.
  constexpr int NQ = (boxvox + 255) / 256;          // 6 for the stride-2 box (9 x 9 x 17)
  const bool piped = a.qvec4 && a.pvec4;
  float4 raw[NQ], praw[MT / 32];
  float qsc[4], qsh[4], psc[4], psh[4];
  const int pcv = tid & 7, pc = cb0 + pcv * 4;
  const int pcl4 = min(pc, (a.Cb - 1) & ~3);      // clamped channel group (16-byte aligned)
  int n_coef = -1;
  auto decode = [&](int tile, int& n, int& oz0, int& oy0, int& ox0) {
    n = tile / tpn;
    int t = tile % tpn;
    const int txi = t % a.tx; t /= a.tx;
    const int tyi = t % a.ty;
    const int tzi = t / a.ty;
    oz0 = tzi * TZ; oy0 = tyi * TY; ox0 = txi * TX;
  };
  auto issue = [&](int tile) {
    int n, oz0, oy0, ox0;
    decode(tile, n, oz0, oy0, ox0);
    const int iz0 = oz0 * SI + dmin, iy0 = oy0 * SI + dmin, ix0 = ox0 * SI + dmin;
    const float* qb = a.q + (long long)n * a.qsn;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int bv = min(tid + 256 * q, boxvox - 1);
      const int bx = bv % BX, by = (bv / BX) % BY, bz = bv / (BX * BY);
      const int iz = min(max(iz0 + bz, 0), a.Dq - 1), iy = min(max(iy0 + by, 0), a.Hq - 1), ix = min(max(ix0 + bx, 0), a.Wq - 1);
      raw[q] = *reinterpret_cast<const float4*>(qb + iz * a.qsd + iy * a.qsh + ix * a.qsw);
    }
    const long long pbo = (long long)n * a.psn;
#pragma unroll
    for (int q = 0; q < MT / 32; ++q) {
      const int v = (tid >> 3) + 32 * q;
      const int xl = v % TX, yl = (v / TX) % TY, zl = v / (TX * TY);
      const int oz = min(oz0 + zl, a.Dp - 1), oy = min(oy0 + yl, a.Hp - 1), ox = min(ox0 + xl, a.Wp - 1);
      praw[q] = ld4_t<PBF>(a.p, pbo + (long long)oz * a.psd + (long long)oy * a.psh + (long long)ox * a.psw + pcl4);
    }
    if (n != n_coef) {
      nl_coeff_vec<4>(a.tq, n, a.Cs, 0, qsc, qsh);
      nl_coeff_vec<4>(a.tp, n, a.Cb, pc, psc, psh);
      n_coef = n;
    }
  };
  auto commit = [&](int tile) {
    int n, oz0, oy0, ox0;
    decode(tile, n, oz0, oy0, ox0);
    const int iz0 = oz0 * SI + dmin, iy0 = oy0 * SI + dmin, ix0 = ox0 * SI + dmin;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int bv = tid + 256 * q;
      if (bv < boxvox) {
        const int bx = bv % BX, by = (bv / BX) % BY, bz = bv / (BX * BY);
        const int iz = iz0 + bz, iy = iy0 + by, ix = ix0 + bx;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned)iz < (unsigned)a.Dq && (unsigned)iy < (unsigned)a.Hq && (unsigned)ix < (unsigned)a.Wq) {
          v.x = nl_apply(raw[q].x, qsc[0], qsh[0], a.tq.relu);
          v.y = a.Cs > 1 ? nl_apply(raw[q].y, qsc[1], qsh[1], a.tq.relu) : 0.f;
          v.z = a.Cs > 2 ? nl_apply(raw[q].z, qsc[2], qsh[2], a.tq.relu) : 0.f;
          v.w = a.Cs > 3 ? nl_apply(raw[q].w, qsc[3], qsh[3], a.tq.relu) : 0.f;
        }
        *reinterpret_cast<float4*>(ql + bv * 4) = v;
      }
    }
#pragma unroll
    for (int q = 0; q < MT / 32; ++q) {
      const int v = (tid >> 3) + 32 * q;
      const int xl = v % TX, yl = (v / TX) % TY, zl = v / (TX * TY);
      const int oz = oz0 + zl, oy = oy0 + yl, ox = ox0 + xl;
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (oz < a.Dp && oy < a.Hp && ox < a.Wp && pc < a.Cb) {
        const float4 x4 = praw[q];
        o.x = nl_apply(x4.x, psc[0], psh[0], a.tp.relu);
        o.y = (pc + 1 < a.Cb) ? nl_apply(x4.y, psc[1], psh[1], a.tp.relu) : 0.f;
        o.z = (pc + 2 < a.Cb) ? nl_apply(x4.z, psc[2], psh[2], a.tp.relu) : 0.f;
        o.w = (pc + 3 < a.Cb) ? nl_apply(x4.w, psc[3], psh[3], a.tp.relu) : 0.f;
      }
      *reinterpret_cast<float4*>(pl + v * 32 + pcv * 4) = o;
    }
  };
  if (piped && t0 < t1) issue(t0);
  for (int tile = t0; tile < t1; ++tile) {
    if (piped) {
      commit(tile);
    } else {
    const int n = tile / tpn;
    int t = tile % tpn;
    const int txi = t % a.tx; t /= a.tx;
    const int tyi = t % a.ty;
    const int tzi = t / a.ty;
    const int oz0 = tzi * TZ, oy0 = tyi * TY, ox0 = txi * TX;
    const int iz0 = oz0 * SI + dmin, iy0 = oy0 * SI + dmin, ix0 = ox0 * SI + dmin;
    {  // Q box: up to 4 channels per voxel
      const float* qb = a.q + (long long)n * a.qsn;
      float sc[4], sh[4];
      nl_coeff_vec<4>(a.tq, n, a.Cs, 0, sc, sh);
      // all of the thread's box voxels are loaded (from clamped addresses) before the first is used
      if (a.qvec4) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int bv = min(tid + 256 * q, boxvox - 1);
          const int bx = bv % BX, by = (bv / BX) % BY, bz = bv / (BX * BY);
          const int iz = min(max(iz0 + bz, 0), a.Dq - 1), iy = min(max(iy0 + by, 0), a.Hq - 1), ix = min(max(ix0 + bx, 0), a.Wq - 1);
          raw[q] = *reinterpret_cast<const float4*>(qb + iz * a.qsd + iy * a.qsh + ix * a.qsw);
        }
      } else {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int bv = min(tid + 256 * q, boxvox - 1);
          const int bx = bv % BX, by = (bv / BX) % BY, bz = bv / (BX * BY);
          const int iz = min(max(iz0 + bz, 0), a.Dq - 1), iy = min(max(iy0 + by, 0), a.Hq - 1), ix = min(max(ix0 + bx, 0), a.Wq - 1);
          const float* src = qb + iz * a.qsd + iy * a.qsh + ix * a.qsw;
          raw[q].x = src[0];
          raw[q].y = src[min(1, a.Cs - 1)]; raw[q].z = src[min(2, a.Cs - 1)]; raw[q].w = src[min(3, a.Cs - 1)];
        }
      }
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int bv = tid + 256 * q;
        if (bv < boxvox) {
          const int bx = bv % BX, by = (bv / BX) % BY, bz = bv / (BX * BY);
          const int iz = iz0 + bz, iy = iy0 + by, ix = ix0 + bx;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if ((unsigned)iz < (unsigned)a.Dq && (unsigned)iy < (unsigned)a.Hq && (unsigned)ix < (unsigned)a.Wq) {
            v.x = nl_apply(raw[q].x, sc[0], sh[0], a.tq.relu);
            v.y = a.Cs > 1 ? nl_apply(raw[q].y, sc[1], sh[1], a.tq.relu) : 0.f;
            v.z = a.Cs > 2 ? nl_apply(raw[q].z, sc[2], sh[2], a.tq.relu) : 0.f;
            v.w = a.Cs > 3 ? nl_apply(raw[q].w, sc[3], sh[3], a.tq.relu) : 0.f;
          }
          *reinterpret_cast<float4*>(ql + bv * 4) = v;
        }
      }
    }
    {  // P tile
      const float* pb = a.p;
      const long long pbo = (long long)n * a.psn;
      if (a.pvec4) {
        const int cv = tid & 7, c = cb0 + cv * 4;
        float sc[4], sh[4];
        nl_coeff_vec<4>(a.tp, n, a.Cb, c, sc, sh);
        const int cl4 = min(c, (a.Cb - 1) & ~3);           // clamped channel group (16-byte aligned)
#pragma unroll
        for (int q = 0; q < MT / 32; ++q) {
          const int v = (tid >> 3) + 32 * q;
          const int xl = v % TX, yl = (v / TX) % TY, zl = v / (TX * TY);
          const int oz = min(oz0 + zl, a.Dp - 1), oy = min(oy0 + yl, a.Hp - 1), ox = min(ox0 + xl, a.Wp - 1);
          praw[q] = ld4_t<PBF>(pb, pbo + (long long)oz * a.psd + (long long)oy * a.psh + (long long)ox * a.psw + cl4);
        }
#pragma unroll
        for (int q = 0; q < MT / 32; ++q) {
          const int v = (tid >> 3) + 32 * q;
          const int xl = v % TX, yl = (v / TX) % TY, zl = v / (TX * TY);
          const int oz = oz0 + zl, oy = oy0 + yl, ox = ox0 + xl;
          float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
          if (oz < a.Dp && oy < a.Hp && ox < a.Wp && c < a.Cb) {
            const float4 x4 = praw[q];
            o.x = nl_apply(x4.x, sc[0], sh[0], a.tp.relu);
            o.y = (c + 1 < a.Cb) ? nl_apply(x4.y, sc[1], sh[1], a.tp.relu) : 0.f;
            o.z = (c + 2 < a.Cb) ? nl_apply(x4.z, sc[2], sh[2], a.tp.relu) : 0.f;
            o.w = (c + 3 < a.Cb) ? nl_apply(x4.w, sc[3], sh[3], a.tp.relu) : 0.f;
          }
          *reinterpret_cast<float4*>(pl + v * 32 + cv * 4) = o;
        }
      } else {
        const int cc = tid & 31, c = cb0 + cc;
        float sc = 0.f, sh = 0.f;
        nl_coeff_vec<1>(a.tp, n, a.Cb, c, &sc, &sh);
        for (int v = tid >> 5; v < MT; v += 8) {
          const int xl = v % TX, yl = (v / TX) % TY, zl = v / (TX * TY);
          const int oz = oz0 + zl, oy = oy0 + yl, ox = ox0 + xl;
          float val = 0.f;
          if (oz < a.Dp && oy < a.Hp && ox < a.Wp && c < a.Cb)
            val = nl_apply(ld1_t<PBF>(pb, pbo + (long long)oz * a.psd + (long long)oy * a.psh + (long long)ox * a.psw + c), sc, sh, a.tp.relu);
          pl[v * 32 + cc] = val;
        }
      }
    }
    }
    __syncthreads();
    if (piped && tile + 1 < t1) issue(tile + 1);
    // voxel v = 2*kk + h: the pair shares (zl, yl) and differs by one x step, so the box offset is a wave-uniform
    // (scalar) term per kk plus a lane term that does not change inside the tile loop
    if (a.bf) {
      // k = h*8 + e of MFMA step kk is voxel 16*kk + 8*h + e: with TX = 8 that is the x-row e = 0..7 at
      // (yl, zl) = ((2*kk + h) % TY, (2*kk + h) / TY): 8 gathered values per operand, packed to bf16
      const int xs = SI * 4;
#pragma unroll 2
      for (int kk = 0; kk < MT / 16; ++kk) {
        const int rowi = 2 * kk + h;
        const int yl = rowi % TY, zl = rowi / TY;
        const float* qp = ql + (((zl * SI) * BY + yl * SI) * BX) * 4 + toffl;
        const float* pp = pl + (rowi * 8) * 32 + r;
        float av[8], bv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { av[e] = qp[e * xs]; bv[e] = pp[e * 32]; }
        wbf16x8 af, bf;
#pragma unroll
        for (int e = 0; e < 8; ++e) { af[e] = (__bf16)av[e]; bf[e] = (__bf16)bv[e]; dbacc += bv[e]; }
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
      }
    } else {
    const float* qlane = ql + toffl + h * SI * 4;
    const float* plane = pl + h * 32 + r;
#pragma unroll 8
    for (int kk = 0; kk < MT / 2; ++kk) {
      const int xl0 = (2 * kk) % TX, yl = ((2 * kk) / TX) % TY, zl = (2 * kk) / (TX * TY);
      const int gaddr = (((zl * SI) * BY + yl * SI) * BX + xl0 * SI) * 4;
      const float av = qlane[gaddr];
      const float b = plane[kk * 64];
      dbacc += b;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b, acc, 0, 0, 0);
    }
    }
    __syncthreads();
  }
  const int sl = sx;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (row < nrows) a.slab[((long long)sl * 128 + row) * a.CBp + cb0 + r] = acc[i];
  }
  if (a.dbpart != nullptr && wave == 0) {
    dbacc += __shfl_xor(dbacc, 32, 64);
    if (h == 0) a.dbpart[(long long)sl * a.CBp + cb0 + r] = dbacc;
  }
}


// ------------------------------------------------------------------ thin-layer weight gradient on transposed reads
// The same contraction as wgrad_small_kernel's bf16 branch - S[(tap, cs)][cb] = sum_o Q[o*si + tap - 1][cs] * P[o][cb], 27 taps,
// operands rounded to bf16, v_mfma_f32_32x32x16_bf16 - with BOTH operands staged once as bf16 rows and read through
// ds_read_b64_tr_b16.  wgrad_small_kernel kept fp32 images and built every fragment from 16 ds_read_b32 + 8 packs: 95
// vector instructions per MFMA (profiles/r03a_pmc_sq_per_kernel.txt), which is what its launches were bound by.  Here
//  * P sits in LDS as it sits in HBM ([voxel][32 channels] bf16, 64-byte rows, NCB column blocks side by side): its fragment
//    is wgrad_tr_kernel's - two transposed reads 4 voxels apart;
//  * Q's box is [voxel][4 channels] bf16, 8 bytes a voxel.  A transposed read takes 4 rows x 16 columns from 16 lane
//    addresses (row = (lane & 15) >> 2, 8-byte chunk = lane & 3) and the hardware does not care where a chunk lies: chunk
//    lp of lane half lc is pointed at TAP 4 lc + lp of the wave's 8 taps, so the 32 columns a wave's fragment holds are
//    (tap, channel) = (column >> 2, column & 3) - the gather costs no instruction.  Wave w owns taps 8 w .. 8 w + 7 (the 5
//    slots past tap 26 re-read tap 26 and are dropped), one accumulator per column block;
//  * a k step is 16 output voxels = two x-rows of the 4 x 4 x 8 tile, as in wgrad_small_kernel.
// Staging: a thread's box voxels / tile items are the same for every tile (decoded once); offsets are 32-bit elements
// (host check); the next tile's loads are issued before this tile's MFMAs.
// PM: storage of the dense operand P - 0: fp32, 8-channel items; 1: bf16, 8-channel items; 2: P is thin as well (<= 4
// channels, fp32 voxels of 16 bytes: the full-resolution R -> R convolutions, both sides <= 4 channels): its tile rows
// hold 4 live columns, the other 28 are zeroed once (the matrix cores are idle either way; what counts is that a voxel
// costs a load, two packs and a store instead of wgrad_tiny_kernel's 243 FMAs on the vector ALU).
// QBF: the thin gathered tensor is bf16-stored, 8 bytes a voxel (the network input of bf16 precision).
template <int SI, int PM, int NCB, bool QBF = false>
__global__ __launch_bounds__(256, 2) void wgrad_thin_tr_kernel(W2Args a) {
  extern __shared__ float lds[];
  constexpr bool PBF = PM == 1, PTHIN = PM >= 2, PTBF = PM == 3;      // PM 3: the thin P is bf16-stored (8-byte voxels)
  static_assert(!PTHIN || NCB == 1, "a thin P is one column block");
  // stride 1: 4 x 8 x 8 tiles (box 6 x 10 x 10 = 2.3 voxels read per output voxel, 2.8 with 4 x 4 x 8; twice the MFMAs
  // behind one round of loads); stride 2: 4 x 4 x 8 (the 9 x 9 x 17 box is 6 staging passes already)
  constexpr int TZ = 4, TY = SI == 1 ? 8 : 4, TX = 8, MT = TZ * TY * TX;
  constexpr int BZ = (TZ - 1) * SI + 3, BY = (TY - 1) * SI + 3, BX = (TX - 1) * SI + 3;
  constexpr int boxvox = BZ * BY * BX;
  constexpr int QBYTES = (boxvox * 8 + 63) / 64 * 64;
  constexpr int NQ = (boxvox + 255) / 256;
  constexpr int NI = PTHIN ? 1 : MT * 4 * NCB / 256;  // items of the dense tile per thread (PTHIN: threads 0..127, one voxel each)
  unsigned char* ql = reinterpret_cast<unsigned char*>(lds);
  unsigned char* pl = ql + QBYTES;                    // NCB planes of [128 voxels][32 channels] bf16
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, r = lane & 31;
  const int lq = (lane & 15) >> 2, lp = lane & 3, lc = (lane >> 4) & 1;
  const int cb0 = blockIdx.y * 32 * NCB;

  // operand addresses (lane parts)
  const int tapl = min(wave * 8 + lc * 4 + lp, 26);
  const unsigned char* aread = ql + ((((tapl / 9) + 0) * BY + (tapl / 3) % 3 + h * SI) * BX + tapl % 3 + lq * SI) * 8;
  const unsigned char* bread = pl + (h * 8 + lq) * 64 + lc * 32 + lp * 8;
  f32x16 acc[NCB];
#pragma unroll
  for (int c = 0; c < NCB; ++c)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[c][i] = 0.f;

  // staging roles (tile-independent)
  int qpos[NQ];                                        // box voxel of pass q: bz << 16 | by << 8 | bx
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int bv = min(tid + 256 * q, boxvox - 1);
    qpos[q] = ((bv / (BX * BY)) << 16) | (((bv / BX) % BY) << 8) | (bv % BX);
  }
  const int c8 = PTHIN ? 0 : tid % (4 * NCB);                   // item p: voxel pv0 + p * (256 / (4 NCB)), channel chunk c8
  const int pv0 = PTHIN ? (tid & (MT - 1)) : tid / (4 * NCB);
  const int pc = cb0 + 8 * c8;
  const bool pcok = PTHIN ? tid < MT : pc < a.Cb;               // (Cb % 8 == 0: a chunk is inside or outside as a whole)
  const unsigned pcl = PTHIN ? 0u : (unsigned)min(pc, a.Cb - 8);
  unsigned char* pst = pl + (c8 >> 2) * (MT * 64) + pv0 * 64 + (c8 & 3) * 16;
  if constexpr (PTHIN) {                                        // columns 4..31 of the tile rows: zero for the whole launch
    for (int i = tid; i < MT * 7; i += 256) *reinterpret_cast<uint2*>(pl + (i / 7) * 64 + 8 + (i % 7) * 8) = make_uint2(0u, 0u);
  }
  const unsigned qsd = (unsigned)a.qsd, qsh = (unsigned)a.qsh, qsw = (unsigned)a.qsw;
  const unsigned psd = (unsigned)a.psd, psh = (unsigned)a.psh, psw = (unsigned)a.psw;
  const float qlo = act_lo(a.tq.relu), plo = act_lo(a.tp.relu);

  const int sx = (int)xcd_contiguous_id(blockIdx.x, gridDim.x);
  const int qset = sx / a.S, sls = sx - qset * a.S;
  const int t0 = qset * a.tiles_set + sls * a.tiles_per_split;
  const int t1 = min((qset + 1) * a.tiles_set, t0 + a.tiles_per_split);
  const int tpn = a.tz * a.ty * a.tx;
  float4 raw[NQ];
  Oct8<PBF> pit[NI];
  float4 pthin = make_float4(0.f, 0.f, 0.f, 0.f);
  unsigned qok = 0u, pok = 0u;
  float qsc[4], qsf[4], psc[8], psf[8], dbs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) dbs[j] = 0.f;
  int n_coef = -1;
  const bool want_db = a.dbpart != nullptr;

  auto issue = [&](int tile) {
    const int n = tile / tpn;
    int t = tile % tpn;
    const int txi = t % a.tx; t /= a.tx;
    const int tyi = t % a.ty;
    const int tzi = t / a.ty;
    const int oz0 = tzi * TZ, oy0 = tyi * TY, ox0 = txi * TX;
    const int iz0 = oz0 * SI - 1, iy0 = oy0 * SI - 1, ix0 = ox0 * SI - 1;
    const float* qb = QBF ? reinterpret_cast<const float*>(reinterpret_cast<const unsigned short*>(a.q) + (long long)n * a.qsn)
                          : a.q + (long long)n * a.qsn;
    qok = 0u;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int iz = iz0 + (qpos[q] >> 16), iy = iy0 + ((qpos[q] >> 8) & 255), ix = ix0 + (qpos[q] & 255);
      const bool ok = (unsigned)iz < (unsigned)a.Dq && (unsigned)iy < (unsigned)a.Hq && (unsigned)ix < (unsigned)a.Wq &&
                      tid + 256 * q < boxvox;
      qok |= (ok ? 1u : 0u) << q;
      const unsigned off = (unsigned)min(max(iz, 0), a.Dq - 1) * qsd + (unsigned)min(max(iy, 0), a.Hq - 1) * qsh +
                           (unsigned)min(max(ix, 0), a.Wq - 1) * qsw;
      if constexpr (QBF) {          // two dwords of the raw register carry the four bf16 channels until they are committed
        const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(qb) + off);
        raw[q].x = __uint_as_float(u.x); raw[q].y = __uint_as_float(u.y);
      } else {
        raw[q] = *reinterpret_cast<const float4*>(qb + off);
      }
    }
    const float* pb = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.p) + (long long)n * a.psn * ((PBF || PTBF) ? 2 : 4));
    pok = 0u;
#pragma unroll
    for (int p = 0; p < NI; ++p) {
      const int v = pv0 + p * (256 / (4 * NCB));
      const int oz = oz0 + v / (TX * TY), oy = oy0 + (v / TX) % TY, ox = ox0 + v % TX;
      const bool ok = pcok && oz < a.Dp && oy < a.Hp && ox < a.Wp;
      pok |= (ok ? 1u : 0u) << p;
      const unsigned off = (unsigned)min(oz, a.Dp - 1) * psd + (unsigned)min(oy, a.Hp - 1) * psh + (unsigned)min(ox, a.Wp - 1) * psw + pcl;
      if constexpr (PTBF) {
        const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(pb) + off);
        pthin.x = __uint_as_float(u.x); pthin.y = __uint_as_float(u.y);
      } else if constexpr (PTHIN) {
        pthin = *reinterpret_cast<const float4*>(pb + off);
      } else {
        pit[p] = oct8_ld<PBF>(pb, off, off + 4);
      }
    }
    if (n != n_coef) {
      nl_coeff_vec<4>(a.tq, n, a.Cs, 0, qsc, qsf);
      nl_coeff_vec<8>(a.tp, n, a.Cb, (int)pcl, psc, psf);
      n_coef = n;
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (tid + 256 * q < boxvox) {
        const unsigned okm = ((qok >> q) & 1u) ? 0xffffffffu : 0u;
        if constexpr (QBF) {
          const unsigned ux = __float_as_uint(raw[q].x), uy = __float_as_uint(raw[q].y);
          raw[q] = make_float4(bf16_bits_to_f32(ux & 0xffffu), __uint_as_float(ux & 0xffff0000u),
                               bf16_bits_to_f32(uy & 0xffffu), __uint_as_float(uy & 0xffff0000u));
        }
        const float v0 = act_max(fmaf(raw[q].x, qsc[0], qsf[0]), qlo);
        const float v1 = a.Cs > 1 ? act_max(fmaf(raw[q].y, qsc[1], qsf[1]), qlo) : 0.f;
        const float v2 = a.Cs > 2 ? act_max(fmaf(raw[q].z, qsc[2], qsf[2]), qlo) : 0.f;
        const float v3 = a.Cs > 3 ? act_max(fmaf(raw[q].w, qsc[3], qsf[3]), qlo) : 0.f;
        uint2 pk;
        pk.x = wpack2(v0, v1) & okm; pk.y = wpack2(v2, v3) & okm;
        *reinterpret_cast<uint2*>(ql + (tid + 256 * q) * 8) = pk;
      }
    }
    if constexpr (PTHIN) {
      if (tid < MT) {
        const unsigned okm = (pok & 1u) ? 0xffffffffu : 0u;
        if constexpr (PTBF) {
          const unsigned ux = __float_as_uint(pthin.x), uy = __float_as_uint(pthin.y);
          pthin = make_float4(bf16_bits_to_f32(ux & 0xffffu), __uint_as_float(ux & 0xffff0000u),
                              bf16_bits_to_f32(uy & 0xffffu), __uint_as_float(uy & 0xffff0000u));
        }
        const float raw4[4] = {pthin.x, pthin.y, pthin.z, pthin.w};
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = __uint_as_float(__float_as_uint(act_max(fmaf(raw4[j], psc[j], psf[j]), plo)) & (j < a.Cb ? okm : 0u));
          dbs[j] += v[j];
        }
        *reinterpret_cast<uint2*>(pst) = make_uint2(wpack2(v[0], v[1]), wpack2(v[2], v[3]));
      }
    }
#pragma unroll
    for (int p = 0; p < (PTHIN ? 0 : NI); ++p) {
      float v[8];
      oct8_f8(pit[p], v);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = act_max(fmaf(v[j], psc[j], psf[j]), plo);
      const unsigned okm = ((pok >> p) & 1u) ? 0xffffffffu : 0u;
      if (want_db) {
#pragma unroll
        for (int j = 0; j < 8; ++j) dbs[j] += __uint_as_float(__float_as_uint(v[j]) & okm);
      }
      uint4 pk;
      pk.x = wpack2(v[0], v[1]) & okm; pk.y = wpack2(v[2], v[3]) & okm;
      pk.z = wpack2(v[4], v[5]) & okm; pk.w = wpack2(v[6], v[7]) & okm;
      *reinterpret_cast<uint4*>(pst + p * (256 / (4 * NCB)) * 64) = pk;
    }
  };

  if (t0 < t1) issue(t0);
  for (int tile = t0; tile < t1; ++tile) {
    commit();
    __syncthreads();
    if (tile + 1 < t1) issue(tile + 1);                 // lands during the MFMAs below
#pragma unroll
    for (int kk = 0; kk < MT / 16; ++kk) {
      const int roff = ((((2 * kk) / TY) * SI * BY + ((2 * kk) % TY) * SI) * BX) * 8;
      const wbf16x8 af = __builtin_bit_cast(wbf16x8, __builtin_shufflevector(
          __builtin_amdgcn_ds_read_tr16_b64_v4i16((wlds4_t)(aread + roff)),
          __builtin_amdgcn_ds_read_tr16_b64_v4i16((wlds4_t)(aread + roff + 4 * SI * 8)), 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
      for (int c = 0; c < NCB; ++c) {
        const wbf16x8 bf = MMTTA_TR_FRAG(bread, c * (MT * 64) + kk * 1024);
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc[c], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  const int sl = sx;
#pragma unroll
  for (int c = 0; c < NCB; ++c)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row32 = (i & 3) + 8 * (i >> 2) + 4 * h;         // (tap of the wave, channel) = (row32 >> 2, row32 & 3)
      const int tap = wave * 8 + (row32 >> 2), cs = row32 & 3;
      if (tap < 27 && cs < a.Cs) a.slab[((long long)sl * 128 + tap * a.Cs + cs) * a.CBp + cb0 + c * 32 + r] = acc[c][i];
    }
  if (want_db) {                                    // thread (voxel slot, chunk c8) holds channels cb0 + 8 c8 .. + 7
    float* red8 = lds;                              // the images are dead: the loop ended with a barrier
#pragma unroll
    for (int j = 0; j < 8; ++j) red8[tid * 8 + j] = dbs[j];
    __syncthreads();
    if (tid < 32 * NCB) {
      float sacc = 0.f;
      if constexpr (PTHIN) {                        // threads 0..127 hold channels 0..3 of their voxel
        if (tid < 4)
          for (int m = 0; m < MT; ++m) sacc += red8[m * 8 + tid];
      } else {
        const int k8 = tid >> 3, j = tid & 7;
        for (int m = 0; m < 256 / (4 * NCB); ++m) sacc += red8[(k8 + 4 * NCB * m) * 8 + j];
      }
      a.dbpart[(long long)sl * a.CBp + cb0 + tid] = sacc;
    }
  }
}

template <int SI, int PM, int NCB, bool QBF>
static void launch_thin_tr_t(const W2Args& a, dim3 grid, hipStream_t s) {
  constexpr int TY = SI == 1 ? 8 : 4;
  constexpr int BZ = 3 * SI + 3, BY = (TY - 1) * SI + 3, BX = 7 * SI + 3;
  constexpr int QBYTES = (BZ * BY * BX * 8 + 63) / 64 * 64;
  size_t lds = QBYTES + (size_t)NCB * (4 * TY * 8) * 64;
  if (lds < 256 * 8 * sizeof(float)) lds = 256 * 8 * sizeof(float);      // the bias-gradient reduction reuses the images
  hipLaunchKernelGGL((wgrad_thin_tr_kernel<SI, PM, NCB, QBF>), grid, dim3(256), lds, s, a);
}

// pm (the plan's form): bit 0 P is bf16-stored, bit 1 P is thin too (stride 1, one column block, fp32-stored Q: wgeometry)
static int launch_thin_tr(const W2Args& a, int si, int pm, int ncb, dim3 grid, hipStream_t s) {
  using Form = void (*)(const W2Args&, dim3, hipStream_t);
#define MMTTA_THIN_FORMS(SI, PM) \
  {{launch_thin_tr_t<SI, PM, 2, true>, launch_thin_tr_t<SI, PM, 2, false>}, {launch_thin_tr_t<SI, PM, 1, true>, launch_thin_tr_t<SI, PM, 1, false>}}
  static constexpr Form forms[2][4][2][2] = {      // [si - 1][3 - pm][one column block][Q fp32-stored]
      {{{}, {nullptr, launch_thin_tr_t<1, 3, 1, false>}}, {{}, {nullptr, launch_thin_tr_t<1, 2, 1, false>}}, MMTTA_THIN_FORMS(1, 1),
       MMTTA_THIN_FORMS(1, 0)},
      {{}, {}, MMTTA_THIN_FORMS(2, 1), MMTTA_THIN_FORMS(2, 0)}};
#undef MMTTA_THIN_FORMS
  const Form form = forms[si - 1][3 - pm][ncb == 1][!a.q_bf];
  MMTTA_CHECK(form != nullptr, MMTTA_ERR_UNSUPPORTED, "wgrad (thin layer): no transposed-read kernel of stride %d, form %d, %d column blocks, "
              "bf16-stored Q %d", si, pm, ncb, a.q_bf);
  form(a, grid, s);
  return launch_status("wgrad small");
}

// small_is_cd == 0: dw[(cb*Cs + cs)*ntaps + tap]   (Conv3d with tiny Cin, ConvTranspose3d with tiny Cout)
// small_is_cd == 1: dw[(cs*Cb + cb)*ntaps + tap]   (1x1x1 Conv3d with tiny Cout)
__global__ void wgrad_small_reduce_kernel(const float* __restrict__ slab, float* __restrict__ dw, int nsl, int ntaps, int Cs,
                                          int Cb, int CBp, int small_is_cd, int accumulate, PSets ps) {
  slab += (long long)blockIdx.y * nsl * 128 * CBp;       // parameter set blockIdx.y
  dw += pset_weight_elems(ps, blockIdx.y);
  const int total = ntaps * Cs * Cb;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int cb = i % Cb, row = i / Cb;
    const int tap = row / Cs, cs = row % Cs;
    float s = 0.f;
    for (int sl = 0; sl < nsl; ++sl) s += slab[((long long)sl * 128 + row) * CBp + cb];
    float* o = dw + (small_is_cd ? ((long long)cs * Cb + cb) : ((long long)cb * Cs + cs)) * ntaps + tap;
    *o = accumulate ? (*o + s) : s;
  }
}

// ------------------------------------------------------------------ tiny x tiny weight gradient (VALU)
// Conv3d k3 s1 with <= 4 channels on BOTH sides (the full-resolution R->R unit of the top ResidualUnit): 1 GFLOP
// over 2 M voxels.  On the matrix cores the 3 dense columns would be padded to 32; here a thread owns a voxel,
// keeps the 9 (ky,kx) x CS x CB products of one kz plane in registers and walks rows (a wave = 64 consecutive x
// of one row; blockIdx.y = kz).  x is read as one 16-byte voxel per neighbour (clamped address, the invalid x
// neighbours are dropped by zeroing dy for that kx), norm+ReLU applied on load.  Lanes are combined once at the
// end; workgroup partials land in dw's own layout so the generic row-sum reduce finishes the job.
struct WTArgs {
  TV x; NL tx;
  TV dy;
  float* part;      // [blocks][ld]: dw layout [cb][cs][27]
  float* dbpart;    // [blocks][4] or null
  int ld;
  int B, ips;       // workgroups and batch items per parameter set
  int BT;           // workgroups of the launch per kz plane (B x sets)
};

template <int CS, int CB, bool HAS_T>
__global__ __launch_bounds__(256) void wgrad_tiny_kernel(WTArgs a) {
  __shared__ float red[4][9 * CS * CB + CB];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // The three kz planes of a unit range read the same dy rows and x rows one plane apart.  As grid rows (blockIdx.y = kz)
  // they ran as three sweeps far apart in time: 3x the HBM traffic (PMC r03a: 206 MB per volume against 67 MB of tensors).
  // Now the three workgroups of a range are neighbours in dispatch order ON ONE XCD (ids 8 apart: workgroups are dealt
  // round-robin over the 8 XCDs), so two of them hit that XCD's L2.
  const unsigned xcd = blockIdx.x & 7u, q3 = blockIdx.x >> 3;
  const int kz = (int)(q3 % 3u);
  const unsigned bv = (q3 / 3u) * 8u + xcd;              // this workgroup's id in a launch of BT workgroups
  if (bv >= (unsigned)a.BT) return;
  const int chunks = (a.dy.w + 63) / 64;
  const int hp = (a.dy.h + 1) / 2;                     // a wave takes two adjacent rows per step
  const long long units = (long long)a.ips * a.dy.d * hp * chunks;       // of ONE parameter set
  const int xsw4 = (int)a.x.sw * 4, dsw4 = (int)a.dy.sw * 4;
  float acc[9][CS][CB];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < CS; ++i)
#pragma unroll
      for (int j = 0; j < CB; ++j) acc[t][i][j] = 0.f;
  float dbs[CB];
#pragma unroll
  for (int j = 0; j < CB; ++j) dbs[j] = 0.f;
  int n_cached = -1;
  float sc[CS], sh[CS];
#pragma unroll
  for (int i = 0; i < CS; ++i) { sc[i] = 1.f; sh[i] = 0.f; }
  long long ufirst, ulast;
  const int sx = (int)xcd_contiguous_id(bv, (unsigned)a.BT);
  const int qset = sx / a.B;                            // workgroup sx = workgroup (sx % B) of parameter set (sx / B)
  unit_range(units, sx - qset * a.B, a.B, ufirst, ulast);
  ufirst += (long long)qset * units; ulast += (long long)qset * units;
  // the unit index is decoded ONCE (three 64-bit divisions) and then advanced by carries: all of it wave-uniform
  int chunk, oyp, oz, n;
  {
    long long u = ufirst + wave;
    chunk = (int)(u % chunks); u /= chunks;
    oyp = (int)(u % hp); u /= hp;
    oz = (int)(u % a.dy.d);
    n = (int)(u / a.dy.d);
  }
  auto advance = [&]() {
    chunk += 4;
    while (chunk >= chunks) {
      chunk -= chunks;
      if (++oyp == hp) { oyp = 0; if (++oz == a.dy.d) { oz = 0; ++n; } }
    }
  };
  for (long long u0 = ufirst + wave; u0 < ulast; u0 += 4, advance()) {
    const int oy0 = 2 * oyp;
    const int iz = oz + kz - 1;
    if ((unsigned)iz >= (unsigned)a.x.d) continue;
    if (HAS_T && n != n_cached) {
      nl_coeff_vec<CS>(a.tx, n, CS, 0, sc, sh);
      n_cached = n;
    }
    const int ox = chunk * 64 + lane;
    const bool on = ox < a.dy.w;
    // all 14 loads of the step (2 dy voxels, 4 x rows x 3 neighbours) go out before the first use, from clamped
    // addresses; what does not exist is dropped by zeroing the dy factor
    const char* dyb = reinterpret_cast<const char*>(a.dy.p + (long long)n * a.dy.sn + (long long)oz * a.dy.sd);
    float4 g4[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
      g4[j] = *reinterpret_cast<const float4*>(dyb + (long long)min(oy0 + j, a.dy.h - 1) * a.dy.sh * 4 +
                                               (unsigned)(min(ox, a.dy.w - 1) * dsw4));
    unsigned boff[3];
    bool okx[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = ox + kx - 1;
      okx[kx] = on && (unsigned)ix < (unsigned)a.x.w;
      boff[kx] = (unsigned)(min(max(ix, 0), a.x.w - 1) * xsw4);
    }
    const char* xb = reinterpret_cast<const char*>(a.x.p + (long long)n * a.x.sn + (long long)iz * a.x.sd);
    float4 xr[4][3];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const char* xrow = xb + (long long)min(max(oy0 - 1 + r, 0), a.x.h - 1) * a.x.sh * 4;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) xr[r][kx] = *reinterpret_cast<const float4*>(xrow + boff[kx]);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bool rowon = oy0 + j < a.dy.h;
      const float gs[4] = {g4[j].x, g4[j].y, g4[j].z, g4[j].w};
      if (kz == 1) {
#pragma unroll
        for (int q = 0; q < CB; ++q) dbs[q] += (on && rowon) ? gs[q] : 0.f;
      }
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int r = j + ky;                       // x row oy0 + j + ky - 1
        const bool rok = rowon && (unsigned)(oy0 - 1 + r) < (unsigned)a.x.h;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const bool ok = rok && okx[kx];
          const float raw[4] = {xr[r][kx].x, xr[r][kx].y, xr[r][kx].z, xr[r][kx].w};
          float g[CB];
#pragma unroll
          for (int q = 0; q < CB; ++q) g[q] = ok ? gs[q] : 0.f;
#pragma unroll
          for (int i = 0; i < CS; ++i) {
            const float xv = HAS_T ? nl_apply(raw[i], sc[i], sh[i], a.tx.relu) : raw[i];
#pragma unroll
            for (int q = 0; q < CB; ++q) acc[ky * 3 + kx][i][q] = fmaf(xv, g[q], acc[ky * 3 + kx][i][q]);
          }
        }
      }
    }
  }
  // lanes -> wave -> workgroup
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < CS; ++i)
#pragma unroll
      for (int j = 0; j < CB; ++j) {
        const float v = wave_sum(acc[t][i][j]);
        if (lane == 0) red[wave][(t * CS + i) * CB + j] = v;
      }
#pragma unroll
  for (int j = 0; j < CB; ++j) {
    const float v = wave_sum(dbs[j]);
    if (lane == 0) red[wave][9 * CS * CB + j] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 9 * CS * CB + CB; e += 256) {
    const float v = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
    if (e < 9 * CS * CB) {
      const int j = e % CB, i = (e / CB) % CS, t = e / (CB * CS);
      a.part[(long long)sx * a.ld + (j * CS + i) * 27 + kz * 9 + t] = v;
    } else if (kz == 1 && a.dbpart != nullptr) {
      a.dbpart[(long long)sx * 4 + (e - 9 * CS * CB)] = v;
    }
  }
}

// ------------------------------------------------------------------ host side: plan (wgeometry), then launch
// The transposed-read kernel's loader: 16-byte items of 8 channels (fp32: two quads), 32-bit element offsets built
// from 24-bit multiply-adds
static bool wtr_ok(const mmtta_tensor* t) {
  if (!quad_aligned(t, 16, is_bf16(t) ? 8 : 4)) return false;
  const int64_t lim24 = (int64_t)1 << 24;
  if (t->sw >= lim24 || t->sh >= lim24 || t->sd >= lim24 || t->d >= lim24 || t->h >= lim24 || t->w >= lim24) return false;
  return item_fits_31(t, roundup(t->c, 8) + 8);
}

// Which main kernel a call runs: the values are the public ids of mmtta_conv_wgrad_kernel (4 and 5 are retired)
enum WRoute : int {
  W_F32_S1 = 0,     // wgrad_f32_kernel, 27 taps, stride 1
  W_F32_S2 = 1,     //                   27 taps, stride 2 (ConvTranspose3d included)
  W_F32_1X1 = 2,    //                   1 tap
  W_SMALL = 3,      // wgrad_small_kernel: <= 4 channels on one side
  W_TINY = 6,       // wgrad_tiny_kernel: <= 4 channels on both sides, fp32 VALU
  W_TR_S1 = 7,      // wgrad_tr_kernel (bf16 operands, transposed reads), stride 1
  W_TR_S2 = 8,      //                                                    stride 2
  W_TR_1X1 = 9,     // wgrad_tr1_kernel: the 1x1x1 streaming kernel of bf16 precision
  W_THIN_TR = 10,   // wgrad_thin_tr_kernel: the thin 27-tap layers of bf16 precision
};
static inline bool route_thin(WRoute r) { return r == W_SMALL || r == W_THIN_TR; }        // W2Args, [128][CDp] slabs
static inline bool route_reduce27(WRoute r) { return r == W_F32_S1 || r == W_F32_S2 || r == W_TR_S1 || r == W_TR_S2; }

// Where the bias gradient comes from
enum WBias {
  WB_MAIN_PARTIALS,     // rows [nsl][CDp] written by the main kernel (its dense operand is dy)
  WB_COLSUMS,           // column sums of dy (launch_channel_sums): dy is the gathered operand
  WB_TINY_PARTIALS,     // the tiny kernel's rows [blocks][4]
};

struct WGeo {
  WRoute route; WBias bias;
  int tiny_blocks;
  int small_is_cd; const mmtta_tensor *q, *pb; bool q_is_x;       // thin family: gathered thin tensor Q, dense tensor P
  const mmtta_tensor *g, *dn;
  int si, ntaps;
  int tz, ty, tx, tiles, S, tps, nsl, CGp, CDp;
  int64_t slab_elems, slab_floats, db_floats, colsum_blocks, pre_floats; int pre_chunks;
  bool convt;
  int ncb = 1;    // 32-column blocks per workgroup (wgrad_tr_kernel NB, wgrad_thin_tr_kernel NCB)
  bool p_thin;    // W_THIN_TR with <= 4 channels on the dense side as well
  int ips, nsets; // batch items per parameter set, sets per launch: tiles / S / nsl / *_floats / colsum_blocks are PER SET
  // ---- the variant of the route (plan_wgrad): what the launchers and the queries read beyond the geometry
  bool leaky;               // x_norm is a LeakyReLU: the call runs the instantiation that builds neither raw nor updating kernels
  int raw;                  // wgrad_raw_bits: bit 0 the module input, bit 1 the gradient go to LDS as loaded (0 under `leaky`)
  bool upd_in_epilogue;     // the main kernel steps the optimizer (never under `leaky`); without a target: the layer admits it
  int g_bf, d_bf, gvec4, dvec4;   // storage and 16-byte accesses of the gathered / dense operand (thin family: of Q / P)
  int form;                 // W_THIN_TR: PM of the kernel; W_SMALL: 0 one tap, 1 27 taps stride 1, 2 stride 2; W_TINY: HAS_T
  int refuse; char why[96]; // no kernel serves the route: part of the plan (the queries answer), returned before the first launch
  int64_t workspace_bytes() const { return (slab_floats + db_floats + pre_floats) * nsets * (int64_t)sizeof(float); }
};

// A/B switches read from the environment once.  MMTTA_WGRAD_PAIR: 0 no paired column blocks, 2: every stride-1 layer too.
// MMTTA_FUSED_UPDATE=0 turns the fused weight update off; the host then takes the separate passes.
static const int g_wgrad_pair = getenv("MMTTA_WGRAD_PAIR") ? atoi(getenv("MMTTA_WGRAD_PAIR")) : 1;
static const int g_fused_update = getenv("MMTTA_FUSED_UPDATE") ? atoi(getenv("MMTTA_FUSED_UPDATE")) : 1;

// `want` slabs of `elems` floats over w.tiles tiles: tiles per slab, the slabs that leaves, and the pre-reduce stage past
// 32 of them.  A split writes `mult` slabs (the four waves of a 1-tap kernel write one each).
static void plan_slabs(WGeo& w, int want, int64_t elems, int mult) {
  const int S = std::min(std::max(want, 1), w.tiles);
  w.tps = (w.tiles + S - 1) / S;
  w.S = (w.tiles + w.tps - 1) / w.tps;
  w.nsl = w.S * mult;
  w.slab_elems = elems;
  w.slab_floats = (int64_t)w.nsl * elems;
  w.pre_chunks = w.nsl > 32 ? (w.nsl + 31) / 32 : 0;
  w.pre_floats = (int64_t)w.pre_chunks * elems;
}

// the bias source and its workspace rows (after the slabs are planned)
static void plan_bias(WGeo& w, WBias src, const mmtta_tensor* dy) {
  w.bias = src;
  if (src == WB_COLSUMS) {
    w.colsum_blocks = (int64_t)w.ips * channel_partial_rows(dy);
    w.db_floats = w.colsum_blocks * 2 * dy->c;
  } else {
    w.db_floats = src == WB_TINY_PARTIALS ? (int64_t)w.tiny_blocks * 4 : (int64_t)w.nsl * w.CDp;
  }
}

static int wgeometry(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_tensor* dy, const mmtta_param_sets* sets, WGeo& w) {
  MMTTA_CHECK(d && x && dy && x->ptr && dy->ptr, MMTTA_ERR_INVALID, "wgrad: null argument");
  {
    const int st = psets_validate(sets, x->n);
    if (st) return st;
  }
  // one parameter set = `ips` consecutive batch items; everything below describes ONE set (the launch repeats it nsets times)
  w.ips = sets ? sets->items_per_set : x->n;
  w.nsets = x->n / w.ips;
  MMTTA_CHECK(d->op == MMTTA_CONV_FWD || d->op == MMTTA_CONVT_FWD, MMTTA_ERR_INVALID,
              "wgrad: desc.op must name the module (CONV_FWD or CONVT_FWD)");
  MMTTA_CHECK(d->ksize == 1 || d->ksize == 3, MMTTA_ERR_UNSUPPORTED, "wgrad: ksize %d", d->ksize);
  MMTTA_CHECK(d->stride == 1 || d->stride == 2, MMTTA_ERR_UNSUPPORTED, "wgrad: stride %d", d->stride);
  // desc.dtype selects the MFMA operand type (fp32, or bf16 for the 27-tap layers); accumulation, slabs and the
  // reduced gradient are fp32 either way
  MMTTA_CHECK(d->dtype == MMTTA_F32 || d->dtype == MMTTA_BF16, MMTTA_ERR_UNSUPPORTED, "wgrad: dtype %d", d->dtype);
  MMTTA_CHECK(is_cl(x) && is_cl(dy), MMTTA_ERR_UNSUPPORTED, "wgrad: tensors must be channels-last");
  MMTTA_CHECK(x->c == d->cin && dy->c == d->cout && x->n == dy->n, MMTTA_ERR_INVALID, "wgrad: channel/batch mismatch");
  w.convt = d->op == MMTTA_CONVT_FWD;
  if (w.convt) MMTTA_CHECK(d->ksize == 3 && d->stride == 2, MMTTA_ERR_UNSUPPORTED, "wgrad: conv_transpose is k3 s2 only");
  w.g = w.convt ? dy : x;
  w.dn = w.convt ? x : dy;
  w.si = d->stride;
  w.ntaps = d->ksize * d->ksize * d->ksize;
  const int gd[3] = {w.g->d, w.g->h, w.g->w}, dd[3] = {w.dn->d, w.dn->h, w.dn->w};
  for (int i = 0; i < 3; ++i) {
    const int want = w.convt ? gd[i] / 2 : (d->stride == 1 ? gd[i] : (gd[i] + 1) / 2);
    MMTTA_CHECK(dd[i] == want && (!w.convt || gd[i] % 2 == 0), MMTTA_ERR_INVALID,
                "wgrad: spatial mismatch on axis %d (fine %d, coarse %d)", i, gd[i], dd[i]);
  }
  const bool bf16 = d->dtype == MMTTA_BF16;
  // both sides <= 4 channels, k3 s1, 16-byte voxel rows: VALU kernel, partials in dw layout
  auto al16 = [](const mmtta_tensor* t) { return t->sc == 1 && quad_aligned(t, 16) && (long long)t->w * t->sw * 4 < (1LL << 31); };
  // fp32 voxels of 16 bytes addressed by 32-bit element offsets inside a batch item (wgrad_thin_tr_kernel's thin operands)
  auto q_ok = [](const mmtta_tensor* t) { return is_f32(t) && quad_aligned(t, 16) && item_fits_31(t, 8); };
  auto q_ok16 = [](const mmtta_tensor* t) { return is_bf16(t) && quad_aligned(t, 8) && item_fits_31(t, 8); };   // ... or bf16 voxels of 8 bytes
  // bf16 precision with the thin layers on the matrix cores (MMTTA_OPT_THIN_MFMA, like their forward / input gradient):
  // the transposed-read kernel below instead of the fp32 vector-ALU kernel
  if (!w.convt && d->cin <= 4 && d->cout <= 4 && d->ksize == 3 && d->stride == 1 && al16(x) && al16(dy) &&
      !(bf16 && g_thin_mfma && g_wgrad_vec && q_ok(x) && (q_ok(dy) || q_ok16(dy)))) {
    w.route = W_TINY;
    const long long units = (long long)w.ips * dy->d * ((dy->h + 1) / 2) * ((dy->w + 63) / 64);
    w.tiny_blocks = (int)std::min((units + 3) / 4, 512LL);
    w.slab_floats = (int64_t)w.tiny_blocks * (27 * d->cin * d->cout);
    plan_bias(w, WB_TINY_PARTIALS, dy);
    return MMTTA_OK;
  }
  // small-channel path: which tensor is the small gathered one (Q) and which the dense one (P)
  if (!w.convt && d->cin <= 4) { w.q = x; w.pb = dy; w.q_is_x = true; }
  else if (!w.convt && d->cout <= 4 && d->ksize == 1 &&
           !(bf16 && d->cin >= 16 && wtr_ok(x) && wtr_ok(dy) && (!is_bf16(dy) || is_bf16(x)) && g_wgrad_vec)) {
    // (in bf16 precision the 1x1x1 streaming kernel below takes these heads too: N padded to 32 costs nothing there)
    w.q = dy; w.pb = x; w.small_is_cd = 1;
  }
  else if (w.convt && d->cout <= 4) { w.q = dy; w.pb = x; }
  if (w.q != nullptr) {
    w.CGp = 128;
    w.CDp = roundup(w.pb->c, 32);
    // bf16 precision, 27 taps: the transposed-read kernel when the operands admit its staging (Q: fp32 voxels of 16 bytes;
    // P: 16-byte items of 8 channels; 32-bit element offsets inside a batch item)
    w.p_thin = w.pb->c <= 4 && w.si == 1 && g_thin_mfma;
    // (a bf16-stored thin tensor - the network input of bf16 precision, a thin gradient - has 8-byte voxels: this kernel only)
    const bool thin_tr = bf16 && w.ntaps == 27 && g_wgrad_vec &&
                         (q_ok(w.q) || (q_ok16(w.q) && !w.p_thin)) &&
                         (w.p_thin ? (q_ok(w.pb) || q_ok16(w.pb)) : (wtr_ok(w.pb) && w.pb->c % 8 == 0));
    w.route = thin_tr ? W_THIN_TR : W_SMALL;
    if (!thin_tr) w.p_thin = false;
    w.ncb = (thin_tr && (w.CDp / 32) % 2 == 0) ? 2 : 1;
    const int TY = (thin_tr && w.si == 1) ? 8 : 4;
    w.tz = (w.pb->d + 3) / 4; w.ty = (w.pb->h + TY - 1) / TY; w.tx = (w.pb->w + 7) / 8;
    w.tiles = w.tz * w.ty * w.tx * w.ips;
    // slabs: one volume in flight 256 / 512 / 768 / 1024 -> 56 / 46 / 57 / 57 us per launch at 128^3; two in flight
    // (method.lanes: 2, the default) 256 edges out 512 for the whole step (41.9 vs 41.5 volumes/s): less slab traffic
    int S = g_tune[3] / (w.CDp / 32 / w.ncb);
    // the transposed-read kernel does little per tile (8 MFMAs a wave behind one round of loads): it hides its memory latency
    // with workgroups per CU (86 - 172 registers: 3 - 5 per SIMD), so it wants 4x the slabs, down to 8 tiles each
    // (24 volumes in flight, per group of 8, 42 -> 168 slabs per volume: 3 -> 3 at 128^3 475 -> 265 us, 4 -> 32 145 -> 123, the
    // up-convolution 262 -> 239; 336: 238 / 128 / 241; 672 slabs: 249 / 142 / 272)
    if (thin_tr) S = std::min(4 * S, std::max(1, w.tiles / 8));
    plan_slabs(w, S, (int64_t)128 * w.CDp, 1);
    plan_bias(w, w.pb == dy ? WB_MAIN_PARTIALS : WB_COLSUMS, dy);        // P carries the output channels, or Q does
    return MMTTA_OK;
  }
  // bf16 operands: the transposed-read kernel, for operand pairs that admit its 16-byte items; anything else (ragged
  // channel slices, MMTTA_OPT_WGRAD_VECTOR_STAGING = 0) computes on the fp32-operand kernel
  // (a gradient may be bf16-stored only next to a bf16-stored module input: x is the gathered operand of a convolution, the
  // dense one of a transposed convolution)
  const bool tr_ok = bf16 && wtr_ok(w.g) && wtr_ok(w.dn) && (!is_bf16(dy) || is_bf16(x)) && g_wgrad_vec;
  const bool tr = tr_ok && w.ntaps == 27, tr1 = tr_ok && !w.convt && w.ntaps == 1 && w.si == 1;
  w.route = tr1 ? W_TR_1X1 : tr ? (w.si == 1 ? W_TR_S1 : W_TR_S2) : w.ntaps == 1 ? W_F32_1X1 : w.si == 1 ? W_F32_S1 : W_F32_S2;
  int TZ = 2, TY = 2;                                                  // tiles are TZ x TY x 8 voxels of the dense operand
  if ((tr && w.si == 1) || tr1) { TZ = 4; TY = 8; }
  else if (w.si == 1) { TZ = 4; TY = 4; }
  else if (tr) { TZ = 2; TY = 4; }
  w.tz = (w.dn->d + TZ - 1) / TZ;
  w.ty = (w.dn->h + TY - 1) / TY;
  w.tx = (w.dn->w + 7) / 8;
  w.tiles = w.tz * w.ty * w.tx * w.ips;
  w.CGp = roundup(w.g->c, 32);
  w.CDp = roundup(w.dn->c, 32);
  // both operands bf16-stored: a workgroup takes two dense column blocks per staged box (wgrad_tr_kernel NB) - every
  // stride-2 layer, and the stride-1 layers of <= 128 dense channels (per group of 8 volumes: conv 32->64 s2 162 -> 112 us,
  // convT 128->32 307 -> 210, convT 256->64 200 -> 144, 64->128 s2 102 -> 64; 64->64 s1 120 -> 98, 128->128 83 -> 73; the
  // 256- and 512-channel stride-1 layers have hundreds of workgroups and want two of them per CU: 512->512 218 -> 224)
  if (tr && g_wgrad_pair && (w.si == 2 || w.CDp <= 128 || g_wgrad_pair >= 2) && is_bf16(w.g) && is_bf16(w.dn) && (w.CDp / 32) % 2 == 0)
    w.ncb = 2;
  // (a pair counts as one block: the launch keeps its workgroup count and takes twice the slabs - measured against the same
  // slabs with half the workgroups, three runs each on one box: 96.5 / 96.1 volumes/s, 94.7 without pairs)
  const int blocks_cc = (w.CGp / 32) * (w.CDp / 32 / w.ncb);
  // workgroups (= slabs x channel blocks) per launch.  One volume in flight: 512 beats 256 by 3 % of the weight-gradient
  // time; two in flight (method.lanes: 2, the default) the other lane fills the CUs and halving the slab traffic wins:
  // 512 / 256 / 128 -> 40.1 / 41.5 / 40.6 volumes/s
  int S = g_tune[2] / blocks_cc;
  if (tr1) S = 1024 / blocks_cc;         // a streaming kernel: enough workgroups to keep HBM busy (slabs are 4 KB each)
  plan_slabs(w, S, (int64_t)w.ntaps * w.CGp * w.CDp, w.ntaps == 1 ? 4 : 1);
  plan_bias(w, w.convt ? WB_COLSUMS : WB_MAIN_PARTIALS, dy);
  return MMTTA_OK;
}

template <int TZ, int TY, int TX, int NTW, bool GBF, bool DBF>
static int launch_wgrad_t(const WArgs& a, int S, hipStream_t s) {
  const int ext = a.ntaps == 1 ? 0 : 2;
  const int BZ = (TZ - 1) * a.si + ext + 1, BY = (TY - 1) * a.si + ext + 1, BX = (TX - 1) * a.si + ext + 1;
  const size_t lds = ((size_t)BZ * BY * BX + TZ * TY * TX) * 32 * sizeof(float);
  auto kern = wgrad_f32_kernel<TZ, TY, TX, NTW, GBF, DBF>;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set = true;
  }
  dim3 grid(S, a.CGp / 32, a.CDp / 32);
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a);
  return launch_status("conv wgrad");
}

template <int TZ, int TY, int TX, int NTW>
static int launch_wgrad(const WArgs& a, int S, hipStream_t s) {
  static constexpr int (*by_storage[2][2])(const WArgs&, int, hipStream_t) = {      // [g_bf][d_bf]
      {launch_wgrad_t<TZ, TY, TX, NTW, false, false>, launch_wgrad_t<TZ, TY, TX, NTW, false, true>},
      {launch_wgrad_t<TZ, TY, TX, NTW, true, false>, launch_wgrad_t<TZ, TY, TX, NTW, true, true>}};
  return by_storage[a.g_bf][a.d_bf](a, S, s);
}

// The fused update (mmtta_conv_wgrad_update_sets): validates the target and fills the kernel's arguments before anything
// is launched
static int check_update_target(const mmtta_conv_desc* d, const WGeo& w, const mmtta_update_target* upd, UpdArgs& ua) {
  MMTTA_CHECK(route_reduce27(w.route), MMTTA_ERR_UNSUPPORTED,
              "wgrad update: the layer's weight gradient does not end in the 27-tap reduction");
  MMTTA_CHECK(upd->w_p && upd->w_m && upd->step && upd->image[0] && (upd->optim.kind == MMTTA_OPTIM_SGD || upd->w_v),
              MMTTA_ERR_INVALID, "wgrad update: null weight, moment, image or step pointer");
  MMTTA_CHECK(upd->b_p == nullptr || (!w.convt && upd->b_m && (upd->optim.kind == MMTTA_OPTIM_SGD || upd->b_v)),
              MMTTA_ERR_UNSUPPORTED, "wgrad update: the bias is updated here for Conv3d only (ConvTranspose3d: b_grad)");
  MMTTA_CHECK(upd->optim.kind >= MMTTA_OPTIM_ADAM && upd->optim.kind <= MMTTA_OPTIM_SGD, MMTTA_ERR_INVALID,
              "wgrad update: optimizer kind %d", upd->optim.kind);
  const mmtta_optim_desc& o = upd->optim;
  MMTTA_CHECK(!(o.kind == MMTTA_OPTIM_SGD && o.nesterov && (o.momentum <= 0.f || o.dampening != 0.f)), MMTTA_ERR_INVALID,
              "wgrad update: nesterov needs momentum > 0 and zero dampening");
  ua.a = OptimArgs{o.lr, o.beta1, o.beta2, o.eps, o.weight_decay, o.momentum, o.dampening, o.nesterov};
  ua.wp = upd->w_p; ua.wm = upd->w_m; ua.wv = upd->w_v;
  ua.bp = upd->b_p; ua.bm = upd->b_m; ua.bv = upd->b_v;
  ua.step = upd->step; ua.w_decay = upd->w_decay ? 1 : 0; ua.b_decay = upd->b_decay ? 1 : 0;
  for (int m = 0; m < 2; ++m) {
    ua.img[m].p = (unsigned short*)upd->image[m];
    ua.img[m].outer = upd->image_outer[m]; ua.img[m].inner = upd->image_inner[m];
    ua.img[m].Kp = ua.img[m].Np = ua.img[m].kn_is_ba = 0;
    if (upd->image[m] == nullptr) continue;
    mmtta_conv_desc dd = *d;
    if (m == 1) dd.op = w.convt ? MMTTA_CONVT_DGRAD : MMTTA_CONV_DGRAD;
    PackImageGeo g;
    const int st = pack_image_geometry(&dd, g);
    if (st) return st;
    MMTTA_CHECK(g.plain_bf16 && g.T == 27, MMTTA_ERR_UNSUPPORTED, "wgrad update: image %d is not a 27-tap bf16 image", m);
    MMTTA_CHECK(g.A == w.dn->c && g.B == w.g->c, MMTTA_ERR_INVALID, "wgrad update: image %d does not match the gradient", m);
    MMTTA_CHECK(((uintptr_t)upd->image[m]) % 16 == 0 && upd->image_outer[m] % 16 == 0 && upd->image_inner[m] % 16 == 0,
                MMTTA_ERR_INVALID, "wgrad update: images must keep 16-byte alignment");
    ua.img[m].Kp = g.Kp; ua.img[m].Np = g.Np; ua.img[m].kn_is_ba = g.kn_is_ba;
  }
  return MMTTA_OK;
}

// Raw staging of wgrad_tr_kernel (MMTTA_OPT_RAW_STAGING bit 1): which operands of the call go to LDS as loaded - bit 0 the
// module input x, bit 1 the gradient dy.  Both tensors bf16-stored (the all-bf16 forms), each in whole 8-channel chunks;
// dy takes no transform, x when its norm-on-load is the identity (none, or neither mean nor scale and no activation).  x goes
// raw next to a raw dy only.  Stride 2 only (convolutions and transposed convolutions: a box of 12x the tile's voxels is
// staged for 28 MFMAs a wave): the stride-1 instantiations were measured slower than their twins (profiles/raw_staging_ab.md:
// 134 against 105 us for the one-block form, which also spills two registers more) and are not built.
static int wgrad_raw_bits(const WGeo& w, const mmtta_norm_on_load* x_norm) {
  if (!(g_raw_staging & 2) || w.route != W_TR_S2) return 0;
  const mmtta_tensor *xin = w.convt ? w.dn : w.g, *grad = w.convt ? w.g : w.dn;
  if (!is_bf16(xin) || !is_bf16(grad) || grad->c % 8 != 0) return 0;
  const bool ident = x_norm == nullptr || (x_norm->mean == nullptr && x_norm->scale == nullptr && x_norm->relu == MMTTA_ACT_NONE);
  return 2 | ((ident && xin->c % 8 == 0) ? 1 : 0);
}

// The update in the epilogue of wgrad_tr_kernel's twins (MMTTA_OPT_WGRAD_EPILOGUE_UPDATE): what a fused-update call must be
// for one workgroup to hold the complete gradient of its block and for upd_optim4's 16-byte form to apply to every tile of
// it.  One slab per set and no pre-reduce; both tensors bf16-stored (the all-bf16 forms are the ones built); whole cg groups
// of 8 in every 32-row block and parameter rows of a multiple of 4 floats (Cg % 32 == 0); dense channels that fill the
// workgroup's column block; the form that is built: a stride-1 convolution with one column block per workgroup.  The
// stride-2 forms (paired column blocks, Conv3d and ConvTranspose3d, transform and raw staging) were built and measured
// slower than their two launches - they run 128 to 384 workgroups of one per CU, and a workgroup's optimizer rounds have
// nothing to overlap with (profiles/update_epilogue_ab.md) - so they are left out and the query says 0 for them.
// Never with the fused update switched off (MMTTA_FUSED_UPDATE=0: mmtta_conv_wgrad_update_sets refuses every call).
static bool wgrad_updates_in_epilogue(const WGeo& w) {
  if (!g_fused_update || !g_wgrad_epilogue_update) return false;
  if (w.route != W_TR_S1 || w.convt || w.ncb != 1) return false;
  if (w.nsl != 1 || w.pre_chunks != 0) return false;
  if (!is_bf16(w.g) || !is_bf16(w.dn)) return false;
  return w.g->c % 32 == 0 && w.dn->c % 32 == 0;
}
// ... and of the target: p / m / v of every set start on 16 bytes (the images are checked by check_update_target)
static bool update_target_vec16(const mmtta_update_target* upd, const PSets& ps, int nsets) {
  const bool keep_m = upd->optim.kind != MMTTA_OPTIM_SGD || upd->optim.momentum != 0.f;
  auto al = [](const void* p) { return p != nullptr && ((uintptr_t)p & 15) == 0; };
  if (!al(upd->w_p) || (keep_m && !al(upd->w_m)) || (upd->optim.kind != MMTTA_OPTIM_SGD && !al(upd->w_v))) return false;
  if (nsets > 1 && (ps.weight_outer % 4 != 0 || (ps.inner != 1 && ps.weight_inner % 4 != 0))) return false;
  return true;
}

// The whole decision of a call: the geometry, then the variant of its route (`upd`: the target of a fused update, or null).
// The one place the family states the LeakyReLU exception and the one caller of the three predicates above.
static int plan_wgrad(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm, const mmtta_tensor* dy,
                      const mmtta_param_sets* sets, const mmtta_update_target* upd, WGeo& w) {
  const int st = wgeometry(d, x, dy, sets, w);
  if (st) return st;
  w.leaky = nl_leaky(x_norm);
  w.raw = w.leaky ? 0 : wgrad_raw_bits(w, x_norm);
  w.upd_in_epilogue = !w.leaky && wgrad_updates_in_epilogue(w) && (upd == nullptr || update_target_vec16(upd, psets(sets), w.nsets));
  const bool thin = route_thin(w.route);
  const mmtta_tensor *g = thin ? w.q : w.g, *dn = thin ? w.pb : w.dn;
  w.g_bf = is_bf16(g) ? 1 : 0; w.gvec4 = quad_aligned(g, thin ? 16 : quad_bytes(g)) ? 1 : 0;
  w.d_bf = is_bf16(dn) ? 1 : 0; w.dvec4 = quad_aligned(dn, quad_bytes(dn)) ? 1 : 0;
  auto refuse = [&w](const char* fmt, int a = 0, int b = 0) {
    if (w.refuse == MMTTA_OK) snprintf(w.why, sizeof(w.why), fmt, a, b);
    w.refuse = MMTTA_ERR_UNSUPPORTED;
  };
  if (w.route == W_TINY) {
    w.form = (x_norm != nullptr && (x_norm->mean != nullptr || x_norm->scale != nullptr)) ? 1 : 0;
    if (!is_f32(x) || !is_f32(dy)) refuse("wgrad (tiny layer): fp32-stored tensors only");
  } else if (w.route == W_THIN_TR) {
    w.form = (w.p_thin ? 2 : 0) | w.d_bf;
  } else if (w.route == W_SMALL) {
    w.form = w.ntaps == 1 ? 0 : w.si;
    if (!is_f32(w.q)) refuse("wgrad (thin layer): the <= 4-channel tensor must be fp32-stored");
    if (w.ntaps == 1 && w.si != 1) refuse("wgrad (thin layer): %d taps with stride %d", w.ntaps, w.si);
  }
  return MMTTA_OK;
}

// ---- the main kernel of each family.  Workspace of a launch, Q = w.nsets sets back to back (set-major) in each region:
// slabs [Q][slab_floats], bias rows [Q][db_floats], pre-reduced slabs [Q][pre_floats]; `dbws` is the second region, or
// null when the main kernel has no bias rows to write
static int launch_tiny_family(const mmtta_conv_desc* d, const WGeo& w, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                              const mmtta_tensor* dy, float* ws, float* dbws, hipStream_t s) {
  WTArgs t;
  t.x = tv(x); t.tx = nl(x_norm); t.dy = tv(dy);
  t.part = ws; t.dbpart = dbws; t.ld = 27 * d->cin * d->cout;
  t.B = w.tiny_blocks; t.ips = w.ips; t.BT = w.tiny_blocks * w.nsets;
#define MMTTA_TINY_ROW(CS, T) \
  {wgrad_tiny_kernel<CS, 1, T>, wgrad_tiny_kernel<CS, 2, T>, wgrad_tiny_kernel<CS, 3, T>, wgrad_tiny_kernel<CS, 4, T>}
  static constexpr decltype(&wgrad_tiny_kernel<1, 1, false>) forms[2][4][4] = {      // [no transform on x][cin - 1][cout - 1]
      {MMTTA_TINY_ROW(1, true), MMTTA_TINY_ROW(2, true), MMTTA_TINY_ROW(3, true), MMTTA_TINY_ROW(4, true)},
      {MMTTA_TINY_ROW(1, false), MMTTA_TINY_ROW(2, false), MMTTA_TINY_ROW(3, false), MMTTA_TINY_ROW(4, false)}};
#undef MMTTA_TINY_ROW
  auto ix = [](int c) { return c >= 1 && c <= 3 ? c - 1 : 3; };
  const dim3 grid(3 * ((t.BT + 7) / 8) * 8), block(256);      // (plane, workgroup) pairs, see the kernel's id decode
  hipLaunchKernelGGL(forms[!w.form][ix(d->cin)][ix(d->cout)], grid, block, 0, s, t);
  return launch_status("wgrad tiny");
}

static int launch_thin_family(const mmtta_conv_desc* d, const WGeo& w, const mmtta_norm_on_load* x_norm, float* ws, float* dbws,
                              hipStream_t s) {
  const int Q = w.nsets;
  W2Args b;
  b.q = (const float*)w.q->ptr; b.qsn = w.q->sn; b.qsd = w.q->sd; b.qsh = w.q->sh; b.qsw = w.q->sw;
  b.Cs = w.q->c; b.Dq = w.q->d; b.Hq = w.q->h; b.Wq = w.q->w;
  b.p = (const float*)w.pb->ptr; b.psn = w.pb->sn; b.psd = w.pb->sd; b.psh = w.pb->sh; b.psw = w.pb->sw;
  b.Cb = w.pb->c; b.Dp = w.pb->d; b.Hp = w.pb->h; b.Wp = w.pb->w;
  b.tq = w.q_is_x ? nl(x_norm) : nl(nullptr);
  b.tp = w.q_is_x ? nl(nullptr) : nl(x_norm);
  b.si = w.si; b.ntaps = w.ntaps;
  b.slab = ws; b.dbpart = dbws;
  b.tz = w.tz; b.ty = w.ty; b.tx = w.tx; b.tiles = w.tiles * Q; b.tiles_per_split = w.tps; b.CBp = w.CDp;
  b.S = w.S; b.tiles_set = w.tiles;
  b.qvec4 = w.gvec4; b.pvec4 = w.dvec4;
  b.q_bf = w.g_bf; b.p_bf = w.d_bf;
  b.bf = (d->dtype == MMTTA_BF16 && w.ntaps == 27) ? 1 : 0;
  b.p_thin = w.p_thin ? 1 : 0;
  if (w.route == W_THIN_TR) return launch_thin_tr(b, w.si, w.form, w.ncb, dim3(w.S * Q, w.CDp / 32 / w.ncb), s);
  const int ext = w.ntaps == 1 ? 0 : 2;
  const int BZ = 3 * w.si + ext + 1, BY = 3 * w.si + ext + 1, BX = 7 * w.si + ext + 1;
  const size_t lds = ((size_t)BZ * BY * BX * 4 + 128 * 32) * sizeof(float);
  static constexpr decltype(&wgrad_small_kernel<false, 1, false>) forms[2][3] = {      // [p_bf][1 tap | 27 taps s1 | 27 taps s2]
      {wgrad_small_kernel<false, 1, false>, wgrad_small_kernel<false, 1, true>, wgrad_small_kernel<false, 2, true>},
      {wgrad_small_kernel<true, 1, false>, wgrad_small_kernel<true, 1, true>, wgrad_small_kernel<true, 2, true>}};
  hipLaunchKernelGGL(forms[w.d_bf][w.form], dim3(w.S * Q, w.CDp / 32), dim3(256), lds, s, b);
  return launch_status("wgrad small");
}

// `ua` (with `ps`, `kind`): the call updates in the main kernel's epilogue (the plan's upd_in_epilogue)
static int launch_main_family(const WGeo& w, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm, float* ws, float* dbws,
                              hipStream_t s, const UpdArgs* ua = nullptr, const PSets* ps = nullptr, int kind = 0) {
  WArgs a;
  a.g = (const float*)w.g->ptr; a.gsn = w.g->sn; a.gsd = w.g->sd; a.gsh = w.g->sh; a.gsw = w.g->sw;
  a.Cg = w.g->c; a.Dgg = w.g->d; a.Hgg = w.g->h; a.Wgg = w.g->w;
  a.dn = (const float*)w.dn->ptr; a.dsn = w.dn->sn; a.dsd = w.dn->sd; a.dsh = w.dn->sh; a.dsw = w.dn->sw;
  a.Cd = w.dn->c; a.Dd = w.dn->d; a.Hd = w.dn->h; a.Wd = w.dn->w;
  // the module input carries the norm-on-load; the gradient tensor is read as is
  a.tg = w.convt ? nl(nullptr) : nl(x_norm);
  a.td = w.convt ? nl(x_norm) : nl(nullptr);
  a.N = x->n;
  a.si = w.si; a.ntaps = w.ntaps;
  a.slab = ws; a.dbpart = dbws;
  a.tz = w.tz; a.ty = w.ty; a.tx = w.tx; a.tiles = w.tiles * w.nsets; a.tiles_per_split = w.tps;
  a.S = w.S; a.tiles_set = w.tiles;
  a.CGp = w.CGp; a.CDp = w.CDp;
  a.g_bf = w.g_bf; a.d_bf = w.d_bf;
  a.convt = w.convt ? 1 : 0;
  a.gvec4 = w.gvec4; a.dvec4 = w.dvec4;
  const int SQ = w.S * w.nsets;          // slabs of the launch
  if (ua != nullptr) return launch_wgrad_tr_upd_s1<4, 8>(a, *ua, *ps, kind, SQ, s);
  switch (w.route) {
    case W_TR_1X1: return launch_wgrad_tr1(a, SQ, s);
    case W_TR_S1: return launch_wgrad_tr<4, 8, 1>(a, SQ, w.ncb, w.raw, s);
    case W_TR_S2: return launch_wgrad_tr<2, 4, 2>(a, SQ, w.ncb, w.raw, s);
    case W_F32_1X1: return launch_wgrad<4, 4, 8, 1>(a, SQ, s);
    case W_F32_S1: return launch_wgrad<4, 4, 8, 7>(a, SQ, s);
    default: return launch_wgrad<2, 2, 8, 7>(a, SQ, s);
  }
}

// Everything behind the main kernel: slabs -> (pre-reduce past 32 slabs) -> the route's reduce kernel -> bias gradient.
// With `upd` the 27-tap reduce is the fused update (optimizer step and both bf16 images in the same pass); `updated`: the
// main kernel has done all of that in its epilogue, a Conv3d's bias included - what is left is a ConvTranspose3d's b_grad.
static int reduce_tail(const WGeo& w, const mmtta_tensor* dy, float* ws, float* dw, float* db, int accumulate,
                       const mmtta_param_sets* sets, const mmtta_update_target* upd, const UpdArgs& ua, bool updated, hipStream_t s) {
  const PSets ps = psets(sets);
  const int Q = w.nsets;
  const bool tiny = w.route == W_TINY, thin = route_thin(w.route);
  float* dbws = ws + w.slab_floats * Q;
  const float* rsrc = ws;
  int rn = w.nsl, st;
  if (w.pre_chunks > 0) {
    float* pre = ws + (w.slab_floats + w.db_floats) * Q;
    const long long elems = w.slab_elems;
    hipLaunchKernelGGL(slab_prereduce_kernel, dim3((unsigned)((elems + 255) / 256), w.pre_chunks, Q), dim3(256), 0, s, ws, pre,
                       w.nsl, elems);
    st = launch_status(thin ? "wgrad small prereduce" : "wgrad prereduce");
    if (st) return st;
    rsrc = pre; rn = w.pre_chunks;
  }
  // bias partials written by the main kernel, [nsl][CDp]: the 27-tap reduce kernels sum them in an extra block column
  const bool db_rides = db != nullptr && w.bias == WB_MAIN_PARTIALS && route_reduce27(w.route);
  const int Cg = thin ? w.q->c : w.g->c, Cd = thin ? w.pb->c : w.dn->c;
  switch (w.route) {
    case W_TINY: {
      const int ld = 27 * Cg * Cd;                                // block partials in dw's own layout [cb][cs][27]
      hipLaunchKernelGGL(db_reduce_kernel, dim3(ld, Q), dim3(64), 0, s, rsrc, dw, w.tiny_blocks, ld, ld, accumulate, ps, 1);
      break;
    }
    case W_SMALL:
    case W_THIN_TR:
      hipLaunchKernelGGL(wgrad_small_reduce_kernel, dim3((w.ntaps * Cg * Cd + 255) / 256, Q), dim3(256), 0, s, rsrc, dw, rn, w.ntaps,
                         Cg, Cd, w.CDp, w.small_is_cd, accumulate, ps);
      break;
    case W_F32_1X1:
    case W_TR_1X1:
      hipLaunchKernelGGL(wgrad_reduce1_kernel, dim3((Cg + 31) / 32, (Cd + 31) / 32, Q), dim3(256), 0, s, rsrc, dw, rn,
                         Cg, Cd, w.CGp, w.CDp, accumulate, ps);
      break;
    default:                  // the 27-tap routes (route_reduce27)
      if (updated) break;
      if (upd != nullptr) {
        static constexpr decltype(&wgrad_update27_kernel<0>) kinds[3] = {      // KIND = mmtta_optim_desc.kind (checked)
            wgrad_update27_kernel<MMTTA_OPTIM_ADAM>, wgrad_update27_kernel<MMTTA_OPTIM_ADAMW>, wgrad_update27_kernel<MMTTA_OPTIM_SGD>};
        const auto kern = kinds[upd->optim.kind];
        hipLaunchKernelGGL(kern, dim3((Cg + UPD_CG - 1) / UPD_CG + (db_rides ? 1 : 0), (Cd + UPD_CD - 1) / UPD_CD, Q),
                           dim3(256), 0, s, rsrc, rn, Cg, Cd, w.CGp, w.CDp, dbws, w.nsl, ps, ua);
      } else {
        hipLaunchKernelGGL(wgrad_reduce27_kernel, dim3(Cg + (db_rides ? 1 : 0), (Cd + 31) / 32, Q), dim3(256), 0, s, rsrc, dw, rn,
                           Cg, Cd, w.CGp, w.CDp, accumulate, dbws, db_rides ? db : nullptr, w.nsl, ps);
      }
  }
  st = launch_status(tiny ? "wgrad tiny reduce" : thin ? "wgrad small reduce" : upd != nullptr ? "wgrad update" : "wgrad reduce");
  if (st || db == nullptr || db_rides) return st;
  int rows = w.nsl, ld = w.CDp;
  if (w.bias == WB_TINY_PARTIALS) { rows = w.tiny_blocks; ld = 4; }
  if (w.bias == WB_COLSUMS) {
    // the gathered operand is dy: bias gradient = per-channel sum of dy (rows are n-major: a set's rows are contiguous)
    st = launch_channel_sums(dy, dbws, s);
    if (st) return st;
    rows = (int)w.colsum_blocks; ld = 2 * dy->c;
  }
  hipLaunchKernelGGL(db_reduce_kernel, dim3(dy->c, Q), dim3(64), 0, s, dbws, db, rows, dy->c, ld, accumulate, ps, 0);
  return launch_status(tiny ? "wgrad tiny reduce" : "bias reduce");
}

// mmtta_conv_wgrad_sets past the checks of its norm-on-load descriptor
int conv_wgrad_body(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                    const mmtta_tensor* dy, float* dw, float* db, int accumulate, void* workspace,
                    int64_t workspace_bytes, const mmtta_param_sets* sets, void* stream, const mmtta_update_target* upd) {
  WGeo w{};
  int st = plan_wgrad(d, x, x_norm, dy, sets, upd, w);
  if (st) return st;
  UpdArgs ua;
  if (upd != nullptr) {
    st = check_update_target(d, w, upd, ua);
    if (st) return st;
    dw = upd->w_p;                       // (not written: the gradient stays in the workspace)
    db = w.convt ? upd->b_grad : upd->b_p;
  }
  MMTTA_CHECK(dw != nullptr, MMTTA_ERR_INVALID, "wgrad: null dw");
  const int64_t need = w.workspace_bytes();
  MMTTA_CHECK(workspace != nullptr && workspace_bytes >= need, MMTTA_ERR_WORKSPACE, "wgrad: workspace %lld bytes, need %lld",
              (long long)workspace_bytes, (long long)need);
  MMTTA_CHECK(w.refuse == MMTTA_OK, w.refuse, "%s", w.why);
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const PSets ps = psets(sets);
  const bool in_epilogue = upd != nullptr && w.upd_in_epilogue;
  // the main kernel writes bias rows only when they are wanted and are its to write
  float* dbws = (db != nullptr && w.bias != WB_COLSUMS) ? ws + w.slab_floats * w.nsets : nullptr;
  if (w.route == W_TINY) st = launch_tiny_family(d, w, x, x_norm, dy, ws, dbws, s);
  else if (route_thin(w.route)) st = launch_thin_family(d, w, x_norm, ws, dbws, s);
  else if (in_epilogue) st = launch_main_family(w, x, x_norm, ws, dbws, s, &ua, &ps, upd->optim.kind);
  else st = launch_main_family(w, x, x_norm, ws, dbws, s);
  // MMTTA_OPT_PROFILE_MAIN_KERNEL_ONLY stops here; a fused-update call still runs its update
  if (st || (g_profile_main_only && upd == nullptr)) return st;
  return reduce_tail(w, dy, ws, dw, db, accumulate, sets, upd, ua, in_epilogue, s);
}

MMTTA_ACT_NS_CLOSE
}  // namespace mmtta

#ifndef MMTTA_ACT_LEAKY_TU
using namespace mmtta;

// The run-time queries: one planning body, then a field of the plan each
static int query_wgrad(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm, const mmtta_tensor* dy,
                       const mmtta_param_sets* sets, WGeo& w) {
  const int st = plan_wgrad(d, x, x_norm, dy, sets, nullptr, w);
  return st < 0 ? st : -st;
}

extern "C" int64_t mmtta_conv_wgrad_workspace_bytes_sets(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_tensor* dy,
                                                         const mmtta_param_sets* sets) {
  WGeo w{};
  return query_wgrad(d, x, nullptr, dy, sets, w) ? -1 : w.workspace_bytes();
}

extern "C" int64_t mmtta_conv_wgrad_workspace_bytes(const mmtta_conv_desc* d, const mmtta_tensor* x,
                                                    const mmtta_tensor* dy) {
  return mmtta_conv_wgrad_workspace_bytes_sets(d, x, dy, nullptr);
}

extern "C" int mmtta_conv_wgrad_plan_sets(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_tensor* dy,
                                          const mmtta_param_sets* sets, int32_t plan[4]) {
  MMTTA_CHECK(plan != nullptr, MMTTA_ERR_INVALID, "wgrad plan: null output");
  WGeo w{};
  const int st = query_wgrad(d, x, nullptr, dy, sets, w);
  if (st == MMTTA_OK) { plan[0] = w.nsl; plan[1] = w.pre_chunks; plan[2] = w.CGp; plan[3] = w.CDp; }
  return st;
}

extern "C" int mmtta_conv_wgrad_kernel(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_tensor* dy) {
  WGeo w{};
  const int st = query_wgrad(d, x, nullptr, dy, nullptr, w);
  return st ? st : w.route;
}

extern "C" int mmtta_conv_wgrad_stages_raw(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                                           const mmtta_tensor* dy) {
  WGeo w{};
  const int st = query_wgrad(d, x, x_norm, dy, nullptr, w);
  return st ? st : w.raw;
}

// the two launching entry points: the descriptor checks, then the body of the translation unit that builds x_norm's activation
static int wgrad_entry(const char* what, const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                       const mmtta_tensor* dy, float* dw, float* db, int accumulate, void* workspace, int64_t workspace_bytes,
                       const mmtta_param_sets* sets, void* stream, const mmtta_update_target* upd) {
  int st = nl_act_check(x_norm, what);
  if (st == MMTTA_OK) st = nl_per_item_check(x_norm, what);
  if (st) return st;
  return (nl_leaky(x_norm) ? leaky::conv_wgrad_body : conv_wgrad_body)(d, x, x_norm, dy, dw, db, accumulate, workspace, workspace_bytes,
                                                                       sets, stream, upd);
}

extern "C" int mmtta_conv_wgrad(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                                const mmtta_tensor* dy, float* dw, float* db, int accumulate, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  return mmtta_conv_wgrad_sets(d, x, x_norm, dy, dw, db, accumulate, workspace, workspace_bytes, nullptr, stream);
}

extern "C" int mmtta_conv_wgrad_sets(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                                     const mmtta_tensor* dy, float* dw, float* db, int accumulate, void* workspace,
                                     int64_t workspace_bytes, const mmtta_param_sets* sets, void* stream) {
  return wgrad_entry("conv_wgrad (x_norm)", d, x, x_norm, dy, dw, db, accumulate, workspace, workspace_bytes, sets, stream, nullptr);
}

extern "C" int mmtta_conv_wgrad_updates_in_epilogue(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                                                    const mmtta_tensor* dy, const mmtta_param_sets* sets) {
  WGeo w{};
  const int st = query_wgrad(d, x, x_norm, dy, sets, w);
  return st ? st : (w.upd_in_epilogue ? 1 : 0);      // (0 wherever mmtta_conv_wgrad_update_sets refuses or takes two launches)
}

extern "C" int mmtta_fused_update_enabled(void) { return g_fused_update != 0 ? 1 : 0; }

extern "C" int mmtta_conv_wgrad_update_sets(const mmtta_conv_desc* d, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                                            const mmtta_tensor* dy, const mmtta_update_target* target, void* workspace,
                                            int64_t workspace_bytes, const mmtta_param_sets* sets, void* stream) {
  MMTTA_CHECK(g_fused_update != 0, MMTTA_ERR_UNSUPPORTED, "wgrad update: switched off (MMTTA_FUSED_UPDATE=0)");
  MMTTA_CHECK(target != nullptr, MMTTA_ERR_INVALID, "wgrad update: null target");
  return wgrad_entry("conv_wgrad_update (x_norm)", d, x, x_norm, dy, nullptr, nullptr, 0, workspace, workspace_bytes, sets, stream, target);
}
#endif  // MMTTA_ACT_LEAKY_TU
