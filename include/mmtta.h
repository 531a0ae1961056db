/*
 * mmtta.h - C ABI of libmmtta.so, the MI355X (gfx950) kernels of the per-volume adaptation
 * hot path of zhm1205/Multimodal_TTA.
 *
 * Boundary rules ("C-ABI layer"):
 *   - plain C: pointers, sizes, POD structs; no torch / C++ types in any signature;
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is allocated or freed
 *     inside, all scratch memory is passed in as a workspace;
 *   - every call is asynchronous on the hipStream_t passed as `void* stream` (0 = default
 *     stream) and safe to capture into a hipGraph (no sync, no malloc, no host readback);
 *   - return value: 0 on success, negative mmtta_status otherwise; never throws.
 *
 * The reference has no native layer.  Each entry point names the torch / MONAI call it
 * stands in for and the reference file:line that reaches it.  "Reference" paths are relative
 * to the upstream repository root.
 *
 * Internal activation layout: channels-last NDHWC ("CL"), element stride 1 along C, described
 * by mmtta_tensor.  Boundary tensors (input volume, returned logits, labels) are NCDHW.
 */
#ifndef MMTTA_H
#define MMTTA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMTTA_ABI_VERSION 2

typedef enum {
  MMTTA_OK = 0,
  MMTTA_ERR_INVALID = -1,     /* bad argument (null pointer, negative size, bad enum) */
  MMTTA_ERR_UNSUPPORTED = -2, /* valid request this build has no kernel for (stated in message) */
  MMTTA_ERR_LAUNCH = -3,      /* hipLaunch / hipGetLastError failure */
  MMTTA_ERR_WORKSPACE = -4    /* workspace too small */
} mmtta_status;

typedef enum { MMTTA_F32 = 0, MMTTA_BF16 = 1 } mmtta_dtype;

/* A 5-D view.  Strides are in ELEMENTS.  Kernels that need channels-last require sc == 1. */
typedef struct {
  void* ptr;
  int32_t n, c, d, h, w;
  int64_t sn, sc, sd, sh, sw;
  int32_t dtype; /* mmtta_dtype */
  int32_t flags; /* MMTTA_TENSOR_* */
} mmtta_tensor;

/* The (sw - c) elements behind every voxel's channels are padding that belongs to this view (a buffer allocated
 * with a channel row padded to 4 floats, not a slice of a wider tensor): kernels may overwrite them with zeros so
 * that a 3-channel voxel is ONE full 16-byte store instead of three partial ones (partial 32-byte sectors cost a
 * read-modify-write in HBM). */
#define MMTTA_TENSOR_OWNS_PAD 1

/* Per-(n,c) normalisation applied to a tensor WHEN IT IS READ ("norm on load"):
 *   v = (x - mean[n*C+c]) * rstd[n*C+c] * (gamma ? gamma[a+c] : 1) + (beta ? beta[a+c] : 0),
 *   a = per_item ? n*C : 0;
 *   then the activation `relu` (an mmtta_act code):
 *     MMTTA_ACT_NONE        v
 *     MMTTA_ACT_RELU        max(v, 0)
 *     MMTTA_ACT_LEAKY_RELU  v > 0 ? v : negative_slope * v   (torch leaky_relu, any finite slope)
 *   and the backward kernels (mmtta_norm_bwd_*, mmtta_combine's adjoint) scale the incoming gradient by the derivative at
 *   `post` (the activation's input): RELU [post > 0], LEAKY_RELU post > 0 ? 1 : negative_slope (torch leaky_relu_backward).
 * mean == NULL means "no transform".  This is MONAI's ADN (Norm -> Dropout(p=0) -> Act) of the
 * producing Convolution, folded into the consumer (reference:
 * src/models/unet_multimodal_midfusion.py:45-55 via monai Convolution/ADN).
 *
 * Layout: `negative_slope` and `_pad2` were appended in ABI version 2 without a version bump.  The library reads
 * `negative_slope` ONLY when relu == MMTTA_ACT_LEAKY_RELU, so a 56-byte descriptor built against the earlier layout (code
 * 0 or 1) is never read past its end; mmtta_conv_epilogue holds this struct as its last member, so the same holds there.
 * A code outside 0..2, or a LEAKY_RELU descriptor with a non-finite slope, is MMTTA_ERR_INVALID in every entry point that
 * takes a descriptor, before anything is launched. */
#define MMTTA_ACT_NONE 0
#define MMTTA_ACT_RELU 1
#define MMTTA_ACT_LEAKY_RELU 2
typedef struct {
  const float* mean;  /* [N*C] or NULL */
  const float* rstd;  /* [N*C] */
  const float* gamma; /* [C] (per_item: [N*C]) or NULL */
  const float* beta;  /* [C] (per_item: [N*C]) or NULL */
  int32_t relu;       /* activation code MMTTA_ACT_* (the name is kept from when ReLU was the only one: 0 / 1 unchanged) */
  /* 0: gamma / beta are one [C] vector for the whole batch.  1: they hold one [C] vector PER BATCH ITEM ([N*C], the
   * gamma_items / beta_items of mmtta_norm_stats_finalize_sets: a group of volumes, each with its own norm affines).
   * Every entry point that reads a norm-on-load honours it; the convolution entry points (mmtta_conv_run*, the epilogue's
   * add_norm, mmtta_conv_wgrad*) read such a descriptor through scale / shift only and refuse one without them
   * (MMTTA_ERR_INVALID). */
  int32_t per_item;
  /* optional precombined form written by mmtta_norm_stats_finalize: v = x*scale[n*C+c] + shift[n*C+c].
   * When given, consumers read ONLY these two arrays (one branch-free vector load per thread instead of four
   * dependent ones); mean / rstd / gamma / beta are still what the backward kernels use. */
  const float* scale; /* [N*C] or NULL */
  const float* shift; /* [N*C] or NULL */
  float negative_slope; /* MMTTA_ACT_LEAKY_RELU only (read for no other code) */
  int32_t _pad2;
} mmtta_norm_on_load;

const char* mmtta_last_error(void);   /* thread-local text for the last non-zero status */
int mmtta_abi_version(void);

/* Measurement aid (bench.py's roofline pass): key MMTTA_OPT_PROFILE_MAIN_KERNEL_ONLY != 0 makes the multi-kernel
 * entry points (mmtta_conv_wgrad: main kernel + slab reductions; split-K mmtta_conv_run: main kernel + finalize)
 * launch ONLY their main kernel, so that two events around the call time exactly the kernel rocprofv3 names.
 * Results of such calls are not valid outputs.  Returns the previous value. */
#define MMTTA_OPT_PROFILE_MAIN_KERNEL_ONLY 1
/* Launch-geometry knobs, read when a convolution is PLANNED or LAUNCHED; they change how work is split, never the
 * result beyond fp32 summation order.  A caller that caches mmtta_conv_plan results (workspace size, statistics rows)
 * must drop them after changing a knob and set knobs before capturing launches into a graph (the Python layer does
 * both: ops.set_option).  Defaults are the measured optimum for four volumes in flight per GPU (DESIGN.md section
 * 3.3); `scripts/sweep_tuning.py` sweeps them inside one process.
 *   SPLITK_BELOW / SPLITK_TARGET  implicit GEMM: split the reduction when a launch has fewer workgroups than BELOW, up
 *                                 to about TARGET workgroups                                    (defaults 96 / 128)
 *   WGRAD_WORKGROUPS              workgroups (slabs x channel blocks) of a weight-gradient launch      (default 128)
 *   WGRAD_THIN_SLABS              slabs of the thin-layer weight gradient (<= 4 channels on one side)   (default 256)
 * Returns the previous value, MMTTA_ERR_INVALID for an unknown key or a value < 1. */
#define MMTTA_OPT_SPLITK_BELOW 2
#define MMTTA_OPT_SPLITK_TARGET 3
#define MMTTA_OPT_WGRAD_WORKGROUPS 4
#define MMTTA_OPT_WGRAD_THIN_SLABS 5
/* 1 (default): the bf16 3x3x3 stride-1 stages of the implicit GEMM use the row-structured loader (8-channel items, a
 * thread owns one (x, channel chunk) column of the halo box, geometry paid once per tile, 32-bit offsets; needs strides
 * < 2^24 and < 2^31 elements per tensor, else the generic loader runs) and request the first passes of stage k+1 while
 * the matrix cores work on stage k; 0: the generic loader, load -> barrier -> MFMA -> barrier as in round 1.  Same
 * results bit for bit. */
#define MMTTA_OPT_IGEMM_PIPELINE 6
/* 1 (default): implicit-GEMM epilogues store 16 bytes per lane through an LDS transposition (same values; the
 * statistics rows sum in a different order); 0: four-byte stores straight from the accumulators (round 1). */
#define MMTTA_OPT_EPILOGUE_VEC16 9
/* 1 (default): the 32-output-channel stride-1 layers of bf16 precision (the 64^3 level of the U-Net) use the lean 4x8x8
 * tile (two row blocks per wave: half the accumulator registers, twice the workgroups: 1024 at 64^3, three to four per CU,
 * so that another workgroup's MFMAs cover a workgroup's staging); 0: the 8x8x8 tile (512 workgroups, two per CU).  Same
 * products in the same order: outputs equal bit for bit, the statistics rows are per tile.  Measured: neutral when the
 * implicit GEMM staged one item per trip (r02c), +1.2 % volumes/s with the row loaders (same-box A/B 65.2 against 64.4).
 * Changes the statistics rows a convolution writes: set before planning. */
#define MMTTA_OPT_IGEMM_LEAN 10
/* Kernel of the bf16-operand weight gradients (csrc/conv_wgrad.hip):
 *   1 (default)  the transposed-read kernels for every operand pair that admits their 16-byte items (16-byte-aligned
 *      rows, strides < 2^24, < 2^31 elements): operands stay [voxel][channel] in LDS as in HBM and ds_read_b64_tr_b16
 *      transposes them on the way into the MFMA (27 taps: wgrad_tr_kernel, 1x1x1: wgrad_tr1_kernel);
 *   0  (and every operand pair the above cannot take) the fp32-operand kernel: exact fp32 products.
 * Equal within the bf16 operand rounding (tests/test_hip_conv.py::test_transposed_read_wgrad). */
#define MMTTA_OPT_WGRAD_VECTOR_STAGING 11
/* Stride-2 transposed forms (ConvTranspose3d forward, input gradient of a stride-2 Conv3d) in bf16 mode: when one
 * workgroup per coarse 4 x 4 x 8 tile and 32 output channels makes at least this many workgroups (default 128), all 8
 * output parity classes of a tile are produced by ONE workgroup from one staged halo box (csrc/conv_igemm.hip,
 * igemm_cls8_kernel) instead of 8 x tiles workgroups that each stage their own; 0: never.  Same products, the taps of a
 * class summed before the channel stages instead of after: equal to the per-class kernel within fp32 summation order.
 * Changes the statistics rows a convolution writes (mmtta_conv_plan reports them): set before planning. */
#define MMTTA_OPT_CLASS_FUSED_MIN_WORKGROUPS 12
/* 1 / 2 (default) / 3: in bf16 precision the 3x3x3 stride-1 convolutions with <= 4 channels on both sides (forward and input
 * gradient of the U-Net's last residual unit) run on v_mfma_f32_4x4x4_16B_bf16 (operands rounded to bf16 like every other
 * matrix-core layer of that mode, one instruction per tap and 64 voxels); 0: fp32 FMAs on the vector ALU
 * (direct_row_kernel), as in fp32 precision.  Measured round 2 (3 -> 3 at 128^3): 33 us against 43 us per launch, +0.5 to
 * +1 % volumes/s; full-size parity against the fp32 oracle unchanged (logits 1.496e-2 vs 1.494e-2 of max, Dice 6e-5).
 * The value picks the workgroup tile: 1 = 8 x 8 x 64 voxels (two workgroups per CU), 2 = 4 x 8 x 64 (four per CU: another
 * workgroup's MFMAs cover a workgroup's staging; same-box A/B 64.1 against 63.7 volumes/s), 3 = 2 x 8 x 64.
 * Changes the statistics rows such a convolution writes: set before planning. */
#define MMTTA_OPT_THIN_MFMA 13
/* 1 (default): the 3x3x3 stride-1 32 -> 32 layers of bf16 precision (forward and input gradient) run igemm_reuse_kernel
 * (route 18 of mmtta_conv_route) when the call does not split K, takes the row-structured loader and the 16-byte epilogue: the lean tile with
 * the rows of a wave's two blocks split by the parity of x, so that neighbouring kx taps share activation fragments (36
 * LDS fragment reads per 16-channel stage instead of 54); 0: the lean tile as before (route 14).  The same MFMAs
 * with the same operands in the same order: outputs and statistics rows equal bit for bit.  A run whose bias is not
 * 16-byte aligned stays on route 14 (its 4-byte epilogue); mmtta_conv_route, which is shown no bias, cannot tell.
 * Measured (profiles/igemm64_reuse_ab.md, same machine, parent against change): 132.6 -> 111.9 us per launch of a group
 * of 8; volumes/s +1.6 % in one alternated series (outside its run-to-run spread), +0.8 % in a second (inside it). */
#define MMTTA_OPT_IGEMM_FRAGMENT_REUSE 14
/* Measurement aid of mmtta_lame_refine: 1 (default) calls that qualify for the tiled kernel take it; 0: every call runs the
 * generic kernel (how profiles/lame_kernels.md compares the two on one input).  Equal within fp32 summation order. */
#define MMTTA_OPT_LAME_TILED 15
/* Raw staging of bf16-stored operands that take no transform (a bit mask; default 3; 0: every launch stages through the
 * transform as before, in the same process).
 *   bit 0  implicit GEMM (csrc/conv_igemm.hip: igemm_raw_kernel, igemm_reuse_raw_kernel, igemm_cls8_raw_kernel): a call
 *          whose x is bf16-stored, in whole 8-channel chunks (x.c % 8 == 0) of 16-byte-aligned items, with no norm-on-load
 *          or one that has neither mean nor scale and no activation, on a bf16-operand tile with y (and the fused add)
 *          bf16-stored too, copies each 16-byte item of the input box to LDS as loaded, under its halo / channel-chunk
 *          mask.  The transform of such an input - unpack, x * 1 + 0, max with -inf, round to bf16 - is the identity on
 *          every finite value and on the infinities, so outputs, statistics rows and split-K sums are equal bit for bit.
 *          mmtta_conv_stages_raw tells whether a call qualifies; mmtta_conv_route reports the same routes either way.
 *   bit 1  the transposed-read 27-tap weight gradient of the stride-2 layers, convolutions and transposed convolutions
 *          (csrc/conv_wgrad.hip: wgrad_tr_raw_kernel; the stride-1 forms measured slower and are not built), with x and
 *          dy both bf16-stored: dy (dy.c % 8 == 0), which never takes a transform, and - next to a raw dy - an x under the rule
 *          of bit 0 go to LDS as loaded, under their masks.  With a bias gradient dy is still unpacked for the fp32 sums.
 *          Slabs, dw and db equal bit for bit; mmtta_conv_wgrad_stages_raw tells which operands qualify.
 * Two documented differences, neither visible in a finite result: a stored -0.0 reaches the matrix cores as -0.0 (the
 * transform made it +0.0; sums start at +0, so no output bit depends on it), and a stored NaN stays a NaN, where the
 * transform's fmaxf(NaN, -inf) turned it into -inf.  Returns the previous value. */
#define MMTTA_OPT_RAW_STAGING 16
/* Two passes over the full-resolution tensors of an entropy-minimisation step that the result does not need (a bit mask;
 * default 3; 0: the launches as before, in the same process).
 *   bit 0  mmtta_conv_head_loss_run_sets: the 3x3x3 stride-1 R -> R head convolution (R <= 4) on the 4x4x4 matrix tiles with
 *          the Bernoulli entropy objective in its epilogue (csrc/conv_direct.hip: conv3_mfma4_loss_kernel).  The logits of a
 *          step are read by the objective alone: they are not stored, and mmtta_entropy_loss_items' pass over them goes.
 *          d(logits) equal bit for bit, the loss within the order of its fp64 partial sums.  mmtta_conv_head_loss_eligible
 *          tells whether a call qualifies; with the bit clear it says no and the entry point refuses.
 *   bit 1  reserved for the paired thin weight gradients of a stride-2 residual block (not built).
 * Returns the previous value. */
#define MMTTA_OPT_HEAD_LOSS_PAIR 17
/* Lean stage and epilogue of the thin full-resolution convolutions (a bit mask; default 3; 0: the launches as before, in the
 * same process).  No route, plan, tile shape, statistics row or workspace size depends on it.
 *   bit 0  the thin-K convolution on the matrix cores (csrc/conv_direct.hip: chan_mfma_lean_kernel, route 13) at stride 2 from
 *          a bf16-stored gathered tensor into a bf16-stored y of exactly 32 or 64 channels, y and a fused add in 16-byte-aligned
 *          rows, without accumulate.  The values of a wave go through a wave-private LDS tile and leave as 16-byte stores (8
 *          channels of one voxel per lane) instead of one 4-byte store per channel pair from half the lanes behind a
 *          cross-lane exchange through LDS; the fused add is read in the same 16-byte items; a tile inside the output drops
 *          its spatial masks; the stage masks the stored voxel instead of unpacking it for any channel count.
 *   bit 1  the gather-GEMM up-convolution (upconv8_lean_kernel) from a bf16-stored input without a norm-on-load transform:
 *          each 16-byte item goes to LDS as loaded, under its in-bounds mask, and a tile inside the output skips the bounds
 *          tests per fine voxel.
 * Every stored value is the same round-to-nearest-even of the same fp32 value and the statistics rows are summed in the
 * same order: outputs and rows equal bit for bit.  mmtta_conv_thin_lean tells which form a call takes.  A call with a
 * LeakyReLU on x or on the fused add keeps the plain kernels.  Returns the previous value. */
#define MMTTA_OPT_THIN_LEAN 18
/* 1 (default): a fused weight update (mmtta_conv_wgrad_update_sets) whose weight gradient plans ONE slab per parameter set
 * steps the optimizer in the epilogue of the transposed-read weight-gradient kernel (csrc/conv_wgrad.hip:
 * wgrad_tr_upd_kernel): the workgroup that holds the complete gradient of a 27 x 32 x 32 block in its registers runs the
 * optimizer on p / m / v and writes both bf16 images, so the slab is neither written nor read back and
 * wgrad_update27_kernel is not launched.  The bias is stepped there too.
 * Taken by a stride-1 3x3x3 Conv3d of bf16 precision with x and dy bf16-stored, cin and cout multiples of 32, one dense
 * column block per workgroup (cout > 128, or an odd number of 32-channel blocks), no pre-reduce, p / m / v of every set on
 * 16 bytes, outside the LeakyReLU instantiation.  The stride-2 forms (Conv3d and ConvTranspose3d) were measured slower than
 * their two launches (profiles/update_epilogue_ab.md) and are not built.  Everything else, and 0, takes the two launches as
 * before, in the same process.  The same sums, optimizer arithmetic and rounding: p, m, v, the bias and both images equal
 * bit for bit.  Workspace sizes and plans do not depend on it.
 * mmtta_conv_wgrad_updates_in_epilogue tells whether a call qualifies.  Returns the previous value. */
#define MMTTA_OPT_WGRAD_EPILOGUE_UPDATE 19
/* 1 (default): a class-fused stride-2 transposed form (route 15) that stages raw (MMTTA_OPT_RAW_STAGING bit 0) runs
 * igemm_cls8_pipe_kernel (csrc/conv_igemm.hip): two weight images in LDS, the image of channel stage k+1 fetched by direct
 * global-to-LDS loads (no registers in between) while the matrix cores work on stage k, and the box items of stage k+1
 * requested at the same point and committed behind the barrier that closes stage k.  0: igemm_cls8_raw_kernel, request ->
 * wait -> commit -> barrier -> MFMA -> barrier, in the same process.  The same MFMAs with the same operands in the same
 * order, the same epilogue: outputs, accumulated / fused-add destinations and statistics rows equal bit for bit.  No route,
 * plan, statistics row or workspace size depends on it; a call that keeps the transform (norm-on-load, fp32-stored
 * tensors, the LeakyReLU instantiation) keeps its kernel.  mmtta_conv_cls8_pipelined tells whether a call qualifies.
 * Returns the previous value. */
#define MMTTA_OPT_CLS8_PIPELINE 20
/* 1 (default): a call that runs the pipelined class-fused kernel (MMTTA_OPT_CLS8_PIPELINE) and whose y - and fused add, if
 * there is one - has a multiple of 8 channels runs igemm_cls8_lean_kernel (csrc/conv_igemm.hip): the same K loop, and for every
 * coarse 4 x 4 x 8 tile whose 8 x 8 x 16 output block lies wholly inside y an epilogue of its own (epilogue_cls8_lean): the
 * row offsets worked out once per tile instead of once per parity class, the fused-add / accumulate operands of the next
 * classes requested while a class is finished, 16-byte stores through a lane-pair exchange, and no statistics arithmetic
 * when no statistics rows are asked for.  A tile on the border of y (an odd output extent, a partial tile) takes the
 * epilogue of igemm_cls8_pipe_kernel inside the same launch.  0: igemm_cls8_pipe_kernel, in the same process.  The same
 * values through the same operations in the same order: outputs, accumulated / fused-add destinations and statistics rows
 * equal bit for bit.  No route, plan, statistics row or workspace size depends on it.  Only bit 0 is read; bit 1 is
 * reserved.  mmtta_conv_cls8_lean_epilogue tells whether a call qualifies.  Returns the previous value. */
#define MMTTA_OPT_CLS8_LEAN_EPILOGUE 21
int mmtta_set_option(int key, int value);

/* ------------------------------------------------------------------ layout (boundary) ---- */
/* NCDHW fp32 <-> channels-last.  Stands in for nothing in the reference: it is the price of
 * the internal layout, paid once per volume on the way in (reference tensor contract:
 * src/datasets/brats.py:343-347, image float32 [C,D,H,W]) and once on the way out
 * (src/evaluation/seg_eval.py:300, logits [B,R,D,H,W]).  Any strides are accepted; `src` is fp32, `dst` fp32 or bf16
 * (round to nearest even: the staged network input of bf16 precision, 8-byte voxels for <= 4 channels). */
int mmtta_copy_strided(const mmtta_tensor* src, const mmtta_tensor* dst, void* stream);

/* ------------------------------------------------------------------ convolution ---------- */
typedef enum {
  MMTTA_CONV_FWD = 0,    /* torch.nn.Conv3d forward,       y = conv(x, W) + b                */
  MMTTA_CONV_DGRAD = 1,  /* its input gradient,            dx = conv_transpose(dy, W)        */
  MMTTA_CONVT_FWD = 2,   /* torch.nn.ConvTranspose3d fwd   (k3 s2 p1 op1), W is [Cin,Cout,k] */
  MMTTA_CONVT_DGRAD = 3  /* its input gradient,            dx = conv(dy, W), stride 2        */
} mmtta_conv_op;

typedef struct {
  int32_t op;      /* mmtta_conv_op */
  int32_t ksize;   /* 1 or 3 (padding (k-1)/2, dilation 1, groups 1) */
  int32_t stride;  /* 1 or 2 (ConvTranspose: 2 only) */
  int32_t cin;     /* channels of the module's INPUT  (Conv3d.in_channels)  */
  int32_t cout;    /* channels of the module's OUTPUT (Conv3d.out_channels) */
  int32_t dtype;   /* arithmetic: MMTTA_F32 (fp32 MFMA, exact fp32) or MMTTA_BF16 */
} mmtta_conv_desc;

/* Size in bytes of the packed weight image for (desc.op): the MFMA-ready copy
 * [tap][K][N] (K = reduction channels, N = produced channels, both zero padded). */
int64_t mmtta_conv_packed_bytes(const mmtta_conv_desc* desc);

/* Repack master weights (torch layout, fp32: Conv3d [Cout,Cin,k,k,k]; ConvTranspose3d
 * [Cin,Cout,k,k,k]) into the image used by mmtta_conv_run for desc.op.
 * Runs once per optimizer step. */
int mmtta_conv_pack_weights(const mmtta_conv_desc* desc, const float* w_master, void* packed, void* stream);

/* The same for MANY images in one launch (every conv of a model, both orientations): the caller builds the
 * table once on the host (pointers are stable: arena + packed buffers), copies it to the device and then calls
 * mmtta_conv_pack_batched once per optimizer step. */
typedef struct {
  mmtta_conv_desc desc;
  const float* w_master;  /* device */
  void* packed;           /* device */
} mmtta_pack_item;
int64_t mmtta_conv_pack_table_bytes(int count);
/* `total` is an opaque work count produced by _table_build and handed back to _pack_batched. */
int mmtta_conv_pack_table_build(const mmtta_pack_item* items, int count, void* table_host, int64_t* total);
int mmtta_conv_pack_batched(const void* table_dev, int count, int64_t total, void* stream);

/* Launch geometry chosen for a problem; filled by mmtta_conv_plan.  It has no run-time operands, so it plans the route of
 * the shape: a call that runs as 16 / 17 / 18 (mmtta_conv_route) is reported as the implicit GEMM it would otherwise be. */
typedef struct {
  int32_t tiles;         /* M tiles (over n and space) per launch                           */
  int32_t launches;      /* 1 (the 8 parity classes of a stride-2 transposed form share one launch) */
  int32_t ksplit;        /* >1: partial sums go through the workspace                        */
  int32_t stats_rows;    /* rows of the [rows][2][C] partial-statistics slab this op writes  */
  int32_t config;        /* kernel id 0..15, see mmtta_conv_route (which template instance runs; for profiling) */
  int32_t _pad;
  int64_t workspace_bytes;
} mmtta_conv_plan_t;

/* `x` is the tensor the op READS, `y` the tensor it PRODUCES (for *_DGRAD: x = dy, y = dx). */
int mmtta_conv_plan(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_tensor* y,
                    mmtta_conv_plan_t* plan);

/* Optional epilogue of mmtta_conv_run: y = acc + bias + T(add), T = norm-on-load of `add`.
 * Fuses MONAI ResidualUnit's `cx + res` (reference: unet_multimodal_midfusion.py:45-55,
 * 121-131 through monai ResidualUnit.forward) into the residual convolution. */
typedef struct {
  const mmtta_tensor* add;          /* NULL: nothing added; same shape as y, channels-last */
  mmtta_norm_on_load add_norm;      /* transform of `add` (mean NULL: added as is)         */
} mmtta_conv_epilogue;

/* One convolution-shaped op as an implicit GEMM on the matrix cores.
 *   Replaces: torch.nn.Conv3d / ConvTranspose3d forward and autograd's input-gradient,
 *   reached from reference src/models/unet.py:68-69 (monai UNet) and
 *   src/models/unet_multimodal_midfusion.py:204-267; backward from
 *   src/core/trainers/seg_trainer.py:142 (loss.backward()).
 *   x        tensor read (channels-last), with an optional norm-on-load
 *   packed   image from mmtta_conv_pack_weights for the same desc
 *   bias     [produced channels] fp32 or NULL
 *   y        tensor written (channels-last); accumulate != 0: y += result
 *   stats    NULL or fp32 [plan.stats_rows][2][C_produced]: per-tile sum / sum of squares of the
 *            values written (input of mmtta_norm_stats_finalize)
 *   workspace  plan.workspace_bytes bytes or NULL when 0 */
int mmtta_conv_run(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                   const void* packed, const float* bias, const mmtta_conv_epilogue* epi,
                   const mmtta_tensor* y, int accumulate, float* stats, void* workspace,
                   int64_t workspace_bytes, void* stream);

/* Which kernel mmtta_conv_run would launch for these operands (host-only, launches nothing; the run itself asks the same
 * planner, csrc/conv_igemm.hip: geometry).  The ids are those of mmtta_conv_plan_t.config, plus the routes that depend
 * on the run-time operands:
 *   0..5 fp32 / 7..12 bf16 implicit GEMM tiles, 14 the lean bf16 tile     6 direct (<= 4 produced channels)
 *   13 thin-K (<= 4 gathered channels)                                    15 class-fused stride-2 transposed form
 *   16 small-K 1x1x1 (fp32, nothing fused)                                17 streaming 1x1x1 (bf16, voxel-dense tensors)
 *   18 the lean bf16 tile with activation fragments shared along x (3x3x3 stride-1 32 -> 32, unsplit; mmtta_conv_plan reports 14)
 * or a negative mmtta error code. */
int mmtta_conv_route(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                     const mmtta_conv_epilogue* epi, const mmtta_tensor* y, int accumulate, const float* stats);

/* Whether mmtta_conv_run would stage the input box of this call raw (MMTTA_OPT_RAW_STAGING bit 0): 1 / 0, or a negative
 * mmtta error code.  Host-only, the operands of mmtta_conv_route, the predicate the launchers themselves ask. */
int mmtta_conv_stages_raw(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                          const mmtta_conv_epilogue* epi, const mmtta_tensor* y, int accumulate, const float* stats);

/* Whether mmtta_conv_run would run this call on the pipelined class-fused kernel (MMTTA_OPT_CLS8_PIPELINE): 1 when the call
 * takes route 15, stages raw and the option is on, else 0, or a negative mmtta error code.  Host-only, the operands of
 * mmtta_conv_route, the predicate the launcher itself asks. */
int mmtta_conv_cls8_pipelined(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                              const mmtta_conv_epilogue* epi, const mmtta_tensor* y, int accumulate, const float* stats);

/* Whether mmtta_conv_run would run this call on the class-fused kernel with the lean interior epilogue
 * (MMTTA_OPT_CLS8_LEAN_EPILOGUE): 1 when mmtta_conv_cls8_pipelined says 1, the option's bit 0 is set and y and the fused add
 * have multiples of 8 channels, else 0, or a negative mmtta error code.  Host-only, the operands of mmtta_conv_route, the
 * predicate the launcher itself asks. */
int mmtta_conv_cls8_lean_epilogue(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                                  const mmtta_conv_epilogue* epi, const mmtta_tensor* y, int accumulate, const float* stats);

/* Which lean kernel of MMTTA_OPT_THIN_LEAN mmtta_conv_run would take for this call: 1 the thin-K convolution (bit 0), 2 the
 * gather-GEMM up-convolution (bit 1), 0 neither, or a negative mmtta error code.  Host-only, the operands of mmtta_conv_route,
 * the predicates the launchers themselves ask. */
int mmtta_conv_thin_lean(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                         const mmtta_conv_epilogue* epi, const mmtta_tensor* y, int accumulate, const float* stats);

/* Which kernel inside routes 6 and 13 mmtta_conv_run would launch for this call:
 *    1 direct_conv_kernel (thread per voxel)                2 direct_klane_kernel (lanes along K = 32 / 64)
 *    3 direct_row_kernel (K <= 4, 3x3x3 stride 1)           4 conv3_mfma4_kernel, fp32-stored thin tensors
 *    5 conv3_mfma4_kernel, every thin tensor bf16-stored    6 direct_upconv_kernel (LDS-staged up-convolution, fp32)
 *    7 upconv_mfma_kernel (the same on the matrix cores)    8 upconv8_kernel (2x2x2 gather GEMM)
 *    9 upconv8_lean_kernel                                  10 pointwise_head_kernel (streaming 1x1x1 head)
 *   11 direct_chan_kernel (thin-K, VALU)                    12 chan_mfma_kernel     13 chan_mfma_lean_kernel
 * 0 for a call of any other route, or the negative mmtta error code the run would return before launching.  Host-only, the
 * operands of mmtta_conv_route; the launchers of the two routes switch on the function this returns. */
int mmtta_conv_thin_kernel(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                           const mmtta_conv_epilogue* epi, const mmtta_tensor* y, int accumulate, const float* stats);

/* ---- per-volume parameter sets: N volumes (or N identical sub-networks) in ONE launch, each with ITS OWN parameters.
 * Episodic adaptation has no cross-volume state: every test volume adapts its own copy of the source weights (SURVEY.md
 * Appendix C), and the M modality encoders of the deep-fusion network are M identical graphs with different weights run
 * one after another by the reference (reference src/models/unet_multimodal_midfusion.py:214-218).  Alone, a volume's
 * launches at the 8^3 / 16^3 / 32^3 levels fill a quarter of the chip or less; here they become the batch items of one
 * launch and the batch index selects the parameter set:
 *     set q of batch item n:   q = n / items_per_set
 *     its parameters:          base + (q / inner) * outer + (q % inner) * inner_stride
 * for the packed weight images (`packed_*`, BYTES) and for what lives in the fp32 parameter arenas: weight gradients
 * (`weight_*`, ELEMENTS) and bias vectors / bias gradients (`bias_*`, ELEMENTS; the arenas of a group of volumes are replicas
 * of one layout, so the outer strides are normally all the replica stride, while the inner ones differ).  Examples:
 * G volumes through a U-Net layer: items_per_set 1, inner 1, outer = replica stride.  G volumes x M modality encoders:
 * batch G*M, items_per_set 1, inner M, inner stride = one encoder's parameters.  The fusion layer the reference applies M
 * times with shared weights: batch G*M, items_per_set M, inner 1 (its weight gradient then sums over the M items of a
 * volume).  NULL = one parameter set for the whole batch (the plain entry points).  Strides must keep 16-byte alignment.
 * Every batch item is computed exactly as if it had been launched alone with its set: same tiles, same reduction splits,
 * same summation order - grouped and one-at-a-time runs agree bit for bit (tests/test_hip_groups.py). */
typedef struct {
  int32_t items_per_set; /* consecutive batch items that share a parameter set (>= 1; must divide N) */
  int32_t inner;         /* sets per outer step (>= 1) */
  int64_t packed_outer, packed_inner; /* BYTES between packed weight images */
  int64_t weight_outer, weight_inner; /* ELEMENTS between weight gradients dw (torch weight layout) */
  int64_t bias_outer, bias_inner;     /* ELEMENTS between bias vectors / bias gradients db */
} mmtta_param_sets;

/* mmtta_conv_run with per-item parameter sets: `packed` and `bias` are the base pointers of set 0. */
int mmtta_conv_run_sets(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                        const void* packed, const float* bias, const mmtta_conv_epilogue* epi,
                        const mmtta_tensor* y, int accumulate, float* stats, void* workspace,
                        int64_t workspace_bytes, const mmtta_param_sets* sets, void* stream);

/* The head convolution of an entropy-minimisation step with the objective as its tail (MMTTA_OPT_HEAD_LOSS_PAIR bit 0):
 * mmtta_conv_run_sets(desc, x, x_norm, packed, bias, epi, y, 0, NULL, ...) followed by mmtta_entropy_loss_items(y, softmax,
 * dlogits, ...) in one launch (plus the finish kernel) that never stores y.  `y` describes the logits the convolution would
 * have produced (shape, strides and storage decide eligibility and the order of dlogits); its memory is not touched.
 *   dlogits   fp32- or bf16-stored gradient of the shape of y, equal bit for bit to the two calls' (pad lanes zero)
 *   partial   mmtta_conv_head_loss_partials doubles: one per workgroup, [item][workgroup of the item]
 *   loss      [N] (per_item != 0: every batch item its own objective, as mmtta_entropy_loss_items), or [1] for N == 1;
 *             equal to the two calls' within the summation order of the fp64 partials
 * A call qualifies when it routes to the 4x4x4 matrix-tile kernel of bf16 precision (mmtta_conv_route 6, desc.op
 * MMTTA_CONV_FWD, 3x3x3 stride 1, <= 4 channels on both sides, MMTTA_OPT_THIN_MFMA != 0) with x, y and the fused add
 * fp32-stored and no LeakyReLU on either; softmax == 0; per_item != 0 or N == 1; y and dlogits in dense 16-byte (bf16: 8-byte)
 * voxel rows, dlogits owning its pad lane (the fast path of mmtta_entropy_loss_items); an item below 2^31 elements and of
 * at most 2048 workgroups (tiles of MMTTA_OPT_THIN_MFMA's depth x 8 x 64 voxels).  Anything else: _eligible returns 0 and
 * _run_sets MMTTA_ERR_UNSUPPORTED before anything is launched - the caller keeps the two calls.  _eligible is host-only and
 * returns 1 / 0 or a negative mmtta error code for descriptors mmtta_conv_run itself would reject; _partials returns -1 for
 * a call that is not route 6. */
int mmtta_conv_head_loss_eligible(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                                  const mmtta_conv_epilogue* epi, const mmtta_tensor* y, const mmtta_tensor* dlogits,
                                  int softmax, int per_item);
int64_t mmtta_conv_head_loss_partials(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_tensor* y);
int mmtta_conv_head_loss_run_sets(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                                  const void* packed, const float* bias, const mmtta_conv_epilogue* epi,
                                  const mmtta_tensor* y, const mmtta_tensor* dlogits, int softmax, int per_item,
                                  double* partial, float* loss, const mmtta_param_sets* sets, void* stream);

/* Weight (and bias) gradient.
 *   Replaces: autograd's weight-gradient of Conv3d / ConvTranspose3d
 *   (reference src/core/trainers/seg_trainer.py:142).
 *   desc.op  MMTTA_CONV_FWD or MMTTA_CONVT_FWD (which module the gradient is for)
 *   x, x_norm the module's forward input (with the transform it was read with)
 *   dy       gradient of the module's output
 *   dw       fp32, torch layout of the module's weight; accumulate != 0: dw += result
 *   db       fp32 [cout] or NULL */
int64_t mmtta_conv_wgrad_workspace_bytes(const mmtta_conv_desc* desc, const mmtta_tensor* x,
                                         const mmtta_tensor* dy);
/* Which weight-gradient kernel mmtta_conv_wgrad picks for this problem (profiling / roofline bookkeeping):
 *   0 fp32 MFMA k3 s1   1 fp32 MFMA k3 s2 (and conv_transpose)   2 fp32 MFMA k1
 *   3 small-channel (wgrad_small_kernel: <= 4 channels on one side)  6 tiny (wgrad_tiny_kernel: <= 4 channels on both sides, fp32 VALU)
 *   7 bf16 operands, transposed reads (wgrad_tr_kernel), k3 s1   8 the same at stride 2 (and conv_transpose)
 *   9 the 1x1x1 streaming kernel of bf16 precision (wgrad_tr1_kernel)
 *   10 the thin 27-tap layers of bf16 precision (wgrad_thin_tr_kernel)          (4 and 5 are retired)
 * or a negative mmtta error code. */
int mmtta_conv_wgrad_kernel(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_tensor* dy);
/* Which operands of this weight gradient the transposed-read kernel would stage raw (MMTTA_OPT_RAW_STAGING bit 1): bit 0
 * the module input x, bit 1 the gradient dy; 0 for every other kernel, or a negative mmtta error code.  Host-only, a
 * field of the plan the launcher itself reads. */
int mmtta_conv_wgrad_stages_raw(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                                const mmtta_tensor* dy);
int mmtta_conv_wgrad(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                     const mmtta_tensor* dy, float* dw, float* db, int accumulate, void* workspace,
                     int64_t workspace_bytes, void* stream);

/* The weight gradient of every parameter set of the batch in one launch sequence: `dw` / `db` are the base pointers of
 * set 0; set q's gradient is the sum over ITS batch items only (slabs never mix sets), reduced in the order the plain call
 * uses for a batch of items_per_set.  Workspace: mmtta_conv_wgrad_workspace_bytes_sets. */
int64_t mmtta_conv_wgrad_workspace_bytes_sets(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_tensor* dy,
                                              const mmtta_param_sets* sets);
int mmtta_conv_wgrad_sets(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                          const mmtta_tensor* dy, float* dw, float* db, int accumulate, void* workspace,
                          int64_t workspace_bytes, const mmtta_param_sets* sets, void* stream);
/* The reduction plan of that launch sequence (bookkeeping for profiles and tests; nothing is launched):
 *   plan[0] partial slabs per set   plan[1] chunks of the pre-reduce stage (0: none; else the last stage reads these)
 *   plan[2], plan[3] the padded channel counts CGp, CDp of a slab's [tap][CGp][CDp] rows */
int mmtta_conv_wgrad_plan_sets(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_tensor* dy,
                               const mmtta_param_sets* sets, int32_t plan[4]);

/* ------------------------------------------------------------------ input pre-pass -------- */
/* Per-channel intensity rule of one image [C,D,H,W] (reference src/datasets/transforms.py:129-223).
 *   legacy != 0: y = (x - mean) / std                                            (:202-223)
 *   else: optional clip to [lo,hi], then optional z-score with mean / std(unbiased=False, floor eps) taken over the
 *   clipped voxels > mask_gt when `masked` and at least min_count of them exist, over all voxels otherwise (:163-198) */
typedef struct {
  int32_t clip, zscore, masked, min_count;
  float lo, hi, mask_gt, eps;
  float mean, std;
  int32_t legacy, _pad;
} mmtta_intensity_rule;
int64_t mmtta_intensity_scratch_bytes(int channels);
/* x, y: n == 1, NCDHW boundary layout (dense voxels per channel); rules: HOST array of x->c entries. */
int mmtta_intensity_normalize(const mmtta_tensor* x, const mmtta_intensity_rule* rules, const mmtta_tensor* y,
                              void* scratch, void* stream);

/* ------------------------------------------------------------------ normalisation -------- */
typedef enum {
  MMTTA_NORM_INSTANCE = 0, /* torch.nn.InstanceNorm3d(affine=False): statistics per (n,c)      */
  MMTTA_NORM_BATCH = 1,    /* torch.nn.BatchNorm3d: statistics per c over (n,d,h,w)            */
  MMTTA_NORM_GROUP = 2     /* torch.nn.GroupNorm: statistics per (n, group of C/groups chans)  */
} mmtta_norm_kind;

/* Turn per-tile partial sums into the per-(n,c) mean / rstd that consumers read.
 *   Replaces: the statistics half of F.instance_norm / F.batch_norm / F.group_norm (biased
 *   variance, eps inside the sqrt), reached from monai ADN "N".
 *   part     fp32 [rows][2][C] from mmtta_conv_run (rows = rows_per_n * N, n-major)
 *   scratch  fp64 [N*C*2] (fp64 totals between the two stages)
 *   count    voxels per (n,c) = D*H*W
 *   running_mean/var, momentum: BatchNorm only.  training != 0: batch statistics are used and
 *            the running buffers get the EMA update (unbiased variance), the "norm-stat
 *            update" of the adaptation step; training == 0: running statistics are used.
 *   mean, rstd   fp32 [N*C] outputs
 *   gamma, beta  [C] affine parameters or NULL; scale, shift  fp32 [N*C] outputs or NULL:
 *                scale = rstd*gamma, shift = beta - mean*scale (the precombined norm-on-load form) */
int mmtta_norm_stats_finalize(int kind, int groups, const float* part, int rows_per_n, int n, int c,
                              int64_t count, float eps, int training, float* running_mean,
                              float* running_var, float momentum, float* mean, float* rstd,
                              const float* gamma, const float* beta, float* scale, float* shift,
                              double* scratch, void* stream);

/* ---- per-volume norm parameter sets: the norm layers of a group of volumes adapted side by side (mmtta_param_sets), each
 * volume with its own norm affines and - BatchNorm - its own running statistics.  Batch item n belongs to set
 * q = n / items_per_set; set q's gamma / beta (and dgamma / dbeta) live q * affine_stride elements behind the base pointers
 * (the arena replica stride), its running_mean / running_var q * stats_stride elements behind theirs.  BatchNorm statistics
 * (and the backward's m1 / m2, dgamma / dbeta) pool over THAT set's items only, in the order the plain entry point uses for
 * a batch of items_per_set: every set computes bit for bit what the plain call computes for its items alone.  Strides must
 * keep 16-byte alignment (multiples of 4 elements); with more than one set, affine_stride must be >= C where affine
 * gradients are written and stats_stride >= C where running statistics are given (sets may share read-only affines with
 * affine_stride 0, never written vectors). */
typedef struct {
  int32_t items_per_set; /* consecutive batch items that share a set (>= 1; must divide N) */
  int32_t _pad;
  int64_t affine_stride; /* ELEMENTS between the gamma / beta / dgamma / dbeta of consecutive sets */
  int64_t stats_stride;  /* ELEMENTS between the running_mean / running_var of consecutive sets */
} mmtta_norm_sets;

/* mmtta_norm_stats_finalize over norm parameter sets: `gamma`, `beta`, `running_mean`, `running_var` are the base pointers of
 * set 0.  training != 0 applies the EMA update to every set's running statistics (BatchNorm; once per set, from the set's
 * batch statistics); training == 0 reads them.  gamma_items / beta_items (fp32 [N*C] or NULL; NULL when gamma / beta is
 * NULL): each item's copy of its set's gamma / beta, the per_item arrays a mmtta_norm_on_load with per_item = 1 points at
 * (the consumers, mmtta_norm_bwd_reduce and mmtta_norm_bwd_apply read them).  Arguments are checked before any launch. */
int mmtta_norm_stats_finalize_sets(int kind, int groups, const float* part, int rows_per_n, int n, int c,
                                   int64_t count, float eps, int training, float* running_mean,
                                   float* running_var, float momentum, float* mean, float* rstd,
                                   const float* gamma, const float* beta, float* scale, float* shift,
                                   float* gamma_items, float* beta_items, double* scratch,
                                   const mmtta_norm_sets* sets, void* stream);

/* Rows per batch item of the partial slabs written by mmtta_channel_stats and
 * mmtta_norm_bwd_reduce for a tensor of this shape (deterministic two-stage reductions). */
int mmtta_reduce_rows_per_n(const mmtta_tensor* t);

/* Per-(n,c) partial sum / sum-of-squares of a tensor that no convolution epilogue produced.
 * part: fp32 [N * mmtta_reduce_rows_per_n(x)][2][C]. */
int mmtta_channel_stats(const mmtta_tensor* x, float* part, void* stream);

/* out = Ta(a) + Tb(b)  (b may be NULL), Ta/Tb = norm-on-load.  Materialises
 * act(norm(y)) [+ residual]: monai ResidualUnit.forward's add with an Identity residual. */
int mmtta_combine(const mmtta_tensor* a, const mmtta_norm_on_load* ta, const mmtta_tensor* b,
                  const mmtta_norm_on_load* tb, const mmtta_tensor* out, void* stream);

/* Backward of norm(+activation), pass 1: per-(n,c) reductions
 *   s1[n,c] = sum dz, s2[n,c] = sum dz * xhat,  dz = dout * act'(post) (see mmtta_norm_on_load),
 *   xhat = (y - mean) * rstd,  post = gamma*xhat + beta.
 *   part: fp32 [N * mmtta_reduce_rows_per_n(y)][2][C].  Replaces the reduction half of
 *   native_*_norm_backward. */
int mmtta_norm_bwd_reduce(const mmtta_tensor* dout, const mmtta_tensor* y, const mmtta_norm_on_load* t,
                          float* part, void* stream);

/* Pass 2 coefficients: from part -> m1, m2 [N*C] (group means of gamma*dz and gamma*dz*xhat) and,
 * if gamma is trained, dgamma / dbeta [C] (accumulate != 0: +=).  training == 0 (BatchNorm on
 * running statistics): m1 = m2 = 0. */
int mmtta_norm_bwd_finalize(int kind, int groups, const float* part, int rows_per_n, int n, int c, int64_t count,
                            const float* gamma, int training, float* m1, float* m2, float* dgamma,
                            float* dbeta, int accumulate, double* scratch /* fp64 [N*C*2] */, void* stream);

/* mmtta_norm_bwd_finalize over norm parameter sets (mmtta_norm_sets): `gamma`, `dgamma`, `dbeta` are the base pointers of
 * set 0; m1 / m2 pool over each set's items (BatchNorm), set q's dgamma / dbeta are the sums over ITS items, written (or,
 * accumulate != 0, added) q * affine_stride elements behind the base pointers. */
int mmtta_norm_bwd_finalize_sets(int kind, int groups, const float* part, int rows_per_n, int n, int c, int64_t count,
                                 const float* gamma, int training, float* m1, float* m2, float* dgamma,
                                 float* dbeta, int accumulate, double* scratch /* fp64 [N*C*2] */,
                                 const mmtta_norm_sets* sets, void* stream);

/* Pass 3: dy = rstd * (gamma*dz - m1 - xhat*m2); dy may alias dout. */
int mmtta_norm_bwd_apply(const mmtta_tensor* dout, const mmtta_tensor* y, const mmtta_norm_on_load* t,
                         const float* m1, const float* m2, const mmtta_tensor* dy, void* stream);

/* The three passes in ONE launch for a small tensor (the deep levels of the U-Net: launch latency was all their cost):
 * InstanceNorm statistics (the m1 / m2 of mmtta_norm_bwd_finalize with kind = MMTTA_NORM_INSTANCE and count = voxels),
 * no affine gradients, <= 4096 voxels per batch item, C a multiple of 32, voxel-dense 16-byte aligned tensors
 * (mmtta_norm_bwd_small_ok answers 1 / 0 on the host).  One workgroup per 32 channels sums dz and dz*xhat over the voxels
 * (64 partials per channel added in a fixed order in fp64) and writes dy; dy may alias dout.  Same formulas as the
 * three-pass form, another fp32 summation order of the two sums.  Measured (unet 4x128^3, four volumes in flight): +0.5 %
 * when taken for <= 512 voxels (the 8^3 levels), -1.7 % when taken up to 4096 (few workgroups, each streaming its voxels
 * twice): the host side of this repository uses it for <= 512. */
int mmtta_norm_bwd_small_ok(const mmtta_tensor* dout, const mmtta_tensor* y, const mmtta_norm_on_load* t,
                            const mmtta_tensor* dy);
int mmtta_norm_bwd_small(const mmtta_tensor* dout, const mmtta_tensor* y, const mmtta_norm_on_load* t, int64_t count,
                         const mmtta_tensor* dy, void* stream);

/* ------------------------------------------------------------------ resampling / glue ---- */
/* nn.Upsample(scale_factor=2, mode="trilinear", align_corners=True) and its adjoint
 * (reference: src/models/unet_multimodal_midfusion.py:114-120,134 via monai UpSample).  Both tensors of a call share one
 * storage type (fp32 or bf16: activations under method.storage, gradients under method.grad_storage); fp32 arithmetic. */
int mmtta_upsample2x_fwd(const mmtta_tensor* x, const mmtta_tensor* y, void* stream);
int mmtta_upsample2x_bwd(const mmtta_tensor* dy, const mmtta_tensor* dx, int accumulate, void* stream);

/* out = sum_i w[i] * in[i], i < count <= 8 (accumulate != 0: out += ...).  The M-way modality
 * means torch.stack(...).mean (reference: unet_multimodal_midfusion.py:221,229,247), the
 * f_shared + residual add (:96) and their adjoints. */
int mmtta_lincomb(int count, const mmtta_tensor* const* in, const float* w, const mmtta_tensor* out,
                  int accumulate, void* stream);

/* Which kernel of csrc/pointwise.hip an entry point would launch for these operands, and on what launch geometry (host-only:
 * launches nothing, dereferences no pointer - pointers are read for their alignment only; the entry points themselves ask the
 * same planners).  `operands` per op:
 *   CHANNEL_STATS {x}            NORM_BWD_REDUCE {dout, y}      NORM_BWD_APPLY / NORM_BWD_SMALL {dout, y, dy}
 *   COMBINE {a, out} or {a, b, out}     LINCOMB {in[0], ..., in[k-1], out}     UPSAMPLE_FWD {x, y}     UPSAMPLE_BWD {dy, dx}
 * `t` is the call's norm-on-load (COMBINE: ta, and `t2` = tb), `m1` / `m2` the coefficient vectors of NORM_BWD_APPLY; NULL
 * for the ops that take none.  Returns MMTTA_OK or the error the entry point itself would report for these operands. */
#define MMTTA_PW_OP_CHANNEL_STATS 0
#define MMTTA_PW_OP_NORM_BWD_REDUCE 1
#define MMTTA_PW_OP_NORM_BWD_APPLY 2
#define MMTTA_PW_OP_NORM_BWD_SMALL 3
#define MMTTA_PW_OP_COMBINE 4
#define MMTTA_PW_OP_LINCOMB 5
#define MMTTA_PW_OP_UPSAMPLE_FWD 6
#define MMTTA_PW_OP_UPSAMPLE_BWD 7
/* kernel families (mmtta_pointwise_route_t.family) */
#define MMTTA_PW_REDUCE 0          /* channel_reduce_kernel<mode, vec, bf16_a, bf16_b> */
#define MMTTA_PW_REDUCE_STREAM 1   /* channel_reduce_stream_kernel<mode, it, bf16_a, bf16_b> */
#define MMTTA_PW_ELEMENTWISE 2     /* elementwise_kernel<mode, vec, bf16_a, bf16_b, bf16_o> */
#define MMTTA_PW_COMBINE8 3        /* combine8_kernel<bf16_a, has_b, it> */
#define MMTTA_PW_NORM_BWD_APPLY8 4 /* norm_bwd_apply8_kernel<bf16_b, it, bf16_a> */
#define MMTTA_PW_NORM_BWD_SMALL 5  /* norm_bwd_small_kernel<bf16_b, bf16_a> */
#define MMTTA_PW_LINCOMB 6         /* lincomb_kernel<vec, count, bf16_a, bf16_o> */
#define MMTTA_PW_UPSAMPLE_FWD 7    /* upsample_fwd_kernel<vec, bf16_a> */
#define MMTTA_PW_UPSAMPLE_BWD 8    /* upsample_bwd_kernel<vec, bf16_a> */
typedef struct {
  int64_t vox_per_row;    /* reductions: voxels per partial row (the last row of an item may be shorter) */
  int64_t work_items;     /* threads' worth of work: voxels x channel vectors */
  int64_t grid_x;         /* workgroups of 256 threads */
  int32_t grid_y;
  int32_t family;         /* MMTTA_PW_* */
  int32_t mode;           /* reductions: 0 sums of x and x^2, 1 norm-backward sums; elementwise: 0 combine, 1 norm-backward apply */
  int32_t vec;            /* channels per thread: 1, 4 or 8 */
  int32_t it;             /* voxels a thread has in flight (template IT); 0: the kernel has no such parameter */
  int32_t count;          /* lincomb: number of inputs (template COUNT) */
  int32_t bf16_a;         /* storage flags of the instantiation: reductions x / y; apply, small: dout; combine: a; lincomb: inputs */
  int32_t bf16_b;         /*   reductions: dout; apply, small: y; combine: b */
  int32_t bf16_o;         /*   the tensor written */
  int32_t has_b;          /* combine: a second source */
  int32_t rows_per_n;     /* reductions: partial rows per batch item */
  int32_t rows_per_block; /* reductions: rows a workgroup walks (the last workgroup of an item may have fewer) */
  int32_t cpl, nvl;       /* channel lanes x voxel lanes of a workgroup (cpl * nvl == 256) */
  int32_t trips;          /* reductions: voxels a lane adds per row, sequentially */
  int32_t cb_passes;      /* channel_reduce_kernel: passes of the channel lanes over C */
  int32_t second_trip;    /* grid-stride kernels: the capped grid makes threads take a second element */
  int32_t leaky;          /* the LeakyReLU instantiation of the family runs */
} mmtta_pointwise_route_t;
int mmtta_pointwise_route(int op, const mmtta_tensor* const* operands, int count, const mmtta_norm_on_load* t,
                          const mmtta_norm_on_load* t2, const float* m1, const float* m2, mmtta_pointwise_route_t* out);

/* ------------------------------------------------------------------ loss ----------------- */
/* Entropy-minimisation objective and its gradient in one pass (BUILD-DEFINED: the reference
 * has no TTA loss; it takes the place of DiceCELoss in the step
 * skeleton of reference src/core/trainers/seg_trainer.py:141-142).
 *   softmax == 0: mean over (n,r,voxel) of H_bern(z) = softplus(z) - z*sigmoid(z)
 *   softmax != 0: mean over (n,voxel)   of H_cat(z)  = logsumexp_r z - sum_r p_r z_r
 *   logits, dlogits  channels-last, same shape; dlogits = dLoss/dlogits.  logits fp32; dlogits fp32, or - softmax == 0, <= 4
 *            channels in dense 4-channel voxel rows - bf16 (8-byte voxels: the thin gradients of method.grad_storage)
 *   partial  fp64 [mmtta_entropy_partials(...)] scratch; loss  fp32 [1] */
int64_t mmtta_entropy_partials(const mmtta_tensor* logits);
int mmtta_entropy_loss(const mmtta_tensor* logits, int softmax, const mmtta_tensor* dlogits,
                       double* partial, float* loss, void* stream);

/* The same objective for N INDEPENDENT volumes in one launch (a group of volumes adapting side by side, each with its
 * own parameters): loss[n] = mean over batch item n alone, dlogits of item n scaled by item n's count - exactly what N
 * calls of mmtta_entropy_loss on the N items would produce (same block partials, same order).
 *   partial  fp64 [N * mmtta_entropy_partials(one item)] scratch; loss  fp32 [N] */
int64_t mmtta_entropy_partials_items(const mmtta_tensor* logits);
int mmtta_entropy_loss_items(const mmtta_tensor* logits, int softmax, const mmtta_tensor* dlogits,
                             double* partial, float* loss, void* stream);

/* SAR's reliable-entropy objective (Niu et al., ICLR 2023) for N INDEPENDENT volumes: only the elements whose entropy lies
 * below `margin` enter the loss (elements: (voxel, region) for softmax == 0, voxel for softmax != 0; H as above).
 *   keep_out[n][voxel][c]  uint8, dense channels-last (c < R for softmax == 0, one byte per voxel otherwise):
 *                          H < margin, ANDed with keep_in when keep_in != NULL (SAR's second pass: keep1 & (H2 < margin))
 *   loss[n]   = sum_{keep} H / |keep| of item n (NaN when nothing is kept);  kept[n] = |keep| (int64)
 *   dlogits   = keep * dH/dz / |keep| (zero when nothing is kept); the scale is read on the device (capturable).
 * Three launches: a pass that writes the mask and fp64 block partials, a per-item finish, a gradient pass that reads the
 * logits and the mask again.  Storages as mmtta_entropy_loss_items (bf16 thin gradients included); with every element kept
 * the gradient is bitwise that of mmtta_entropy_loss_items.  `margin` must be finite and positive; keep_out may be keep_in.
 *   partial  fp64 [mmtta_entropy_filtered_partials(logits)] scratch */
int64_t mmtta_entropy_filtered_partials(const mmtta_tensor* logits);
int mmtta_entropy_filtered_items(const mmtta_tensor* logits, int softmax, float margin, const uint8_t* keep_in,
                                 uint8_t* keep_out, const mmtta_tensor* dlogits, double* partial, float* loss,
                                 int64_t* kept, void* stream);

/* ---- MEMO (Zhang, Levine, Finn, NeurIPS 2022) over the mirrored views of a volume.  A batch of G volumes x V views is
 * [G * V, D, H, W, C], item g * V + v = view v of volume g = the volume mirrored along the axes of mask view_axes[v]
 * (bit 0 = W, bit 1 = H, bit 2 = D; view_axes[0] must be 0: view 0 is the volume itself).  `views` is 1, 2, 4 or 8;
 * `view_axes` is a HOST array of `views` masks, read at launch.  Mirroring is exact on the voxel grid and its own inverse,
 * so every kernel below addresses a voxel of the volume's own frame and its image in each view directly.
 *
 * Bit 4 (value 16) of a code transposes H and W BEFORE the mirrors of bits 0-2; bit 4 stays unused (a code with it is
 * invalid, as before), so the valid codes are 0..7 and 16..23.  For a volume x and
 * a view y, both [D, H, W, C]:  y = flip(x.transpose(H, W) if code & 16 else x, dims of code & 7), and bringing a view back
 * to the frame is the inverse, flip then transpose (such a view is not its own inverse).  In coordinates, frame voxel
 * (d, h, w) sits at view voxel (fd(d), fh(w), fw(h)) with bit 4 and at (fd(d), fh(h), fw(w)) without, f* = the mirror of
 * that VIEW axis where its bit is set.  A quarter turn of the (H, W) plane (torch.rot90(x, k, dims = (H, W))) is code 18
 * (k = 1), 3 (k = 2) or 17 (k = 3).  A code with bit 4 needs h == w on every tensor of the call (MMTTA_ERR_INVALID, the
 * message names both extents).  A call in which no code has bit 4 launches the mirror group's kernels with their
 * arguments, bit for bit; with one, mmtta_memo_loss_items (sigmoid head, <= 4 regions in dense 16-byte rows) and
 * mmtta_memo_ensemble (sigmoid head, dense 16-byte rows, `out` owning its pad lanes, which then take 0) run tiled kernels
 * that load a transposed view along the view's W and turn the tile through LDS; every other path (generic Bernoulli,
 * categorical, generic ensemble, mmtta_mirror_views, mmtta_augment_views) follows the coordinate map alone and is
 * uncoalesced for transposed views.  mmtta_memo_partials is one formula for both.
 *
 * mmtta_mirror_views: y[g * V + v] = x[g] under view v's code (transposed where bit 4 is set, then mirrored).  x [G, D, H, W, C] and y [G * V, D, H, W, C]
 *   channels-last with dense rows of one width, fp32 or bf16 (the 8-byte voxel rows of the network input included); a
 *   voxel's whole row moves intact, pad lanes included (y must own them).  Bit-exact.
 *
 * mmtta_memo_loss_items: every volume g is its own objective (as in mmtta_entropy_loss_items).  With u_v = view v's logits
 *   brought back to the volume's frame:
 *     softmax == 0:  pbar = 1/V sum_v sigmoid(u_v);   loss[g] = mean over (voxel, region) of H_bern(pbar)
 *     softmax != 0:  pbar = 1/V sum_v softmax_r(u_v); loss[g] = mean over voxel of -sum_r pbar_r log pbar_r
 *   dlogits of view v = dloss[g]/dlogits, written in view v's own frame (u_v = view v's logits flipped, then - bit 4 -
 *   transposed).  With transposed views the fast path gives, for equal frame-aligned rows, the gradient bits of the
 *   mirror kernel.  One streaming pass (a thread owns a voxel of
 *   the volume's frame, reads its V rows and writes its V gradient rows) and the per-volume finish.  Loss and gradient
 *   are finite for every finite fp32 logit: 1 - pbar is never formed by subtraction and x log x is taken at
 *   max(x, smallest normal) (softmax != 0: log pbar is a log-sum-exp over the views' log-softmaxes).  Storages as mmtta_entropy_loss_items: fp32 logits; fp32 gradients, or - softmax == 0, <= 4
 *   channels in dense 4-channel voxel rows - bf16.  G volumes in one call are bit for bit G calls on one volume each.
 *   views == 1 (nothing to mirror, the marginal is the one prediction) IS mmtta_entropy_loss_items: the same kernels, the
 *   same bits, and mmtta_memo_partials(logits, 1) == mmtta_entropy_partials_items(logits).
 *   partial  fp64 [mmtta_memo_partials(logits, views)] scratch; loss  fp32 [G]
 *
 * mmtta_memo_ensemble: out [G, D, H, W, C] fp32 = logit(pbar) (softmax == 0; +-87.3365 = -ln(smallest normal) where pbar
 *   or 1 - pbar underflows; views == 1 returns the logits) or log pbar (softmax != 0), in the volume's frame (every view
 *   brought back by its inverse: flip, then - bit 4 - transpose).
 *
 * Bad arguments (null pointers, views outside {1, 2, 4, 8}, N no multiple of views, a code outside 0..7 and 16..23, a code with bit
 * 4 on tensors with h != w, shape mismatches) are MMTTA_ERR_INVALID, storages without a kernel (and more than 65535 volumes in one call) MMTTA_ERR_UNSUPPORTED, both before
 * anything is launched. */
int mmtta_mirror_views(const mmtta_tensor* x, const mmtta_tensor* y, int views, const int32_t* view_axes, void* stream);
int64_t mmtta_memo_partials(const mmtta_tensor* logits, int views);
int mmtta_memo_loss_items(const mmtta_tensor* logits, int softmax, int views, const int32_t* view_axes,
                          const mmtta_tensor* dlogits, double* partial, float* loss, void* stream);
int mmtta_memo_ensemble(const mmtta_tensor* logits, int softmax, int views, const int32_t* view_axes,
                        const mmtta_tensor* out, void* stream);

/* ---- CoTTA (Wang et al., CVPR 2022): the student's consistency loss against the teacher's soft target, and the pass after
 * the student's optimizer step (teacher EMA + stochastic restore).
 *
 * mmtta_consistency_loss_items: every batch item is its own objective (as in mmtta_entropy_loss_items).  `logits` z and
 *   `target` t are [N, D, H, W, C] fp32 in one frame; t is what mmtta_memo_ensemble writes - logit(pbar) (softmax == 0) or
 *   log pbar (softmax != 0) - and takes no gradient:
 *     softmax == 0:  q = sigmoid(t);  loss[n] = mean over (voxel, region) of -q log sigmoid(z) - (1 - q) log sigmoid(-z)
 *                    dlogits = (sigmoid(z) - q) / count
 *     softmax != 0:  loss[n] = mean over voxel of -sum_r exp(t_r) log softmax(z)_r;  dlogits = (softmax(z) - exp(t)) / count
 *   One streaming pass and the per-item finish (fixed-order fp64 sums, no atomics).  Loss and gradient are finite for every
 *   finite fp32 input: log sigmoid(z) = min(z, 0) - log1p(exp(-|z|)), 1 - q is never formed by subtraction, and both
 *   sigmoids are taken at the logit held inside +-87.3365 (the ensemble's bound; t_r is held at -3e38 from below) by the
 *   same instructions, so target == logits gives a gradient of exactly zero - as does, for the softmax head, the target
 *   mmtta_memo_ensemble makes from the same logits with one view.  Storages as mmtta_entropy_loss_items: fp32 gradients, or
 *   - softmax == 0, <= 4 channels, all three tensors in dense 4-channel voxel rows - bf16 (the fp32 value rounded).  N
 *   items in one call are bit for bit N calls on one item each.
 *   partial  fp64 [mmtta_consistency_partials(logits)] scratch; loss  fp32 [N]
 *
 * mmtta_cotta_update_sets: ONE pass over the first n elements of each of `sets` parameter sets (set s of w at
 *   s * w_stride, of teacher at s * teacher_stride; `source` [n] is shared):
 *     teacher <- a teacher + b w      a = (float)alpha, b = (float)(1 - alpha) (the difference taken in double), fp32
 *                                     products and sum with separate roundings; alpha == 1 leaves the teacher's bits
 *     w_i <- source_i where u_i < restore_p (the source BITS), else unchanged
 *   u_i = (word >> 8) * 2^-24, compared in fp32, where word is number i & 3 of the four outputs of Philox4x32-10 (Salmon
 *   et al., SC 2011; Random123's and curand's generator, written out in the kernel) with key (seed & 0xffffffff, seed >> 32)
 *   and counter (i >> 2, *step, ordinals[s], 0).  `step` is the arena's DEVICE step counter, read after the optimizer
 *   advanced it (1 for the first step), so a replayed graph draws fresh numbers; `ordinals` is a DEVICE int32 [sets] array
 *   with one number per volume (not the set index: a group of volumes then equals the same volumes one at a time).
 *   restored[s] (int64) = the number of restored elements of set s, summed from int64 block partials in a fixed order.
 *   12 B read and 8 B written per parameter.  n need not be a multiple of 4; strides are, buffers are 16-byte aligned.
 *   partial  int64 [mmtta_cotta_update_partials(n, sets)] scratch
 *
 * Bad arguments (null pointers, shape mismatches, alpha outside [0, 1], restore_p outside [0, 1), bad strides) are
 * MMTTA_ERR_INVALID, storages without a kernel MMTTA_ERR_UNSUPPORTED, both before anything is launched. */
int64_t mmtta_consistency_partials(const mmtta_tensor* logits);
int mmtta_consistency_loss_items(const mmtta_tensor* logits, const mmtta_tensor* target, int softmax,
                                 const mmtta_tensor* dlogits, double* partial, float* loss, void* stream);
int64_t mmtta_cotta_update_partials(int64_t n, int sets);
int mmtta_cotta_update_sets(float* w, float* teacher, const float* source, int64_t n, int sets, int64_t w_stride,
                            int64_t teacher_stride, double alpha, float restore_p, uint64_t seed, const int32_t* step,
                            const int32_t* ordinals, int64_t* partial, int64_t* restored, void* stream);

/* ---- Affine (rotate / scale / shift) teacher views of CoTTA and PETAL - csrc/affine.hip.  The views of a volume are
 * `first` coded views (mmtta_memo_ensemble's mirror / turn codes, view 0 = the volume itself) followed by `count` affine
 * views, views = first + count, 2 <= views <= 8, first >= 1, count >= 1; item g * views + v of a batch is view v of volume
 * g.  The teacher's predictions take no gradient, so both directions are gathers: no adjoint, no scatter, no atomics.
 *
 * A matrix is 12 fp32 numbers, row-major 3 x 4.  For the voxel (d, h, w) a thread owns, the sampled coordinate of axis k is
 *     p_k = fmaf(m[4k], d, fmaf(m[4k + 1], h, fmaf(m[4k + 2], w, m[4k + 3])))          (fp32, this order)
 * and "trilinear", for both entry points, is: with f = floor(p_k), t = p_k - f per axis, corner f weighs 1 - t and corner
 * f + 1 weighs t; the value is the sum over the 8 corners f + {0, 1}^3 that lie INSIDE the tensor of (w_d * w_h) * w_w times
 * the corner's value, accumulated with fmaf in the order 000, 001, .. 111 of (d, h, w); corners outside contribute 0 (and
 * every corner does once an axis has p_k outside (-1, extent) or not finite); a corner of weight 0 is not read.  Up to
 * rounding this is torch.nn.functional.grid_sample(mode = "bilinear", padding_mode = "zeros", align_corners = True) on
 * 5-D input.  The coordinates are VOXEL coordinates: a rotation does not account for anisotropic spacing.
 *
 * mmtta_affine_views: x [G, D, H, W, C], y [G * views, D, H, W, C], channels-last dense rows of one width, both fp32 or both
 *   bf16 (the 8-byte bf16 voxel rows of the network input included).  `matrices` is DEVICE fp32 [G, count, 12], matrix
 *   (g, j) maps a voxel of view first + j to the coordinate of x[g] it samples; `matrices_host` is its HOST copy, read at
 *   launch for the argument checks.  Writes items g * views + first + j, j < count, as the trilinear resample of x[g]; the
 *   other items of y are not touched.  A thread owns one output voxel row (rows wider than 4 lanes: a quad of it; rows no
 *   16- / 8-byte access fits: a lane): 8 row gathers, fp32 arithmetic, one store; the pad lanes (y must own them) take 0;
 *   bf16 output is the fp32 result rounded to nearest even.  An identity matrix reproduces x by value, an integer
 *   translation is the exact shift with zero fill.
 *
 * mmtta_affine_ensemble: logits [G * views, D, H, W, R] fp32, every view in its own frame; out [G, D, H, W, R] fp32 in the
 *   volume's frame.  `view_axes` is a HOST array of `views` codes: views < first carry mirror / turn codes with
 *   mmtta_memo_ensemble's meaning (view_axes[0] == 0) and are read through the exact coordinate map, views >= first must
 *   carry 0.  `inv` is DEVICE fp32 [G, count, 12], matrix (g, j) maps a voxel of the volume's frame to the coordinate of
 *   view first + j that shows it (the inverse of mmtta_affine_views' matrix); `inv_host` is its HOST copy.  Probabilities are
 *   interpolated, not logits; tri() is the trilinear value above:
 *     softmax == 0:  P = sum_coded sigmoid(u_v) + sum_affine tri(sigmoid(z_v)),  Q = the same sums of sigmoid(-.),
 *                    out = log P - log Q held inside +-87.3365; 1 - p is never formed by subtraction, and the common
 *                    denominator (first + the coverages) cancels
 *     softmax != 0:  P_r = the same sums of the softmax rows,  Wt = first + sum_affine (sum of the inside corners' weights),
 *                    out_r = log(P_r / Wt), held at -3e38 from below
 *   A frame voxel whose image falls outside an affine view is predicted by the remaining views alone (view 0 always
 *   covers).  Paths: R <= 4 in dense 16-byte rows with `out` owning its pad lanes (they take 0; a thread owns a voxel), any
 *   R and strides (sigmoid head; a thread owns a (voxel, region) pair), up to 16 classes (softmax head).  G volumes in one
 *   call are bit for bit G calls on one volume each.
 *
 * Bad arguments (null pointers, views outside 2 .. 8, count < 1, first < 1, first + count != views, N no multiple of views,
 * a code != 0 on an affine view or an invalid code on a coded one, a code with bit 4 at h != w, an extent < 2, a
 * non-finite matrix entry, shape mismatches) are MMTTA_ERR_INVALID, storages without a kernel (an item of 2^31 elements or
 * more, more than 65535 items along the grid) MMTTA_ERR_UNSUPPORTED, both before anything is launched. */
int mmtta_affine_views(const mmtta_tensor* x, const mmtta_tensor* y, int views, int first, int count,
                       const float* matrices_host, const float* matrices, void* stream);
int mmtta_affine_ensemble(const mmtta_tensor* logits, int softmax, int views, const int32_t* view_axes, int first, int count,
                          const float* inv_host, const float* inv, const mmtta_tensor* out, void* stream);

/* ---- PETAL (Brahma & Rai, CVPR 2023): the restore of CoTTA's pass above, ranked by the step's own gradient - csrc/petal.hip.
 * The magnitude key of a gradient element is key(g) = bits(g) & 0x7fffffff, an unsigned integer: a total order over zeros
 * (+0 == -0), denormals, infinities and NaNs (above the infinities) that no float comparison mode changes.
 *
 * The segment table: a DEVICE int64 array of [count][3] rows (start, length, rank), relative to a parameter set, followed by
 *   [count + 1] running chunk counts (entry r = the sum of mmtta_magnitude_select_chunks(length) over the rows before r).  Rows
 *   are ascending and disjoint; start is a multiple of 4, length >= 1 is anything, 0 <= rank < length.  `table_host` is the
 *   HOST copy of the same array, read at launch for the argument checks.
 *
 * mmtta_magnitude_select_sets: gamma_out[s][r] (uint32 [sets][count]) = the rank-th smallest key (0-based, an element's own
 *   bits) among g[s * set_stride + start .. + length) of row r.  A radix select over the 31 key bits in digits of 11 / 10 /
 *   10 bits.  Rows of class 0 (mmtta_magnitude_select_class(length) == 0) are selected by one workgroup with their keys in
 *   LDS; rows of class 1 are cut into chunks, one workgroup each: per digit an LDS histogram, its non-empty bins added to
 *   the row's global table with integer atomics, and a launch that picks the bin and clears the table.  One launch for a
 *   table without class-1 rows, seven otherwise - whatever the data and `sets`; no host read-back; integer sums only, so the
 *   result does not depend on scheduling.  scratch: mmtta_magnitude_select_scratch_bytes(count, sets) bytes, contents
 *   arbitrary (prepared by the first launch).
 *
 * mmtta_petal_update_sets: ONE pass over the first n elements of each of `sets` parameter sets:
 *     teacher <- a teacher + b w      exactly mmtta_cotta_update_sets' arithmetic (alpha == 1 leaves the teacher's bits)
 *     w_i <- source_i (the source BITS) where i lies in a row r and key(g_i) < gamma[s][r]; else unchanged
 *   Elements whose key equals the threshold stay, so a row with an all-zero gradient restores nothing; elements of no row
 *   (alignment padding) are never restored.  restored[s] (int64) = the number of restored elements of set s, summed from
 *   int64 block partials in a fixed order.  16-byte accesses, the last elements of a ragged n one by one; a workgroup finds
 *   the rows of its elements by two searches of the table and keeps them in LDS.
 *   partial  int64 [mmtta_petal_update_partials(n, sets)] scratch
 *
 * Bad arguments (null pointers, sets < 1, strides that are no multiples of 4 or below n - for the select: below the end of the
 * last row -, rows out of order, overlapping or behind n, a start that is no multiple of 4, length < 1, rank outside [0, length),
 * chunk counts that do not match the rows, alpha outside [0, 1]) are MMTTA_ERR_INVALID; more than 2^20 rows, 65535 sets, a row
 * of 2^31 elements or more and misaligned buffers MMTTA_ERR_UNSUPPORTED; both before anything is launched.  Sets beyond
 * `sets` and elements beyond n are not written. */
int mmtta_magnitude_select_class(int64_t length);          /* 0: one workgroup, 1: chunked; -1: length < 1 */
int64_t mmtta_magnitude_select_chunks(int64_t length);     /* chunks of a row (0 for class 0) */
int64_t mmtta_magnitude_select_scratch_bytes(int count, int sets);
int mmtta_magnitude_select_sets(const float* g, const int64_t* table, const int64_t* table_host, int count, int sets,
                                int64_t set_stride, uint32_t* gamma_out, void* scratch, void* stream);
int64_t mmtta_petal_update_partials(int64_t n, int sets);
int mmtta_petal_update_sets(float* w, float* teacher, const float* source, const float* g, const uint32_t* gamma,
                            const int64_t* table, const int64_t* table_host, int count, int64_t n, int sets,
                            int64_t w_stride, int64_t teacher_stride, int64_t g_stride, double alpha, int64_t* partial,
                            int64_t* restored, void* stream);

/* ---- Intensity-augmented views of the staged input - csrc/augment.hip.  The views of MEMO and CoTTA above, each with a
 * pointwise intensity transform on top of its mirror: a batch of G volumes x V views is [G * V, D, H, W, C] as for
 * mmtta_mirror_views (`views`, `view_axes` and their rules are that entry point's; masks may repeat and may all be 0).
 * Both entry points take channels-last tensors of <= 4 channels in dense 4-channel voxel rows, fp32 (16-byte rows) or bf16
 * (the 8-byte voxel rows of the network input), base pointers aligned to a row.
 *
 * mmtta_intensity_range: range[g][c] = (min, max) of channel c over the voxels of volume g, fp32 [G][C][2] on the device,
 *   exact; the pad lanes of the rows never enter.  Block partials and a fixed per-volume finish, no atomics.
 *   partial  fp32 [mmtta_intensity_range_partials(x)] scratch, 16-byte aligned
 *
 * mmtta_augment_views: y[g * V + v] = x[g] under view v's code (mmtta_mirror_views' codes, bit 4 = H and W transposed
 *   first, h == w, included) and transformed, in one pass: a thread owns a voxel
 *   row of the volume's frame, loads it once and stores it V times (W rows apart for a transposed view: uncoalesced).  `table` is a DEVICE array fp32 [G * V][C][4], 16-byte
 *   aligned, with the row (g, a, b, sigma) of every (volume, view, channel); `table_host` is the HOST copy of the same
 *   array, read at launch for the one check that needs its values: the rows of view 0 must be the identity (1, 1, 0, 0).
 *   `range` is what mmtta_intensity_range wrote for x, `ordinals` a DEVICE int32 [G] array with one number per volume (as
 *   in mmtta_cotta_update_sets: the number, not the batch slot, enters the draw, so G volumes in one call are bit for bit G
 *   calls on one volume each).  On a value x of channel c, with (lo, hi) = range[g][c], in this order, every operation in
 *   fp32 and rounded on its own (no fused multiply-add):
 *     g != 1:     x <- ((x - lo) / (hi - lo))^g * (hi - lo) + lo     (the power as exp2(g * log2(t)), t = 0 gives 0)
 *                 x <- x * a;  x <- x + b
 *     sigma > 0:  x <- x + sigma * n
 *   and a bf16 row takes the result rounded to nearest even once.  n is the standard normal of (voxel, channel, view,
 *   volume): Philox4x32-10 (as in mmtta_cotta_update_sets) with key (seed & 0xffffffff, seed >> 32) at the counter
 *   (i, (q << 8) | v, ordinals[g], 1), i = the voxel's linear index in the volume's own (unmirrored, unturned) frame, q = c / 4 (0
 *   here); words (0, 1) give R = sqrt(-2 ln(((w0 >> 8) + 1) 2^-24)), theta = 2 pi (w1 >> 8) 2^-24 and channel 4q takes
 *   R cos theta, channel 4q + 1 R sin theta; words (2, 3) give channels 4q + 2 and 4q + 3 the same way.  A channel whose row
 *   is the identity, a channel with hi == lo, every channel of view 0 and the pad lanes move their BITS (y must own its pad
 *   lanes); a call whose table is all identity is mmtta_mirror_views bit for bit.
 *
 * Bad arguments (null pointers, views outside {1, 2, 4, 8}, N no multiple of views, a code outside 0..7 and 16..23 or with bit 4 on
 * h != w, shape mismatches, a view 0 row that is not the identity) are MMTTA_ERR_INVALID, layouts without a kernel (and more than 65535 volumes in one call)
 * MMTTA_ERR_UNSUPPORTED, both before anything is launched. */
int64_t mmtta_intensity_range_partials(const mmtta_tensor* x);
int mmtta_intensity_range(const mmtta_tensor* x, float* partial, float* range, void* stream);
int mmtta_augment_views(const mmtta_tensor* x, const mmtta_tensor* y, int views, const int32_t* view_axes,
                        const float* table_host, const float* table, const float* range, uint64_t seed,
                        const int32_t* ordinals, void* stream);

/* ------------------------------------------------------------------ EATA ----------------- */
/* EATA (Niu et al., ICML 2022) - csrc/eata.hip.
 *
 * mmtta_entropy_weighted_items: the weighted reliable entropy of N independent items.  Elements, margin, mask layout, partial
 *   layout, storages (fp32 logits; fp32 or - on the <= 4-region fast path - bf16 thin gradients) and the three launches are
 *   those of mmtta_entropy_filtered_items without `keep_in`; the entropy arithmetic is that entry point's, so keep_out and
 *   kept equal its results bit for bit.  Per item, with c = exp(margin - H) (a constant of the gradient, 1 < c <= e^margin):
 *     keep = H < margin;  loss = sum_keep c H / |keep|;  dlogits = keep * c * dH/dz / |keep|
 *   An empty filter gives loss NaN, kept 0 and a zero gradient.  N items in one call equal N calls bit for bit.
 *   Softmax head: `keep` is decided with the filtered entry point's H = lse(z) - sum p z (hence the equal masks), while c,
 *   the loss and the gradient use H in the shifted form log sum exp(z - max) - sum p (z - max), which does not carry the
 *   largest logit's rounding.  The two differ at fp32 rounding level; an element they put on different sides of the margin
 *   is kept with c = 1 (c is held to exp(margin - min(H, margin))), so there 1 <= c.
 *     partial  fp64 [mmtta_entropy_weighted_partials(logits)] scratch
 *
 * mmtta_pseudo_label_loss_items: the loss the Fisher estimate differentiates, per item, one pass + finish, the storages of
 *   mmtta_consistency_loss_items.  Sigmoid head: y = 1[z >= 0], loss = mean over (voxel, region) of BCE(z, y) =
 *   log1p(exp(-|z|)), dlogits = (sigmoid(z) - y) / count.  Softmax head: y = one-hot of the first arg max, loss = mean over
 *   voxels of lse(z) - max z, dlogits = (softmax(z) - y) / count.
 *     partial  fp64 [mmtta_pseudo_label_partials(logits)] scratch
 *
 * mmtta_fisher_accumulate_sets: F_i <- F_i + g_{s,i}^2 for s = 0 .. sets-1 in that order over [0, n) of `grads` (set s starts
 *   at s * set_stride); fp32, the product and the sum rounded separately.  mmtta_fisher_scale: F_i <- F_i / count (IEEE fp32
 *   division; count >= 1), the end of an estimate.  n need not be a multiple of 4; set_stride is, buffers are 16-byte aligned.
 *
 * mmtta_fisher_penalty_sets: over [0, n) of the first `sets` of `replicas` arena replicas ([replica][set_stride]), with the
 *   shared `fisher` and `source` spans ([n]):
 *     g += 2 lambda F (w - source);  penalty[s] = lambda sum_i F_i (w_i - source_i)^2
 *   fp32 elementwise arithmetic with separate roundings, fp64 block partials summed per set in a fixed order.  16 B read and
 *   4 B written per parameter and set.  n and set_stride multiples of 4, n <= set_stride, 1 <= sets <= replicas, lambda
 *   finite and >= 0, buffers 16-byte aligned.
 *     partial  fp64 [mmtta_fisher_penalty_partials(n, sets)] scratch;  penalty  fp32 [sets]
 *
 * Bad arguments (null pointers, shape mismatches, a margin that is not finite and positive, a bad lambda, count or stride)
 * are MMTTA_ERR_INVALID, storages without a kernel MMTTA_ERR_UNSUPPORTED, both before anything is launched. */
int64_t mmtta_entropy_weighted_partials(const mmtta_tensor* logits);
int mmtta_entropy_weighted_items(const mmtta_tensor* logits, int softmax, float margin, uint8_t* keep_out,
                                 const mmtta_tensor* dlogits, double* partial, float* loss, int64_t* kept, void* stream);
int64_t mmtta_pseudo_label_partials(const mmtta_tensor* logits);
int mmtta_pseudo_label_loss_items(const mmtta_tensor* logits, int softmax, const mmtta_tensor* dlogits, double* partial,
                                  float* loss, void* stream);
int mmtta_fisher_accumulate_sets(float* fisher, const float* grads, int64_t n, int sets, int64_t set_stride, void* stream);
int mmtta_fisher_scale(float* fisher, int64_t n, float count, void* stream);
int64_t mmtta_fisher_penalty_partials(int64_t n, int sets);
int mmtta_fisher_penalty_sets(const float* w, float* g, const float* fisher, const float* source, int64_t n, int sets,
                              int replicas, int64_t set_stride, float lambda, double* partial, float* penalty, void* stream);

/* ------------------------------------------------------------------ DeYO ----------------- */
/* DeYO (Lee et al., ICLR 2024, "Entropy is not Enough for Test-Time Adaptation") - csrc/deyo.hip.
 *
 * The patch grid of both entry points: grid[3] = (gd, gh, gw) patches per axis, every count >= 1 and a divisor of its extent,
 *   2 <= P = gd gh gw <= 4096; slot j (row-major over the grid) covers the voxels j (+) o, o the offset inside the patch.
 *   `table` is device int32 [N][2][P]: row 0 of batch item n is its permutation `perm` (slot j of the shuffled volume holds
 *   patch perm[j]), row 1 the inverse (the content of patch s went to slot inv[s]).  The kernels clamp every entry they read
 *   to [0, P): whatever the table holds, no access leaves the item (the result is then unspecified).
 *
 * mmtta_patch_shuffle: y[n, j (+) o] = x[n, perm_n[j] (+) o].  Channels-last [N,D,H,W,C] of equal shape, row width and
 *   storage (fp32 or bf16); whole voxel rows are copied, pad lanes included, bit-exact - the contract of mmtta_mirror_views,
 *   so `y` must own the pad lanes of its rows.  `x` and `y` may not overlap (an in-place call is MMTTA_ERR_INVALID).  A
 *   gather of contiguous runs of W / gw voxel rows with 16 / 8-byte accesses, one launch, no LDS.
 *
 * mmtta_deyo_loss_items: the reliable entropy of N independent items, filtered and weighted by the pseudo-label probability
 *   difference between `logits` (z) and `logits_shuffled` (z', the logits of the shuffled volume).  Elements, margins (nats),
 *   mask layout, launch geometry, storages (fp32 logits; fp32 or - on the <= 4-region fast path - bf16 thin gradients) and the
 *   three launches are those of mmtta_entropy_weighted_items; the entropy arithmetic is that entry point's, so kept_entropy
 *   equals the `kept` of mmtta_entropy_filtered_items at `margin` bit for bit.  z''(v) = z' at the voxel where the content of
 *   v went, read from `logits_shuffled` through row 1 of the table (one more voxel row per voxel; no un-shuffled copy is
 *   written).  Per element, with y^ the hard prediction of z (sigmoid head: 1[z >= 0]; softmax head: the first arg max):
 *     PLPD  = p(z)[y^] - p(z'')[y^]         (sigmoid head: sigmoid(|z|) - sigmoid(s z''), s = +1 where z >= 0, else -1)
 *     keep1 = H < margin;  keep = keep1 and PLPD > plpd_threshold
 *     a     = exp(margin0 - H) + exp(PLPD)  (a constant of the gradient)
 *   and per item  kept_entropy = |keep1|;  kept = |keep|;  loss = sum_keep a H / kept;  dlogits = keep * a * dH/dz / kept.
 *   Nothing kept gives loss NaN, kept 0 and a zero gradient.  N items in one call equal N calls bit for bit.
 *     keep_out  uint8, one byte per element (N*D*H*W*R, softmax head N*D*H*W): keep
 *     partial   fp64 [mmtta_deyo_partials(logits)] scratch (block partials of the sum and of the two counts)
 *     loss      fp32 [N];  kept, kept_entropy  int64 [N]
 *
 * Bad arguments (null pointers, shape or storage mismatches between x and y, a grid that does not divide the extents, P < 2,
 * P > 4096, a margin that is not finite and positive, a threshold that is not finite with -1 <= threshold < 1) are
 * MMTTA_ERR_INVALID, storages without a kernel MMTTA_ERR_UNSUPPORTED, both before anything is launched. */
int mmtta_patch_shuffle(const mmtta_tensor* x, const mmtta_tensor* y, const int32_t* grid, const int32_t* table, void* stream);
int64_t mmtta_deyo_partials(const mmtta_tensor* logits);
int mmtta_deyo_loss_items(const mmtta_tensor* logits, const mmtta_tensor* logits_shuffled, const int32_t* grid,
                          const int32_t* table, int softmax, float margin, float margin0, float plpd_threshold,
                          uint8_t* keep_out, const mmtta_tensor* dlogits, double* partial, float* loss, int64_t* kept,
                          int64_t* kept_entropy, void* stream);

/* ------------------------------------------------------------------ LAME ----------------- */
/* LAME (Boudiaf et al., CVPR 2022, "Parameter-free Online Test-time Adaptation") - csrc/lame.hip.  The weights stay as they
 * are; the OUTPUTS are corrected: posteriors that stay close to the model's own (a KL term) while spatial neighbours with
 * similar inputs agree (a Laplacian term).  The paper's concave-convex iteration z_i <- q_i (.) exp(weight sum_j w_ij z_j),
 * renormalised, runs in logit space (elements as everywhere: sigmoid head (voxel, region) pairs, softmax head voxels):
 *     sigmoid head   l_i(t+1)   = l0_i   + weight * sum_j w_ij tanh(l_j(t) / 2)          every region on its own
 *     softmax head   l_ik(t+1)  = l0_ik  + weight * sum_j w_ij softmax(l_j(t))_k         no re-centring
 *   l(0) = l0 = `logits0`; `iterations` synchronous (Jacobi) iterations, ping-pong between `work` and `out`, one launch each
 *   (+ one memset node that clears `flipped`), all queued on `stream` without synchronisation.  The result is in `out`
 *   whatever the parity of `iterations`; `logits0` is never written; the three buffers are pairwise distinct.
 *   j: the 6 / 18 / 26 (`connectivity`) spatial neighbours of voxel i inside the same batch item; a neighbour outside the
 *   volume contributes nothing.  w_ij = a_ij / n with n = connectivity (a constant: w stays symmetric and sum_j w_ij <= 1, so
 *   `weight` is the largest logit shift of one iteration).
 *   a_ij = exp(-sum_{c present} (x_ic - x_jc)^2 / (2 sigma^2)) on the staged input `x` [N,D,H,W,C] (fp32 or bf16 as staged,
 *   converted to fp32; differences and sum in fp32); bit c of `channel_mask` marks channel c present.  sigma == 0: a_ij = 1,
 *   `x` is not read (it may be null) and the mask is ignored.
 *   flipped int64 [N]: per item the elements whose hard prediction changed - sigmoid head 1[l(T) >= 0] != 1[l0 >= 0],
 *   softmax head a different FIRST arg max.  Integer block sums and one atomic per workgroup: the same in every run.
 *   N items in one call equal N calls bit for bit.
 * `logits0`, `work`, `out`: channels-last fp32 [N,D,H,W,R] of one shape and row width.  Two routes:
 *   tiled    R <= 4, C <= 4, dense 16-byte logit rows (and dense 4-element rows of `x`): a workgroup stages a 4 x 8 x 32 tile
 *            of y = tanh(l / 2) (or the softmax row) and of x with a one-voxel halo in LDS and computes the affinities on the
 *            fly.  Rows of `out` / `work` are one 16-byte store - pad lanes written as 0 - when R == 4 or the view is
 *            MMTTA_TENSOR_OWNS_PAD; else R 4-byte stores, pad lanes left as they are.
 *   generic  everything else up to R <= 16 and C <= 16: one thread per voxel from global memory; pad lanes left as they are.
 * MMTTA_ERR_INVALID before anything is launched: null pointers, shape or row-width mismatches, aliased buffers, a
 * connectivity other than 6 / 18 / 26, iterations outside 1 .. 64, a weight that is not finite and in (0, 16], a sigma that
 * is negative or not finite, sigma > 0 with no bit of channel_mask among the C channels.  R > 16 or C > 16, storages without
 * a kernel and items of 2^31 elements or more are MMTTA_ERR_UNSUPPORTED. */
int mmtta_lame_refine(const mmtta_tensor* logits0, const mmtta_tensor* x, uint32_t channel_mask, int softmax, int connectivity,
                      float weight, float sigma, int iterations, const mmtta_tensor* work, const mmtta_tensor* out,
                      int64_t* flipped, void* stream);

/* ------------------------------------------------------------------ do-no-harm guard ------ */
/* An output-level check of one adapted volume against the prediction the same method gives before its first step -
 * csrc/guard.hip.  Where the adapted hard prediction has collapsed or exploded relative to that reference, the reference
 * logits are put back.  The hard prediction is the evaluator's (mmtta_mask_dice_counts), per channel on either head:
 * 1 / (1 + expf(-z)) >= threshold in fp32; a NaN logit is background.
 *
 * mmtta_guard_counts: counts int64 [N][R][3] = (s, a, i) = |reference mask|, |adapted mask|, |both| per (item, region),
 *   zeroed by the call (one memset node) and filled by ONE streaming pass that reads both tensors once (32 B per voxel on
 *   the dense route).  A wave reduces each bit by ballot and population count; a workgroup adds its sums with one integer
 *   atomic per count.  Integer sums: the same in every run, and N items in one call equal N calls.
 * mmtta_guard_select: every workgroup reads its item's 3 R counts and evaluates the rule itself (no decision launch, no
 *   host read); the first workgroup of an item writes fallback int32 [N][R] (1: the region's logits are the reference's).
 *   With Q = 2^16, A = min_agreement_q16, G = max_growth_q16, H = max_shrink_q16, m = min_voxels, region (n, r) FAILS iff
 *       A > 0 and max(s, a) >= max(m, 1) and 2 i Q < A (s + a)        the Dice of the two masks is below A / Q
 *    or G > 0 and a Q > G max(s, m)                                    the region grew more than G / Q times
 *    or H > 0 and s Q > H max(a, m)                                    the region shrank more than H / Q times
 *   in unsigned 64-bit arithmetic (no overflow for items below 2^31 voxels); equality passes in every clause; A = G = H = 0
 *   never fails.  MMTTA_GUARD_SCOPE_VOLUME: an item with a failing region has every channel returned (all its flags are 1);
 *   MMTTA_GUARD_SCOPE_REGION: the failing channels only.  The workgroups of a passing item exit at once: its `logits`,
 *   pad lanes included, are not touched.  `counts` need not come from mmtta_guard_counts.
 * `reference`, `adapted` / `logits`: channels-last fp32 [N,D,H,W,R] of one shape and row width.  Two routes, as
 * mmtta_lame_refine's: dense 16-byte rows for R <= 4 (one 16-byte load per voxel and tensor; under the volume scope a failing
 * row is one 16-byte store when R == 4 or `logits` is MMTTA_TENSOR_OWNS_PAD - its pad lanes then take the reference's -
 * else the failing channels are 4-byte stores and pad lanes stay as they are), and one thread per voxel on any
 * channels-last rows up to R <= 16 (pad lanes stay as they are).  Vector stores only, no float atomics, no scratch.
 * MMTTA_ERR_INVALID before anything is launched: null pointers, shape or row-width mismatches between the two tensors,
 * `reference` aliased by `logits`, a threshold that is not finite and in (0, 1), min_agreement_q16 > Q, max_growth_q16 /
 * max_shrink_q16 neither 0 nor in [Q, 1024 Q], min_voxels < 0, an unknown scope.  R > 16, storages or strides without a
 * kernel (bf16, channel stride != 1), more than 65535 items and items of 2^31 voxels or more are MMTTA_ERR_UNSUPPORTED. */
#define MMTTA_GUARD_SCOPE_VOLUME 0
#define MMTTA_GUARD_SCOPE_REGION 1
typedef struct mmtta_guard_rule {
  uint32_t min_agreement_q16; /* A: 0 (off) .. 65536 */
  uint32_t max_growth_q16;    /* G: 0 (off) or 65536 .. 1024 * 65536 */
  uint32_t max_shrink_q16;    /* H: likewise */
  int32_t min_voxels;         /* m: 0 .. 2^31 - 1 */
  int32_t scope;              /* MMTTA_GUARD_SCOPE_* */
  int32_t reserved;           /* 0 */
} mmtta_guard_rule;
int mmtta_guard_counts(const mmtta_tensor* reference, const mmtta_tensor* adapted, float threshold, int64_t* counts,
                       void* stream);
int mmtta_guard_select(const int64_t* counts, const mmtta_guard_rule* rule, const mmtta_tensor* reference,
                       const mmtta_tensor* logits, int32_t* fallback, void* stream);

/* ------------------------------------------------------------------ CRF-regularised entropy */
/* The entropy objective plus a pairwise grid-CRF (Potts) regulariser, loss and gradient in one pass - csrc/crf.hip (Tang et
 * al., ECCV 2018, "On Regularized Losses for Weakly-supervised CNN Segmentation"; the contour term of Hu et al., MICCAI
 * 2021, "Fully Test-time Adaptation for Image Segmentation").  Where mmtta_lame_refine corrects the outputs, this term sits
 * inside the step, so the weights learn the spatial prior.  Every batch item is its own objective (elements as everywhere:
 * sigmoid head (voxel, region) pairs, softmax head voxels; E = D H W R or D H W of ONE item, n = `connectivity`):
 *     L = H + weight * P                              H: the mean entropy of mmtta_entropy_loss_items
 *     P = 1 / (2 n E) * sum_i sum_{j in N(i)} a_ij phi(p_i, p_j)         (ordered pairs, hence the 1 / 2)
 *     phi   form 0, Potts:      sigmoid head  sum_r [p_ir (1 - p_jr) + (1 - p_ir) p_jr];  softmax head  1 - sum_k p_ik p_jk
 *           form 1, quadratic:  sum_r (p_ir - p_jr)^2  on both heads
 *     p = sigmoid(l) per region (softmax == 0) or softmax(l) per voxel (softmax != 0)
 *   N(i): the 6 / 18 / 26 spatial neighbours of voxel i inside the same batch item; a neighbour outside the volume
 *   contributes nothing.  a_ij = exp(-sum_{c present} (x_ic - x_jc)^2 / (2 sigma^2)) on the staged input `x` [N,D,H,W,C]
 *   (fp32 or bf16 as staged, converted to fp32; differences and sum in fp32); bit c of `channel_mask` marks channel c
 *   present.  sigma == 0: a_ij = 1, `x` is not read (it may be null) and the mask is ignored.
 *   dlogits = dH/dl + weight * dP/dl, a gather (no scatter, no floating-point atomics): with g = dP/dp,
 *     Potts      sigmoid head  g_ir = 1 / (n E) sum_j a_ij (1 - 2 p_jr);   softmax head  g_ik = 1 / (n E) sum_j a_ij (-p_jk)
 *     quadratic  g_ik = 1 / (n E) sum_j a_ij 2 (p_ik - p_jk)
 *     sigmoid head  dP/dl_ir = g_ir p_ir (1 - p_ir);   softmax head  dP/dl_ik = p_ik (g_ik - sum_m p_im g_im)
 *   loss[n] = L, entropy[n] = H, pairwise[n] = P of item n (fp32 [N] each), from fp64 block partials summed in a fixed
 *   order: two runs give the same bits, and N items in one call equal N calls bit for bit.
 *   partial  fp64 [mmtta_crf_partials(logits)] scratch.
 * Two launches - the main pass and a per-item finish - queued on `stream` without synchronisation or host read (capturable).
 * `logits` channels-last fp32 [N,D,H,W,R], never written; `dlogits` of the same shape and row width.  Two routes:
 *   tiled    R <= 4, C <= 4, dense 16-byte logit rows, dense 4-element rows of `dlogits` and of `x`: a workgroup stages a
 *            4 x 8 x 32 tile of p and of x with a one-voxel halo in LDS and computes the affinities on the fly.  `dlogits`
 *            fp32, or - sigmoid head - bf16 (8-byte voxels: the thin gradients of method.grad_storage).  A row of `dlogits`
 *            is one 16- / 8-byte store - pad lanes written as 0 - when R == 4 or the view is MMTTA_TENSOR_OWNS_PAD; else R
 *            element stores, pad lanes left as they are.
 *   generic  everything else up to R <= 16 and C <= 16: one thread per voxel from global memory, fp32 `dlogits`, pad lanes
 *            left as they are.
 * MMTTA_ERR_INVALID before anything is launched: null pointers, a shape or row-width mismatch between `logits` and
 * `dlogits`, `x` of another spatial shape, a connectivity other than 6 / 18 / 26, a form other than 0 / 1, a weight that is
 * not finite and in (0, 16], a sigma that is negative, not finite or so small that 1 / (2 sigma^2) overflows fp32 (below about
 * 4.6e-20), sigma > 0 with no bit of channel_mask among the C channels, `dlogits` aliasing `logits` or `x`.  R > 16 or C > 16, storages without a kernel (logits that are not fp32, a
 * bf16 `dlogits` off the sigmoid head's tiled route, views that are not channels-last), items of 2^31 elements or more and
 * more than 65535 items (gridDim.y carries the item) are MMTTA_ERR_UNSUPPORTED. */
int64_t mmtta_crf_partials(const mmtta_tensor* logits);
int mmtta_crf_entropy_items(const mmtta_tensor* logits, const mmtta_tensor* x, uint32_t channel_mask, int softmax,
                            int connectivity, int form, float weight, float sigma, const mmtta_tensor* dlogits,
                            double* partial, float* loss, float* entropy, float* pairwise, void* stream);

/* ------------------------------------------------------------------ entropy minus a regional nuclear norm */
/* Batch nuclear-norm maximisation over a grid of boxes - csrc/nuclear.hip (Cui et al., CVPR 2020, "Towards Discriminability
 * and Diversity: Batch Nuclear-norm Maximization"; the regional nuclear-norm term of Hu et al., MICCAI 2021, "Fully Test-time
 * Adaptation for Image Segmentation").  Entropy minimisation is content when the minority class collapses; the nuclear norm
 * of the prediction matrix rewards confidence AND every class staying alive.  Every batch item is its own objective:
 *     L = entropy_weight * H - weight * N              H: the mean entropy of mmtta_entropy_loss_items (E elements)
 *     N = 1 / Q * sum_A nu(A),     nu(A) = sum_k sqrt(lambda_k + eps m) / sqrt(m min(m, K))
 *   The volume is cut into boxes of [bd, bh, bw] voxels that start at multiples of the box size (an entry of 0, or one >= the
 *   extent: the whole extent; border boxes are smaller, nothing is padded).  A box of m voxels gives
 *     softmax head  one m x K matrix A with the rows p_i = softmax(l_i), K = R;
 *     sigmoid head  per region r one m x 2 matrix with the rows (p_ir, 1 - p_ir), p = sigmoid(l);
 *   Q is the number of matrices of the item, lambda_k >= 0 the eigenvalues of G = A^T A (clamped at 0).  With eps -> 0, nu is
 *   ||A||_* / sqrt(m min(m, K)) in (0, 1]; the smoothing keeps it differentiable at rank-deficient boxes.
 *   dN/dA = A M / Q, M = c V diag(1 / sqrt(lambda_k + eps m)) V^T, c = 1 / sqrt(m min(m, K));  with g_i = (A M)_i / Q
 *     softmax head  dN/dl_ik = p_ik (g_ik - sum_j p_ij g_ij);
 *     sigmoid head  dN/dl_ir = [(A M)_i0 - (A M)_i1] / Q * p_ir (1 - p_ir);
 *   dlogits = entropy_weight * dH/dl - weight * dN/dl.
 *   loss[n] = L, entropy[n] = H, nuclear[n] = N of item n (fp32 [N] each).
 *   scratch  fp64 [mmtta_nuclear_scratch(logits, softmax, bd, bh, bw)] (-1 on bad arguments).
 * Four launches whatever the data and the box - the Gram pass (fp64 partials of the boxes' Gram entries and entropy, one
 * read of the logits), the spectrum pass (per matrix: the partials summed in a fixed order, the eigenproblem in fp64 - closed
 * form for 2 x 2, cyclic Jacobi up to 16 x 16 -, nu and the coefficients of M), the gradient pass (a second read of the
 * logits) and a per-item finish - queued on `stream` without synchronisation or host read (capturable).  No floating-point
 * atomics and no scatter: two runs give the same bits, N items in one call equal N calls bit for bit, and a box's gradient
 * depends on its own voxels only.  `logits` channels-last fp32 [N,D,H,W,R], never written; `dlogits` of the same shape and
 * row width.  Two routes:
 *   fast     R <= 4, dense 16-byte logit rows, dense 4-lane rows of `dlogits` - fp32, or bf16 on the sigmoid head (8-byte
 *            voxels: the thin gradients of method.grad_storage).  A row of `dlogits` is one store, pad lanes written 0, when
 *            R == 4 or the view is MMTTA_TENSOR_OWNS_PAD; else R element stores, pad lanes left as they are.
 *   generic  everything else up to R <= 16: fp32 `dlogits`, pad lanes left as they are.
 * MMTTA_ERR_INVALID before anything is launched: null pointers, a shape or row-width mismatch, `dlogits` aliasing `logits`
 * (equal or overlapping), a negative block entry, a weight not finite or outside (0, 16], an entropy_weight not finite or
 * outside [0, 16], an eps not finite or outside [1e-6, 0.1].  MMTTA_ERR_UNSUPPORTED: R > 16, logits that are not fp32, a bf16
 * `dlogits` off the sigmoid head's fast route, views that are not channels-last, items of 2^31 elements or more, more than
 * 65535 items (gridDim.y carries the item), a scratch of 2^31 fp64 elements or more. */
int64_t mmtta_nuclear_scratch(const mmtta_tensor* logits, int softmax, int bd, int bh, int bw);
int mmtta_nuclear_entropy_items(const mmtta_tensor* logits, int softmax, int bd, int bh, int bw, float entropy_weight,
                                float weight, float eps, const mmtta_tensor* dlogits, double* scratch, float* loss,
                                float* entropy, float* nuclear, void* stream);

/* ------------------------------------------------------------------ input normaliser */
/* A per-volume intensity map in front of the network that adapts while the network may stay frozen - csrc/input_norm.hip
 * (Karani et al., MedIA 2021, "Test-time adaptable neural networks for robust medical image segmentation").  Volume n and
 * channel c carry theta[n][c] = (s, b, g, 0), fp32 [N][C][4] on the device:
 *     u  = x                                                  gamma == 0
 *     u  = ((x - lo) / (hi - lo))^exp(g) (hi - lo) + lo       gamma != 0 (the power as mmtta_augment_views computes it)
 *     x' = exp(s) u + b                                       (product and sum rounded on their own)
 *   `range` is what mmtta_intensity_range wrote for the raw volume ([N][C][2]: lo, hi); a channel with hi == lo has u = x.
 *   Bit c of `keep_mask` says channel c is present: an absent channel is left alone and has no gradient.
 * mmtta_input_norm_apply: y = x' in one streaming pass.  `x` the raw staged volume, fp32 channels-last rows of 4 lanes
 *   (<= 4 channels), never written; `y` of the same shape, fp32 or bf16 rows of 4 lanes, owning its pad lanes.  16-byte loads;
 *   16-byte stores (bf16: one per pair of voxels, an unpaired voxel at either end of an item takes 8 bytes).  A channel
 *   whose theta row is all zero, an absent channel and the pad lanes pass through: the same bits in fp32, one rounding in bf16.
 * mmtta_input_norm_grad: the reduced input gradient of the network's first level,
 *     grad[n][c] = (dL/ds, dL/db, dL/dg, 0) = sum_v dX'[n,c,v] * dx'/dtheta (x[n,c,v]),     fp32 [N][C][4]
 *     dX'[n,c,i] = keep_c * sum_branches sum_o sum_taps W_r[o,c,t] * dy_r[n,o,(i + 1 - t) / 2]
 *   over the one or two convolutions that read the input (`branches`: k = 3, stride 2, pad 1, C -> c0 with c0 a multiple of 4
 *   up to 64; anything else is MMTTA_ERR_UNSUPPORTED).  dy_r is the gradient of branch r's output as the backward left it -
 *   channels-last [N, ceil(D/2), ceil(H/2), ceil(W/2), c0], fp32 or bf16 (both branches alike), possibly a channel slice of a
 *   wider tensor -, W_r the fp32 weights in torch layout [c0, C, 3, 3, 3]; item n reads the set `set_stride` * n elements
 *   behind `weight` (0: one set).  dX never reaches memory: a workgroup gathers it for a tile of 4 x 8 x 64 input voxels
 *   from the weights in LDS, multiplies by the derivatives and writes 12 fp64 partials; a second launch sums them in a
 *   fixed order and writes grad.  dL/dg is 0 with gamma == 0 or hi == lo; rounding x' to bf16 counts as the identity.
 *   With lr > 0 that launch also takes torch.optim.Adam's step on theta (betas 0.9 / 0.999, eps 1e-8, no decay; fp64
 *   arithmetic, fp32 state `exp_avg` / `exp_avg_sq` [N][C][4]; `step` a device int32 [N] this call advances, a volume whose
 *   step is 0 starts from zero moments) and clamps (s, b, g) to +- (bound_log_scale, bound_shift, bound_log_gamma); g moves
 *   only with gamma != 0, an absent channel not at all.  lr == 0: theta is only read, the last three pointers may be null.
 *   partial  fp64 [mmtta_input_norm_grad_partials(x)] (-1 on a null or empty tensor; host-only).
 * No floating-point atomics and no scatter: two runs give the same bits and N items in one call equal N calls bit for bit.
 * Both queue on `stream` without synchronisation or host read (capturable).  MMTTA_ERR_INVALID before anything is launched:
 * null pointers, a shape mismatch (x / y, or dy against the input's output extents), y == x, n_branches outside {1, 2},
 * branches that differ in channels or storage, a negative set stride, lr or a bound not finite or out of range.
 * MMTTA_ERR_UNSUPPORTED: more than 4 input channels, rows that are not dense 4-lane voxel rows, an x that is not fp32,
 * k != 3 or stride != 2, c0 not a multiple of 4 or above 64, misaligned buffers, items of 2^31 elements or more, more than
 * 65535 volumes. */
typedef struct mmtta_input_norm_branch {
  const mmtta_tensor* dy;
  const float* weight;
  int64_t set_stride;
  int32_t ksize, stride;
} mmtta_input_norm_branch;
int mmtta_input_norm_apply(const mmtta_tensor* x, const mmtta_tensor* y, const float* theta, const float* range,
                           uint32_t keep_mask, int gamma, void* stream);
int64_t mmtta_input_norm_grad_partials(const mmtta_tensor* x);
int mmtta_input_norm_grad(const mmtta_tensor* x, const mmtta_input_norm_branch* branches, int n_branches, float* theta,
                          const float* range, uint32_t keep_mask, int gamma, double* partial, float* grad, float* exp_avg,
                          float* exp_avg_sq, int32_t* step, double lr, double bound_log_scale, double bound_shift,
                          double bound_log_gamma, void* stream);

/* ------------------------------------------------------------------ bias field */
/* A smooth multiplicative field per volume and modality in front of the network - csrc/bias_field.hip: the receive-coil
 * intensity non-uniformity of MRI, learned in the step as the input normaliser's (s, b, g) are.  Volume n and channel c carry
 * theta[n][c][k], fp32 [N][C][20] on the device (rows of 20 whatever the order; the first K are read and written):
 *     F_c(z, y, x) = sum_k theta_ck phi_k(z, y, x)         x'_c = (x_c - a_c) exp(F_c) + a_c
 *   phi_(a,b,c) = P_a(t_z) P_b(t_y) P_c(t_x), Legendre polynomials of the voxel-centre coordinates t_i = (2 i + 1) / n - 1 (n = 1:
 *   t = 0), the terms with a + b + c <= `order` in the order (a + b + c, a, b, c) ascending: K = 1, 4, 10, 20 for order 0 .. 3.
 *   Term 0 is the constant: the global log-gain.  `tables_d`, `tables_h`, `tables_w`: fp32 [4][extent] on the device, T[a][i] =
 *   P_a(t_i) (the host evaluates them in float64 and rounds once).  a_c is the intensity the field leaves fixed: `anchor` =
 *   MMTTA_BIAS_ANCHOR_MIN the channel's minimum range[n][c][0] (`range` is what mmtta_intensity_range wrote for the raw
 *   volume), MMTTA_BIAS_ANCHOR_ZERO 0.  The arithmetic, all fp32 and nothing contracted: phi_k = (T_d[a][z] T_h[b][y]) T_w[c][x]
 *   rounded in that order; F = fmaf(theta_k, phi_k, F) from 0.f in ascending k; E = expf(F); d = x - a; v = d E; x' = v + a.
 *   Bit c of `keep_mask` says channel c is present: an absent channel is left alone and has no gradient.
 * mmtta_bias_field_apply: y = x' in one streaming pass, x and y as mmtta_input_norm_apply takes them (the raw fp32 rows of 4
 *   lanes, never written; fp32 or bf16 rows that own their pad lanes; 16-byte loads and stores, the bf16 pairs as there).  A
 *   channel whose K coefficients are all zero, an absent channel and the pad lanes pass through: the same bits in fp32, one
 *   rounding in bf16.  A workgroup holds the three tables in LDS, 16 (D + H + W) bytes.
 * mmtta_bias_field_grad: the reduced input gradient of the network's first level against the basis,
 *     grad[n][c][k] = sum_v dX'[n,c,v] (x[n,c,v] - a_c) exp(F_c(v)) phi_k(v)  +  2 l2 theta_ck (k >= 1),    fp32 [N][C][20]
 *   (the terms past K are written 0), dX' and `branches` as mmtta_input_norm_grad's - the same gather, one copy in
 *   csrc/input_gather.h -, F recomputed as the map computes it, every product in fp32 and every sum over voxels in fp64 in a
 *   fixed order: 4 K fp64 partials per tile of 4 x 8 x 64 input voxels, a second launch (one workgroup per volume) sums
 *   them.  With lr > 0 that launch also takes torch.optim.Adam's step on theta (as mmtta_input_norm_grad: betas 0.9 / 0.999,
 *   eps 1e-8, no decay, fp64 arithmetic, fp32 state `exp_avg` / `exp_avg_sq` [N][C][20], `step` a device int32 [N], zero
 *   moments at step 0) and clamps theta_c0 to +- bound_gain and theta_ck, k >= 1, to +- bound_field.  An absent channel has
 *   grad = 0 exactly and keeps its theta.  lr == 0: theta is only read, the last three pointers may be null.
 *   partial  fp64 [mmtta_bias_field_grad_partials(x, order)] = N x tiles x 4 K (-1 on a null or empty tensor or an order
 *   outside 0 .. 3; host-only).
 * No floating-point atomics and no scatter: two runs give the same bits and N items in one call equal N calls bit for bit.
 * Both queue on `stream` without synchronisation or host read (capturable).  MMTTA_ERR_INVALID before anything is launched:
 * what mmtta_input_norm_apply / _grad refuse so, a null table, a negative order, an anchor that is neither constant, l2 not
 * finite or negative.  MMTTA_ERR_UNSUPPORTED: what they refuse so, order > 3, an extent above 512 voxels (the LDS budget of
 * the tables), misaligned theta, range or tables. */
#define MMTTA_BIAS_ANCHOR_MIN 0
#define MMTTA_BIAS_ANCHOR_ZERO 1
int mmtta_bias_field_apply(const mmtta_tensor* x, const mmtta_tensor* y, const float* theta, const float* range,
                           const float* tables_d, const float* tables_h, const float* tables_w, int order, int anchor,
                           uint32_t keep_mask, void* stream);
int64_t mmtta_bias_field_grad_partials(const mmtta_tensor* x, int order);
int mmtta_bias_field_grad(const mmtta_tensor* x, const mmtta_input_norm_branch* branches, int n_branches, float* theta,
                          const float* range, const float* tables_d, const float* tables_h, const float* tables_w, int order,
                          int anchor, uint32_t keep_mask, double* partial, float* grad, float* exp_avg, float* exp_avg_sq,
                          int32_t* step, double lr, double bound_gain, double bound_field, double l2, void* stream);

/* ------------------------------------------------------------------ modality consistency */
/* The cross-modal objective of modcons_tta - csrc/modcons.hip (in the family of MM-TTA, Shin et al., CVPR 2022): the
 * prediction from all modalities should agree with the prediction from each subset of them.  A batch of G volumes x V views
 * is [G * V, D, H, W, C], item g * V + v = view v of volume g; view 0 keeps every present modality, view v >= 1 a subset.
 *
 * mmtta_modality_views: y[g * V + v] = x[g] with channel c kept iff bit c of keep_masks[v] is set (`keep_masks`: a HOST
 *   array of `views` masks, 1 <= views <= 8, read at launch; a bit outside the channels is MMTTA_ERR_INVALID).  x
 *   [G, D, H, W, C] and y [G * V, D, H, W, C] channels-last, fp32 or bf16 alike, C <= 32.  A kept value keeps its bits; a
 *   dropped channel is stored as +0, never as x * 0 - a NaN, an infinity or -0 there does not reach the view.  Dense rows of
 *   4 lanes with C <= 4 (both tensors; y owning its pad lanes or C == 4) take one 16-byte (fp32) or 8-byte (bf16) load per
 *   voxel and V stores; every other layout a per-element path.  The pad lanes that y owns are written 0.
 *
 * mmtta_modcons_loss_items: every volume g is its own objective (as in mmtta_entropy_loss_items).  Elements i are (voxel,
 *   region) pairs (softmax == 0) or voxels (softmax != 0), n of them per volume; p_v = sigmoid(z_v) resp. softmax(z_v):
 *     entropy[g]        = H_g   = 1/n sum_i H(p_0,i)
 *     view_kl[g][v - 1] = K_g,v = 1/n sum_i KL(p_0,i || p_v,i)          v = 1 .. V-1 (Bernoulli per element, categorical per voxel)
 *     consistency[g]    = C_g   = 1/(V-1) sum_v K_g,v
 *     loss[g]           = entropy_weight * H_g + weight * C_g
 *     dlogits of view v >= 1:  weight / ((V-1) n) * (p_v - p_0)
 *     dlogits of view 0:       entropy_weight / n * dH/dz_0 + (detach ? 0 : weight / ((V-1) n) * sum_v dKL(p_0 || p_v)/dz_0)
 *                              Bernoulli: dKL/dz_0 = p_0 (1 - p_0) (z_0 - z_v);  categorical: p_0,k [(log p_0,k - log p_v,k) - KL_i]
 *     disagree[g][v - 1] = #{ i : hard(z_v,i) != hard(z_0,i) },  hard = (z >= 0) resp. the first arg max
 *   The Bernoulli KL is sigmoid(a) (a - b) + softplus(b) - softplus(a) with the parts of the size of the logits cancelled
 *   exactly ([a >= 0] (a - b) + max(b, 0) - max(a, 0) is |b| where the signs differ, else 0), held at 0 from below: finite and
 *   non-negative for every pair of finite logits with a finite difference; views with equal bits give KL = 0, a gradient of 0
 *   for v >= 1 and disagree = 0 exactly.  View 0's entropy term and its gradient are the bits of mmtta_entropy_loss_items on
 *   the same path (fast, generic, categorical) - on the categorical head while the voxel's largest |logit| is below 16; from
 *   there on the shifted form log sum e - sum p (z - max), exact to fp32 rounding at any magnitude.
 *   One launch over loss_blocks(one item) x G workgroups of 256 threads - a thread owns a
 *   voxel (fast path, categorical) or a (voxel, region) pair (generic path) of all V views, reads every logit once and writes
 *   every gradient once - and one finish launch (one workgroup per volume).  No scatter, no floating-point atomics; the fp64
 *   block partials - rows [entropy | KL per view | disagreement per view] - are summed in a fixed order, so G volumes in one
 *   call are bit for bit G calls on one volume each.  Storages as mmtta_entropy_loss_items: fp32 logits; fp32 gradients, or -
 *   softmax == 0, <= 4 channels in dense 4-channel voxel rows that own their pad - bf16; softmax != 0: up to 16 classes.
 *   partial  fp64 [mmtta_modcons_partials(logits, views)] scratch = (2 V - 1) rows x loss_blocks(one item) x G (host-only;
 *            -1 on a null tensor, views outside 2 .. 8, a batch that is no multiple of views, an empty extent)
 *   loss, entropy, consistency  fp32 [G];  view_kl  fp32 [G][V-1];  disagree  int64 [G][V-1]
 *
 * MMTTA_ERR_INVALID before anything is launched: null pointers, views outside 2 .. 8 (1 .. 8 for the views' staging), a batch
 * that is no multiple of views, shape mismatches, `dlogits` overlapping `logits` (`y` overlapping `x`), a weight that is not
 * finite or negative.  MMTTA_ERR_UNSUPPORTED: storages without a kernel (a bf16 gradient off the fast path included), items
 * of 2^31 elements or more, more than 65535 volumes. */
int mmtta_modality_views(const mmtta_tensor* x, const mmtta_tensor* y, int views, const uint32_t* keep_masks, void* stream);
int64_t mmtta_modcons_partials(const mmtta_tensor* logits, int views);
int mmtta_modcons_loss_items(const mmtta_tensor* logits, int softmax, int views, float weight, float entropy_weight, int detach,
                             const mmtta_tensor* dlogits, double* partial, float* loss, float* entropy, float* consistency,
                             float* view_kl, int64_t* disagree, void* stream);

/* ------------------------------------------------------------------ sliding windows */
/* Sliding-window adaptation and inference (window_tta) - csrc/window.hip: a volume of any extents is cut into overlapping
 * windows of the network's own extents (the roi), the network runs on every window as a batch item, and the windows meet
 * again under an importance weight.  A batch of G volumes x W_n windows is [G * W_n, rd, rh, rw, C], item g * W_n + w = window
 * w of volume g.  The grid is separable: per axis a list of `count` starts (ascending; a single negative start on an axis the
 * volume is shorter than the roi along), w = (kd * count_h + kh) * count_w + kw, origin o_w = (start_d[kd], start_h[kh],
 * start_w[kw]); W_n = count_d * count_h * count_w <= 32.
 *   origins  int32 [W_n][3], on the device (a replayed graph reads the current volume's) - and for the crop also on the host
 *   tables   device fp32: A_d [count_d][rd] | A_h [count_h][rh] | A_w [count_w][rw] in one buffer, A_axis[k][i] = the importance
 *            weight of index i of a window divided by the sum of the weights of all windows over position start_k + i - and 0
 *            where that position lies outside the volume.  The weight of window w at its voxel (i, j, k) is
 *            a = (A_d[kd][i] * A_h[kh][j]) * A_w[kw][k], rounded in fp32 in that order by every kernel.  The host builds the
 *            tables (multimodal_tta_amd/window.py); nothing here checks that they sum to 1.
 *
 * mmtta_window_views: y[g * W_n + w] = x[g] cropped at o_w, x [G, D, H, W, C] and y [G * W_n, rd, rh, rw, C] channels-last,
 *   fp32 or bf16 alike.  A kept value keeps its bits (NaN payloads, infinities, -0); a voxel outside the volume takes
 *   `pad_value` (rounded to nearest even for bf16 rows) in the C channels; the pad lanes that y owns take +0.  Dense rows of
 *   4 lanes with C <= 4 (both tensors; y owning its pad lanes or C == 4) take one 16-byte (fp32) or 8-byte (bf16) load and
 *   store per voxel; every other layout a per-element path.  Every origin must leave its window a voxel of the volume
 *   (-r < o < extent per axis, checked on `origins_host`): the kernels bound every read by the volume's extents.
 *
 * mmtta_window_entropy_items: every volume g is its own objective,
 *     loss[g]  = 1/(N R) sum_w sum_voxels a_w H_bern(sigmoid z_w)       (softmax != 0: 1/N and the categorical entropy)
 *     dlogits  = a_w H'(z_w) / (N R)                                     whole rows stored, +0 where a_w == 0
 *   N = D H W of the volume in `windows` - every voxel of the volume counts once, shared among the windows that see it; the
 *   voxels outside it count 0.  This is mmtta_entropy_loss_items' walk (voxel_loss.h: fast, any-stride and categorical paths)
 *   with the window's three table rows in LDS; a launch over loss_blocks(one item) x items workgroups and a finish launch that
 *   sums the fp64 block partials of a volume's W_n items in ascending order.  The Bernoulli heads use the entropy objective's
 *   own per-logit arithmetic; the categorical head its shifted form log sum e - sum p (z - max), exact to fp32 rounding at any
 *   magnitude (the plain form lse - sum p z carries the rounding of lse times the mean logit: 2e-5 of the largest gradient of
 *   two classes at |z| = 10).  With extents equal to the roi (one window, a == 1 by construction) the call IS
 *   mmtta_entropy_loss_items, bit for bit, and the tables are not read.  No atomics: G volumes in one call are bit for bit G
 *   calls on one volume each.  Storages as mmtta_entropy_loss_items; roi <= 512 per axis.
 *   partial  fp64 [mmtta_window_partials(logits)] scratch = loss_blocks(one item) x items (host-only; -1 on a null tensor or
 *            an empty extent);  loss  fp32 [G]
 *
 * mmtta_window_blend: out[g](v) = sum_w a_w(v) z_w(v - o_w) over the windows that cover voxel v of the volume, a gather: a
 *   thread owns an output voxel, finds per axis the starts that cover it and accumulates fma(a_w, z_w, acc) from +0 in
 *   ascending window order, in fp32.  logits [G * W_n, rd, rh, rw, R] and out [G, D, H, W, R] fp32 channels-last; R <= 4 in
 *   dense 16-byte rows (out owning its pad, which takes +0, or R == 4) takes 16-byte accesses, every other layout a
 *   per-element path.  Where one window covers a voxel and a == 1 the result is that window's logit bit for bit (a logit
 *   of -0 comes back as +0: the sum starts from +0).
 *
 * MMTTA_ERR_INVALID before anything is launched: null pointers, a count outside 1 .. 32, more than 32 windows, a batch that
 * is no multiple of W_n, extents that are not the volume tensor's, an origin that misses the volume, overlapping tensors.
 * MMTTA_ERR_UNSUPPORTED: storages without a kernel, items of 2^31 elements or more, volumes of 2^29 voxels or more. */
typedef struct mmtta_window_grid {
  int32_t extent[3]; /* the volume's D, H, W */
  int32_t count[3];  /* starts per axis */
} mmtta_window_grid;
int mmtta_window_views(const mmtta_tensor* x, const mmtta_tensor* y, const mmtta_window_grid* windows,
                       const int32_t* origins_host, const int32_t* origins, float pad_value, void* stream);
int64_t mmtta_window_partials(const mmtta_tensor* logits);
int mmtta_window_entropy_items(const mmtta_tensor* logits, int softmax, const mmtta_window_grid* windows, const float* tables,
                               const mmtta_tensor* dlogits, double* partial, float* loss, void* stream);
int mmtta_window_blend(const mmtta_tensor* logits, const mmtta_tensor* out, const mmtta_window_grid* windows,
                       const int32_t* origins, const float* tables, void* stream);

/* ------------------------------------------------------------------ optimizer ------------ */
/* torch.optim.Adam (amsgrad=False, coupled L2) over a flat parameter arena, two segments:
 * [0, n_decay) with weight_decay, [n_decay, n) without - the decay / no-decay groups of
 * reference src/core/experiment_manager.py:199-237; hyper-parameters
 * configs/training/default.yaml:30-39.  `step` is a device int32 incremented by this call
 * (t starts at 1), so a captured graph replays correctly.  The call that finds *step == 0 starts from ZERO moments whatever
 * m / v hold (torch creates the state as zeros) and does not read them: resetting the optimizer is `*step = 0`, no buffer
 * needs clearing.  SURVEY.md Appendix E K8. */
int mmtta_adam_step(float* p, const float* g, float* m, float* v, int64_t n, int64_t n_decay, float lr,
                    float beta1, float beta2, float eps, float weight_decay, int32_t* step, void* stream);

/* The three optimizers the reference's factory can build (reference src/core/experiment_manager.py:199-210:
 * torch.optim.SGD / Adam / AdamW, chosen by `training.optimizer`, hyper-parameters from
 * `training.optimizers.<name>`, configs/training/default.yaml:11-45) over the same arena layout:
 *   ADAM   as mmtta_adam_step;
 *   ADAMW  p *= 1 - lr*weight_decay (decay segment), then the Adam update without the L2 term;
 *   SGD    g += weight_decay*p (decay segment); buf = g on the first step, momentum*buf + (1-dampening)*g after;
 *          g = nesterov ? g + momentum*buf : buf (momentum 0: plain);  p -= lr*g.   `m` is the momentum buffer,
 *          `v` is unused (may be NULL).  With momentum 0 torch keeps no buffer: `m` is neither read nor written (it must
 *          still be a valid, aligned pointer).
 * All buffers 16-byte aligned, n_decay a multiple of 4 (the arena guarantees both). */
enum { MMTTA_OPTIM_ADAM = 0, MMTTA_OPTIM_ADAMW = 1, MMTTA_OPTIM_SGD = 2 };
typedef struct mmtta_optim_desc {
  int32_t kind;
  float lr, beta1, beta2, eps, weight_decay;
  float momentum, dampening;
  int32_t nesterov;
} mmtta_optim_desc;
int mmtta_optim_step(const mmtta_optim_desc* desc, float* p, const float* g, float* m, float* v, int64_t n,
                     int64_t n_decay, int32_t* step, void* stream);

/* mmtta_optim_step over `sets` replicas of the arena in one launch (a group of volumes, each adapting its own copy):
 * replica r occupies [r * set_stride, r * set_stride + n) of p / g / m / v, its first n_decay elements decay.  One shared
 * step counter, advanced once.  set_stride a multiple of 4. */
int mmtta_optim_step_sets(const mmtta_optim_desc* desc, float* p, const float* g, float* m, float* v, int64_t n,
                          int64_t n_decay, int sets, int64_t set_stride, int32_t* step, void* stream);

/* Weight gradient, optimizer step and repack of a 27-tap layer in one pass (per parameter set).  The weight-gradient
 * kernel writes its slabs as mmtta_conv_wgrad_sets does; the reduction of the slabs then feeds the optimizer of the layer's
 * weight (and bias) directly and writes the new weights into both bf16 packed images - bit for bit what
 * mmtta_conv_wgrad_sets + mmtta_optim_step_sets + mmtta_conv_pack_batched give.  The step counter is read, not advanced.
 * Layers whose gradient does not end in the 27-tap reduction, and non-bf16 images, are MMTTA_ERR_UNSUPPORTED.
 * Switched off (MMTTA_ERR_UNSUPPORTED) by MMTTA_FUSED_UPDATE=0 in the environment; mmtta_fused_update_enabled says which. */
typedef struct mmtta_update_target {
  mmtta_optim_desc optim;
  float* w_p; float* w_m; float* w_v;  /* weight, its moments: set 0, set strides of mmtta_param_sets.weight_* */
  float* b_p; float* b_m; float* b_v;  /* bias and its moments (Conv3d only; NULL: no bias, or not updated here) */
  float* b_grad;                       /* ConvTranspose3d: its bias gradient lands here, for the arena optimizer */
  void* image[2];                      /* forward and input-gradient images of set 0 (image[1] may be NULL) */
  int64_t image_outer[2], image_inner[2]; /* BYTES between the images of sets, as mmtta_param_sets.packed_* */
  const int32_t* step;                 /* device step counter (read) */
  int32_t w_decay, b_decay;            /* the parameter group decays (weight_decay applies) */
} mmtta_update_target;
int mmtta_fused_update_enabled(void);
int mmtta_conv_wgrad_update_sets(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                                 const mmtta_tensor* dy, const mmtta_update_target* target, void* workspace,
                                 int64_t workspace_bytes, const mmtta_param_sets* sets, void* stream);
/* Whether mmtta_conv_wgrad_update_sets would step the optimizer in the epilogue of this call's weight-gradient kernel
 * (MMTTA_OPT_WGRAD_EPILOGUE_UPDATE): 1 / 0, or a negative mmtta error code.  Host-only, a field of the plan the launcher
 * itself reads; planned with a target it also needs p / m / v of every set on 16 bytes, which a query cannot see. */
int mmtta_conv_wgrad_updates_in_epilogue(const mmtta_conv_desc* desc, const mmtta_tensor* x, const mmtta_norm_on_load* x_norm,
                                         const mmtta_tensor* dy, const mmtta_param_sets* sets);

/* mmtta_optim_step_sets over a table of segments of every replica (the parameters a fused weight-gradient update does not
 * cover).  `segments` is a DEVICE int64 table: `count` rows (start, length, decay) relative to a replica, start and length
 * multiples of 4, followed by the `count` running starts of the rows (0, length0, length0 + length1, ...).  `total` = sum
 * of the lengths.  Same arithmetic as mmtta_optim_step_sets; the shared step counter is advanced once, after the launch. */
int mmtta_optim_step_segments(const mmtta_optim_desc* desc, float* p, const float* g, float* m, float* v, const int64_t* segments,
                              int count, int64_t total, int sets, int64_t set_stride, int32_t* step, void* stream);

/* The ascent of a sharpness-aware step (SAM, as SAR uses it) over the first `sets` of `replicas` arena replicas
 * ([replica][set_stride]): per replica r, over [0, n),
 *   saved = p;  p += g * (rho / (||g||_2 + 1e-12))
 * with ||g||_2 from a deterministic two-stage fp64 sum of g^2 and fp32 scale / product / sum as torch computes them.
 * Replica r of `saved` starts at r * saved_stride (saved_stride >= n: [sets][n] holds only what the ascent rewrites).
 * Restoring the weights is a plain copy of `saved` back.  n, set_stride and saved_stride multiples of 4, n <= set_stride,
 * 1 <= sets <= replicas, rho finite and >= 0, buffers 16-byte aligned.
 *   partial  fp64 [mmtta_sam_ascent_partials(n, sets)] scratch */
int64_t mmtta_sam_ascent_partials(int64_t n, int sets);
int mmtta_sam_ascent_sets(float* p, const float* g, float* saved, int64_t saved_stride, double* partial, int64_t n, int sets,
                          int replicas, int64_t set_stride, float rho, void* stream);

/* ------------------------------------------------------------------ evaluation tail ------ */
/* sigmoid -> (>= threshold) -> uint8 mask; GT (> 0.5); per (n,r) integer counts
 * inter = sum p&g, psum = sum p, gsum = sum g.  Replaces reference
 * src/evaluation/seg_eval.py:304-306 and the three reductions of :55-60.
 *   logits  fp32, any strides;  label  any strides, fp32 {0,1};
 *   counts  int64 [N][R][3], zeroed by this call;  mask  uint8 NCDHW [N,R,D,H,W] or NULL */
int mmtta_mask_dice_counts(const mmtta_tensor* logits, const mmtta_tensor* label, float threshold,
                           int64_t* counts, uint8_t* mask, void* stream);

/* Sums behind monai DiceCELoss as the reference builds it - evaluator: sigmoid=True, hard-coded, for
 * ``evaluation.loss.report_loss`` (reference src/evaluation/seg_eval.py:209-220,395-400; SURVEY.md
 * Appendix A.5).  out fp64 [N][R*3+1] (block partials go through `scratch`, mmtta_dice_ce_scratch_bytes; they are
 * summed in a fixed order: reproducible): per region (sum p*y, sum p, sum y) with
 * p = sigmoid(z) (squares of p, y when squared_pred), then the CE numerator: BCE-with-logits with
 * pos_weight = weight[0] when R == 1, soft-label softmax cross entropy with class weights otherwise.
 * The few scalar operations that turn the sums into the loss value are host arithmetic. */
int64_t mmtta_dice_ce_scratch_bytes(const mmtta_tensor* logits);
/* softmax != 0 (a `training.criterion.softmax: true` head, reference src/core/trainers/seg_trainer.py:41-54): the Dice
 * probabilities are softmax over the channels instead of per-channel sigmoids (R > 1; the CE term is softmax CE either way). */
int mmtta_dice_ce_sums(const mmtta_tensor* logits, const mmtta_tensor* label, const float* weight,
                       int squared_pred, int softmax, double* out, void* scratch, void* stream);

/* d(lambda_dice * Dice + lambda_ce * CE)/d(logits) of the same loss (reduction mean), from the sums above (left
 * on the device): the supervised step of reference src/core/trainers/seg_trainer.py:141-142 without autograd.
 * Class weights scale the Dice terms only when more than one Dice channel exists (monai); include_background == 0
 * drops channel 0 from the Dice mean when R > 1. */
int mmtta_dice_ce_grad(const mmtta_tensor* logits, const mmtta_tensor* label, const float* weight, int squared_pred,
                       int softmax, int jaccard, int include_background, float lambda_dice, float lambda_ce, float smooth_nr,
                       float smooth_dr, const double* sums, const mmtta_tensor* dlogits, void* stream);

/* Calibration of the evaluation tail: a reliability histogram with Brier and NLL sums per (volume, region), from the
 * logits and the label in one pass.
 *   logits  fp32, any strides (the channels-last view of <= 4 channels in 16-byte voxel rows is read 16 bytes wide; its
 *           pad lanes are never used);  label  fp32, any strides, ground truth = label > 0.5;  bins in [1, 64]
 *   out     fp64 [N][Rout][3 * bins + 2], written whole by the call: per bin (element count, sum of confidence,
 *           correct count), then the Brier sum, then the NLL sum.  Counts are exact integers.
 * softmax == 0 (R <= 256, Rout = R): every (voxel, region) is a Bernoulli element.  prediction = z >= 0, confidence
 *   c = 1 / (1 + exp(-|z|)), correct = (prediction == ground truth), Brier term (sigmoid(z) - y)^2, NLL term
 *   max(z, 0) - z y + log1p(exp(-|z|)).
 * softmax != 0 (2 <= R <= 16, Rout = 1; more classes: MMTTA_ERR_UNSUPPORTED): every voxel is one element.  prediction =
 *   argmax z, label class = argmax of the label channels (lowest index on ties, both), c = 1 / sum_k exp(z_k - z_max),
 *   Brier term sum_k (p_k - y_k)^2 with y the one-hot label class, NLL term log-sum-exp(z) - z_label.
 * Bins are the intervals (k/B, (k+1)/B]: index min(B - 1, max(0, (int)ceilf(c * B) - 1)) in fp32.
 * scope 0: every element.  scope 1 ("union"): only elements whose prediction or ground truth is foreground (sigmoid head:
 *   of the pair's own region; softmax head: predicted or labelled class != 0).
 * Everything is summed as integers (confidence in units of 2^-28, exact; Brier terms of 2^-30; NLL terms of 2^-24, one
 * term saturating at 255 nats), so the table does not depend on scheduling: two calls agree bit for bit, and a batch
 * gives the tables of its items computed alone.  At most 2^31 - 1 voxels per volume and 65535 volumes per call.
 * mmtta_calibration_scratch_bytes: 0 (this build needs none; `scratch` may be NULL then), -1 on bad arguments. */
int64_t mmtta_calibration_scratch_bytes(const mmtta_tensor* logits, int bins);
int mmtta_calibration_bins(const mmtta_tensor* logits, const mmtta_tensor* label, int softmax, int bins, int scope,
                           double* out, void* scratch, void* stream);

/* Connected-component filtering of the evaluation tail: 3-D labelling of every (volume, region) mask, then a size
 * filter, an optional keep-the-largest filter and the Dice counts of what is left.  Replaces a host
 * `scipy.ndimage.label` (with `generate_binary_structure(3, 1 | 2 | 3)`) over a mask copied off the device, the usual
 * post-processing of BraTS / HECKTOR pipelines; the reference evaluator has no counterpart.
 *   mask_in, mask_out  uint8 [N,R,D,H,W] dense (the `mask` output of mmtta_mask_dice_counts; non-zero = foreground);
 *                      may be the same buffer.  mask_out holds 0 / 1.
 *   label        fp32 any strides, ground truth = label > 0.5, or NULL (then `counts` must be NULL)
 *   connectivity 6, 18 or 26
 *   min_voxels   HOST int64 [R], read before return: components of fewer voxels are removed (0 and 1 remove nothing)
 *   keep_largest HOST int32 [R], read before return: non-zero keeps only the largest component of the region
 *   counts       int64 [N][R][3] on the device or NULL: inter, psum, gsum of the FILTERED mask against the label, as
 *                mmtta_mask_dice_counts defines them; zeroed by this call
 *   stats        int64 [N][R][3] on the device or NULL: components of the raw mask, components kept, voxels removed
 *   labels       int32 [N,R,D,H,W] dense on the device or NULL: labels of the RAW mask
 *   scratch      mmtta_components_scratch_bytes(N*R, D, H, W) bytes (negative: unsupported extent)
 * Label convention: a component's label is 1 + the smallest linear index (z*H*W + y*W + x) of its voxels inside its own
 * (n, r) volume; 0 is background.  Order: the size filter first, then `keep_largest` among the survivors; equal sizes
 * go to the smaller label; when nothing survives `min_voxels` the region comes back empty and `kept` is 0.
 * A fixed sequence of launches on `stream` that depends on the shape alone: no host read, no convergence flag.  All sums
 * are integers: two calls agree bit for bit and a batch gives what its items give alone.
 * Limits: every extent >= 1 (no multiple of anything), D*H*W <= 2^31 - 2, R <= 64, N*R <= 65535, and fewer than 2^32 - 256 voxels per
 * call with every mask rounded up to a multiple of 256 (a larger batch is split by the caller).  Anything else is refused with MMTTA_ERR_INVALID / _UNSUPPORTED before anything is queued. */
int64_t mmtta_components_scratch_bytes(int64_t n_masks, int64_t d, int64_t h, int64_t w);
int mmtta_components_filter(const uint8_t* mask_in, uint8_t* mask_out, const mmtta_tensor* label, int n, int r, int d, int h,
                            int w, int connectivity, const int64_t* min_voxels, const int32_t* keep_largest, int64_t* counts,
                            int64_t* stats, int32_t* labels, void* scratch, void* stream);

/* Lesion-wise scores of the evaluation tail, after the BraTS-2023 lesion-wise evaluation: every ground-truth lesion is
 * scored on its own, every unmatched predicted component counts against the volume.  Replaces a host
 * `scipy.ndimage.binary_dilation` and two `scipy.ndimage.label` per (volume, region) over masks copied off the device.
 * Per (n, r), with P = mask != 0 and G = label > 0.5:
 *   Gd        G dilated `iterations` (0 ... 8) times with the 6 / 18 / 26 neighbourhood (`dilation_connectivity`), voxels
 *             outside the volume are background: scipy's binary_dilation(G, generate_binary_structure(3, 1 | 2 | 3), iterations)
 *   lesions   the 26-connected components of Gd; lesion g's own voxels are G within component g; g is KEPT iff it has at
 *             least min_lesion_voxels[r] own voxels
 *   matching  a 26-connected component of P is matched to lesion g iff one of its voxels lies in component g of Gd (it may
 *             match several lesions and counts for each; lesions that are not kept still match)
 *   Dice      P_g = union of the whole components matched to g, inter = |P_g & own_g|, den = |P_g| + |own_g|;
 *             q_g = (2 inter 2^30 + den / 2) / den in unsigned 64-bit integer division, 0 for an unmatched lesion
 *   mask      uint8 [N,R,D,H,W] dense, not written;  label  fp32, any strides
 *   min_lesion_voxels  HOST int64 [R], read before return
 *   stats     int64 [N][R][7] on the device, zeroed by this call: lesions, lesions kept, kept lesions with a match,
 *             predicted components, matched components, sum of q_g over the kept lesions, voxels of unmatched components
 *   labels    int32 [N,R,D,H,W] dense on the device or NULL: on the voxels of G the lesion's label (1 + the smallest linear
 *             index of its Gd component, the convention of mmtta_components_filter), 0 elsewhere
 *   scratch   mmtta_lesionwise_scratch_bytes(N*R, D, H, W) bytes (negative: unsupported extent)
 * A fixed sequence of launches on `stream` that depends on the shape alone: no host read, no convergence flag.  Everything
 * is an integer: two calls agree bit for bit and a batch gives what its items give alone.  Limits: those of
 * mmtta_components_filter.  Anything else is refused with MMTTA_ERR_INVALID / _UNSUPPORTED before anything is queued. */
int64_t mmtta_lesionwise_scratch_bytes(int64_t n_masks, int64_t d, int64_t h, int64_t w);
int mmtta_lesionwise_scores(const uint8_t* mask, const mmtta_tensor* label, int n, int r, int d, int h, int w, int iterations,
                            int dilation_connectivity, const int64_t* min_lesion_voxels, int64_t* stats, int32_t* labels,
                            void* scratch, void* stream);

/* Lesion-wise HD95 of the evaluation tail, the other half of the BraTS-2023 lesion-wise score.  Runs right behind
 * mmtta_lesionwise_scores and only reads what that call left in its scratch: nothing is labelled twice.  Lesions, own
 * voxels, kept / found and matching are exactly those of mmtta_lesionwise_scores.  For every lesion g that is kept and has
 * a match, with A_g = its own voxels and P_g = the union of the whole predicted components matched to it:
 *   edge(X)   X & ~erode6(X), outside the volume counts as background (the edges of mmtta_surface_distances)
 *   d(X->Y)   for every voxel of edge(X) the Euclidean distance to the nearest voxel of edge(Y), weighted by `spacing`: the
 *             squared distance in fp64 as (dz sd)^2 + ((dy sh)^2 + (dx sw)^2), the minimum over every candidate (brute
 *             force: ties cannot change it), then sqrt to float32
 *   hd_g      max(quantile_q(d(P_g->A_g)), quantile_q(d(A_g->P_g))), q = percentile / 100, linear interpolation in float32
 *             like torch.quantile (the quantile of mmtta_surface_distances); always finite
 * A lesion's distances go to the surface of ITS components only, and a component matched to two lesions is measured
 * against each of them.
 *   mask, label, n ... w, min_lesion_voxels   those of the mmtta_lesionwise_scores call
 *   spacing   HOST, 3 doubles in D, H, W order, read before return;  percentile in [0, 100]
 *   lesionwise_scratch  the scratch of a mmtta_lesionwise_scores call with the same mask, label, shape and
 *             min_lesion_voxels, queued on the same stream immediately before; only read
 *   hd_stats  int64 [N][R][3] on the device, zeroed by this call: hd_q = sum over the scored lesions of
 *             round(hd_g 2^20) (each rounded once, in fp64), lesions scored (= kept lesions with a match unless the mask
 *             overflows), overflow
 *   lesion_hd fp32 [N,R,D,H,W] dense on the device or NULL: filled with NaN, then hd_g at index (lesion label - 1) of every
 *             scored lesion
 *   scratch   mmtta_lesionwise_hd95_scratch_bytes(N*R, D, H, W) bytes (negative: unsupported extent), a function of the
 *             shape alone
 * The volume's score is host arithmetic on integers:
 *   lw_hd95 = (hd_q / 2^20 + penalty ((kept - found) + false-positive components)) / (kept + false-positive components),
 * valid iff that denominator is > 0, with the counts of mmtta_lesionwise_scores.
 * Overflow: the surface of P_g is gathered into one list per lesion, so a component's edge voxels are held once per lesion
 * it matches; the pool of those lists has 2 D H W entries per mask.  A mask whose lists (summed over its kept lesions) do
 * not fit writes nothing beyond its pool: none of its lesions is scored, `overflow` counts them, hd_q and lesions scored
 * stay 0; the other masks of the batch are unaffected and the call returns normally.
 * Cost: sum over the pairs of |edge(c)| |edge(A_g)| distance evaluations per direction, spread over the whole device in
 * work units of (lesion, direction, 128 sources).  A fixed sequence of launches on `stream` that depends on the shape
 * alone: no host read, no convergence flag.  Segments are handed out by atomic bumps; the results depend on neither their
 * order nor their placement: two calls agree bit for bit and a batch gives what its items give alone.
 * Limits: those of mmtta_lesionwise_scores, and every extent <= 1024.  Anything else - a null argument, a spacing that is
 * not positive and finite, a percentile outside [0, 100], a label of another shape or not fp32 - is refused with
 * MMTTA_ERR_INVALID / _UNSUPPORTED and a message naming the argument, before anything is queued. */
int64_t mmtta_lesionwise_hd95_scratch_bytes(int64_t n_masks, int64_t d, int64_t h, int64_t w);
int mmtta_lesionwise_hd95(const uint8_t* mask, const mmtta_tensor* label, int n, int r, int d, int h, int w,
                          const double* spacing, double percentile, const int64_t* min_lesion_voxels,
                          const void* lesionwise_scratch, int64_t* hd_stats, float* lesion_hd,
                          void* scratch, void* stream);

/* Hole filling and region nesting of the evaluation tail, the steps that follow the component filter in common BraTS /
 * HECKTOR post-processing.  Replaces a host `scipy.ndimage.binary_fill_holes` per (volume, region) over a mask copied off
 * the device and a nesting fix in numpy; the reference evaluator has no counterpart.  Per (n, r), in this order:
 *   holes     B = voxels where mask == 0.  The components of B are taken at `fill_connectivity` (6, 18 or 26; 6 is scipy's
 *             default structure and the dual of a 26-connected foreground).  A component is OPEN if one of its voxels lies
 *             on a face of the volume (z in {0, D-1}, y in {0, H-1} or x in {0, W-1}), otherwise it is a HOLE.  A hole of
 *             region r is filled iff fill_holes[r] != 0 and (max_hole_voxels[r] == 0 or its size <= max_hole_voxels[r]).
 *             Without a cap this is binary_fill_holes(mask, generate_binary_structure(3, 1 | 2 | 3)) exactly.  Holes are
 *             counted for every region, whether or not it fills them.
 *   nesting   `chain` = c_0 ... c_k, distinct region indices, innermost first; chain_len 0 (then `chain` may be NULL) or >= 2.
 *             nest_mode 0 (clip): new[c_i] = old[c_i] & old[c_i+1] & ... & old[c_k];
 *             nest_mode 1 (grow): new[c_i] = old[c_0] | ... | old[c_i];   "old" = after filling.
 *             Regions outside the chain pass through unchanged.
 *   mask      uint8 [N,R,D,H,W] dense on the device (non-zero = foreground), rewritten IN PLACE as 0 / 1; nothing else the
 *             caller owns is written apart from `counts` and `stats`
 *   label     fp32 any strides, ground truth = label > 0.5, or NULL (then `counts` must be NULL)
 *   fill_holes       HOST int32 [R], read before return
 *   max_hole_voxels  HOST int64 [R], read before return, >= 0 (0: no cap)
 *   chain     HOST int32 [chain_len], read before return
 *   counts    int64 [N][R][3] on the device or NULL: inter, psum, gsum of the FINAL mask against the label, as
 *             mmtta_mask_dice_counts defines them; zeroed by this call
 *   stats     int64 [N][R][4] on the device, zeroed by this call: holes, holes filled, voxels filled, voxels the nesting
 *             changed
 *   scratch   mmtta_mask_fill_nest_scratch_bytes(N*R, D, H, W) bytes (negative: unsupported extent)
 * Five launches on `stream` that depend on the shape alone (a tile pass of its own over the complement, where a tile that is
 * all background skips the union-find; the merge and flatten passes of mmtta_components_filter; a border pass; a finish
 * pass): no host read, no convergence flag.  All sums are integers: two calls agree bit for bit and a batch gives what its
 * items give alone.  MMTTA_FILL_UNIFORM_TILES=0 in the environment (read once) switches the all-background shortcut of the
 * tile pass off, for measurements; the results are the same.  Limits: those of mmtta_components_filter.  Anything else -
 * a null argument, a connectivity other than 6 / 18 / 26, a negative cap, a chain of length 1 or longer than R or with a
 * repeated or out-of-range index, a nest_mode other than 0 / 1, a label of another shape or not fp32 - is refused with
 * MMTTA_ERR_INVALID / _UNSUPPORTED and a message naming the argument, before anything is queued. */
int64_t mmtta_mask_fill_nest_scratch_bytes(int64_t n_masks, int64_t d, int64_t h, int64_t w);
int mmtta_mask_fill_nest(uint8_t* mask, const mmtta_tensor* label, int n, int r, int d, int h, int w, int fill_connectivity,
                         const int32_t* fill_holes, const int64_t* max_hole_voxels, const int32_t* chain, int chain_len,
                         int nest_mode, int64_t* counts, int64_t* stats, void* scratch, void* stream);

/* Surface metrics of the evaluation tail: percentile Hausdorff distance and average surface distance per
 * (volume, region).  Replaces the MONAI calls of reference src/evaluation/seg_eval.py:312-340
 * (`HausdorffDistanceMetric(include_background=True, reduction="none", percentile=95, directed=False)` built at
 * :226-234 and `compute_average_surface_distance(..., symmetric=evaluation.surface.asd_symmetric)`), which run
 * scipy on the host.  Edge voxels = mask minus its 6-neighbourhood erosion; distances are exact Euclidean, weighted
 * by `spacing` (host pointer, 3 doubles in D,H,W order: the order the reference hands `evaluation.seg.spacing` to
 * MONAI); the quantile interpolates linearly in float32 like torch.quantile.
 *   pred_mask  uint8 [N,R,D,H,W] dense (the `mask` output of mmtta_mask_dice_counts)
 *   label      fp32 any strides, ground truth = label > 0.5 (reference :306)
 *   hd, asd    fp32 [N*R] on the device.  Both edge sets empty: hd = asd = NaN; exactly one empty: hd = NaN,
 *              asd = +inf (MONAI returns inf distances there); the caller applies the reference's penalty and
 *              sanitising (:342-355).
 *   scratch    mmtta_surface_scratch_bytes(N*R, D, H, W) bytes (negative: extent above 1024 per axis).
 * Results do not depend on scheduling (radix select + integer fixed-point sum): bitwise reproducible. */
int64_t mmtta_surface_scratch_bytes(int64_t n_masks, int64_t d, int64_t h, int64_t w);
int mmtta_surface_distances(const uint8_t* pred_mask, const mmtta_tensor* label, const double* spacing,
                            double percentile, int asd_symmetric, float* hd, float* asd, void* scratch, void* stream);

/* Normalised surface Dice (NSD) of the evaluation tail per (volume, region): the share of each surface that lies within a
 * tolerance of the other one.  MONAI's SurfaceDiceMetric on the edges of mmtta_surface_distances (voxel counts, not
 * Nikolov's surface-element areas):
 *   edge(X)   X & ~erode6(X), outside the volume counts as background
 *   d(v, u)   (float)sqrt(d2), d2 in fp64 as fma(dz sd, dz sd, fma(dy sh, dy sh, (dx sw)^2)) of the offset (dz, dy, dx)
 *   hit       a voxel v of edge(A) against B at tolerance tau: some u of edge(B) has d(v, u) <= (float)tau
 *   NSD_tau   (hits(edge P -> edge G) + hits(edge G -> edge P)) / (|edge P| + |edge G|), host arithmetic on the counts;
 *             valid iff the ground truth is non-empty, like Dice (then |edge G| >= 1; an empty prediction scores 0)
 * No distance transform: a bounded search over bit-packed edge masks.  Per axis a the window radius is r_a = the largest
 * k >= 0 with (float)sqrt((k s_a)^2) <= (float)max(tolerances), found by a loop on the host, so the window holds every
 * offset that can be a hit; r_a <= 8 on every axis, a larger window is refused (mmtta_surface_distances is the tool for
 * large distances).  Cost: linear in the volume, independent of the size of the surfaces.
 *   pred_mask    uint8 [N,R,D,H,W] dense on the device (non-zero = foreground)
 *   label        fp32 any strides, ground truth = label > 0.5
 *   spacing      HOST, 3 doubles in D, H, W order, read before return, positive and finite
 *   tolerances   HOST, n_tolerances doubles (1 ... 4), read before return, each finite and >= 0, in the units of `spacing`
 *   counts       int64 [N*R][n_tolerances][4] on the device, zeroed by this call: hits edge P -> edge G, |edge P|,
 *                hits edge G -> edge P, |edge G|
 *   scratch      mmtta_surface_dice_scratch_bytes(N*R, D, H, W) bytes (negative: an extent above 1024 or more than 65535 masks)
 * Two launches on `stream` that depend on the shape alone.  Integer counts only: two calls agree bit for bit and a batch
 * gives what its items give alone.  Anything else - a null argument, 0 or more than 4 tolerances, a negative or non-finite
 * tolerance, a spacing that is not positive and finite, a window above 8, a label that is not fp32 - is refused with
 * MMTTA_ERR_INVALID / _UNSUPPORTED and a message naming the argument, before anything is queued. */
int64_t mmtta_surface_dice_scratch_bytes(int64_t n_masks, int64_t d, int64_t h, int64_t w);
int mmtta_surface_dice(const uint8_t* pred_mask, const mmtta_tensor* label, const double* spacing, const double* tolerances,
                       int n_tolerances, int64_t* counts, void* scratch, void* stream);

/* Lesion-wise NSD of the evaluation tail (with lesion-wise Dice the BraTS-2024 pair).  Runs right behind
 * mmtta_lesionwise_scores on the same stream and only reads what that call left in its scratch: nothing is labelled twice.
 * Lesions, own voxels, kept / found, matching and false-positive components are exactly those of mmtta_lesionwise_scores.
 * For every lesion g that is kept and found, with A_g = its own voxels and P_g = the union of the whole predicted components
 * matched to it (edge, d and hit as in mmtta_surface_dice; edge(A_g) = edge(G) within the lesion, edge(P_g) = edge(P)
 * within the matched components, a component's edge voxels count once per lesion it matches):
 *   nsd_{g,tau} = (hits(edge A_g -> edge P_g) + hits(edge P_g -> edge A_g)) / (|edge A_g| + |edge P_g|)
 * Only voxels of P_g are candidates for A_g and the reverse: the nearer surface of an unmatched component does not count.
 * A predicted edge voxel within tau of several lesions is a hit for each of them once, exactly, for any number of lesions
 * in its window.
 *   mask, n ... w, min_lesion_voxels   those of the mmtta_lesionwise_scores call
 *   spacing, tolerances, n_tolerances  as in mmtta_surface_dice, with its window limit
 *   lesionwise_scratch  the scratch of a mmtta_lesionwise_scores call with the same mask, shape and min_lesion_voxels,
 *               queued on the same stream before; only read
 *   nsd_stats   int64 [N*R][n_tolerances] on the device, zeroed by this call: sum over the scored lesions of
 *               floor((hits 2^30 + floor(den / 2)) / den), nsd_{g,tau} in units of 2^-30 rounded once, in integers
 *   lesion_nsd  fp32 [N*R][n_tolerances][D*H*W] dense on the device or NULL: filled with NaN, then (float)(hits / den) at
 *               index (lesion label - 1) of every scored lesion
 *   scratch     mmtta_lesionwise_nsd_scratch_bytes(N*R, D, H, W) bytes (negative: unsupported extent), a function of the
 *               shape alone
 * The volume's score is host arithmetic on integers: lw_nsd_tau = (nsd_stats / 2^30) / (kept lesions + false-positive
 * components), valid iff that denominator is > 0; a kept lesion without a match and a false-positive component add 0.
 * Six launches on `stream` that depend on the shape alone: no host read, no convergence flag; integer counts only.
 * Limits: those of mmtta_lesionwise_scores.  Anything else is refused with MMTTA_ERR_INVALID / _UNSUPPORTED and a message
 * naming the argument, before anything is queued.
 * mmtta_lesionwise_nsd_list_slots(): how many distinct lesions a thread of the edge P_g -> edge A_g direction keeps in
 * registers; a window that holds more is walked by the launch for marked voxels (for tests that must reach that launch). */
int mmtta_lesionwise_nsd_list_slots(void);
int64_t mmtta_lesionwise_nsd_scratch_bytes(int64_t n_masks, int64_t d, int64_t h, int64_t w);
int mmtta_lesionwise_nsd(const uint8_t* mask, int n, int r, int d, int h, int w, const double* spacing,
                         const double* tolerances, int n_tolerances, const int64_t* min_lesion_voxels,
                         const void* lesionwise_scratch, int64_t* nsd_stats, float* lesion_nsd, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMTTA_H */
