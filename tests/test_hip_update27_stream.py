"""The 16-byte form of the fused weight update (``wgrad_update27_kernel``: a thread owns 4 consecutive output channels of a
slab row, and 4 consecutive floats of a parameter row).  Every check is BITWISE against the separate passes - weight
gradient, arena optimizer, batched repack - at the smallest shapes where the new code can go wrong: channel tails that mask
lanes of a float4 or send a block to the 4-byte form, slab counts with and without a tail trip and through the pre-reduce
stage, one and several parameter sets (a family with ``inner`` > 1 included), every optimizer kind at step 0 and later, with
and without a bias, with one image and with both.

The table-driven launch for the small layers is not part of this build (the per-layer launches stay), so it has no test
here."""
import os
import sys

import pytest
import torch

from test_hip_conv import cl, ref_module  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class _Ctl:
    use_sets = True


WGRAD_WORKGROUPS = 4          # MMTTA_OPT_WGRAD_WORKGROUPS: workgroups a weight-gradient launch aims for (sets the slab count)


def run_case(*args, **kw):
    """_run_case under the library's default slab planning (the knob is process wide and the adaptation tests tune it)."""
    from multimodal_tta_amd import ops

    prev = ops.set_option(WGRAD_WORKGROUPS, 128)
    try:
        return _run_case(*args, **kw)
    finally:
        ops.set_option(WGRAD_WORKGROUPS, prev)


def _run_case(cin, cout, stride, transposed, shape, opt="adam", decay=True, Q=1, inner=1, steps=2, bias=True, both_images=True,
              want_nsl=None, want_pre=None):
    """`steps` fused updates of one layer against reduce + optimizer + pack, everything compared with torch.equal after each
    step.  Q parameter sets of one volume each; `inner` > 1 stores them as families ([outer][inner] strides)."""
    from multimodal_tta_amd import ops
    from multimodal_tta_amd._lib import MmttaError

    assert ops.fused_update_enabled()
    torch.manual_seed(101 + 7 * cin + cout + Q)
    d, h, w = shape
    mod = ref_module(cin, cout, 3, stride, transposed)
    wshape, wnum = tuple(mod.weight.shape), mod.weight.numel()
    boff = (wnum + 3) // 4 * 4
    total = boff + (cout + 3) // 4 * 4
    spec = ops.OptimSpec(name=opt, lr=1e-2, weight_decay=5e-2, momentum=0.9 if (opt == "sgd" and decay) else 0.0)
    P = torch.zeros(Q, total, device="cuda")
    P[:, :wnum] = 0.05 * torch.randn(Q, wnum, device="cuda")
    P[:, boff:boff + cout] = 0.05 * torch.randn(Q, cout, device="cuda")
    M = torch.zeros(Q, total, device="cuda")
    V = torch.zeros(Q, total, device="cuda")
    M[:, :wnum] = 1e-3 * torch.randn(Q, wnum, device="cuda")      # step 0 must not read these
    V[:, :wnum] = 1e-6 * torch.rand(Q, wnum, device="cuda")
    x = cl(torch.randn(Q, cin, d, h, w))

    def make_op():
        op = ops.ConvOp(cin, cout, 3, stride, transposed, "cuda", dtype=ops.BF16, n_sets=Q)
        op.need_dgrad = both_images
        if Q > 1:
            # set q lives (q // inner) outer + (q % inner) inner strides behind set 0: rows of `total` either way
            op.set_param_sets(1, inner, total * inner, total if inner > 1 else 0, total * inner, total if inner > 1 else 0, _Ctl())
        return op

    opA, opB = make_op(), make_op()
    if not opA.plain_bf16_images():
        # a side under 16 channels keeps a thin-K fragment image behind the bf16 one: the fused entry point does not take
        # such a layer (it stays with the separate passes), and must say so instead of writing half an update
        PB, MB, VB = P.clone(), M.clone(), V.clone()
        stepB = torch.zeros(1, dtype=torch.int32, device="cuda")
        target = opB.update_target(spec, PB[0, :wnum], MB[0, :wnum], VB[0, :wnum], PB[0, boff:boff + cout], MB[0, boff:boff + cout],
                                   VB[0, boff:boff + cout], None, decay, decay, stepB)
        gy = cl(torch.randn(Q, cout, *opA.out_shape(torch.empty(1, d, h, w, 1))[1:4]))
        with pytest.raises(MmttaError):
            opB.wgrad_update(x, None, gy, target)
        torch.cuda.synchronize()
        assert torch.equal(PB, P) and torch.equal(MB, M) and torch.equal(VB, V)
        return None

    # A: separate passes
    PA, MA, VA, GA = P.clone(), M.clone(), V.clone(), torch.zeros(Q, total, device="cuda")
    stepA = torch.zeros(1, dtype=torch.int32, device="cuda")
    items = []
    for g in range(Q):
        wv = PA[g, :wnum].view(wshape)
        items.append((opA.d_fwd, wv, opA.packed_image(False, g)))
        if both_images:
            items.append((opA.d_dgrad, wv, opA.packed_image(True, g)))
    packer = ops.BatchedPacker(items, "cuda")
    packer.run()
    # B: fused
    PB, MB, VB, GB = P.clone(), M.clone(), V.clone(), torch.zeros(Q, total, device="cuda")
    stepB = torch.zeros(1, dtype=torch.int32, device="cuda")
    for g in range(Q):
        opB.pack(PB[g, :wnum].view(wshape), g)
    bias_here = bias and not transposed            # (a transposed layer's bias stays with the arena optimizer)
    sl = slice(boff, boff + cout)
    target = opB.update_target(spec, PB[0, :wnum], MB[0, :wnum], VB[0, :wnum],
                               PB[0, sl] if bias_here else None, MB[0, sl] if bias_here else None,
                               VB[0, sl] if bias_here else None, GB[0, sl] if (bias and transposed) else None,
                               decay, decay, stepB)
    segs = [] if (bias_here or not bias) else [(boff, total - boff, decay)]
    table, total_left = ops.optim_segments_table(segs, "cuda") if segs else (torch.zeros(1, dtype=torch.int64, device="cuda"), 0)

    oshape = opA.out_shape(torch.empty(1, d, h, w, 1))[1:4]
    plan = opB.wgrad_plan(x, cl(torch.zeros(Q, cout, *oshape)))
    if want_nsl is not None:
        assert plan["nsl"] == want_nsl, plan
    if want_pre is not None:
        assert (plan["pre_chunks"] > 0) == want_pre, plan
    for t in range(steps):
        gy = cl(torch.randn(Q, cout, *oshape))
        opA.wgrad(x, None, gy, GA[0, :wnum].view(wshape), GA[0, sl] if bias else None)
        ops.optim_step_sets(spec, PA, GA, MA, VA, total, total if decay else 0, Q, stepA)
        packer.run()
        opB.wgrad_update(x, None, gy, target)
        ops.optim_step_segments(spec, PB, GB, MB, VB, table, len(segs), total_left, Q, stepB)
        torch.cuda.synchronize()
        where = f"step {t}, plan {plan}"
        assert int(stepA) == int(stepB) == t + 1, where
        if bias:
            assert torch.equal(PA, PB), f"weights / bias, {where}"
            assert torch.equal(MA, MB), f"first moments, {where}"
            if opt != "sgd":
                assert torch.equal(VA, VB), f"second moments, {where}"
        else:
            # (without a bias the separate passes still step the bias rows with a zero gradient: the weights are the check)
            assert torch.equal(PA[:, :wnum], PB[:, :wnum]), f"weights, {where}"
            assert torch.equal(MA[:, :wnum], MB[:, :wnum]), f"first moments, {where}"
            if opt != "sgd":
                assert torch.equal(VA[:, :wnum], VB[:, :wnum]), f"second moments, {where}"
            assert torch.equal(PB[:, sl], P[:, sl]) and torch.equal(MB[:, sl], M[:, sl]), f"the bias moved, {where}"
        assert torch.equal(opA.packed_fwd, opB.packed_fwd), f"forward images, {where}"
        if both_images:
            assert torch.equal(opA.packed_dgrad, opB.packed_dgrad), f"input-gradient images, {where}"
    assert not torch.equal(PB[:, :wnum], P[:, :wnum]), "the step moved no weight"
    return plan


# ---- channel tails: Cg not a multiple of 8 (a partial cg tile: 4-byte parameter rows), Cd not a multiple of 32 nor of 4
# (masked lanes of a float4), and one aligned layer.  (12, 40) and (8, 36) have a side under 16 channels, which the fused
# entry point refuses by contract (run_case checks the refusal); (28, 36) and (36, 22) put the same tails where it runs.
TAILS = [(12, 40), (8, 36), (20, 33), (32, 64), (28, 36), (36, 22)]


@pytest.mark.gpu
@pytest.mark.parametrize("Q", [1, 3])
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("cin,cout", TAILS)
def test_channel_tails(cin, cout, transposed, Q):
    shape = (4, 4, 8) if transposed else (8, 8, 8)
    run_case(cin, cout, 2 if transposed else 1, transposed, shape, Q=Q)


# ---- slab counts: no tail trip (4 per trip), tails of 1 / 3 / 1 slabs, two whole trips, and the pre-reduce route.  The
# stride-1 bf16 kernel takes 4 x 8 x 8 output voxels per tile, the stride-2 / transposed one 2 x 4 x 8 (of the coarse
# grid), and a layer this small gets one slab per tile up to 32 slabs, chunks of 32 beyond.
SLABS = [
    (32, 64, 1, False, (4, 8, 8), 1, False),
    (32, 64, 1, False, (12, 8, 8), 3, False),
    (32, 64, 1, False, (20, 8, 8), 5, False),
    (32, 64, 1, False, (16, 16, 16), 16, False),
    (32, 64, 2, False, (16, 16, 16), 8, False),
    (64, 32, 2, True, (6, 4, 8), 3, False),
    (32, 64, 1, False, (20, 16, 16), 20, False),
    (32, 64, 1, False, (32, 16, 32), None, True),
    (20, 33, 2, False, (16, 32, 64), None, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("Q", [1, 3])
@pytest.mark.parametrize("cin,cout,stride,transposed,shape,nsl,pre", SLABS)
def test_slab_counts(cin, cout, stride, transposed, shape, nsl, pre, Q):
    plan = run_case(cin, cout, stride, transposed, shape, Q=Q, want_nsl=nsl, want_pre=pre)
    if pre:
        assert plan["nsl"] > 32 and plan["pre_chunks"] == (plan["nsl"] + 31) // 32, plan


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,transposed", [(32, 64, False), (20, 33, False), (64, 32, True)])
def test_family_of_sets(cin, cout, transposed):
    """Four sets stored as two families of two (``inner`` = 2): the set index splits into outer and inner strides."""
    run_case(cin, cout, 2 if transposed else 1, transposed, (4, 4, 8) if transposed else (12, 8, 8), Q=4, inner=2)


@pytest.mark.gpu
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("opt,decay", [("adam", True), ("adam", False), ("adamw", True), ("sgd", True), ("sgd", False)])
@pytest.mark.parametrize("cin,cout", [(32, 64), (20, 33)])
def test_optimizers_and_step_counter(cin, cout, opt, decay, bias):
    """Adam, AdamW with decay, SGD with momentum (`decay`) and without: step 0 (stale moments ignored) and two more."""
    run_case(cin, cout, 1, False, (12, 8, 8), opt=opt, decay=decay, Q=3, steps=3, bias=bias)


@pytest.mark.gpu
@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("cin,cout,stride,transposed", [(32, 64, 1, False), (64, 32, 2, True), (20, 33, 2, False)])
def test_images(cin, cout, stride, transposed, both):
    """A forward-only layer writes one image, the others both; a convolution and a transposed convolution put the two
    orientations ([T][K = cg][N = cd] and [T][K = cd][N = cg]) on opposite images."""
    run_case(cin, cout, stride, transposed, (4, 4, 8) if transposed else (8, 8, 8), Q=3, both_images=both)


def test_update_kernels_have_no_scratch_and_no_spills():
    """Resource figures of the built code objects (scripts/kernel_resources.py): the update kernels and the reduction they
    must agree with keep everything in registers."""
    import __graft_entry__ as ge
    ge.build()
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    table = kernel_resources.figures(os.path.join(ROOT, "multimodal_tta_amd", "csrc", "libmmtta.so"))
    upd = {k: v for k, v in table.items() if "wgrad_update27_kernel" in k}
    assert len(upd) >= 3, sorted(table)[:20]
    for k, v in list(upd.items()) + [(k, v) for k, v in table.items() if "wgrad_reduce27_kernel" in k]:
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
        assert v["vgpr"] <= 128, (k, v)            # four 256-thread blocks per CU
