"""The head convolution with the entropy objective in its epilogue (MMTTA_OPT_HEAD_LOSS_PAIR, option 17, bit 0:
conv3_mfma4_loss_kernel behind mmtta_conv_head_loss_run_sets) against the two launches it replaces on the same tensors in the
same process: the plain convolution followed by ``ops.entropy_loss_items`` under option 17 = 0.

The epilogue computes the value the plain kernel stores and hands it to the same per-logit function (voxel_loss.h:
bernoulli_entropy_terms), scales the gradient by the same fp32 1 / count and rounds it with the same conversion, so
d(logits) - pad lanes included - is compared with torch.equal for fp32 and for bf16 gradient storage.  A voxel's entropy is
summed over its regions in the same order in fp32; what differs is the order in which the fp64 accumulators and partials
are added (one partial per 4 x 8 x 64 tile instead of one per grid-stride workgroup).  An fp64 sum of at most 3 * 10^4 fp32
terms carries a relative error below 1e-11, far inside half an fp32 ulp, so the two fp32 losses are equal or - when the
exact sum sits at a rounding boundary - neighbours: the bound is 1 ulp.  The output buffer is filled with a sentinel and must
come back untouched.

Extents come from the kernel's 4 x 8 x 64 tile: exactly one tile, ragged in every axis (8 tiles), three x tiles with a
ragged last one, and a single voxel.  The logits are driven through the fused add so that values near 0, +-30 and +-1e4
occur: the saturated branches of the entropy terms (exp underflow, the log1p series, t * p at large |t|).
"""
import math

import pytest
import torch

GPU = pytest.mark.gpu
OPT = 17
EXTENTS = {"one-tile": (4, 8, 64), "ragged-8-tiles": (5, 9, 65), "three-x-tiles": (3, 10, 130), "one-voxel": (1, 1, 1)}


def _inputs(R, n, shape, sets):
    d, h, w = shape
    g = torch.Generator().manual_seed(1700 + 97 * R + 13 * n + sum(shape) + (5 if sets else 0))
    rnd = lambda *s: torch.randn(*s, generator=g)
    nw = n if sets else 1
    x = rnd(n, R, d, h, w) * 1.5 + 0.25
    # the residual decides the size of a logit: a third near 0, the rest spread over +-30 and +-1e4 (and plain noise)
    pick = torch.randint(0, 6, (n, R, d, h, w), generator=g)
    levels = torch.tensor([0.0, 0.0, 30.0, -30.0, 1e4, -1e4])
    res = levels[pick] + rnd(n, R, d, h, w) * 0.5
    return dict(x=x, res=res, w=rnd(nw, R, R, 3, 3, 3) * (R * 27) ** -0.5, b=rnd(nw, 4) * 0.1,
                sc=rnd(n * R).abs() + 0.5, sh=rnd(n * R) * 0.3, rsc=1.0 + rnd(n * R) * 0.01, rsh=rnd(n * R) * 0.05)


def _make_op(inp, R, n, sets):
    from multimodal_tta_amd import ops

    class Ctl:
        use_sets = True

    nw = n if sets else 1
    op = ops.ConvOp(R, R, 3, 1, False, "cuda", dtype=ops.BF16, n_sets=nw)
    for j in range(nw):
        op.pack(inp["w"][j].cuda().contiguous(), j)
    if sets:
        op.set_param_sets(1, 1, 128, 0, 4, 0, Ctl())      # item j reads image j and bias row j (rows of 4: 16-byte strides)
    return op, inp["b"].cuda().contiguous()


def _whole_rows(t):
    """The 4-lane rows behind a channels-last view (pad lanes included)."""
    n, d, h, w, _ = t.shape
    return t.as_strided((n, d, h, w, 4), t.stride())


def _within_one_ulp(a, b):
    up, down = torch.nextafter(a, torch.full_like(a, math.inf)), torch.nextafter(a, torch.full_like(a, -math.inf))
    return bool(((a == b) | (b == up) | (b == down)).all())


@GPU
@pytest.mark.parametrize("sets", [False, True], ids=["one-set", "sets"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("extent", list(EXTENTS))
def test_head_loss_epilogue_gives_the_two_launches_bits(extent, R, n, sets):
    from multimodal_tta_amd import ops
    from test_hip_conv import cl

    shape = EXTENTS[extent]
    d, h, w = shape
    inp = _inputs(R, n, shape, sets)
    op, bias = _make_op(inp, R, n, sets)
    x, res = cl(inp["x"]), cl(inp["res"])
    nl_of = lambda sc, sh, relu: ops.NL(sc.cuda(), sc.cuda(), relu=relu, scale=sc.cuda(), shift=sh.cuda())
    equal_losses = total_losses = 0
    for with_norm in (False, True):
        x_nl = nl_of(inp["sc"], inp["sh"], True) if with_norm else None
        add_nl = nl_of(inp["rsc"], inp["rsh"], False) if with_norm else None
        for gdt in (torch.float32, torch.bfloat16):
            tag = f"{extent} R={R} n={n} sets={sets} norm={with_norm} {gdt}"
            fresh_dz = lambda: ops.new_cl(n, d, h, w, R, "cuda", ldc=4, dtype=gdt)
            # ---- the two launches (option 17 = 0: the query says no)
            prev = ops.set_option(OPT, 0)
            try:
                y = ops.new_cl(n, d, h, w, R, "cuda", ldc=4, zero=True)
                dz_ref = fresh_dz()
                _whole_rows(dz_ref).fill_(float("nan"))
                assert not op.head_loss_eligible(x, x_nl, y, dz_ref, add=res, add_nl=add_nl), tag
                op.forward(x, x_nl, bias, y, add=res, add_nl=add_nl)
                partial = torch.zeros(ops.entropy_partials_items(y), dtype=torch.float64, device="cuda")
                loss_ref = torch.full((n,), float("nan"), device="cuda")
                ops.entropy_loss_items(y, dz_ref, partial, loss_ref)
            finally:
                ops.set_option(OPT, prev)
            # ---- the one launch
            prev = ops.set_option(OPT, 3)
            try:
                y2 = ops.new_cl(n, d, h, w, R, "cuda", ldc=4)
                _whole_rows(y2).fill_(-777.0)
                dz = fresh_dz()
                _whole_rows(dz).fill_(float("nan"))
                assert op.head_loss_eligible(x, x_nl, y2, dz, add=res, add_nl=add_nl), tag
                partial2 = torch.full((op.head_loss_partials(x, y2),), float("nan"), dtype=torch.float64, device="cuda")
                loss = torch.full((n,), float("nan"), device="cuda")
                op.forward_head_loss(x, x_nl, bias, y2, dz, partial2, loss, add=res, add_nl=add_nl)
            finally:
                ops.set_option(OPT, prev)
            torch.cuda.synchronize()
            z = y.float().abs()
            if d * h * w * n * R >= 1000:      # the scaling did what it is there for
                assert (z < 2).any() and ((z > 20) & (z < 40)).any() and (z > 5e3).any(), tag
            assert torch.equal(_whole_rows(y2), torch.full_like(_whole_rows(y2), -777.0)), f"{tag}: the logits were written"
            assert torch.equal(_whole_rows(dz_ref).view(torch.int16 if gdt == torch.bfloat16 else torch.int32),
                               _whole_rows(dz).view(torch.int16 if gdt == torch.bfloat16 else torch.int32)), f"{tag}: dlogits differ"
            assert bool(torch.isfinite(loss).all()) and not bool(torch.isnan(partial2).any()), tag
            assert _within_one_ulp(loss_ref, loss), f"{tag}: loss {loss.tolist()} vs {loss_ref.tolist()}"
            equal_losses += int((loss == loss_ref).sum())
            total_losses += n
    print(f"{extent} R={R} n={n} sets={sets}: {equal_losses} of {total_losses} losses exactly equal")


@GPU
def test_entmin_adaptation_with_and_without_the_head_loss_epilogue(monkeypatch):
    """entmin_tta on a 4 x 16 x 16 x 64 volume pair, S = 3, group 2, bf16 precision: option 17 = 3 against 0.  The gradients
    are equal bit for bit, so the weights, the final logits and the Dice counts are; the per-step losses are the two fp32
    roundings of one fp64 sum (1 ulp)."""
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import SMALL, build_pair, root_cfg, volume

    calls = {"tail": 0}
    real = ops.ConvOp.forward_head_loss

    def counted(self, *a, **k):
        calls["tail"] += 1
        return real(self, *a, **k)

    monkeypatch.setattr(ops.ConvOp, "forward_head_loss", counted)
    vols = [volume(i, shape=(16, 16, 64)) for i in range(2)]
    x = torch.cat([v[0] for v in vols]).cuda()
    label = torch.cat([v[1] for v in vols]).cuda().contiguous()
    out = {}
    for opt in (0, 3):
        prev = ops.set_option(OPT, opt)
        try:
            cfg = root_cfg(SMALL, steps=3, lr=1e-3, group=2, precision="bf16", tune_volumes=4)
            _, hip = build_pair(SMALL)
            plug = get_plugin("entmin_tta")(cfg).setup(hip, "cuda")
            before = calls["tail"]
            res = plug.adapt_volume(x)
            counts = torch.zeros(2 * 3 * 3, dtype=torch.int64, device="cuda")
            ops.mask_dice_counts(res["logits_cl"], label, 0.5, counts)
            torch.cuda.synchronize()
            out[opt] = (res["logits_cl"].clone(), res["losses"].clone(), counts.clone(), calls["tail"] - before)
        finally:
            ops.set_option(OPT, prev)
    assert out[0][3] == 0 and out[3][3] >= 1, f"head-loss launches: {out[0][3]} at option 0, {out[3][3]} at option 3"
    assert torch.equal(out[0][0], out[3][0]), "final logits differ"
    assert torch.equal(out[0][2], out[3][2]), "Dice counts differ"
    assert out[0][1].shape == (3, 2) and _within_one_ulp(out[0][1], out[3][1]), f"losses {out[3][1].tolist()} vs {out[0][1].tolist()}"
    print(f"{int((out[0][1] == out[3][1]).sum())} of 6 per-step losses exactly equal")
