"""The cases of tests/loss_metric_classes.py on the GPU: mmtta_mask_dice_counts, mmtta_dice_ce_sums / mmtta_dice_ce_grad,
mmtta_optim_step / _sets / _segments and mmtta_intensity_normalize against their float64 references, with the bounds of that
module.  Outputs are NaN- or sentinel-filled before the call and sit between guard elements; every byte outside the written
view (guards, pad lanes, the gap between replicas, elements outside the segments, moment buffers the kernel must leave alone)
is compared before and after.  The worst err / bound of every family is printed (DESIGN.md records them)."""
import ctypes as C

import pytest
import torch

import loss_metric_classes as lm

pytestmark = pytest.mark.gpu

GUARD = 64               # elements on either side of an output (256 bytes of fp32: the views stay 16-byte aligned)
WORST = {}
NAN = float("nan")
ids = lambda cases: [c.name for c in cases]


def record(family, err, bound):
    ratio = float(err) / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    return ratio


def guarded(numel, dtype, fill):
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + numel]


def bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 2: torch.int16, 1: torch.uint8}[t.element_size()]) if t.is_floating_point() else t


def assert_untouched(name, buf, before, written=None):
    """`buf` (flat, guards included) against its snapshot everywhere except where `written` (bool over the inner view)."""
    same = bits(buf) == bits(before)
    if written is not None:
        same[GUARD:GUARD + written.numel()] |= written.reshape(-1).to(same.device)
    assert bool(same.all()), f"{name}: {int((~same).sum())} elements outside the written view changed"


def cl_buffer(t_ncdhw, ldc):
    """NCDHW cpu tensor -> (buffer [N,D,H,W,ldc] NaN-filled, its [.., :C] view) on the device."""
    n, c, d, h, w = t_ncdhw.shape
    buf = torch.full((n, d, h, w, ldc), NAN, device="cuda")
    view = buf[..., :c]
    view.copy_(t_ncdhw.permute(0, 2, 3, 4, 1))
    return buf, view


# ============================================================================= mask + Dice counts
@pytest.mark.parametrize("case", lm.DICE_CASES, ids=ids(lm.DICE_CASES))
def test_mask_dice_counts_equal_the_reference(case):
    from multimodal_tta_amd import ops
    o = lm.make_dice(case.name)
    z, lab = o["z"].float(), o["lab"].float().cuda()
    n, r, d, h, w = z.shape
    if case.layout == "ncdhw":
        zbuf = zview = z.cuda().contiguous()
    else:
        zbuf, zview = cl_buffer(z, r if case.layout == "cl" else (r + 3) // 4 * 4)
    z0, lab0 = zbuf.clone(), lab.clone()
    cbuf, counts = guarded(n * r * 3, torch.int64, -7)
    mbuf, mask = guarded(n * r * d * h * w, torch.uint8, 0xCD) if case.mask else (None, None)
    c0, m0 = cbuf.clone(), (mbuf.clone() if case.mask else None)
    ops.mask_dice_counts(zview, lab, case.thr, counts.view(n, r, 3), mask.view(n, r, d, h, w) if case.mask else None,
                         logits_channels_last=case.layout != "ncdhw")
    torch.cuda.synchronize()
    got = counts.view(n, r, 3).cpu()
    if case.mask:
        got_mask = mask.view(n, r, d, h, w).cpu()
        wrong = int((got_mask != o["pred"]).sum())
        assert wrong == 0, f"{wrong} mask voxels differ from sigmoid(z) >= thr in float64"
        assert_untouched("mask", mbuf, m0, torch.ones(mask.numel(), dtype=torch.bool))
    assert torch.equal(got, o["counts"]), (got - o["counts"]).abs().max().item()
    assert_untouched("counts", cbuf, c0, torch.ones(counts.numel(), dtype=torch.bool))
    assert torch.equal(bits(zbuf), bits(z0)) and torch.equal(lab, lab0), "an input was written"


# ============================================================================= DiceCE sums and gradient
def run_dce(case, o, channels_last, items=slice(None)):
    """-> (sums [N, 3R+1] float64, gradient [N,R,D,H,W] fp32, both on the cpu) of one launch pair over the items `items`."""
    from multimodal_tta_amd import ops
    z, y = o["z"][items].float(), o["y"][items].float().cuda().contiguous()
    n, r, d, h, w = z.shape
    wt = None if o["w"] is None else o["w"].float().cuda()
    opt = case.opts
    ldc = (r + 3) // 4 * 4            # the trainer's dlogits: rows padded to 4
    if channels_last:
        zbuf, zview = cl_buffer(z, r)
        gbuf, ginner = guarded(n * d * h * w * ldc, torch.float32, NAN)
        gview = ginner.view(n, d, h, w, ldc)[..., :r]
        written = torch.zeros((n, d, h, w, ldc), dtype=torch.bool)
        written[..., :r] = True
    else:
        zbuf = zview = z.cuda().contiguous()
        gbuf, ginner = guarded(n * r * d * h * w, torch.float32, NAN)
        gview = ginner.view(n, r, d, h, w)
        written = torch.ones(ginner.numel(), dtype=torch.bool)
    sbuf, sums = guarded(n * (3 * r + 1), torch.float64, NAN)
    z0, y0, g0, s0 = zbuf.clone(), y.clone(), gbuf.clone(), sbuf.clone()
    ops.dice_ce_sums(zview, y, wt, opt["squared_pred"], sums, logits_channels_last=channels_last, softmax=case.softmax)
    ops.dice_ce_grad(zview, y, wt, opt["squared_pred"], opt["jaccard"], opt["include_background"], opt["lambda_dice"], opt["lambda_ce"],
                     sums, gview, logits_channels_last=channels_last, smooth_nr=opt["smooth_nr"], smooth_dr=opt["smooth_dr"],
                     softmax=case.softmax)
    torch.cuda.synchronize()
    assert_untouched("sums", sbuf, s0, torch.ones(sums.numel(), dtype=torch.bool))
    assert_untouched("dlogits (guards and pad lanes)", gbuf, g0, written)
    assert torch.equal(bits(zbuf), bits(z0)) and torch.equal(y, y0), "an input was written"
    grad = (gview.permute(0, 4, 1, 2, 3) if channels_last else gview).contiguous().cpu()
    return sums.view(n, 3 * r + 1).cpu(), grad


@pytest.mark.parametrize("case", lm.DCE_CASES, ids=ids(lm.DCE_CASES))
def test_dice_ce_sums_and_gradient(case):
    o = lm.make_dce(case.name)
    fam = ("softmax" if case.softmax else "sigmoid")
    s_cl, g_cl = run_dce(case, o, True)
    s_nc, g_nc = run_dce(case, o, False)
    # the traversal does not depend on the strides; a second run gives the same bits
    assert torch.equal(bits(s_cl), bits(s_nc)), "channels-last and NCDHW sums differ"
    assert torch.equal(bits(g_cl), bits(g_nc)), "channels-last and NCDHW gradients differ"
    s2, g2 = run_dce(case, o, True)
    assert torch.equal(bits(s2), bits(s_cl)) and torch.equal(bits(g2), bits(g_cl)), "a second run differs"
    # the sums
    assert torch.isfinite(s_cl).all() and torch.isfinite(g_cl).all()
    err, bound = (s_cl - o["sums"]).abs(), o["sum_bounds"]
    r3 = 3 * case.R
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.inf, 0.0).double())
    print(f"{case.name}: sums worst err / bound Dice {ratio[:, :r3].max().item():.3f}, CE numerator {ratio[:, r3].max().item():.3f}")
    record(f"DiceCE {fam} Dice sums", ratio[:, :r3].max().item(), 1.0)
    record(f"DiceCE {fam} CE numerator", ratio[:, r3].max().item(), 1.0)
    assert (err <= bound).all(), f"sums outside their bounds: worst err / bound {ratio.max().item():.3f}"
    # the loss the project reports from them
    _, lbound = lm.dce_loss_from_sums(case, o["sums"], o["sum_bounds"])
    got = lm.dce_loss_from_sums(case, s_cl)
    lerr = abs(got - o["loss64"])
    print(f"{case.name}: loss {got:.9g} (float64 {o['loss64']:.9g}) err {lerr:.2e}, derived bound {lbound:.2e}, "
          f"held {1e-5 * abs(o['loss64']):.2e}")
    record(f"DiceCE {fam} loss", lerr, min(lbound, 1e-5 * abs(o["loss64"])))
    assert lerr <= lbound and lerr <= 1e-5 * abs(o["loss64"])
    # the gradient
    gerr = (g_cl.double() - o["grad64"]).abs().max().item()
    print(f"{case.name}: gradient err {gerr:.2e} = {gerr / o['grad64'].abs().max().item():.2e} of max, measured bound "
          f"{o['grad_measured']:.2e}, held {o['grad_held']:.2e}")
    record(f"DiceCE {fam} gradient", gerr, o["grad_bound"])
    assert gerr <= o["grad_bound"]
    # item n of the batch = that item alone (the sums; the gradient's scales hold the batch size)
    if case.N > 1:
        for i in range(case.N):
            s1, _ = run_dce(case, o, True, slice(i, i + 1))
            assert torch.equal(bits(s1[0]), bits(s_cl[i])), f"item {i} alone differs from item {i} of the batch"


# ============================================================================= optimizers
@pytest.mark.parametrize("case", lm.OPT_CASES, ids=ids(lm.OPT_CASES))
def test_optimizers(case):
    from multimodal_tta_amd import ops
    ref = lm.make_opt(case.name)
    kind, kw = lm.hyper(case.hp)
    reps, stride, used, active, decay = lm.opt_layout(case)
    p0, m0, v0, grads = lm.opt_operands(case)
    b = kw.get("betas", (0.9, 0.999))
    spec = ops.OptimSpec(name=kind, lr=kw["lr"], beta1=b[0], beta2=b[1], eps=kw.get("eps", 1e-8), weight_decay=kw["weight_decay"],
                         momentum=kw.get("momentum", 0.0), dampening=kw.get("dampening", 0.0), nesterov=kw.get("nesterov", False))
    total = reps * stride
    shape = (reps, stride)
    pbuf, P = guarded(total, torch.float32, NAN)
    gbuf, G = guarded(total, torch.float32, NAN)
    mbuf, M = guarded(total, torch.float32, NAN)              # garbage at step 0: the first step must not read it
    vbuf, V = guarded(total, torch.float32, float("inf"))
    P.copy_(p0.float().reshape(-1))
    if case.step0:
        M.copy_(m0.float().reshape(-1))
        V.copy_(v0.float().reshape(-1))
    Vv = V.view(shape) if kind != "sgd" else None
    step = torch.full((1,), case.step0, dtype=torch.int32, device="cuda")
    p_before, m_before, v_before = pbuf.clone(), mbuf.clone(), vbuf.clone()
    table = None
    if case.mode == "segments":
        table, seg_total = ops.optim_segments_table(case.segs, "cuda")
        assert seg_total == int(active.sum())
    for g in grads:
        G.copy_(g.float().reshape(-1))
        g_before = gbuf.clone()
        if case.mode == "plain":
            ops.optim_step(spec, P, G, M, None if Vv is None else V, case.n_decay, step)
        elif case.mode == "sets":
            ops.optim_step_sets(spec, P.view(shape), G.view(shape), M.view(shape), Vv, case.n, case.n_decay, used, step)
        else:
            ops.optim_step_segments(spec, P.view(shape), G.view(shape), M.view(shape), Vv, table, len(case.segs), seg_total, used, step)
        torch.cuda.synchronize()
        assert torch.equal(bits(gbuf), bits(g_before)), "the gradient was written"
    assert int(step.item()) == case.step0 + case.steps
    written = torch.zeros(shape, dtype=torch.bool)
    written[:used] = active
    assert_untouched("p", pbuf, p_before, written)
    keeps_m = kind != "sgd" or kw["momentum"] != 0.0
    # SGD without momentum keeps no buffer: `m` is neither read nor written, on the vector path and on the ragged tail
    assert_untouched("m", mbuf, m_before, written if keeps_m else None)
    assert_untouched("v", vbuf, v_before, written if kind != "sgd" else None)
    got = {"p": P, "m": M if keeps_m else None, "v": V if kind != "sgd" else None}
    for q in ("p", "m", "v"):
        assert (got[q] is None) == (ref[q] is None)
        if ref[q] is None:
            continue
        x = lm.opt_flat(case, got[q].view(shape).cpu(), active).double()
        assert torch.isfinite(x).all(), f"{q} is not finite (a garbage moment was read?)"
        err = (x - ref[q]).abs().max().item()
        ratio = record(f"optimizer {kind} {q}", err, ref["bounds"][q])
        print(f"{case.name}: {q} err {err:.2e}, bound {ref['bounds'][q]:.2e} ({ratio:.3f})")
        assert err <= ref["bounds"][q], f"{q}: err {err:.3e} > bound {ref['bounds'][q]:.3e}"


# ============================================================================= intensity normalisation
def run_intensity(case, x):
    """The C entry point itself on a contiguous [1,C,D,H,W] image -> (y cpu, partial sums [C, 256, 5], coef [C, 2])."""
    from multimodal_tta_amd import _lib, transforms
    from multimodal_tta_amd.ops import check, ptr, stream_ptr
    c, (d, h, w) = case.C, case.shape
    lib = _lib.load()
    rules = transforms.build_rules(c, **lm.int_kwargs(case))
    arr = (_lib.IntensityRule * c)(*rules)
    x5 = x.float().cuda().contiguous().unsqueeze(0)
    x0 = x5.clone()
    ybuf, yin = guarded(c * d * h * w, torch.float32, NAN)
    y5 = yin.view(1, c, d, h, w)
    nbytes = int(lib.mmtta_intensity_scratch_bytes(c))
    assert nbytes == c * 256 * 5 * 8 + c * 2 * 4
    scratch = torch.full((nbytes + 256,), 0xEE, dtype=torch.uint8, device="cuda")
    y_before = ybuf.clone()
    tx, ty = _lib.desc_ncdhw(x5), _lib.desc_ncdhw(y5)
    check(lib.mmtta_intensity_normalize(C.byref(tx), arr, C.byref(ty), ptr(scratch), stream_ptr()), "intensity_normalize")
    torch.cuda.synchronize()
    assert_untouched("y", ybuf, y_before, torch.ones(yin.numel(), dtype=torch.bool))
    assert bool((scratch[nbytes:] == 0xEE).all()), "bytes past the scratch buffer were written"
    assert torch.equal(bits(x5), bits(x0)), "the input was written"
    part = scratch[:c * 256 * 5 * 8].view(torch.float64).view(c, 256, 5).cpu()
    coef = scratch[c * 256 * 5 * 8:nbytes].view(torch.float32).view(c, 2).cpu()
    return y5[0].cpu(), part, coef


@pytest.mark.parametrize("case", lm.INT_CASES, ids=ids(lm.INT_CASES))
def test_intensity_normalize(case):
    from multimodal_tta_amd.transforms import normalize_image
    o = lm.make_int(case.name)
    x, ref = o["x"], o["ref"]
    dhw = x[0].numel()
    geo = lm.int_geometry(dhw)
    y, part, coef = run_intensity(case, x)
    # the product's wrapper gives the same bits (a non-contiguous view included)
    xd = x.float().cuda()
    if case.strided:
        wide = torch.full((case.C,) + case.shape[:2] + (2 * case.shape[2],), NAN, device="cuda")
        wide[..., ::2] = xd
        xd = wide[..., ::2]
        assert not xd.is_contiguous()
    yp = normalize_image(xd, **lm.int_kwargs(case)).cpu()
    assert torch.equal(bits(yp), bits(y)), "normalize_image differs from the entry point on the same image"
    assert normalize_image(xd, normalize=False) is xd
    assert torch.isfinite(y).all()
    for ch in range(case.C):
        if o["exact"][ch]:
            assert torch.equal(bits(y[ch]), bits(ref[ch].float())), f"channel {ch}: clip / no-op is not bit exact"
            continue
        err = (y[ch].double() - ref[ch]).abs().max().item()
        ratio = record("intensity legacy output" if not case.rules else "intensity z-scored output", err, o["bounds"][ch])
        print(f"{case.name} channel {ch}: err {err:.2e}, bound {o['bounds'][ch]:.2e} ({ratio:.3f})")
        assert err <= o["bounds"][ch], f"channel {ch}: err {err:.3e} > bound {o['bounds'][ch]:.3e}"
    # the statistics: fp64 sums of exact terms (a double holds an fp32 value and its square), then mu and sd as fp32
    trips = -(-dhw // (geo["sblocks"] * 256))
    L = trips + 8 + -(-geo["sblocks"] // 64) + 6 + 4          # fp64 additions on the longest chain, and var's three operations
    for ch, st in enumerate(o["stats"] if case.rules else []):
        if st is None:
            continue
        sums = part[ch, :geo["sblocks"]].sum(0)
        assert sums[0].item() == st["sums"][0], f"channel {ch}: masked count {sums[0].item()} != {st['sums'][0]}"
        for k in range(1, 5):
            err, bound = abs(sums[k].item() - st["sums"][k]), dhw * lm.D53 * st["terms"][k]
            record("intensity statistics (fp64 sums)", err, bound)
            assert err <= bound, f"channel {ch} sum {k}: err {err:.3e} > {bound:.3e}"
        mu, sd = coef[ch, 0].item(), coef[ch, 1].item()
        used = (1, 2) if st["masked_used"] else (3, 4)
        msq = st["sums"][used[1]] / st["n"]
        dvar = L * lm.D53 * (msq + st["mu"] ** 2)
        bmu = lm.U * abs(st["mu"]) + L * lm.D53 * st["terms"][used[0]] / st["n"]
        record("intensity mu", abs(mu - st["mu"]), bmu)
        assert abs(mu - st["mu"]) <= bmu, f"channel {ch}: mu {mu!r} against {st['mu']!r}"
        if st["sd"] == lm.f32(1e-6):
            assert sd == st["sd"], f"channel {ch}: sd {sd!r} is not eps"
        else:
            bsd = lm.U * st["sd"] + dvar / (2 * st["sd"]) * 1.001
            record("intensity sd", abs(sd - st["sd"]), bsd)
            assert abs(sd - st["sd"]) <= bsd, f"channel {ch}: sd {sd!r} against {st['sd']!r} (bound {bsd:.2e})"


def test_zz_print_the_worst_err_over_bound_per_family():
    """Not a limit: the table DESIGN.md records."""
    for fam in sorted(WORST):
        print(f"worst err / bound  {fam:45s} {WORST[fam]:.3f}")
