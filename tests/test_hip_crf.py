"""CRF-regularised entropy on the GPU: ``mmtta_crf_entropy_items`` (tiled and generic route) against the float64 restatement of
``crf_reference.py``, the bitwise properties (N items = N calls, two runs, inputs untouched, pad lanes) and the plugin
``crf_tta`` against a restatement of the oracle's adaptation loop with the loss swapped.

Tolerances of the kernel comparisons.  The fp32 run of the restatement sits, on exactly the inputs of these cases, at
3.2e-6 of the gradient's maximum from the float64 run and at 4.5e-8 relative in H and P (``test_crf_host.py``:
FP32_GRADIENT = 3.3e-6, FP32_LOSS = 5e-8).  fp32 gradients: max-norm error <= 4 x FP32_GRADIENT x max |reference gradient|
(the factor for another summation order and the hardware exponential); bf16 gradients: that plus 2^-8 |ref| per element (one
bf16 rounding is 2^-9 relative at the top of a binade and 2^-8 at its bottom, so these cases come to 99 % of their bound and
rest on the fp32 allowance, of which the kernel's fp32 error takes a few percent); ``loss``, ``entropy``, ``pairwise``: 1e-5 relative, the figure of the DiceCE sums test.

Shapes are the smallest at which a tile can go wrong, not the workload's: exactly one 4 x 8 x 32 tile, one voxel more in every
axis, (9, 10, 35), (1, 5, 70) and (3, 17, 4).  Every case runs N = 2 different volumes."""
import copy
import functools

import numpy as np
import pytest
import torch

from crf_reference import crf, crf_torch
from test_crf_host import (FP32_GRADIENT, GENERIC_C, GENERIC_R, GENERIC_SEED, GENERIC_SHAPES, N, SHAPES, case_seed,
                           generic_case_table, gpu_case_table, inputs)

pytestmark = pytest.mark.gpu

GRAD_TOL = 4.0 * FP32_GRADIENT
SUM_TOL = 1e-5


# ----------------------------------------------------------------------------- the shared references and the runner
@functools.lru_cache(maxsize=None)
def reference(shape, R, C, seed, bf16, conn, weight, sigma, softmax, form, present):
    """The float64 restatement of every item, computed once per case and shared (never written)."""
    l, x = inputs(shape, R, C, seed, bf16)
    out = [crf(l[n], x[n], conn, weight, sigma, softmax, form, present) for n in range(N)]
    for r in out:
        r["dlogits"].setflags(write=False)
    return out


def device_cl(a, dtype=torch.float32, ldc=None, owns=True, sentinel=float("nan")):
    """A channels-last device tensor [N,D,H,W,c] holding ``a`` in rows of ``ldc`` elements whose pad lanes hold ``sentinel``;
    ``owns``: the view is flagged as the owner of its pad lanes (what the pool's buffers are).  Returns (view, base)."""
    from multimodal_tta_amd import ops
    n, d, h, w, c = a.shape
    ldc = ops.row_pad(c, dtype) if ldc is None else ldc
    base = torch.full((n, d, h, w, ldc), sentinel, dtype=dtype, device="cuda")
    view = base[..., :c] if ldc != c else base
    view.copy_(torch.from_numpy(np.array(a)).to(dtype))
    if owns and ldc != c:
        view._mmtta_owns_pad = True
    return view, base


def run(l, x, conn, weight, sigma, softmax, form, present=None, xdtype=torch.float32, gdtype=torch.float32, ldc=None, owns=True):
    """One call on fresh buffers -> (dlogits [N,D,H,W,R] fp32, {loss, entropy, pairwise} [N], the tensors for further checks)."""
    from multimodal_tta_amd import ops
    zl, zl_base = device_cl(l, ldc=ldc, owns=owns)
    dl, dl_base = device_cl(np.zeros_like(l), dtype=gdtype, ldc=ldc, owns=owns)
    xd, xd_base = device_cl(x, dtype=xdtype) if x is not None else (None, None)
    n = l.shape[0]
    part = torch.full((ops.crf_partials(zl),), float("nan"), dtype=torch.float64, device="cuda")
    sums = {k: torch.full((n,), float("nan"), device="cuda") for k in ("loss", "entropy", "pairwise")}
    ops.crf_entropy_items(zl, xd, dl, part, sums["loss"], sums["entropy"], sums["pairwise"], connectivity=conn, weight=weight,
                          sigma=sigma, form=form, present=present, softmax=softmax)
    torch.cuda.synchronize()
    keep = dict(l=zl_base, dl=dl_base, x=xd_base)
    return dl.float().cpu().numpy(), {k: v.cpu().numpy() for k, v in sums.items()}, keep


def check(got, sums, ref, bf16_grad=False):
    """Hold one call's items to the restatement; returns the worst gradient error over its bound (printed by the callers)."""
    worst = 0.0
    for n, r in enumerate(ref):
        g = r["dlogits"]
        err = np.abs(got[n].astype(np.float64) - g)
        bound = GRAD_TOL * np.abs(g).max() + (2.0 ** -8 * np.abs(g) if bf16_grad else 0.0)
        worst = max(worst, float((err / bound).max()))
        for key, want in (("entropy", r["H"]), ("pairwise", r["P"]), ("loss", r["L"])):
            have = float(sums[key][n])
            assert abs(have - want) <= SUM_TOL * abs(want), f"item {n}: {key} {have!r} vs {want!r}"
    print(f"worst gradient error / bound = {worst:.3f}")
    assert worst <= 1.0, f"worst gradient error / bound = {worst:.3f}"
    return worst


# ----------------------------------------------------------------------------- the cases
CASES = gpu_case_table()


def test_the_cases_cover_what_they_should():
    for softmax in (False, True):
        mine = [c for c in CASES if c[0] == softmax]
        assert {c[1] for c in mine} == {"potts", "quadratic"} and {c[2] for c in mine} == {6, 18, 26}
        assert {c[3] for c in mine} == {0.0, 1.0}
        aff = [c for c in mine if c[3] > 0]
        assert {c[6] for c in aff} == {False, True} and {c[5] for c in aff} == {2, 4}
        for form in ("potts", "quadratic"):
            assert {c[2] for c in mine if c[1] == form} == {6, 18, 26}
    assert {c[4] for c in CASES} == {1, 3, 4}
    assert {c[7] for c in CASES if not c[0]} == {False, True} and not any(c[7] for c in CASES if c[0])
    assert {c[1] for c in CASES if c[7]} == {"potts", "quadratic"}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("softmax,form,conn,sigma,R,C,xbf,gbf", CASES)
def test_tiled_kernel_matches_the_float64_restatement(softmax, form, conn, sigma, R, C, xbf, gbf, shape):
    l, x = inputs(shape, R, C, case_seed(R, C), xbf)
    ref = reference(shape, R, C, case_seed(R, C), xbf, conn, 1.0, sigma, softmax, form, None)
    got, sums, keep = run(l, x, conn, 1.0, sigma, softmax, form, xdtype=torch.bfloat16 if xbf else torch.float32,
                          gdtype=torch.bfloat16 if gbf else torch.float32)
    check(got, sums, ref, bf16_grad=gbf)
    if R < 4:          # the view owns its pad lanes: a row is one whole store, pad lanes zero
        assert (keep["dl"][..., R:] == 0).all(), "pad lanes of `dlogits` are not zero"


@pytest.mark.parametrize("shape", GENERIC_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("softmax,form,conn,sigma,xbf", generic_case_table())
def test_generic_kernel_matches_the_float64_restatement(softmax, form, conn, sigma, xbf, shape):
    """R = 5, C = 6: rows of 8 elements, past the tiled route."""
    R, C = GENERIC_R, GENERIC_C
    l, x = inputs(shape, R, C, GENERIC_SEED, xbf)
    ref = reference(shape, R, C, GENERIC_SEED, xbf, conn, 1.0, sigma, softmax, form, None)
    got, sums, keep = run(l, x, conn, 1.0, sigma, softmax, form, xdtype=torch.bfloat16 if xbf else torch.float32)
    check(got, sums, ref)
    assert torch.isnan(keep["dl"][..., R:]).all(), "the generic route leaves pad lanes as they are"


@pytest.mark.parametrize("softmax", [False, True])
@pytest.mark.parametrize("form", ["potts", "quadratic"])
def test_generic_kernel_takes_thin_rows_the_tiled_route_cannot(form, softmax):
    """R = 3 in rows of 3 floats (no pad): not 16-byte rows, so the generic kernel runs."""
    shape, R, C = (5, 9, 33), 3, 4
    l, x = inputs(shape, R, C, case_seed(R, C), False)
    ref = reference(shape, R, C, case_seed(R, C), False, 26, 2.0, 1.0, softmax, form, None)
    got, sums, _ = run(l, x, 26, 2.0, 1.0, softmax, form, ldc=3)
    check(got, sums, ref)


@pytest.mark.parametrize("softmax,gbf", [(False, False), (False, True), (True, False)],
                         ids=["sigmoid-fp32", "sigmoid-bf16", "softmax-fp32"])          # (the softmax head writes fp32 gradients only)
def test_pad_lanes_of_views_that_do_not_own_them_are_preserved(softmax, gbf):
    shape, R, C = (5, 9, 33), 3, 4
    l, x = inputs(shape, R, C, case_seed(R, C), False)
    ref = reference(shape, R, C, case_seed(R, C), False, 26, 1.0, 1.0, softmax, "potts", None)
    got, sums, keep = run(l, x, 26, 1.0, 1.0, softmax, "potts", owns=False, gdtype=torch.bfloat16 if gbf else torch.float32)
    check(got, sums, ref, bf16_grad=gbf)
    assert torch.isnan(keep["dl"][..., R:]).all(), "a pad lane was written"


@pytest.mark.parametrize("softmax", [False, True])
@pytest.mark.parametrize("xbf", [False, True])
def test_a_masked_out_channel_does_not_enter_the_affinity(xbf, softmax):
    """Channel 2 holds large values; the mask leaves it out.  The result equals the restatement without that channel, and
    changing the channel's values changes no bit."""
    shape, R, C = (9, 10, 35), 3, 4
    l, x = inputs(shape, R, C, 31, xbf)
    x = x.copy()
    x[..., 2] *= 64.0          # (a power of two: still bf16-representable)
    present = (True, True, False, True)
    masked = [crf(l[n], x[n], 26, 1.0, 1.0, softmax, "potts", present) for n in range(N)]
    unmasked = [crf(l[n], x[n], 26, 1.0, 1.0, softmax, "potts") for n in range(N)]
    assert abs(masked[0]["P"] - unmasked[0]["P"]) > 1e-2 * masked[0]["P"], "the large channel makes no difference"
    xd = torch.bfloat16 if xbf else torch.float32
    got, sums, _ = run(l, x, 26, 1.0, 1.0, softmax, "potts", present=present, xdtype=xd)
    check(got, sums, masked)
    assert abs(float(sums["pairwise"][0]) - unmasked[0]["P"]) > SUM_TOL * unmasked[0]["P"]
    x2 = x.copy()
    x2[..., 2] = -3.0 * x2[..., 2] + 1.0
    again, sums2, _ = run(l, x2, 26, 1.0, 1.0, softmax, "potts", present=present, xdtype=xd)
    assert np.array_equal(got.view(np.int32), again.view(np.int32)), "the absent channel reached the gradient"
    for k in sums:
        assert np.array_equal(sums[k].view(np.int32), sums2[k].view(np.int32)), f"the absent channel reached `{k}`"


# ----------------------------------------------------------------------------- bitwise properties
@pytest.mark.parametrize("softmax,R,C,xbf,gbf", [(False, 3, 4, True, True), (False, 3, 4, False, False), (True, 3, 4, True, False),
                                                 (False, 5, 6, False, False), (True, 5, 6, False, False)],
                         ids=["tiled-bf16", "tiled", "tiled-softmax", "generic", "generic-softmax"])
def test_items_equal_calls_runs_repeat_and_inputs_stay(softmax, R, C, xbf, gbf):
    shape = (5, 9, 33)
    l, x = inputs(shape, R, C, 5, xbf)
    kw = dict(xdtype=torch.bfloat16 if xbf else torch.float32, gdtype=torch.bfloat16 if gbf else torch.float32)
    both, s_both, keep = run(l, x, 26, 1.5, 1.0, softmax, "potts", **kw)
    # the inputs, pad lanes included, hold the bits they held
    _, l_base_again = device_cl(l)
    _, x_base_again = device_cl(x, dtype=kw["xdtype"])
    bits = lambda t: t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    assert torch.equal(bits(keep["l"]), bits(l_base_again)), "`logits` was written"
    assert torch.equal(bits(keep["x"]), bits(x_base_again)), "`x` was written"
    again, s_again, _ = run(l, x, 26, 1.5, 1.0, softmax, "potts", **kw)
    assert np.array_equal(both.view(np.int32), again.view(np.int32)), "two runs differ"
    for k in s_both:
        assert np.array_equal(s_both[k].view(np.int32), s_again[k].view(np.int32)), f"two runs differ in `{k}`"
    for n in range(N):
        one, s_one, _ = run(l[n:n + 1], x[n:n + 1], 26, 1.5, 1.0, softmax, "potts", **kw)
        assert np.array_equal(one.view(np.int32), both[n:n + 1].view(np.int32)), f"item {n} differs from a call of its own"
        for k in s_both:
            assert s_one[k].view(np.int32)[0] == s_both[k].view(np.int32)[n], f"item {n}: `{k}` differs from a call of its own"


@pytest.mark.parametrize("R", [3, 5], ids=["tiled", "generic"])
def test_sigma_zero_reads_no_input_and_accepts_a_null_one(R):
    shape = (5, 9, 33)
    l, x = inputs(shape, R, 4, case_seed(R, 4), False)
    a, sa, _ = run(l, None, 18, 1.0, 0.0, False, "quadratic")
    b, sb, _ = run(l, x, 18, 1.0, 0.0, False, "quadratic")
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    for k in sa:
        assert np.array_equal(sa[k].view(np.int32), sb[k].view(np.int32))
    check(a, sa, reference(shape, R, 4, case_seed(R, 4), False, 18, 1.0, 0.0, False, "quadratic", None))


@pytest.mark.parametrize("softmax", [False, True])
@pytest.mark.parametrize("R,ldc", [(3, None), (5, None), (3, 3)], ids=["tiled", "generic", "generic-thin"])
def test_constant_logits_have_no_quadratic_term_and_the_entropy_gradient(R, ldc, softmax):
    """One item, the same logits in every voxel: every difference p_i - p_j is an exact 0, so ``pairwise`` is exactly 0 and the
    gradient is that of ``mmtta_entropy_loss_items``."""
    from multimodal_tta_amd import ops
    shape = (5, 9, 33)
    row = np.array([0.8, -1.7, 2.9, 0.3, -0.6], dtype=np.float32)[:R]
    l = np.broadcast_to(row, (1,) + shape + (R,)).copy()
    _, x = inputs(shape, R, 4, case_seed(R, 4), False)
    got, sums, _ = run(l, x[:1], 26, 4.0, 1.0, softmax, "quadratic", ldc=ldc)
    assert float(sums["pairwise"][0]) == 0.0
    assert sums["loss"].view(np.int32)[0] == sums["entropy"].view(np.int32)[0]
    zl, _ = device_cl(l, ldc=ldc)
    dl, _ = device_cl(np.zeros_like(l), ldc=ldc)
    part = torch.zeros(ops.entropy_partials_items(zl), dtype=torch.float64, device="cuda")
    loss = torch.zeros(1, device="cuda")
    ops.entropy_loss_items(zl, dl, part, loss, softmax=softmax)
    torch.cuda.synchronize()
    want = dl.cpu().numpy().astype(np.float64)
    assert np.abs(got - want).max() <= GRAD_TOL * np.abs(want).max()
    assert abs(float(sums["entropy"][0]) - float(loss[0])) <= SUM_TOL * float(loss[0])


def test_ops_crf_entropy_items_refuses_bad_arguments_on_the_device():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.ops import MmttaError
    l, x = inputs(SHAPES[0], 3, 4, 1, False)
    zl, _ = device_cl(l)
    dl, _ = device_cl(l)
    xd, _ = device_cl(x)
    part = torch.zeros(ops.crf_partials(zl), dtype=torch.float64, device="cuda")
    s = [torch.zeros(N, device="cuda") for _ in range(3)]
    kw = dict(connectivity=26, weight=1.0, sigma=1.0)
    with pytest.raises(MmttaError, match="aliased"):
        ops.crf_entropy_items(zl, xd, zl, part, *s, **kw)
    with pytest.raises(MmttaError, match="sigma > 0"):
        ops.crf_entropy_items(zl, None, dl, part, *s, **kw)
    with pytest.raises(MmttaError, match="channel_mask"):
        ops.crf_entropy_items(zl, xd, dl, part, *s, present=[False] * 4, **kw)
    with pytest.raises(MmttaError, match="partial"):
        ops.crf_entropy_items(zl, xd, dl, part[:3], *s, **kw)
    with pytest.raises(MmttaError, match="entropy must"):
        ops.crf_entropy_items(zl, xd, dl, part, s[0], s[1][:1], s[2], **kw)
    with pytest.raises(MmttaError, match="connectivity"):
        ops.crf_entropy_items(zl, xd, dl, part, *s, **dict(kw, connectivity=8))
    with pytest.raises(MmttaError, match="weight"):
        ops.crf_entropy_items(zl, xd, dl, part, *s, **dict(kw, weight=0.0))


# ----------------------------------------------------------------------------- the plugin
def crf_cfg(model_cfg, steps, weight=1.0, sigma=1.0, connectivity=26, form="potts", name="crf_tta", lr=1e-3, **method):
    from test_hip_tta import root_cfg
    cfg = root_cfg(model_cfg, steps=steps, lr=lr, **method)
    cfg["method"]["name"] = name
    cfg["method"]["crf"] = {"weight": weight, "sigma": sigma, "connectivity": connectivity, "form": form}
    return cfg


def adapt_reference(model, x, cfg, steps, softmax=False, missing=(), moddrop_p=0.0, moddrop_seed=0, masked_means=False,
                    affinity_sees_draws=False):
    """``oracle.adapt_volume``'s loop with the loss swapped for the torch L of ``crf_reference`` (the oracle's model,
    ``select_params``, optimizer factory and seeded dropout masks unchanged; episodic) -> logits and the per-step records.
    The affinity takes the run's base mask in every step: the dropout draws do not enter it.  ``masked_means``: the model is
    given the step's mask (deep fusion), and a branch absent in a step gets a zero gradient, as in ``oracle.adapt_volume``."""
    import oracle
    c = cfg["method"]["crf"]
    source = copy.deepcopy(model.state_dict())
    named = oracle.select_params(model, "all")
    opt = oracle.build_optimizer(named, cfg["training"])
    gen = torch.Generator().manual_seed(int(moddrop_seed)) if moddrop_p > 0.0 else None
    present = oracle.tta.modality_mask(x.shape[1], missing, 0.0, None)
    x_cl = x[0].permute(1, 2, 3, 0)          # the affinity reads the volume as staged: absent channels masked out, not zeroed
    rec = {"losses": [], "entropy": [], "pairwise": []}
    model.train()
    for _ in range(int(steps)):
        drawn = oracle.tta.modality_mask(x.shape[1], missing, moddrop_p, gen)
        xin = oracle.tta.apply_modality_mask(x, drawn)
        opt.zero_grad()
        z = model(xin, present=drawn) if masked_means else model(xin)
        x_step = xin[0].permute(1, 2, 3, 0) if affinity_sees_draws else x_cl          # (the wrong loop: see its one caller)
        L, H, P = crf_torch(z[0].permute(1, 2, 3, 0), x_step, c["connectivity"], c["weight"], c["sigma"], softmax, c["form"],
                            present)
        L.backward()
        if masked_means:
            for _, q in named:
                if q.grad is None:
                    q.grad = torch.zeros_like(q)
        opt.step()
        for k, v in (("losses", L), ("entropy", H), ("pairwise", P)):
            rec[k].append(float(v.item()))
    model.eval()
    with torch.no_grad():
        xin = oracle.tta.apply_modality_mask(x, present)
        logits = model(xin, present=present) if masked_means else model(xin)
    model.load_state_dict(source)
    return logits, rec


def plugin_run(name, cfg, xs, model_cfg=None):
    """Adapt the volumes ``xs`` (one call each) with a fresh plugin -> (plugin, [logits NCDHW on the host], [records])."""
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import SMALL, build_pair
    _, hip = build_pair(model_cfg or SMALL)
    plug = get_plugin(name)(cfg).setup(hip, "cuda")
    outs, results = [], []
    for x in xs:
        r = plug.adapt_volume(x.cuda())
        torch.cuda.synchronize()
        outs.append(plug.logits(r).cpu().clone())
        results.append({k: v.cpu().clone() for k, v in r.items() if k != "logits_cl"})
    return plug, outs, results


def records_close(res, rec):
    for key in ("losses", "entropy", "pairwise"):
        got = res[key].tolist()
        assert len(got) == len(rec[key])
        for t, (a, b) in enumerate(zip(got, rec[key])):
            assert abs(a - b) <= 1e-4 * abs(b) + 1e-6, f"step {t}: {key} {a} vs the reference loop's {b}"


def logits_close_to_float64(z_hip, ref_model, x, cfg, steps, **kw):
    """``test_hip_tta.logits_close``'s rule on the swapped loop: the HIP path sits as close to a float64 run as the fp32 run of
    the same loop does (x 3), or within 2e-3 of max |logits|."""
    z32, rec = adapt_reference(copy.deepcopy(ref_model), x, cfg, steps, **kw)
    z64, _ = adapt_reference(copy.deepcopy(ref_model).double(), x.double(), cfg, steps, **kw)
    scale = z64.abs().max().item()
    e_ref = (z32.double() - z64).abs().max().item() / scale
    e_hip = (z_hip.double() - z64).abs().max().item() / scale
    print(f"HIP vs fp64 loop {e_hip:.3e}; fp32 loop vs fp64 loop {e_ref:.3e}")
    assert e_hip <= max(2e-3, 3.0 * e_ref), f"HIP vs fp64 loop {e_hip:.3e}; fp32 loop vs fp64 loop {e_ref:.3e}"
    return rec


@pytest.mark.parametrize("form,sigma", [("potts", 0.0), ("quadratic", 1.0)])
def test_plugin_matches_the_oracle_loop_with_the_loss_swapped(form, sigma):
    from test_hip_tta import SMALL, build_pair, volume
    x = volume(0)[0]
    cfg = crf_cfg(SMALL, steps=3, weight=1.0, sigma=sigma, form=form, group=1)
    ref, _ = build_pair(SMALL)
    plug, outs, res = plugin_run("crf_tta", cfg, [x])
    assert type(plug).__name__ == "CrfRegularizedTTA" and plug.fused_update
    rec = logits_close_to_float64(outs[0], ref, x, cfg, 3)
    records_close(res[0], rec)
    print("pairwise per step:", res[0]["pairwise"].tolist())
    if sigma == 0.0:
        assert res[0]["pairwise"][-1] < res[0]["pairwise"][0], "the pairwise term did not decrease"
    for t in range(3):
        want = res[0]["entropy"][t].double() + 1.0 * res[0]["pairwise"][t].double()
        assert abs(float(res[0]["losses"][t]) - float(want)) <= 1e-6 * float(want)


def test_weight_zero_is_entmin_bit_for_bit():
    from test_hip_tta import SMALL, volume
    xs = [volume(0)[0], volume(1)[0]]
    cfg = crf_cfg(SMALL, steps=2, weight=0.0, group=1)
    _, ent, ent_res = plugin_run("entmin_tta", cfg, xs)
    _, got, res = plugin_run("crf_tta", cfg, xs)
    for a, b, ra, rb in zip(ent, got, ent_res, res):
        assert torch.equal(a, b) and torch.equal(ra["losses"], rb["losses"])
        assert torch.equal(rb["entropy"], rb["losses"]) and rb["pairwise"].tolist() == [0.0, 0.0]


def test_plugin_group_equals_one_at_a_time_and_graph_equals_eager():
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import SMALL, build_pair, volume
    G = 2
    vols = [volume(i)[0] for i in range(G)]
    keys = ("losses", "entropy", "pairwise")
    runs = {}
    for group, use_graph in ((G, True), (1, True), (G, False)):
        cfg = crf_cfg(SMALL, steps=3, group=group, tune_volumes=2, use_graph=use_graph)
        _, hip = build_pair(SMALL)
        plug = get_plugin("crf_tta")(cfg).setup(hip, "cuda")
        if group == G:
            r = plug.adapt_volume(torch.cat(vols).cuda())
            runs[(group, use_graph)] = (plug.logits(r).cpu(),) + tuple(r[k].cpu() for k in keys)
        else:
            rs = []
            for v in vols:          # (the results are views of the plugin's buffers: read before the next volume)
                r = plug.adapt_volume(v.cuda())
                rs.append((plug.logits(r).cpu(),) + tuple(r[k].cpu().clone() for k in keys))
            runs[(group, use_graph)] = (torch.cat([r[0] for r in rs]),) + tuple(torch.stack([r[i] for r in rs], 1)
                                                                                 for i in range(1, 4))
    assert runs[(G, True)][1].shape == (3, G) and (runs[(G, True)][3] > 0).all(), "the pairwise term is not in the run"
    for a, b in zip(runs[(G, True)], runs[(1, True)]):
        assert torch.equal(a, b), "grouped run differs from one volume at a time"
    for a, b in zip(runs[(G, True)], runs[(G, False)]):
        assert torch.equal(a, b), "graph replay differs from eager launches"


def test_bf16_precision_tracks_the_fp32_loop():
    """The bounds of ``test_bf16_precision_tracks_the_fp32_oracle`` at the reference's learning rate: per-step records within
    1e-2 relative, logits within 3e-2 of max |logits|, at most 1 % of the mask voxels differ, Dice within 2e-2."""
    import oracle
    from test_hip_tta import SMALL, build_pair, volume
    x, y = volume(5)
    cfg = crf_cfg(SMALL, steps=3, lr=1e-5, group=1, precision="bf16")
    ref, _ = build_pair(SMALL)
    z_ref, rec = adapt_reference(ref, x, cfg, 3)
    plug, outs, res = plugin_run("crf_tta", cfg, [x])
    for key in ("losses", "entropy", "pairwise"):
        for a, b in zip(res[0][key].tolist(), rec[key]):
            assert abs(a - b) <= 1e-2 * abs(b), (key, a, b)
    err = (outs[0] - z_ref).abs().max().item() / z_ref.abs().max().item()
    m_hip, m_ref = torch.sigmoid(outs[0]) >= 0.5, torch.sigmoid(z_ref) >= 0.5
    mism = (m_hip != m_ref).float().mean().item()
    d_ref, _, _ = oracle.binary_dice_iou(m_ref.to(torch.uint8), (y > 0.5).to(torch.uint8))
    d_hip, _, _ = oracle.binary_dice_iou(m_hip.to(torch.uint8), (y > 0.5).to(torch.uint8))
    ddice = (d_hip - d_ref).abs().max().item()
    print(f"bf16: logits rel err {err:.3e}, mask mismatch {mism:.3e}, dDice {ddice:.3e}")
    assert err > 1e-6, "bf16 path not taken"
    assert err < 3e-2 and mism <= 1e-2 and ddice <= 2e-2


def test_plugin_on_the_softmax_head():
    import oracle
    from test_hip_tta import SMALL, volume
    mcfg = dict(SMALL, num_classes=4)
    cfg = crf_cfg(mcfg, steps=2, group=1)
    cfg["training"]["criterion"]["softmax"] = True
    cfg["training"]["criterion"]["sigmoid"] = False
    x = volume(1, R=4)[0]
    torch.manual_seed(42)
    ref = oracle.UNet(mcfg)
    plug, outs, res = plugin_run("crf_tta", cfg, [x], model_cfg=mcfg)
    assert plug.softmax
    rec = logits_close_to_float64(outs[0], ref, x, cfg, 2, softmax=True)
    records_close(res[0], rec)


def test_plugin_on_the_deep_fusion_network():
    """The staged [n,D,H,W,M] volume of the deep-fusion net is the affinity input."""
    import oracle
    from multimodal_tta_amd.models import MultimodalUNetDeepFusion
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import volume
    dcfg = dict(name="unet_multimodal_deepfusion", num_modalities=4, num_classes=3, spatial_dims=3,
                channels=[4, 8, 16, 32, 64], strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)
    cfg = crf_cfg(dcfg, steps=2, group=1, lr=1e-4)
    x = volume(1)[0]
    torch.manual_seed(42)
    ref = oracle.MultimodalUNetDeepFusion(dcfg)
    hip = MultimodalUNetDeepFusion(dcfg)
    hip.load_state_dict(ref.state_dict())
    plug = get_plugin("crf_tta")(cfg).setup(hip, "cuda")
    r = plug.adapt_volume(x.cuda())
    torch.cuda.synchronize()
    _, rec = adapt_reference(ref, x, cfg, 2)
    records_close({k: r[k].cpu() for k in ("losses", "entropy", "pairwise")}, rec)
    assert torch.isfinite(plug.logits(r)).all()


DEEPFUSION = dict(name="unet_multimodal_deepfusion", num_modalities=4, num_classes=3, spatial_dims=3,
                  channels=[4, 8, 16, 32, 64], strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)


def test_deep_fusion_with_modality_dropout_keeps_the_draws_out_of_the_affinity():
    """The deep-fusion runtime does not mask on load: the loop re-stages the volume every step with that step's draw zeroed.
    The stencil reads a copy staged under the base mask, so the records are those of the loop whose affinity never sees a
    draw - and not those of a loop whose affinity reads the re-staged volume."""
    import oracle
    from multimodal_tta_amd.models import MultimodalUNetDeepFusion
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import volume
    steps, missing, p, seed = 3, [1], 0.5, 0
    gen = torch.Generator().manual_seed(seed)
    base = oracle.tta.modality_mask(4, missing, 0.0, None)
    draws = [oracle.tta.modality_mask(4, missing, p, gen) for _ in range(steps)]
    assert any(d != base for d in draws), "no step drops a modality: the case shows nothing"
    cfg = crf_cfg(DEEPFUSION, steps=steps, group=1, lr=1e-4, missing_modalities=missing,
                  moddrop={"enabled": True, "p": p, "seed": seed})
    x = volume(1)[0]
    torch.manual_seed(42)
    ref = oracle.MultimodalUNetDeepFusion(DEEPFUSION)
    hip = MultimodalUNetDeepFusion(DEEPFUSION)
    hip.load_state_dict(ref.state_dict())
    plug = get_plugin("crf_tta")(cfg).setup(hip, "cuda")
    assert not getattr(plug.rt, "input_mask_on_load", False)
    r = plug.adapt_volume(x.cuda())
    torch.cuda.synchronize()
    got = {k: r[k].cpu() for k in ("losses", "entropy", "pairwise")}
    _, rec = adapt_reference(ref, x, cfg, steps, missing=missing, moddrop_p=p, moddrop_seed=seed, masked_means=True)
    records_close(got, rec)
    assert torch.isfinite(plug.logits(r)).all()
    # the loop whose affinity reads the re-staged volume (the draw's channel zeroed: no difference there) gives another
    # pairwise term in the first step that drops a modality: the comparison above tells the two apart
    t = next(i for i, d in enumerate(draws) if d != base)
    _, wrong = adapt_reference(ref, x, cfg, t + 1, missing=missing, moddrop_p=p, moddrop_seed=seed, masked_means=True,
                               affinity_sees_draws=True)
    assert abs(wrong["pairwise"][t] - rec["pairwise"][t]) > 1e-2 * rec["pairwise"][t]
    assert abs(float(got["pairwise"][t]) - wrong["pairwise"][t]) > 1e-2 * rec["pairwise"][t]


def test_plugin_masks_the_missing_modality_out_of_the_affinity():
    from test_hip_tta import SMALL, build_pair, volume
    x = volume(3)[0]
    cfg = crf_cfg(SMALL, steps=2, group=1, missing_modalities=[1])
    ref, _ = build_pair(SMALL)
    _, outs, res = plugin_run("crf_tta", cfg, [x])
    rec = logits_close_to_float64(outs[0], ref, x, cfg, 2, missing=[1])
    records_close(res[0], rec)
    # with the absent channel in the affinity the first step's pairwise term is another one: the case shows something
    with torch.no_grad():
        z = ref(x * torch.tensor([1.0, 0.0, 1.0, 1.0]).view(1, -1, 1, 1, 1))
        _, _, P_all = crf_torch(z[0].permute(1, 2, 3, 0), x[0].permute(1, 2, 3, 0), 26, 1.0, 1.0, False, "potts", None)
    assert abs(float(P_all) - rec["pairwise"][0]) > 1e-3 * rec["pairwise"][0]


def test_plugin_with_modality_dropout_keeps_the_base_mask_in_the_affinity():
    """The seeded per-step draws mask the network's input; the affinity keeps the run's base mask."""
    from test_hip_tta import SMALL, build_pair, volume
    x = volume(4)[0]
    drop = dict(missing=[1], moddrop_p=0.5, moddrop_seed=7)
    cfg = crf_cfg(SMALL, steps=3, group=1, missing_modalities=[1], moddrop={"enabled": True, "p": 0.5, "seed": 7})
    ref, _ = build_pair(SMALL)
    _, outs, res = plugin_run("crf_tta", cfg, [x])
    rec = logits_close_to_float64(outs[0], ref, x, cfg, 3, **drop)
    records_close(res[0], rec)


def test_seg_tta_eval_runs_the_method_and_returns_finite_metrics():
    import math
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    from test_hip_tta import SMALL, build_pair
    cfg = crf_cfg(SMALL, steps=2, group=1, lanes=1)
    cfg["dataset"]["synthetic"]["num_volumes"] = 2
    cfg["dataset"]["synthetic"]["shape"] = [32, 32, 32]
    loader = get_dataset_builder("brats")(cfg).get_loader("test")
    _, hip = build_pair(SMALL)
    strat = get_evaluation_strategy("seg_tta_eval")(cfg)
    got = strat.evaluate_epoch(hip, loader, torch.device("cuda"))
    assert type(strat.plugin).__name__ == "CrfRegularizedTTA"
    assert {"et_dc", "tc_dc", "wt_dc", "avg_dc", "miou", "loss"} <= set(got)
    assert all(math.isfinite(float(v)) for v in got.values()), got
    assert 0.0 <= got["avg_dc"] <= 1.0 and got["loss"] > 0.0
