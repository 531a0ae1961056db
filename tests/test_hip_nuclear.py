"""Entropy minus a regional nuclear norm on the GPU: ``mmtta_nuclear_entropy_items`` (fast and generic route) against the float64
restatement of ``nuclear_reference.py``, the bitwise properties (N items = N calls, two runs, inputs untouched, pad lanes, a
box's gradient depends on its own voxels only) and the plugin ``bnm_tta`` against a restatement of the oracle's adaptation
loop with the loss swapped.

Tolerances of the kernel comparisons.  The fp32 run of the restatement sits, on exactly the inputs of these cases, at 9.4e-6
of the gradient's maximum from the float64 run and at 1.1e-7 relative in H and N (``test_nuclear_host.py``:
FP32_GRADIENT = 1.0e-5, FP32_LOSS = 1.3e-7).  fp32 gradients: max-norm error <= 4 x FP32_GRADIENT x max |reference gradient|
(the factor of ``test_hip_crf.py``, for another summation order and the hardware exponential); bf16 gradients: that plus
2^-8 |ref| per element (one bf16 rounding); ``loss``, ``entropy``, ``nuclear``: 1e-5 relative, the project's figure for sums.

Shapes are the smallest at which the passes can go wrong, not the workload's: (5, 9, 33), (1, 5, 70), (3, 17, 4) - ragged
against the boxes [4,4,8], [2,3,5], [1,1,1], [0,4,0] and more than one workgroup for the whole-volume box -, (16, 16, 32)
with boxes of [16,16,16] (several workgroups per box) and (3, 3, 3) with boxes of [2,2,2] (a one-voxel corner box: fewer rows
than classes on the softmax head); three cases run R = 16, the most the entry point takes.  Every case runs N = 2 different
volumes, eps = 1e-4."""
import copy
import functools

import numpy as np
import pytest
import torch

from nuclear_reference import boxes, nuclear, nuclear_torch
from test_nuclear_host import EPS, FP32_GRADIENT, N, case_id, case_seed, gpu_case_table, inputs

pytestmark = pytest.mark.gpu

GRAD_TOL = 4.0 * FP32_GRADIENT
SUM_TOL = 1e-5
KEYS = ("losses", "entropy", "nuclear")


# ----------------------------------------------------------------------------- the shared references and the runner
@functools.lru_cache(maxsize=None)
def reference(shape, R, seed, block, weight, entropy_weight, softmax):
    """The float64 restatement of every item, computed once per case and shared (never written)."""
    l = inputs(shape, R, seed)
    out = [nuclear(l[n], block, weight, entropy_weight, EPS, softmax) for n in range(N)]
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


def run(l, block, weight, entropy_weight, softmax, gdtype=torch.float32, ldc=None, owns=True, eps=EPS):
    """One call on fresh buffers -> (dlogits [N,D,H,W,R] fp32, {loss, entropy, nuclear} [N], the tensors for further checks)."""
    from multimodal_tta_amd import ops
    zl, zl_base = device_cl(l, ldc=ldc, owns=owns)
    dl, dl_base = device_cl(np.zeros_like(l), dtype=gdtype, ldc=ldc, owns=owns)
    n = l.shape[0]
    scratch = torch.full((ops.nuclear_scratch(zl, block, softmax),), float("nan"), dtype=torch.float64, device="cuda")
    sums = {k: torch.full((n,), float("nan"), device="cuda") for k in ("loss", "entropy", "nuclear")}
    ops.nuclear_entropy_items(zl, dl, scratch, sums["loss"], sums["entropy"], sums["nuclear"], block=list(block), weight=weight,
                              entropy_weight=entropy_weight, eps=eps, softmax=softmax)
    torch.cuda.synchronize()
    keep = dict(l=zl_base, dl=dl_base)
    return dl.float().cpu().numpy(), {k: v.cpu().numpy() for k, v in sums.items()}, keep


def check(got, sums, ref, bf16_grad=False):
    """Hold one call's items to the restatement; returns the worst gradient error over its bound."""
    worst = 0.0
    for n, r in enumerate(ref):
        g = r["dlogits"]
        err = np.abs(got[n].astype(np.float64) - g)
        bound = GRAD_TOL * np.abs(g).max() + (2.0 ** -8 * np.abs(g) if bf16_grad else 0.0)
        worst = max(worst, float((err / bound).max()))
        for key, want in (("entropy", r["H"]), ("nuclear", r["N"]), ("loss", r["L"])):
            have = float(sums[key][n])
            print(f"item {n}: {key} {have!r} vs {want!r} ({abs(have - want) / abs(want):.2e} relative)")
            assert abs(have - want) <= SUM_TOL * abs(want), f"item {n}: {key} {have!r} vs {want!r}"
    print(f"worst gradient error / bound = {worst:.3f}")
    assert worst <= 1.0, f"worst gradient error / bound = {worst:.3f}"
    return worst


# ----------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("case", gpu_case_table(), ids=case_id)
def test_kernels_match_the_float64_restatement(case):
    shape, block, softmax, R, gbf, ew, w, ldc = case
    seed = case_seed(shape, R)
    l = inputs(shape, R, seed)
    ref = reference(shape, R, seed, block, w, ew, softmax)
    got, sums, keep = run(l, block, w, ew, softmax, gdtype=torch.bfloat16 if gbf else torch.float32, ldc=ldc)
    check(got, sums, ref, bf16_grad=gbf)
    if R > 4:          # the generic route leaves pad lanes as they are
        assert torch.isnan(keep["dl"][..., R:]).all(), "the generic route wrote a pad lane"
    elif R < 4 and ldc is None:          # the view owns its pad lanes: a row is one whole store, pad lanes zero
        assert (keep["dl"][..., R:] == 0).all(), "pad lanes of `dlogits` are not zero"


@pytest.mark.parametrize("softmax,gbf", [(False, False), (False, True), (True, False)],
                         ids=["sigmoid-fp32", "sigmoid-bf16", "softmax-fp32"])          # (the softmax head writes fp32 gradients only)
def test_pad_lanes_of_views_that_do_not_own_them_are_preserved(softmax, gbf):
    shape, R, block = (5, 9, 33), 3, (4, 4, 8)
    seed = case_seed(shape, R)
    l = inputs(shape, R, seed)
    ref = reference(shape, R, seed, block, 1.0, 1.0, softmax)
    got, sums, keep = run(l, block, 1.0, 1.0, softmax, owns=False, gdtype=torch.bfloat16 if gbf else torch.float32)
    check(got, sums, ref, bf16_grad=gbf)
    assert torch.isnan(keep["dl"][..., R:]).all(), "a pad lane was written"


# ----------------------------------------------------------------------------- bitwise properties
@pytest.mark.parametrize("softmax,R,gbf,block", [(False, 3, True, (4, 4, 8)), (False, 3, False, (0, 0, 0)), (True, 4, False, (2, 3, 5)),
                                                 (False, 5, False, (4, 4, 8)), (True, 5, False, (0, 0, 0))],
                         ids=["fast-bf16", "fast", "fast-softmax", "generic", "generic-softmax"])
def test_items_equal_calls_runs_repeat_and_inputs_stay(softmax, R, gbf, block):
    shape = (5, 9, 33)
    l = inputs(shape, R, 5)
    kw = dict(gdtype=torch.bfloat16 if gbf else torch.float32)
    both, s_both, keep = run(l, block, 1.5, 1.0, softmax, **kw)
    _, l_base_again = device_cl(l)          # the inputs, pad lanes included, hold the bits they held
    assert torch.equal(keep["l"].view(torch.int32), l_base_again.view(torch.int32)), "`logits` was written"
    again, s_again, _ = run(l, block, 1.5, 1.0, softmax, **kw)
    assert np.array_equal(both.view(np.int32), again.view(np.int32)), "two runs differ"
    for k in s_both:
        assert np.array_equal(s_both[k].view(np.int32), s_again[k].view(np.int32)), f"two runs differ in `{k}`"
    for n in range(N):
        one, s_one, _ = run(l[n:n + 1], block, 1.5, 1.0, softmax, **kw)
        assert np.array_equal(one.view(np.int32), both[n:n + 1].view(np.int32)), f"item {n} differs from a call of its own"
        for k in s_both:
            assert s_one[k].view(np.int32)[0] == s_both[k].view(np.int32)[n], f"item {n}: `{k}` differs from a call of its own"


@pytest.mark.parametrize("softmax,R", [(False, 3), (True, 4), (False, 5), (True, 5)],
                         ids=["fast", "fast-softmax", "generic", "generic-softmax"])
def test_a_box_reads_its_own_voxels_only(softmax, R):
    """Other logits in one box change the gradient there, and no bit of ``dlogits`` in any other box."""
    shape, block = (5, 9, 33), (4, 4, 8)
    l = inputs(shape, R, 9)
    a, _, _ = run(l, block, 2.0, 1.0, softmax)
    bx = boxes(shape, block)
    sl = bx[7]          # an inner box: z 0:4, y 4:8, x 16:24
    l2 = l.copy()
    l2[(slice(None),) + sl] = -0.5 * l2[(slice(None),) + sl] + 0.25
    b, _, _ = run(l2, block, 2.0, 1.0, softmax)
    inside = np.zeros(shape, dtype=bool)
    inside[sl] = True
    assert not np.array_equal(a[:, inside], b[:, inside]), "the changed box kept its gradient"
    assert np.array_equal(a[:, ~inside].view(np.int32), b[:, ~inside].view(np.int32)), "another box's gradient changed"


@pytest.mark.parametrize("softmax", [False, True])
@pytest.mark.parametrize("R,ldc", [(3, None), (5, None), (3, 3)], ids=["fast", "generic", "generic-thin"])
def test_constant_logits_give_tents_gradient_plus_the_nuclear_part(R, ldc, softmax):
    """One item, the same logits in every voxel: every box has rank 1.  With ``entropy_weight: 1`` the gradient is that of
    ``mmtta_entropy_loss_items`` minus ``weight`` times the restatement's nuclear part, and ``nuclear`` is the restatement's."""
    from multimodal_tta_amd import ops
    shape, block, weight = (5, 9, 33), (4, 4, 8), 2.5
    row = np.array([0.8, -1.7, 2.9, 0.3, -0.6], dtype=np.float32)[:R]
    l = np.broadcast_to(row, (1,) + shape + (R,)).copy()
    ref = nuclear(l[0], block, weight, 1.0, EPS, softmax)
    got, sums, _ = run(l, block, weight, 1.0, softmax, ldc=ldc)
    zl, _ = device_cl(l, ldc=ldc)
    dl, _ = device_cl(np.zeros_like(l), ldc=ldc)
    part = torch.zeros(ops.entropy_partials_items(zl), dtype=torch.float64, device="cuda")
    loss = torch.zeros(1, device="cuda")
    ops.entropy_loss_items(zl, dl, part, loss, softmax=softmax)
    torch.cuda.synchronize()
    want = dl.cpu().numpy().astype(np.float64)[0] - weight * ref["dnuclear"]
    assert np.abs(got[0] - want).max() <= GRAD_TOL * np.abs(want).max()
    assert abs(float(sums["entropy"][0]) - float(loss[0])) <= SUM_TOL * float(loss[0])
    assert abs(float(sums["nuclear"][0]) - ref["N"]) <= SUM_TOL * ref["N"]


def test_ops_nuclear_entropy_items_refuses_bad_arguments_on_the_device():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.ops import MmttaError
    l = inputs((5, 9, 33), 3, 1)
    zl, _ = device_cl(l)
    dl, _ = device_cl(l)
    block = [4, 4, 8]
    scratch = torch.zeros(ops.nuclear_scratch(zl, block), dtype=torch.float64, device="cuda")
    assert scratch.numel() == N * 30 * (10 + 3 + 1 + 3)
    s = [torch.zeros(N, device="cuda") for _ in range(3)]
    with pytest.raises(MmttaError, match="aliased"):
        ops.nuclear_entropy_items(zl, zl, scratch, *s, block=block, weight=1.0)
    with pytest.raises(MmttaError, match="scratch"):
        ops.nuclear_entropy_items(zl, dl, scratch[:-1], *s, block=block, weight=1.0)
    with pytest.raises(MmttaError, match="scratch"):          # (sized for boxes of [4,4,8]: the whole-volume box needs less, [1,1,1] more)
        ops.nuclear_entropy_items(zl, dl, scratch, *s, block=[1, 1, 1], weight=1.0)
    with pytest.raises(MmttaError, match="scratch"):
        ops.nuclear_entropy_items(zl, dl, scratch.float(), *s, block=block, weight=1.0)
    with pytest.raises(MmttaError, match="entropy must"):
        ops.nuclear_entropy_items(zl, dl, scratch, s[0], s[1][:1], s[2], block=block, weight=1.0)
    with pytest.raises(MmttaError, match="nuclear must"):
        ops.nuclear_entropy_items(zl, dl, scratch, s[0], s[1], s[2][:1], block=block, weight=1.0)
    with pytest.raises(MmttaError, match="weight"):
        ops.nuclear_entropy_items(zl, dl, scratch, *s, block=block, weight=0.0)
    with pytest.raises(MmttaError, match="eps"):
        ops.nuclear_entropy_items(zl, dl, scratch, *s, block=block, weight=1.0, eps=0.5)
    with pytest.raises(MmttaError, match="block"):
        ops.nuclear_entropy_items(zl, dl, scratch, *s, block=[4, 4, -8], weight=1.0)


# ----------------------------------------------------------------------------- the plugin
# (on the sigmoid head of the small network H and N both start near 0.64: the default weight of these runs keeps L = H - weight N
# away from 0, where a relative bound on `losses` would ask for more than its two terms can give)
def bnm_cfg(model_cfg, steps, weight=2.5, entropy_weight=1.0, block=(0, 0, 0), eps=EPS, lr=1e-3, **method):
    from test_hip_tta import root_cfg
    cfg = root_cfg(model_cfg, steps=steps, lr=lr, **method)
    cfg["method"]["name"] = "bnm_tta"
    cfg["method"]["bnm"] = {"weight": weight, "entropy_weight": entropy_weight, "block": list(block), "eps": eps}
    return cfg


def adapt_reference(model, x, cfg, steps, softmax=False, missing=(), masked_means=False):
    """``oracle.adapt_volume``'s loop with the loss swapped for the torch L of ``nuclear_reference`` (the oracle's model,
    ``select_params`` and optimizer factory unchanged; episodic) -> logits and the per-step records."""
    import oracle
    c = cfg["method"]["bnm"]
    source = copy.deepcopy(model.state_dict())
    named = oracle.select_params(model, "all")
    opt = oracle.build_optimizer(named, cfg["training"])
    present = oracle.tta.modality_mask(x.shape[1], missing, 0.0, None)
    xin = oracle.tta.apply_modality_mask(x, present)
    rec = {k: [] for k in KEYS}
    model.train()
    for _ in range(int(steps)):
        opt.zero_grad()
        z = model(xin, present=present) if masked_means else model(xin)
        L, H, Nn = nuclear_torch(z[0].permute(1, 2, 3, 0), c["block"], c["weight"], c["entropy_weight"], c["eps"], softmax)
        L.backward()
        opt.step()
        for k, v in (("losses", L), ("entropy", H), ("nuclear", Nn)):
            rec[k].append(float(v.item()))
    model.eval()
    with torch.no_grad():
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
    for key in KEYS:
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


def losses_are_the_weighted_sum(res, entropy_weight, weight):
    for t in range(len(res["losses"])):
        want = entropy_weight * res["entropy"][t].double() - weight * res["nuclear"][t].double()
        assert abs(float(res["losses"][t]) - float(want)) <= 1e-6, (t, float(res["losses"][t]), float(want))


@pytest.mark.parametrize("block,entropy_weight,weight", [((0, 0, 0), 1.0, 2.5), ((8, 8, 8), 0.0, 1.0)], ids=["whole", "8x8x8"])
def test_plugin_matches_the_oracle_loop_with_the_loss_swapped(block, entropy_weight, weight):
    from test_hip_tta import SMALL, build_pair, volume
    x = volume(0)[0]
    cfg = bnm_cfg(SMALL, steps=3, weight=weight, entropy_weight=entropy_weight, block=block, group=1)
    ref, _ = build_pair(SMALL)
    plug, outs, res = plugin_run("bnm_tta", cfg, [x])
    assert type(plug).__name__ == "NuclearNormTTA" and plug.fused_update
    rec = logits_close_to_float64(outs[0], ref, x, cfg, 3)
    records_close(res[0], rec)
    print("nuclear per step:", res[0]["nuclear"].tolist())
    assert res[0]["nuclear"][-1] > res[0]["nuclear"][0], "the nuclear term did not increase"
    losses_are_the_weighted_sum(res[0], entropy_weight, weight)


def test_weight_zero_is_entmin_bit_for_bit():
    from test_hip_tta import SMALL, volume
    xs = [volume(0)[0], volume(1)[0]]
    cfg = bnm_cfg(SMALL, steps=2, weight=0.0, group=1)
    _, ent, ent_res = plugin_run("entmin_tta", cfg, xs)
    _, got, res = plugin_run("bnm_tta", cfg, xs)
    for a, b, ra, rb in zip(ent, got, ent_res, res):
        assert torch.equal(a, b) and torch.equal(ra["losses"], rb["losses"])
        assert torch.equal(rb["entropy"], rb["losses"]) and rb["nuclear"].tolist() == [0.0, 0.0]


def test_plugin_group_equals_one_at_a_time_and_graph_equals_eager():
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import SMALL, build_pair, volume
    G = 2
    vols = [volume(i)[0] for i in range(G)]
    runs = {}
    for group, use_graph in ((G, True), (1, True), (G, False)):
        cfg = bnm_cfg(SMALL, steps=3, block=(16, 16, 16), group=group, tune_volumes=2, use_graph=use_graph)
        _, hip = build_pair(SMALL)
        plug = get_plugin("bnm_tta")(cfg).setup(hip, "cuda")
        if group == G:
            r = plug.adapt_volume(torch.cat(vols).cuda())
            runs[(group, use_graph)] = (plug.logits(r).cpu(),) + tuple(r[k].cpu() for k in KEYS)
        else:
            rs = []
            for v in vols:          # (the results are views of the plugin's buffers: read before the next volume)
                r = plug.adapt_volume(v.cuda())
                rs.append((plug.logits(r).cpu(),) + tuple(r[k].cpu().clone() for k in KEYS))
            runs[(group, use_graph)] = (torch.cat([r[0] for r in rs]),) + tuple(torch.stack([r[i] for r in rs], 1)
                                                                                 for i in range(1, 4))
    assert runs[(G, True)][1].shape == (3, G) and (runs[(G, True)][3] > 0).all(), "the nuclear term is not in the run"
    for a, b in zip(runs[(G, True)], runs[(1, True)]):
        assert torch.equal(a, b), "grouped run differs from one volume at a time"
    for a, b in zip(runs[(G, True)], runs[(G, False)]):
        assert torch.equal(a, b), "graph replay differs from eager launches"
    with pytest.raises(ValueError, match="method.group"):
        plug.adapt_volume(torch.cat(vols + vols[:1]).cuda())


def test_bf16_precision_tracks_the_fp32_loop():
    """The bounds of ``test_bf16_precision_tracks_the_fp32_oracle`` at the reference's learning rate: per-step records within
    1e-2 relative, logits within 3e-2 of max |logits|, at most 1 % of the mask voxels differ, Dice within 2e-2."""
    import oracle
    from test_hip_tta import SMALL, build_pair, volume
    x, y = volume(5)
    cfg = bnm_cfg(SMALL, steps=3, lr=1e-5, group=1, precision="bf16")
    ref, _ = build_pair(SMALL)
    z_ref, rec = adapt_reference(ref, x, cfg, 3)
    plug, outs, res = plugin_run("bnm_tta", cfg, [x])
    for key in KEYS:
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
    cfg = bnm_cfg(mcfg, steps=2, weight=1.0, block=(8, 8, 8), group=1)
    cfg["training"]["criterion"]["softmax"] = True
    cfg["training"]["criterion"]["sigmoid"] = False
    x = volume(1, R=4)[0]
    torch.manual_seed(42)
    ref = oracle.UNet(mcfg)
    plug, outs, res = plugin_run("bnm_tta", cfg, [x], model_cfg=mcfg)
    assert plug.softmax
    rec = logits_close_to_float64(outs[0], ref, x, cfg, 2, softmax=True)
    records_close(res[0], rec)
    losses_are_the_weighted_sum(res[0], 1.0, 1.0)          # (H starts near log 4, N near 0.5)


def test_plugin_on_the_deep_fusion_network():
    import oracle
    from multimodal_tta_amd.models import MultimodalUNetDeepFusion
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import volume
    dcfg = dict(name="unet_multimodal_deepfusion", num_modalities=4, num_classes=3, spatial_dims=3,
                channels=[4, 8, 16, 32, 64], strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)
    cfg = bnm_cfg(dcfg, steps=2, block=(16, 16, 16), group=1, lr=1e-4)
    x = volume(1)[0]
    torch.manual_seed(42)
    ref = oracle.MultimodalUNetDeepFusion(dcfg)
    hip = MultimodalUNetDeepFusion(dcfg)
    hip.load_state_dict(ref.state_dict())
    plug = get_plugin("bnm_tta")(cfg).setup(hip, "cuda")
    r = plug.adapt_volume(x.cuda())
    torch.cuda.synchronize()
    _, rec = adapt_reference(ref, x, cfg, 2)
    records_close({k: r[k].cpu() for k in KEYS}, rec)
    assert torch.isfinite(plug.logits(r)).all()


def test_plugin_with_a_missing_modality():
    from test_hip_tta import SMALL, build_pair, volume
    x = volume(3)[0]
    cfg = bnm_cfg(SMALL, steps=2, group=1, missing_modalities=[1])
    ref, _ = build_pair(SMALL)
    _, outs, res = plugin_run("bnm_tta", cfg, [x])
    rec = logits_close_to_float64(outs[0], ref, x, cfg, 2, missing=[1])
    records_close(res[0], rec)


def test_seg_tta_eval_runs_the_method_and_returns_finite_metrics():
    import math
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    from test_hip_tta import SMALL, build_pair
    cfg = bnm_cfg(SMALL, steps=2, group=1, lanes=1)
    cfg["dataset"]["synthetic"]["num_volumes"] = 2
    cfg["dataset"]["synthetic"]["shape"] = [32, 32, 32]
    loader = get_dataset_builder("brats")(cfg).get_loader("test")
    _, hip = build_pair(SMALL)
    strat = get_evaluation_strategy("seg_tta_eval")(cfg)
    got = strat.evaluate_epoch(hip, loader, torch.device("cuda"))
    assert type(strat.plugin).__name__ == "NuclearNormTTA"
    assert {"et_dc", "tc_dc", "wt_dc", "avg_dc", "miou", "loss"} <= set(got)
    assert all(math.isfinite(float(v)) for v in got.values()), got
    assert 0.0 <= got["avg_dc"] <= 1.0
