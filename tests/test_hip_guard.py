"""The do-no-harm guard on the GPU: ``mmtta_guard_counts`` against NumPy and against the evaluator's own count kernel,
``mmtta_guard_select`` against ``guard.decide`` on hand-written counts, the plugins with the guard inert and with a forced
fall-back (bit for bit against the unguarded plugin), and the evaluator's paired source / adapted keys.

Every comparison here is exact: the counts are integers, the select copies bits, and the plugin statements are identities
between two runs of the same launches.  Shapes are the smallest at which a route can go wrong: 5 x 6 x 7 (less than one
2048-voxel chunk, no multiple of a wave) and 16^3 (two chunks) for the counts, 4 x 4 x 8 for the select, 4 x 32^3 for the
plugins."""
import copy
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 3
Q = 1 << 16
BIG = (1 << 31) - 1
PAD_REF, PAD_OUT = 111.0, 222.0          # what the pad lanes of the reference / of the logits hold in the select tests


def device_cl(a, ldc=None, owns=True, sentinel=float("nan")):
    """A channels-last fp32 device tensor [N,D,H,W,c] holding ``a`` in rows of ``ldc`` elements whose pad lanes hold
    ``sentinel``; ``owns``: the view is flagged as the owner of its pad lanes (what the pool's buffers are) -> (view, base)."""
    n, d, h, w, c = a.shape
    ldc = (c + 3) // 4 * 4 if ldc is None else ldc
    base = torch.full((n, d, h, w, ldc), sentinel, dtype=torch.float32, device="cuda")
    view = base[..., :c] if ldc != c else base
    view.copy_(torch.from_numpy(np.array(a)))
    if owns and ldc != c:
        view._mmtta_owns_pad = True
    return view, base


# ----------------------------------------------------------------------------- counts
@functools.lru_cache(maxsize=None)
def logit_pair(shape, R, threshold, seed):
    """Two logit tensors of N items, every value at least 1e-3 away from logit(threshold) - where fp32 and float64 agree on
    the side whatever the rounding of expf - and, at threshold 0.5, a plane of exact zeros in each (another plane in each):
    sigmoid(0) = 0.5 >= 0.5 is foreground.  Returned with their NumPy counts [N,R,3]; never written."""
    rng = np.random.default_rng(seed)
    edge = math.log(threshold / (1.0 - threshold))
    pair = []
    for _ in range(2):
        side = rng.choice([-1.0, 1.0], (N,) + tuple(shape) + (R,))
        z = (edge + side * (1e-3 + np.abs(rng.normal(0.0, 3.0, side.shape)))).astype(np.float32)
        assert (np.abs(z.astype(np.float64) - edge) >= 0.99e-3).all()
        pair.append(z)
    if threshold == 0.5:
        pair[0][:, 0] = 0.0
        pair[1][:, :, 0] = 0.0
    ms, ma = (z.astype(np.float64) >= edge for z in pair)
    counts = np.stack([ms.sum(axis=(1, 2, 3)), ma.sum(axis=(1, 2, 3)), (ms & ma).sum(axis=(1, 2, 3))], axis=-1).astype(np.int64)
    for z in pair:
        z.setflags(write=False)
    return pair[0], pair[1], counts


COUNT_CASES = [(3, 4, True), (4, 4, True), (1, 4, True), (5, 8, True), (3, 3, False), (3, 4, False)]      # R, row width, owns pad


@pytest.mark.parametrize("threshold", [0.5, 0.3])
@pytest.mark.parametrize("shape", [(5, 6, 7), (16, 16, 16)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("R,ldc,owns", COUNT_CASES)
def test_counts_equal_numpy_and_the_evaluators_kernel(R, ldc, owns, shape, threshold):
    from multimodal_tta_amd import ops
    zr, za, want = logit_pair(shape, R, threshold, 10 * R + ldc)
    ref, _ = device_cl(zr, ldc, owns)
    ada, _ = device_cl(za, ldc, owns)
    counts = torch.full((N, R, 3), -7, dtype=torch.int64, device="cuda")          # the call zeroes it
    ops.guard_counts(ref, ada, threshold, counts)
    got = counts.cpu().numpy()
    assert (got == want).all(), (got.tolist(), want.tolist())
    # s and a are the `pred` column of mmtta_mask_dice_counts on the same logits
    label = torch.zeros((N, R) + tuple(shape), dtype=torch.float32, device="cuda")
    for k, z in enumerate((ref, ada)):
        dc = torch.zeros((N, R, 3), dtype=torch.int64, device="cuda")
        ops.mask_dice_counts(z, label, threshold, dc, None, logits_channels_last=True)
        assert torch.equal(dc[..., 1], counts[..., k])
    # N items in one call equal N calls
    for n in range(N):
        one = torch.full((1, R, 3), -7, dtype=torch.int64, device="cuda")
        ops.guard_counts(ref[n:n + 1], ada[n:n + 1], threshold, one)
        assert torch.equal(one[0], counts[n])


def test_counts_of_infinite_and_nan_logits():
    from multimodal_tta_amd import ops
    shape = (2, 3, 5)
    zr = np.full((1,) + shape + (3,), np.inf, dtype=np.float32)
    za = np.full((1,) + shape + (3,), -np.inf, dtype=np.float32)
    zr[..., 1] = -np.inf
    za[..., 2] = np.inf
    zr[0, 0, 0, 0, 2] = np.nan          # a NaN logit is background, as for the evaluator
    ref, _ = device_cl(zr)
    ada, _ = device_cl(za)
    counts = torch.zeros((1, 3, 3), dtype=torch.int64, device="cuda")
    for thr in (0.5, 0.3, 0.999):
        ops.guard_counts(ref, ada, thr, counts)
        assert counts.cpu().tolist() == [[[30, 0, 0], [0, 0, 0], [29, 30, 29]]]


def test_counts_refuse_unsupported_layouts_before_any_launch():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.ops import MmttaError
    zr, za, _ = logit_pair((5, 6, 7), 3, 0.5, 34)
    ref, _ = device_cl(zr)
    ada, _ = device_cl(za)
    counts = torch.full((N, 3, 3), -7, dtype=torch.int64, device="cuda")
    with pytest.raises(MmttaError, match="status -2"):
        ops.guard_counts(ref.to(torch.bfloat16), ada.to(torch.bfloat16), 0.5, counts)
    wide = torch.zeros((1, 2, 2, 2, 17), dtype=torch.float32, device="cuda")
    with pytest.raises(MmttaError, match="status -2"):
        ops.guard_counts(wide, wide.clone(), 0.5, torch.full((1, 17, 3), -7, dtype=torch.int64, device="cuda"))
    with pytest.raises(MmttaError, match="unit stride"):          # no channels-last view at all
        ops.guard_counts(ref.permute(0, 4, 1, 2, 3), ada.permute(0, 4, 1, 2, 3), 0.5,
                         torch.full((N, 7, 3), -7, dtype=torch.int64, device="cuda"))
    with pytest.raises(MmttaError, match="row width"):
        ops.guard_counts(ref, device_cl(za, 8)[0], 0.5, counts)
    with pytest.raises(MmttaError, match="threshold"):
        ops.guard_counts(ref, ada, 1.0, counts)
    with pytest.raises(MmttaError, match="counts"):
        ops.guard_counts(ref, ada, 0.5, counts[:1])
    torch.cuda.synchronize()
    assert (counts == -7).all(), "a refused call wrote its output"


# ----------------------------------------------------------------------------- select
SHAPE_S = (4, 4, 8)


def _rule(agree=0.0, grow=0.0, shrink=0.0, m=0, scope="volume"):
    from multimodal_tta_amd.guard import GuardRule
    return GuardRule(int(round(agree * Q)), int(round(grow * Q)), int(round(shrink * Q)), m, scope)


# (rule arguments, counts [N][R=3] of (s, a, i)): each clause at and one past its boundary, the extremes, mixed batches
SELECT_CASES = [
    (dict(agree=0.5), [[(10, 6, 4)] * 3, [(10, 6, 3), (8, 8, 8), (8, 8, 8)], [(8, 8, 8), (8, 8, 8), (10, 7, 4)]]),
    (dict(agree=0.5, m=11), [[(10, 6, 0)] * 3, [(11, 6, 0), (1, 1, 1), (1, 1, 1)], [(1, 1, 1), (6, 11, 0), (1, 1, 1)]]),
    (dict(grow=4.0), [[(5, 21, 5), (5, 20, 5), (5, 20, 5)], [(5, 20, 5)] * 3, [(5, 20, 5), (5, 20, 5), (5, 21, 5)]]),
    (dict(grow=4.0, m=10), [[(0, 41, 0), (0, 40, 0), (0, 40, 0)], [(5, 40, 5)] * 3, [(5, 41, 5), (0, 0, 0), (0, 0, 0)]]),
    (dict(shrink=4.0), [[(21, 5, 5), (20, 5, 5), (20, 5, 5)], [(20, 5, 5)] * 3, [(20, 5, 5), (21, 5, 5), (20, 5, 5)]]),
    (dict(shrink=4.0, m=10), [[(41, 0, 0), (40, 0, 0), (40, 0, 0)], [(40, 0, 0)] * 3, [(0, 0, 0), (0, 0, 0), (41, 3, 0)]]),
    (dict(agree=1.0, grow=1024.0, shrink=1024.0), [[(BIG, BIG, BIG - 1), (BIG, BIG, BIG), (0, 0, 0)], [(BIG, BIG, BIG)] * 3,
                                                     [(BIG // 1024, BIG // 1024 * 1024 + 1, BIG // 1024), (0, 0, 0), (1, 1, 1)]]),
    (dict(agree=1.0, grow=1024.0, shrink=1024.0), [[(BIG, BIG, BIG)] * 3, [(0, 0, 0)] * 3,
                                                     [(BIG // 1024, BIG // 1024 * 1024, BIG // 1024)] * 3]),      # nothing fails
    (dict(), [[(100, 1, 0)] * 3, [(1, 100, 0)] * 3, [(50, 50, 0)] * 3]),                                            # the monitor
    (dict(agree=0.5, grow=4.0, shrink=4.0, m=64), [[(1000, 100, 100)] * 3, [(63, 0, 0), (0, 63, 0), (63, 63, 0)],
                                                     [(500, 500, 100), (500, 500, 500), (0, 0, 0)]]),                # the shipped numbers
    (dict(agree=1.0), [[(5, 5, 4)] * 3, [(5, 5, 5), (5, 5, 5), (6, 5, 5)], [(1, 0, 0), (0, 0, 0), (0, 0, 0)]]),    # every item fails
]


@functools.lru_cache(maxsize=None)
def select_inputs(R):
    rng = np.random.default_rng(50 + R)
    zr = rng.normal(0.0, 3.0, (N,) + SHAPE_S + (R,)).astype(np.float32)
    zl = rng.normal(0.0, 3.0, (N,) + SHAPE_S + (R,)).astype(np.float32)
    zr.setflags(write=False)
    zl.setflags(write=False)
    return zr, zl


@pytest.mark.parametrize("scope", ["volume", "region"])
@pytest.mark.parametrize("R,ldc,owns", [(3, 4, True), (3, 4, False), (4, 4, True), (1, 4, True), (5, 8, True), (3, 3, False)])
@pytest.mark.parametrize("case", range(len(SELECT_CASES)))
def test_select_follows_decide_and_copies_bits(case, R, ldc, owns, scope):
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.guard import decide
    kw, rows = SELECT_CASES[case]
    rule = _rule(scope=scope, **kw)
    rows = [[vol[r % 3] for r in range(R)] for vol in rows]          # the case's three regions, cycled over R
    want = decide(rows, rule)
    zr, zl = select_inputs(R)
    ref, ref_base = device_cl(zr, ldc, owns, PAD_REF)
    lg, lg_base = device_cl(zl, ldc, owns, PAD_OUT)
    before = lg_base.clone()
    counts = torch.tensor(rows, dtype=torch.int64, device="cuda")
    flags = torch.full((N, R), -7, dtype=torch.int32, device="cuda")
    ops.guard_select(counts, rule, ref, lg, flags)
    torch.cuda.synchronize()
    assert flags.cpu().tolist() == want
    assert torch.equal(ref_base.cpu(), device_cl(zr, ldc, owns, PAD_REF)[1].cpu()), "the reference was written"
    bits = lambda t: t.contiguous().view(torch.int32)
    whole_rows = scope == "volume" and ldc == 4 and (R == 4 or owns)          # one 16-byte store per failing row
    for n in range(N):
        if not any(want[n]):          # a passing item: bit-identical, pad lanes included
            assert torch.equal(bits(lg_base[n]), bits(before[n])), f"item {n} passed and was written"
            continue
        for r in range(ldc):
            got, was = bits(lg_base[n, ..., r]), bits(before[n, ..., r])
            if r < R and want[n][r]:
                assert torch.equal(got, bits(ref_base[n, ..., r])), f"item {n} channel {r} is not the reference's"
            elif r >= R and whole_rows:
                assert torch.equal(got, bits(ref_base[n, ..., r])), f"item {n} pad lane {r}: the row is one store"
            else:
                assert torch.equal(got, was), f"item {n} lane {r} changed"


def test_the_select_cases_cover_what_they_should():
    from multimodal_tta_amd.guard import decide
    per_scope = {s: [decide(rows, _rule(scope=s, **kw)) for kw, rows in SELECT_CASES] for s in ("volume", "region")}
    assert [[1, 1, 1], [0, 0, 0], [1, 1, 1]] in per_scope["volume"]          # items 0 and 2 fail, item 1 passes
    assert any(f == [[0, 0, 0]] * 3 for f in per_scope["volume"]) and any(f == [[1, 1, 1]] * 3 for f in per_scope["volume"])
    assert any(any(0 < sum(v) < 3 for v in f) for f in per_scope["region"])          # only the failing channel
    for k in ("agree", "grow", "shrink"):
        assert any(set(kw) - {"m"} == {k} for kw, _ in SELECT_CASES)          # each clause alone


def test_select_refuses_bad_arguments_on_the_device():
    from multimodal_tta_amd import _lib, ops
    from multimodal_tta_amd.ops import MmttaError
    zr, zl = select_inputs(3)
    ref, _ = device_cl(zr)
    lg, base = device_cl(zl)
    before = base.clone()
    counts = torch.full((N, 3, 3), 5, dtype=torch.int64, device="cuda")
    flags = torch.full((N, 3), -7, dtype=torch.int32, device="cuda")
    with pytest.raises(MmttaError, match="aliased"):
        ops.guard_select(counts, _rule(agree=1.0), ref, ref, flags)
    with pytest.raises(MmttaError, match="row width"):
        ops.guard_select(counts, _rule(agree=1.0), device_cl(zr, 8)[0], lg, flags)
    with pytest.raises(MmttaError, match="max_growth_q16"):
        ops.guard_select(counts, _lib.GuardRule(0, 5, 0, 0, 0, 0), ref, lg, flags)
    with pytest.raises(MmttaError, match="fallback"):
        ops.guard_select(counts, _rule(agree=1.0), ref, lg, flags.to(torch.int64))
    torch.cuda.synchronize()
    assert (flags == -7).all() and torch.equal(base.view(torch.int32), before.view(torch.int32))


# ----------------------------------------------------------------------------- the plugins
INERT = dict(enable=True, min_agreement=0.0, max_growth=0.0, max_shrink=0.0, min_voxels=0, scope="volume", threshold=None)
FORCED = dict(INERT, min_agreement=1.0)          # any flipped voxel of any region returns the volume
HOT = 2e-2                                       # a learning rate at which three steps move the mask
WIDE = [32, 64, 128, 256, 512]
DEEP = dict(name="unet_multimodal_deepfusion", num_modalities=4, num_classes=3, spatial_dims=3, channels=[4, 8, 16, 32, 64],
            strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)


def base_cfg(name, model_cfg, steps, lr, **method):
    from test_hip_tta import root_cfg
    cfg = root_cfg(model_cfg, steps=steps, lr=lr, **method)
    cfg["method"]["name"] = name
    if name == "sar_tta":
        cfg["method"]["sar"] = {"e_margin": 0.8, "rho": 0.05}
    if name == "lame_tta":
        cfg["method"]["lame"] = {"iterations": 3, "weight": 1.0, "sigma": 1.0, "connectivity": 26}
    if name == "memo_tta":
        cfg["method"]["memo"] = {"mirror_axes": ["w"], "ensemble": True}
    if name == "innorm_tta":
        cfg["method"]["innorm"] = {"lr": 1e-2, "gamma": False, "bound": {"log_scale": 0.7, "shift": 1.0, "log_gamma": 0.7}}
    if name == "window_tta":
        cfg["method"]["window"] = {"roi": [32, 32, 32]}
    return cfg


def guarded(cfg, block):
    cfg = copy.deepcopy(cfg)
    cfg["method"]["guard"] = dict(block)
    return cfg


def build_model(model_cfg):
    import oracle
    from multimodal_tta_amd.models import MultimodalUNetDeepFusion
    from test_hip_tta import build_pair
    if model_cfg["name"] != "unet_multimodal_deepfusion":
        return build_pair(model_cfg)[1]
    torch.manual_seed(42)
    ref = oracle.MultimodalUNetDeepFusion(model_cfg)
    hip = MultimodalUNetDeepFusion(model_cfg)
    hip.load_state_dict(ref.state_dict())
    return hip


def run(cfg, calls, steps=None):
    """A fresh plugin of ``cfg`` on a fresh model with the fixed weights, one ``adapt_volume`` per entry of ``calls`` ->
    the results, every tensor cloned (the plugin's buffers are reused by the next call)."""
    from multimodal_tta_amd.registry import get_plugin
    plug = get_plugin(cfg["method"]["name"])(cfg).setup(build_model(cfg["model"]), "cuda")
    out = []
    for x in calls:
        r = plug.adapt_volume(x.cuda()) if steps is None else plug.adapt_volume(x.cuda(), steps=steps)
        torch.cuda.synchronize()
        out.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()})
    return out


def counts_of(reference, logits, threshold=0.5):
    from multimodal_tta_amd import ops
    n, r = logits.shape[0], logits.shape[-1]
    c = torch.zeros((n, r, 3), dtype=torch.int64, device="cuda")
    ops.guard_counts(reference, logits, threshold, c)
    return c


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def vol(i, shape=(32, 32, 32)):
    from test_hip_tta import volume
    return volume(i, shape=shape)[0]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_an_inert_guard_changes_nothing_and_counts_the_two_predictions(precision):
    from test_hip_tta import SMALL
    mcfg = dict(SMALL, channels=WIDE) if precision == "bf16" else SMALL
    cfg = base_cfg("entmin_tta", mcfg, 2, HOT, group=1, precision=precision)
    xs = [vol(0), vol(1)]
    plain, source, on = run(cfg, xs), run(cfg, xs, steps=0), run(guarded(cfg, INERT), xs)
    for p, s, g in zip(plain, source, on):
        assert same_bits(g["losses"], p["losses"]) and same_bits(g["logits_cl"], p["logits_cl"])
        assert same_bits(g["guard_reference_cl"], s["logits_cl"])
        assert g["guard_fallback"].dtype == torch.int32 and g["guard_fallback"].cpu().tolist() == [[0, 0, 0]]
        assert g["guard_counts"].dtype == torch.int64
        assert torch.equal(g["guard_counts"], counts_of(s["logits_cl"], p["logits_cl"]))
        assert set(g) - set(p) == {"guard_counts", "guard_fallback", "guard_reference_cl"}


FALLBACK_CASES = [("entmin_tta", "unet", "fp32"), ("sar_tta", "unet", "fp32"), ("lame_tta", "unet", "fp32"),
                  ("memo_tta", "unet", "fp32"), ("innorm_tta", "unet", "fp32"), ("window_tta", "unet", "fp32"),
                  ("entmin_tta", "deepfusion", "fp32"), ("entmin_tta", "unet", "bf16")]


@pytest.mark.parametrize("name,model,precision", FALLBACK_CASES)
def test_a_forced_fallback_returns_the_steps_0_prediction_bit_for_bit(name, model, precision):
    from test_hip_tta import SMALL
    mcfg = DEEP if model == "deepfusion" else dict(SMALL, channels=WIDE) if precision == "bf16" else SMALL
    cfg = base_cfg(name, mcfg, 3, HOT, group=1, precision=precision)
    x = vol(2, (32, 48, 32)) if name == "window_tta" else vol(2)
    source = run(cfg, [x], steps=0)[0]
    got = run(guarded(cfg, FORCED), [x])[0]
    s, a, i = got["guard_counts"].cpu().unbind(-1)
    flips = int((s + a - 2 * i).sum())
    print(f"{name} {model} {precision}: s, a, i = {got['guard_counts'].cpu().tolist()}, flips {flips}")
    assert flips > 0, "the adapted mask is the source's: the learning rate moved nothing and the case shows nothing"
    assert got["guard_fallback"].cpu().tolist() == [[1, 1, 1]]
    assert same_bits(got["logits_cl"], source["logits_cl"]), "the returned logits are not the steps = 0 prediction"
    assert same_bits(got["guard_reference_cl"], source["logits_cl"])
    assert tuple(got["logits_cl"].shape[1:4]) == tuple(x.shape[2:])          # (window_tta: at the volume's extents)
    assert len(got["losses"]) == 3


OTHER_PLUGINS = {
    "eata_tta": ("eata", {"e_margin": 0.8, "fisher_alpha": 0.0, "fisher": {"volumes": 2, "path": None}}),
    "deyo_tta": ("deyo", {"e_margin": 0.8, "e_margin0": 0.6, "plpd_threshold": 0.05, "patches": [2, 2, 2], "seed": 0}),
    "crf_tta": ("crf", {"weight": 1.0, "sigma": 1.0, "connectivity": 26, "form": "potts"}),
    "bnm_tta": ("bnm", {"weight": 2.5, "entropy_weight": 1.0, "block": [0, 0, 0], "eps": 1e-6}),
    "modcons_tta": ("modcons", {"subsets": "leave_one_out", "weight": 1.0, "entropy_weight": 1.0, "detach": True}),
    "biasfield_tta": ("biasfield", {"lr": 1e-2, "order": 2, "anchor": "min", "l2": 0.0, "bound": {"gain": 0.7, "field": 0.2}}),
    "cotta_tta": ("cotta", {"mirror_axes": ["w"], "alpha": 0.9, "restore_p": 0.2, "seed": 0}),
    "petal_tta": ("petal", {"mirror_axes": ["w"], "alpha": 0.9, "quantile": 0.2}),
    "memo_tta": ("memo", {"mirror_axes": ["w"], "ensemble": False}),
}


@pytest.mark.parametrize("name", sorted(OTHER_PLUGINS))
def test_the_other_plugins_take_the_guard_through_the_shared_loop(name):
    """Every plugin registered beyond those above: the inert guard leaves its records and logits as they are, its reference
    is its own ``steps = 0`` prediction, and a forced fall-back returns it."""
    from test_hip_tta import SMALL
    section, block = OTHER_PLUGINS[name]
    cfg = base_cfg(name, SMALL, 2, HOT, group=1, episodic=True)
    cfg["method"][section] = copy.deepcopy(block)
    x = vol(5)
    plain, source, on = run(cfg, [x])[0], run(cfg, [x], steps=0)[0], run(guarded(cfg, INERT), [x])[0]
    for k, v in plain.items():
        assert (same_bits(on[k].float(), v.float()) if torch.is_tensor(v) else on[k] == v), f"{name}: `{k}` differs under the inert guard"
    assert same_bits(on["guard_reference_cl"], source["logits_cl"]) and int(on["guard_fallback"].sum()) == 0
    assert torch.equal(on["guard_counts"], counts_of(source["logits_cl"], plain["logits_cl"]))
    s, a, i = on["guard_counts"].cpu().unbind(-1)
    assert int((s + a - 2 * i).sum()) > 0, "the adapted mask is the source's: the case shows nothing"
    back = run(guarded(cfg, FORCED), [x])[0]
    assert same_bits(back["logits_cl"], source["logits_cl"]) and back["guard_fallback"].cpu().tolist() == [[1, 1, 1]]


def test_scope_region_returns_the_failing_channel_only():
    from multimodal_tta_amd.guard import decide, parse_guard
    from test_hip_tta import SMALL
    cfg = base_cfg("entmin_tta", SMALL, 3, HOT, group=1)
    x = vol(3)
    plain, source = run(cfg, [x])[0], run(cfg, [x], steps=0)[0]
    counts = counts_of(source["logits_cl"], plain["logits_cl"])
    s, a, i = counts.cpu()[0].unbind(-1)
    agreement = [2 * int(i[r]) / max(1, int(s[r] + a[r])) for r in range(3)]
    cut = sorted(agreement)[1]          # between the regions: the one(s) below it fail, the rest pass
    block = dict(INERT, min_agreement=float(np.nextafter(np.float32(cut), np.float32(0))), scope="region")
    gcfg = guarded(cfg, block)
    want = decide(counts, parse_guard(gcfg).rule)
    got = run(gcfg, [x])[0]
    print("agreement", agreement, "flags", want)
    assert 0 < sum(want[0]) < 3, "no region or every region fails: the case shows nothing"
    assert got["guard_fallback"].cpu().tolist() == want and torch.equal(got["guard_counts"], counts)
    for r in range(3):
        src = source if want[0][r] else plain
        assert same_bits(got["logits_cl"][..., r], src["logits_cl"][..., r])


def test_a_group_equals_one_at_a_time_and_graph_equals_eager():
    from test_hip_tta import SMALL
    G = 3
    vols = [vol(i) for i in range(G)]
    runs = {}
    for group, use_graph in ((G, True), (1, True), (G, False)):
        cfg = guarded(base_cfg("entmin_tta", SMALL, 3, HOT, group=group, tune_volumes=4, use_graph=use_graph), FORCED)
        rs = run(cfg, [torch.cat(vols)] if group == G else vols)
        runs[(group, use_graph)] = tuple(torch.cat([r[k] for r in rs]) for k in ("logits_cl", "guard_counts", "guard_fallback")) + \
            ((rs[0]["losses"] if group == G else torch.stack([r["losses"] for r in rs], 1)),)
    s, a, i = runs[(G, True)][1].unbind(-1)
    assert ((s + a - 2 * i).sum(-1) > 0).all() and (runs[(G, True)][2] == 1).all(), "the fall-back is not in the run"
    for a_, b_ in zip(runs[(G, True)], runs[(1, True)]):
        assert torch.equal(a_, b_), "grouped run differs from one volume at a time"
    for a_, b_ in zip(runs[(G, True)], runs[(G, False)]):
        assert torch.equal(a_, b_), "graph replay differs from eager launches"
    # the monitor on the same runs: the adapted logits come back, with the same counts
    mon = run(guarded(base_cfg("entmin_tta", SMALL, 3, HOT, group=G, tune_volumes=4), INERT), [torch.cat(vols)])[0]
    assert torch.equal(mon["guard_counts"], runs[(G, True)][1]) and int(mon["guard_fallback"].sum()) == 0
    assert not same_bits(mon["logits_cl"], runs[(G, True)][0])


def test_steps_0_never_falls_back_under_the_shipped_thresholds():
    from multimodal_tta_amd.guard import DEFAULTS
    from test_hip_tta import SMALL
    cfg = base_cfg("entmin_tta", SMALL, 3, HOT, group=1)
    x = vol(1)
    source = run(cfg, [x], steps=0)[0]
    for block in (dict(DEFAULTS, enable=True), FORCED):
        got = run(guarded(cfg, block), [x], steps=0)[0]
        s, a, i = got["guard_counts"].cpu().unbind(-1)
        assert torch.equal(s, a) and torch.equal(a, i) and int(s.sum()) > 0
        assert int(got["guard_fallback"].sum()) == 0 and same_bits(got["logits_cl"], source["logits_cl"])


def test_missing_modalities_and_modality_dropout_use_the_base_mask_twice():
    from test_hip_tta import SMALL
    x = vol(4)
    for extra in (dict(missing_modalities=[1]), dict(missing_modalities=[1], moddrop={"enabled": True, "p": 0.5, "seed": 3})):
        cfg = base_cfg("entmin_tta", SMALL, 3, HOT, group=1, **extra)
        plain, source, on = run(cfg, [x])[0], run(cfg, [x], steps=0)[0], run(guarded(cfg, INERT), [x])[0]
        assert same_bits(on["logits_cl"], plain["logits_cl"]) and same_bits(on["losses"], plain["losses"])
        assert same_bits(on["guard_reference_cl"], source["logits_cl"])
        back = run(guarded(cfg, FORCED), [x])[0]
        assert same_bits(back["logits_cl"], source["logits_cl"]) and int(back["guard_fallback"].sum()) == 3


# ----------------------------------------------------------------------------- the evaluator
REGIONS = ("et", "tc", "wt")


@functools.lru_cache(maxsize=None)
def evaluated(block, steps, postprocess):
    """One pass of ``seg_tta_eval`` over 4 synthetic volumes, 2 lanes x group 2 -> (metrics, per-volume table)."""
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    from test_hip_tta import SMALL, build_pair
    cfg = base_cfg("entmin_tta", SMALL, steps, HOT, group=2, lanes=2, tune_volumes=4)
    if block is not None:
        cfg["method"]["guard"] = dict(block)
    cfg["dataset"]["synthetic"]["num_volumes"] = 4
    cfg["dataset"]["synthetic"]["shape"] = [32, 32, 32]
    if postprocess:
        cfg["evaluation"].setdefault("postprocess", {})
        cfg["evaluation"]["postprocess"].update(enable=True, min_voxels=64, keep_largest=True, nesting=["ET", "TC", "WT"])
    loader = get_dataset_builder("brats")(cfg).get_loader("test")
    strat = get_evaluation_strategy("seg_tta_eval")(cfg)
    got = strat.evaluate_epoch(build_pair(SMALL)[1], loader, torch.device("cuda"))
    assert strat.lanes == 2 and strat.group == 2 and strat.last_table.shape[0] == 4
    return got, strat.last_table.clone()


def frozen(block):
    return tuple(sorted(block.items(), key=lambda kv: kv[0]))


def evaluated_with(block, steps, postprocess=False):
    m, t = evaluated(None if block is None else frozen(block), steps, postprocess)
    return dict(m), t


def test_evaluator_with_the_guard_inert_adds_the_source_keys_and_moves_nothing():
    off, t_off = evaluated_with(None, 3)
    on, t_on = evaluated_with(INERT, 3)
    src, t_src = evaluated_with(None, 0)
    assert set(off) < set(on) and t_on.shape[1] == t_off.shape[1] + 15
    for k, v in off.items():
        assert on[k] == v, (k, on[k], v)          # every existing key, exactly
    assert torch.equal(t_on[:, :t_off.shape[1]], t_off)
    pairs = [k for k in src if k.endswith("_dc")]
    assert {"et_dc", "tc_dc", "wt_dc", "avg_dc"} <= set(pairs) and any(k.startswith("dom/") for k in pairs)
    for k in pairs:
        assert on[k[:-3] + "_src_dc"] == src[k], (k, on[k[:-3] + "_src_dc"], src[k])
    R = 3
    for r, name in enumerate(REGIONS):
        valid = t_off[:, 3 + 2 * R + r] > 0.5
        assert torch.equal(valid, t_src[:, 3 + 2 * R + r] > 0.5) and int(valid.sum()) > 0
        d, s = t_off[valid, 3 + r], t_src[valid, 3 + r]
        total = 0.0
        for v in (d - s).tolist():          # (the volumes in index order, as the accumulator adds them)
            total += v
        gain = total / int(valid.sum())
        assert on[f"{name}_dc_gain"] == gain, (name, on[f"{name}_dc_gain"], gain)
        # ... which is the difference of the two tables' means up to the rounding of float64 sums of four numbers
        assert abs(gain - (float(d.mean()) - float(s.mean()))) <= 4 * 2.0 ** -52
        assert on[f"{name}_harmed"] == float((d < s).sum() / valid.sum())
        assert on[f"{name}_guard_fallback"] == 0.0 and on[f"{name}_guard_flips"] > 0.0
        assert 0.0 < on[f"{name}_guard_agreement"] < 1.0
    assert any(on[f"{n}_dc_gain"] != 0.0 for n in REGIONS), "adaptation changed no Dice: the case shows nothing"


def test_evaluator_with_a_forced_fallback_scores_the_source_prediction():
    on, _ = evaluated_with(FORCED, 3)
    src, _ = evaluated_with(None, 0)
    for k in [k for k in src if k.endswith("_dc")]:
        assert on[k] == on[k[:-3] + "_src_dc"] == src[k], k
    for k in on:
        if k.endswith("_guard_fallback"):
            assert on[k] == 1.0, k
        if k.endswith("_harmed") or k.endswith("_dc_gain"):
            assert on[k] == 0.0, k
    assert on["miou"] == src["miou"]


def test_the_source_dice_goes_through_the_same_post_processing():
    on, _ = evaluated_with(INERT, 3, True)
    src, _ = evaluated_with(None, 0, True)
    raw, _ = evaluated_with(None, 0)
    off, _ = evaluated_with(None, 3, True)
    for k, v in off.items():
        assert on[k] == v, k
    pairs = [k for k in src if k.endswith("_dc")]
    for k in pairs:
        assert on[k[:-3] + "_src_dc"] == src[k], (k, on[k[:-3] + "_src_dc"], src[k])
    assert any(src[k] != raw[k] for k in pairs), "the filter removed nothing from the source masks: the case shows nothing"
