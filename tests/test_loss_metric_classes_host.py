"""The case tables of tests/loss_metric_classes.py without a GPU: every case reaches the launch class it names, the float64
restatements agree with torch.optim / the oracle, the conditions that keep the GPU comparisons of
tests/test_hip_loss_metric_classes.py honest hold for the chosen shapes and seeds (each bound catches the mistake it is there
for), and the C entry points refuse bad arguments by status code before they launch anything."""
import ctypes as C

import numpy as np
import pytest
import torch

import loss_metric_classes as lm
import oracle
from multimodal_tta_amd import _lib

INVALID, UNSUPPORTED = -1, -2
ids = lambda cases: [c.name for c in cases]


def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


# ============================================================================= mask + Dice counts
@pytest.mark.parametrize("case", lm.DICE_CASES, ids=ids(lm.DICE_CASES))
def test_dice_case_reaches_its_class(case):
    n, d, h, w = case.shape
    geo = lm.dice_geometry(case.R, d * h * w)
    bad = {k: (geo[k], v) for k, v in case.want if geo[k] != v}
    assert not bad, f"{case.name} ({case.klass}): (got, wanted) = {bad}; launch {geo}"


def test_dice_table_covers_the_launch_classes():
    geo = {c.name: lm.dice_geometry(c.R, c.shape[1] * c.shape[2] * c.shape[3]) for c in lm.DICE_CASES}
    assert {c.R for c in lm.DICE_CASES} == {1, 2, 3, 4, 5, 8, 129, 256}
    assert {g["rp"] for g in geo.values()} == {1, 2, 4, 8, 256}
    assert any(g["nvl"] == 1 and g["capped"] and g["trips"] > 1 for g in geo.values())
    assert any(g["nvl"] == 64 and g["capped"] and g["trips"] > 1 for g in geo.values())
    assert any(g["idle_lanes"] for g in geo.values()) and any(1 < g["bpn"] < 1024 for g in geo.values())
    assert {c.layout for c in lm.DICE_CASES} == {"cl", "cl_pad", "ncdhw"}
    assert {(c.mask, lm.f32(c.thr)) for c in lm.DICE_CASES} == {(m, lm.f32(t)) for m in (True, False) for t in (0.5, 0.3)}
    assert any(c.shape[0] == 3 for c in lm.DICE_CASES)
    big = [c for c in lm.DICE_CASES if c.R * c.shape[1] * c.shape[2] * c.shape[3] > 3e6]
    assert [c.name for c in big] == ["r3_capped_104"], "only the capped R = 3 case may be large"


@pytest.mark.parametrize("case", lm.DICE_CASES, ids=ids(lm.DICE_CASES))
def test_dice_operands_decide_every_voxel(case):
    o = lm.make_dice(case.name)
    z, lab = o["z"], o["lab"]
    assert torch.equal(z, lm.rf32(z)) and torch.equal(lab, lm.rf32(lab))
    assert ((torch.sigmoid(z) - o["thr32"]).abs() >= lm.MARGIN).all(), "a logit sits on the threshold"
    for v in lm.ODD_LABELS:
        assert (lab == v).any(), f"no label of value {v}"
    assert lm.ODD_LABELS[1] > 0.5 and np.float32(lm.ODD_LABELS[1]) == lm.ODD_LABELS[1]
    cnt = o["counts"]
    n = case.shape[0]
    if n > 1 or case.R > 1:
        assert cnt[n // 2, case.R - 1, 2] == 0 and cnt[n - 1, 0, 1] == 0          # an empty label region, an empty prediction
    assert (cnt[..., 1] > 0).any() and (cnt[..., 0] > 0).any()
    if n > 1:
        assert not torch.equal(cnt[0], cnt[1])


def test_dice_resampling_is_rare_and_ends():
    """A logit within MARGIN of a threshold is a few-per-million event: the draw is resampled in place, not reshaped."""
    moved = sum(lm.make_dice(c.name)["resampled"] for c in lm.DICE_CASES)
    total = sum(lm.make_dice(c.name)["z"].numel() for c in lm.DICE_CASES)
    assert moved <= 1e-5 * total, (moved, total)


# ============================================================================= DiceCE
def _dce_desc(case):
    d, h, w = case.shape
    return _lib.Tensor(0x10000, case.N, case.R, d, h, w, case.R * d * h * w, d * h * w, h * w, w, 1, _lib.F32, 0)


@pytest.mark.parametrize("case", lm.DCE_CASES, ids=ids(lm.DCE_CASES))
def test_dce_case_reaches_its_class(case):
    t = _dce_desc(case)
    nbytes = lib().mmtta_dice_ce_scratch_bytes(C.byref(t))
    bpn = nbytes // (case.N * (3 * case.R + 1) * 8)
    assert nbytes == bpn * case.N * (3 * case.R + 1) * 8
    assert lm.BPN_CLASSES[case.klass](bpn), f"{case.name}: {bpn} partial blocks per item is not {case.klass}"
    if case.klass == "bpn=1024":
        dhw = case.shape[0] * case.shape[1] * case.shape[2]
        assert dhw < 8192 * 256 < case.N * dhw          # the gradient's second trip; the item index changes inside the first


def test_dce_table_covers_heads_options_and_classes():
    assert {c.klass for c in lm.DCE_CASES} == set(lm.BPN_CLASSES)
    small = [c for c in lm.DCE_CASES if c.klass == "bpn<64" and not c.special]
    heads = {(c.head, c.R) for c in small}
    assert heads == {("sigmoid", r) for r in (1, 2, 3, 4, 8)} | {("softmax", r) for r in (2, 3, 4, 8)}
    assert {(c.head, c.R, c.option) for c in small} == {(h, r, o) for h, r in heads for o in lm.DCE_OPTIONS}
    assert {c.shape[0] * c.shape[1] * c.shape[2] for c in small} == {105, 720}
    assert {c.labels for c in lm.DCE_CASES} == {"nested", "onehot", "soft"}
    assert {c.special for c in lm.DCE_CASES} == {"", "empty_label", "dead_logits", "both", "saturated"}
    assert {c.option for c in lm.DCE_CASES if c.klass != "bpn<64"} >= set(lm.SHIPPED)
    sm = {lm.DCE_OPTIONS[o].get("smooth_nr", lm.DCE_DEFAULTS["smooth_nr"]) for o in lm.DCE_OPTIONS}
    assert sm == {lm.f32(1e-5), lm.f32(1e-3), 1.0}
    assert sum(c.shape[0] >= 104 for c in lm.DCE_CASES) == 1


@pytest.mark.parametrize("case", lm.DCE_CASES, ids=ids(lm.DCE_CASES))
def test_dce_restated_sums_give_the_oracle_loss_and_the_bounds_catch_mistakes(case):
    o = lm.make_dce(case.name)
    z, y, w = o["z"], o["y"], o["w"]
    assert torch.equal(z, lm.rf32(z)) and torch.equal(y, lm.rf32(y))
    assert np.isfinite(o["loss64"]) and torch.isfinite(o["grad64"]).all()
    # the plain restatement of the sums is the oracle's loss
    loss, lbound = lm.dce_loss_from_sums(case, o["sums"], o["sum_bounds"])
    assert abs(loss - o["loss64"]) <= 1e-11 * abs(o["loss64"]), (loss, o["loss64"])
    assert lbound <= 1e-5 * abs(o["loss64"]), f"derived loss bound {lbound:.2e} is wider than the project's 1e-5 relative"
    assert o["grad_measured"] <= o["grad_held"], "the measured gradient bound is wider than the one the project holds"
    R = case.R
    q = [3 * r + 1 for r in range(R)]
    # one voxel (the last of the last item, p >= 1 / R in every channel) removed from the reference
    keep = torch.ones(z.shape[2:], dtype=torch.bool)
    keep[-1, -1, -1] = False
    s1, _ = lm.dce_sums(case, z[-1:, :, keep].unsqueeze(-1).unsqueeze(-1), y[-1:, :, keep].unsqueeze(-1).unsqueeze(-1), w)
    gap = (s1[0] - o["sums"][-1]).abs()
    assert (gap[q] > o["sum_bounds"][-1][q]).all(), (gap[q], o["sum_bounds"][-1][q])
    # the last partial workgroup of 256 voxels removed
    dhw = keep.numel()
    last = dhw % 256 or 256
    zf, yf = z[-1:].reshape(1, R, dhw, 1, 1), y[-1:].reshape(1, R, dhw, 1, 1)
    s2, _ = lm.dce_sums(case, zf[:, :, :dhw - last], yf[:, :, :dhw - last], w) if dhw > last else (torch.zeros_like(s1), None)
    gap = (s2[0] - o["sums"][-1]).abs()
    assert (gap[q] > o["sum_bounds"][-1][q]).all()
    # include_background ignored
    if R > 1 and not case.opts["include_background"]:
        zz = z.clone().requires_grad_(True)
        wrong = lm.dce_loss_module(case, torch.float64, include_background=True)(zz, y)
        wrong.backward()
        assert abs(wrong.item() - o["loss64"]) > lbound
        assert (zz.grad - o["grad64"]).abs().max().item() > o["grad_bound"]


def test_dce_saturated_cases_hold_every_saturated_value():
    for case in (c for c in lm.DCE_CASES if c.special == "saturated"):
        z = lm.make_dce(case.name)["z"]
        assert set(z.unique().tolist()) == set(lm.SATURATED) | {lm.PLANTED}


# ============================================================================= optimizers
@pytest.mark.parametrize("case", lm.OPT_CASES, ids=ids(lm.OPT_CASES))
def test_optimizer_restatement_is_torch_in_float64(case):
    kind, kw = lm.hyper(case.hp)
    reps, stride, used, active, decay = lm.opt_layout(case)
    p0, m0, v0, grads = lm.opt_operands(case)
    fl = lambda t: lm.opt_flat(case, t, active)
    args = (fl(p0), [fl(g) for g in grads], fl(m0), fl(v0), decay[active].repeat(used), case.step0)
    want = lm.opt_torch(kind, kw, *args, torch.float64)
    ref = lm.make_opt(case.name)
    for name, a, b in zip("pmv", (ref["p"], ref["m"], ref["v"]), want):
        assert (a is None) == (b is None), name
        if a is not None:
            assert (a - b).abs().max().item() <= 1e-12 * b.abs().max().item(), (case.name, name)
    assert (ref["m"] is None) == (kind == "sgd" and kw["momentum"] == 0.0) and (ref["v"] is None) == (kind == "sgd")
    assert 0.5 <= fl(p0).abs().min() and fl(p0).abs().max() < 1.5


def test_optimizer_table_covers_the_launch_classes():
    plain = [c for c in lm.OPT_CASES if c.mode == "plain" and c.steps == 5]
    assert {(c.hp, c.n) for c in plain} == {(h, n) for h in lm.HYPER for n in (36, 1036, 1037, 1038, 1039)}
    for c in plain:
        assert c.n_decay % 4 == 0 and c.n_decay <= c.n
    assert {(c.n_decay == 0, c.n_decay == c.n // 4 * 4) for c in plain} == {(True, False), (False, False), (False, True)}
    big = [c for c in lm.OPT_CASES if c.mode == "plain" and c.n > lm.GRID_ELEMS]
    assert {lm.hyper(c.hp)[0] for c in big} == {"adam", "adamw", "sgd"} and all(c.steps == 2 for c in big)
    assert all(c.n >= lm.GRID_ELEMS + 1028 for c in big) and any(c.n % 4 for c in big)
    segs = [c for c in lm.OPT_CASES if c.mode == "segments"]
    assert any(len(c.segs) == 1 for c in segs) and any(len(c.segs) == 300 for c in segs)
    assert any(sum(s[1] for s in c.segs) > lm.GRID_ELEMS for c in segs)
    for c in segs:
        ends = [a + n for a, n, _ in c.segs]
        assert all(a % 4 == 0 and n % 4 == 0 for a, n, _ in c.segs) and max(ends) <= c.stride
        if len(c.segs) > 1:
            assert all(c.segs[i + 1][0] > ends[i] for i in range(len(c.segs) - 1)), "the segments leave no gaps"
            assert {s[2] for s in c.segs} == {True, False}
    sets = [c for c in lm.OPT_CASES if c.mode == "sets"]
    assert sets and all(c.replicas == 3 and c.used == 2 and c.stride == c.n + 64 for c in sets)
    assert any(c.step0 == 9999 and lm.hyper(c.hp)[1]["betas"][1] == lm.f32(0.9999) and c.steps == 1 for c in lm.OPT_CASES)


@pytest.mark.parametrize("case", [c for c in lm.OPT_CASES if c.name.endswith("_n1036_ndmid") and lm.HYPER[c.hp][1]["weight_decay"]],
                         ids=lambda c: c.name)
def test_optimizer_bound_catches_a_decay_boundary_off_by_four(case):
    ref = lm.make_opt(case.name)
    for nd in (case.n_decay + 4, case.n_decay - 4):
        moved = (lm.opt_reference(case, nd)["p"] - ref["p"]).abs()
        assert int((moved > ref["bounds"]["p"]).sum()) == 4, (case.name, nd, moved.max().item(), ref["bounds"]["p"])


# ============================================================================= intensity
@pytest.mark.parametrize("case", lm.INT_CASES, ids=ids(lm.INT_CASES))
def test_intensity_restatement_is_the_oracle_in_float64(case):
    o = lm.make_int(case.name)
    x = o["x"]
    assert torch.equal(x, lm.rf32(x))
    want = oracle.normalize_image(x, **lm.int_kwargs(case))
    assert want.dtype == torch.float64
    for ch in range(case.C):
        scale = max(want[ch].abs().max().item(), 1e-30)
        assert (o["ref"][ch] - want[ch]).abs().max().item() <= 1e-9 * scale, (case.name, ch)
        if o["exact"][ch]:
            assert torch.equal(o["ref"][ch], want[ch])


def test_intensity_table_covers_the_launch_classes():
    geo = {c.name: lm.int_geometry(c.shape[0] * c.shape[1] * c.shape[2]) for c in lm.INT_CASES}
    assert {c.shape[0] * c.shape[1] * c.shape[2] for c in lm.INT_CASES} >= {100, 17280, 41 ** 3, 104 ** 3}
    assert {c.C for c in lm.INT_CASES} >= {1, 2, 8}
    g = geo["c8_41"]
    assert g["sblocks"] == 256 and g["stats_second_trip"] and g["finalize_second_trip"] and not g["apply_second_trip"]
    g = geo["c1_104"]
    assert g["apply_second_trip"] and g["apply_blocks"] == 4096
    assert geo["c8_17280"]["sblocks"] == 68 and geo["c8_100"]["sblocks"] == 1
    assert sum(c.shape[0] >= 104 for c in lm.INT_CASES) == 1 and [c.C for c in lm.INT_CASES if c.shape[0] >= 104] == [1]
    assert any(c.rules == tuple(range(8)) for c in lm.INT_CASES) and any(not c.rules and c.C == 4 for c in lm.INT_CASES)
    assert any(c.strided for c in lm.INT_CASES) and any(c.const for c in lm.INT_CASES)


@pytest.mark.parametrize("case", [c for c in lm.INT_CASES if c.rules == tuple(range(8))], ids=lambda c: c.name)
def test_intensity_eight_rules_prove_what_they_are_there_for(case):
    o = lm.make_int(case.name)
    x, st, rules = o["x"], o["stats"], lm.int_rules(case)
    dhw = x[0].numel()
    # 1: a mean far from zero; 2: mask_gt = -inf passes every voxel; 5: every clipped voxel passes, not every raw one
    assert abs(st[1]["mu"]) > 5e3 * st[1]["sd"] and st[2]["sums"][0] == dhw and st[5]["sums"][0] == dhw and (x[5] <= -1.0).any()
    assert 16 <= st[0]["sums"][0] < dhw and st[0]["masked_used"] and (x[0].abs() > 2.0).any()
    # 6 / 7: the masked count sits exactly at min_count, and one below it
    assert st[6]["sums"][0] == st[7]["sums"][0] == lm.SPARSE
    assert rules[6]["zscore"]["min_count"] == lm.SPARSE and rules[7]["zscore"]["min_count"] == lm.SPARSE + 1
    assert st[6]["masked_used"] and not st[7]["masked_used"]
    # `>` for `>=` at min_count, and masking before the clip, move the reference by more than the bound
    wrong, _ = lm.int_restated(x, rules, strict_count=True)
    assert (wrong[6] - o["ref"][6]).abs().max().item() > o["bounds"][6] and torch.equal(wrong[7], o["ref"][7])
    wrong, _ = lm.int_restated(x, rules, mask_before_clip=True)
    assert (wrong[5] - o["ref"][5]).abs().max().item() > o["bounds"][5]
    # the last voxel of a channel removed from its all-voxel sums moves them by more than the bound of the fp64 sums
    for ch in (0, 1, 2, 6, 7):
        last = x[ch].reshape(-1)[-1]
        if "clip" in rules[ch]:
            last = last.clamp(*rules[ch]["clip"])
        assert abs(last.item()) > dhw * lm.D53 * st[ch]["terms"][3] and last.item() ** 2 > dhw * lm.D53 * st[ch]["terms"][4]


def test_intensity_constant_channel_reaches_eps():
    o = lm.make_int("c2_const")
    assert o["stats"][1]["sd"] == lm.f32(1e-6) and (o["ref"][1] == 0).all()


# ============================================================================= host refusals, by status code
def _t(n=1, c=3, d=4, h=4, w=4, ptr=0x10000, dtype=None):
    return _lib.Tensor(ptr, n, c, d, h, w, c * d * h * w, d * h * w, h * w, w, 1, _lib.F32 if dtype is None else dtype, 0)


def _r(t):
    return None if t is None else C.byref(t)


def test_dice_counts_refusals():
    L = lib()
    z, y, cnt = _t(), _t(), 0x20000
    call = lambda a, b, c_=cnt: L.mmtta_mask_dice_counts(_r(a), _r(b), 0.5, c_, None, None)
    for args in ((None, y), (z, None), (z, y, None), (_t(ptr=None), y), (z, _t(ptr=None))):
        assert call(*args) == INVALID and b"null" in L.mmtta_last_error()
    for other in (_t(n=2), _t(c=2), _t(d=5), _t(h=5), _t(w=5)):
        assert call(z, other) == INVALID and b"shape" in L.mmtta_last_error()
    assert call(_t(c=257), _t(c=257)) == UNSUPPORTED and b"256" in L.mmtta_last_error()
    assert call(_t(dtype=_lib.BF16), y) == UNSUPPORTED and call(z, _t(dtype=_lib.BF16)) == UNSUPPORTED


def test_dice_ce_refusals():
    L = lib()
    z, y, g, buf = _t(), _t(), _t(), 0x20000
    sums = lambda a, b, out=buf, scr=buf: L.mmtta_dice_ce_sums(_r(a), _r(b), None, 0, 0, out, scr, None)
    grad = lambda a, b, c_, s=buf: L.mmtta_dice_ce_grad(_r(a), _r(b), None, 0, 0, 0, 1, 1.0, 1.0, 1e-5, 1e-5, s, _r(c_), None)
    for args in ((None, y), (z, None), (z, y, None), (z, y, buf, None), (_t(ptr=None), y), (z, _t(ptr=None))):
        assert sums(*args) == INVALID and b"null" in L.mmtta_last_error()
    for args in ((None, y, g), (z, None, g), (z, y, None), (z, y, g, None), (z, y, _t(ptr=None))):
        assert grad(*args) == INVALID and b"null" in L.mmtta_last_error()
    for other in (_t(n=2), _t(c=2), _t(d=5), _t(h=5), _t(w=5)):
        assert sums(z, other) == INVALID and grad(z, other, g) == INVALID and grad(z, y, other) == INVALID
        assert b"shape" in L.mmtta_last_error()
    nine = _t(c=9)
    assert sums(nine, nine) == UNSUPPORTED and grad(nine, nine, nine) == UNSUPPORTED
    assert L.mmtta_dice_ce_scratch_bytes(C.byref(nine)) == -1 and L.mmtta_dice_ce_scratch_bytes(None) == -1
    assert L.mmtta_dice_ce_scratch_bytes(C.byref(_t(c=0))) == -1
    assert L.mmtta_dice_ce_scratch_bytes(C.byref(_t(c=8))) == 25 * 8
    bf = _t(dtype=_lib.BF16)
    assert sums(bf, y) == UNSUPPORTED and sums(z, bf) == UNSUPPORTED
    assert grad(bf, y, g) == UNSUPPORTED and grad(z, bf, g) == UNSUPPORTED and grad(z, y, bf) == UNSUPPORTED


def test_intensity_refusals():
    L = lib()
    rule = lambda **kw: _lib.IntensityRule(kw.get("clip", 0), kw.get("zscore", 0), 0, 16, 0.0, 0.0, float("-inf"), 1e-6,
                                           kw.get("mean", 0.0), kw.get("std", 1.0), kw.get("legacy", 0), 0)
    rules = lambda c, **kw: (_lib.IntensityRule * c)(*[rule(**kw) for _ in range(c)])
    x, y, scr = _t(), _t(ptr=0x30000), 0x20000
    call = lambda a, b, r=rules(3), s=scr: L.mmtta_intensity_normalize(_r(a), r, _r(b), s, None)
    for args in ((None, y), (x, None), (x, y, None), (x, y, rules(3), None), (_t(ptr=None), y), (x, _t(ptr=None))):
        assert call(*args) == INVALID and b"null" in L.mmtta_last_error()
    assert call(_t(n=2), _t(n=2)) == UNSUPPORTED and b"one image" in L.mmtta_last_error()
    assert call(_t(c=9), _t(c=9), rules(9)) == UNSUPPORTED and L.mmtta_intensity_scratch_bytes(9) == -1
    assert L.mmtta_intensity_scratch_bytes(0) == -1 and L.mmtta_intensity_scratch_bytes(8) == 8 * 256 * 5 * 8 + 8 * 2 * 4
    for other in (_t(c=2), _t(d=5), _t(h=5), _t(w=5)):
        assert call(x, other) == INVALID and b"shape" in L.mmtta_last_error()
    loose = _t()
    loose.sw, loose.sh, loose.sd = 2, 8, 32
    assert call(loose, y) == UNSUPPORTED and call(x, loose) == UNSUPPORTED and b"dense" in L.mmtta_last_error()
    assert call(_t(dtype=_lib.BF16), y) == UNSUPPORTED
    assert call(x, y, rules(3, legacy=1, std=0.0)) == INVALID and b"std" in L.mmtta_last_error()


def test_optimizer_refusals():
    L = lib()
    desc = lambda kind=_lib.OPTIM_ADAM, **kw: _lib.OptimDesc(kind, 1e-3, 0.9, 0.999, 1e-8, 0.0, kw.get("momentum", 0.0),
                                                           kw.get("dampening", 0.0), kw.get("nesterov", 0))
    P, G, M, V, S = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    step = lambda d, p=P, g=G, m=M, v=V, n=64, nd=32, s=S: L.mmtta_optim_step(_r(d), p, g, m, v, n, nd, s, None)
    sets = lambda d, k, stride, n=64: L.mmtta_optim_step_sets(_r(d), P, G, M, V, n, 32, k, stride, S, None)
    segs = lambda d, table, count, total, k=1, stride=128, p=P, v=V: L.mmtta_optim_step_segments(_r(d), p, G, M, v, table, count, total,
                                                                                                 k, stride, S, None)
    a = desc()
    assert step(None) == INVALID and b"null desc" in L.mmtta_last_error()
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(s=None), dict(n=-4), dict(nd=-4)):
        assert step(a, **kw) == INVALID
    assert step(a, nd=68) == INVALID                                   # n_decay > n
    assert step(a, v=None) == INVALID and b"second-moment" in L.mmtta_last_error()
    assert step(desc(_lib.OPTIM_ADAMW), v=None) == INVALID
    assert step(desc(3)) == INVALID and b"kind" in L.mmtta_last_error()
    assert step(desc(-1)) == INVALID
    for kw in (dict(p=P + 4), dict(g=G + 8), dict(m=M + 4), dict(v=V + 12), dict(nd=30)):
        assert step(a, **kw) == UNSUPPORTED and b"16-byte" in L.mmtta_last_error()
    sgd = _lib.OPTIM_SGD
    assert step(desc(sgd, nesterov=1, momentum=0.0), v=None) == INVALID and b"nesterov" in L.mmtta_last_error()
    assert step(desc(sgd, nesterov=1, momentum=0.9, dampening=0.1), v=None) == INVALID
    assert step(a, n=0, nd=0) == 0                                     # nothing to do: returns before any launch
    assert sets(a, 2, 60) == INVALID and b"stride" in L.mmtta_last_error()           # stride < n
    assert sets(a, 2, 66) == INVALID and sets(a, 0, 64) == INVALID and sets(a, 1, -4) == INVALID
    assert sets(None, 1, 64) == INVALID
    assert sets(desc(sgd, nesterov=1), 1, 64) == INVALID
    T = 0x60000
    assert segs(None, T, 1, 4) == INVALID
    assert segs(a, None, 1, 8) == INVALID and b"no table" in L.mmtta_last_error()
    assert segs(a, T, 0, 8) == INVALID and b"no table" in L.mmtta_last_error()
    assert segs(a, T, 1, 6) == INVALID and segs(a, T, 1, 8, stride=126) == INVALID and segs(a, T, 1, 8, k=0) == INVALID
    assert segs(a, T, -1, 8) == INVALID and segs(a, T, 1, -8) == INVALID
    assert segs(desc(3), T, 1, 8) == INVALID and segs(a, T, 1, 8, v=None) == INVALID and segs(a, T, 1, 8, p=None) == INVALID
    assert segs(a, T, 1, 8, p=P + 4) == UNSUPPORTED
    assert segs(desc(sgd, nesterov=1, momentum=0.9, dampening=0.5), T, 1, 8) == INVALID
