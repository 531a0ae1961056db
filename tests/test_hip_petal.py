"""PETAL adaptation (``petal_tta``) on the GPU: the magnitude select and the teacher / ranked-restore pass against the NumPy
restatement of tests/test_petal_host.py, bit for bit (the thresholds' bits, the restored positions, the counts), and the
plugin against a PETAL restatement on the oracle networks - CoTTA's restatement of tests/test_hip_cotta.py with the restore
mask taken per tensor from its own gradient - under that file's bounds, plus the bitwise properties (quantile 0 = CoTTA
without restore, grouped = one volume at a time, graph replay = eager)."""
import copy
import math

import numpy as np
import pytest
import torch

from test_hip_cotta import bits, check_against_reference, consistency_loss, cotta_cfg, layout_of, teacher_target
from test_hip_memo import BATCH
from test_hip_tta import SMALL, build_pair, volume
from test_petal_host import keys_of, rank_restore

pytestmark = pytest.mark.gpu

SENTINEL = -7


# ----------------------------------------------------------------------------- 1. select + update against the NumPy rule
def lay_out(lengths_ranks, gap=0):
    """Rows (start, length, rank) for (length, rank) pairs: every start the next multiple of 4 (+ ``gap`` quads)."""
    rows, at = [], 0
    for length, rank in lengths_ranks:
        rows.append((at, length, rank))
        at = (at + length + 3) // 4 * 4 + 4 * gap
    return rows


def boundary():
    """The first length the chunked kernels serve, by the library's class query."""
    from multimodal_tta_amd import ops
    lo, hi = 1, 1 << 30
    assert ops.magnitude_select_class(lo) == 0 and ops.magnitude_select_class(hi) == 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ops.magnitude_select_class(mid) == 0 else (lo, mid)
    return hi


def run_petal(g, w, teacher, source, rows, n, sets, alpha):
    """The two entry points on copies of the buffers, outputs prefilled with a sentinel and the select's scratch with
    garbage: (gamma uint32 [rows of g][count], w, teacher, restored) on the host."""
    from multimodal_tta_amd import ops
    g, w, teacher, source = g.cuda(), w.cuda().clone(), teacher.cuda().clone(), source.cuda()
    table = ops.rank_segments_table(rows, "cuda")
    gamma = torch.full((g.shape[0], len(rows)), SENTINEL, dtype=torch.int32, device="cuda")
    scratch = torch.full((ops.magnitude_select_scratch(table, sets),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ops.magnitude_select_sets(g, table, sets, gamma, scratch)
    partial = torch.full((ops.petal_update_partials(n, sets),), SENTINEL, dtype=torch.int64, device="cuda")
    restored = torch.full((g.shape[0],), SENTINEL, dtype=torch.int64, device="cuda")
    ops.petal_update_sets(w, teacher, source, g, gamma, table, n, sets, alpha, partial, restored)
    torch.cuda.synchronize()
    return gamma.cpu().numpy().view(np.uint32), w.cpu(), teacher.cpu(), restored.cpu()


def check_petal(g, w0, t0, source, rows, n, sets, alpha):
    """Bit for bit against ``rank_restore``: the thresholds, the restored positions (source bits there, old bits elsewhere),
    the counts; the teacher within ``test_hip_cotta.check_update``'s bound; nothing written past ``sets`` or ``n``."""
    gamma, w1, t1, restored = run_petal(g, w0, t0, source, rows, n, sets, alpha)
    masks = []
    for s in range(g.shape[0]):
        if s >= sets:
            assert (gamma[s].view(np.int32) == SENTINEL).all() and int(restored[s]) == SENTINEL, f"set {s} was written"
            assert torch.equal(bits(w1[s]), bits(w0[s])) and torch.equal(bits(t1[s]), bits(t0[s])), f"set {s} was written"
            continue
        want_gamma, mask = rank_restore(g[s, :n].numpy(), rows)
        assert gamma[s].tolist() == want_gamma.tolist(), f"set {s}: thresholds {gamma[s]} vs {want_gamma}"
        mask = torch.from_numpy(mask)
        want = torch.where(mask, source[:n], w0[s, :n])
        assert torch.equal(bits(w1[s, :n]), bits(want)), f"set {s}: the restored positions differ from the rule's"
        assert torch.equal(bits(w1[s, n:]), bits(w0[s, n:])) and torch.equal(bits(t1[s, n:]), bits(t0[s, n:])), "written past n"
        assert int(restored[s]) == int(mask.sum()), (s, int(restored[s]), int(mask.sum()))
        ref = alpha * t0[s, :n].double() + (1.0 - alpha) * w0[s, :n].double()
        bound = 2.0 ** -22 * torch.maximum(t0[s, :n].abs(), w0[s, :n].abs()).double()
        assert ((t1[s, :n].double() - ref).abs() <= bound).all()
        masks.append(mask)
    return gamma, w1, t1, restored, masks


def buffers(gen, rows_of_w, n, extra=(5, 1, 3)):
    """w, teacher, g-shaped widths past n (multiples of 4) and a source, all random."""
    widths = [(n + 3) // 4 * 4 + 4 * e for e in extra]
    w = torch.randn((rows_of_w, widths[0]), generator=gen)
    teacher = torch.randn((rows_of_w, widths[1]), generator=gen)
    source = torch.randn(widths[0], generator=gen)
    return w, teacher, source, widths[2]


def test_small_rows_every_rank_three_replicas_in_a_four_row_buffer():
    gen = torch.Generator().manual_seed(71)
    pairs = [(length, rank) for length in (1, 2, 3, 5, 32, 243, 1003)
             for rank in sorted({0, length - 1, math.floor(0.2 * length)})]
    rows = lay_out(pairs)
    n = rows[-1][0] + rows[-1][1]          # 1003 elements in the last row: no multiple of 4, the tail goes one by one
    assert n % 4 != 0
    G = 3
    w, teacher, source, gw = buffers(gen, G + 1, n)
    g = torch.randn((G + 1, gw), generator=gen) * torch.logspace(-8, 2, gw).roll(17)
    _, _, _, restored, masks = check_petal(g, w, teacher, source, rows, n, G, 0.9)
    for s in range(G):          # distinct values: exactly `rank` elements of every row
        for start, length, rank in rows:
            assert int(masks[s][start:start + length].sum()) == rank
    assert restored[:G].tolist() == [sum(r[2] for r in rows)] * G


def test_dispatch_boundary_and_a_row_wider_than_one_grid_trip():
    from multimodal_tta_amd import ops
    b = boundary()
    assert ops.magnitude_select_class(b - 1) == 0 and ops.magnitude_select_class(b) == 1
    wide = 4 * 4096 * 256 + 4 * 1000 + 2          # test_update_covers_a_span_wider_than_its_grid's span
    rows = lay_out([(b - 1, (b - 1) // 5), (b, b // 5), (b + 1, b), (wide, math.floor(0.03 * wide)), (7, 3)], gap=1)
    n = rows[-1][0] + rows[-1][1]
    gen = torch.Generator().manual_seed(72)
    w, teacher, source, gw = buffers(gen, 1, n)
    g = torch.randn((1, gw), generator=gen) * 1e-3
    _, _, _, restored, _ = check_petal(g, w, teacher, source, rows, n, 1, 0.999)
    print(f"boundary {b}: restored {int(restored[0])} of {n}")
    assert abs(int(restored[0]) - sum(r[2] for r in rows)) <= 8          # (ties among 4 M normal draws are rare, not excluded)


@pytest.mark.parametrize("length", [1000, 50003])
def test_every_value_class_and_a_tie_at_the_threshold(length):
    """Negatives, denormals, +-0, infinities, and a run of 40 % equal values that straddles the rank: the threshold is the
    tied value and nothing equal to it is restored."""
    gen = torch.Generator().manual_seed(73)
    v = torch.randn(length, generator=gen) * 1e-2
    v[:length // 20] = 0.0
    v[length // 20:length // 10] = -0.0
    v[length // 10:length // 10 + length // 20] = 1e-41 * torch.arange(1, length // 20 + 1)          # denormals
    v[-7:] = torch.tensor([float("inf"), float("-inf"), 3e38, -3e38, 1e-45, -1e-45, float("inf")])
    tie = 2.5e-3
    idx = torch.randperm(length - 7, generator=gen)[:int(0.4 * length)]
    v[idx] = tie * torch.where(torch.rand(len(idx), generator=gen) < 0.5, -1.0, 1.0)
    k = keys_of(v.numpy())
    tie_key = keys_of(np.array([tie], dtype=np.float32))[0]
    first = int((k < tie_key).sum())
    rank = first + int(0.2 * length)                       # inside the run of equal keys
    assert 0 < first < rank < first + int((k == tie_key).sum()) - 1
    v = v[torch.randperm(length, generator=gen)]
    rows = [(8, length, rank)]
    n = 8 + length
    w, teacher, source, gw = buffers(gen, 2, n)
    g = torch.zeros((2, gw))
    g[0, 8:8 + length] = v
    g[1, 8:8 + length] = -v.flip(0)
    gamma, w1, _, restored, masks = check_petal(g, w, teacher, source, rows, n, 2, 0.5)
    assert gamma[:, 0].tolist() == [int(tie_key)] * 2
    assert restored.tolist() == [first, first] and first < rank
    assert not masks[0][8:8 + length][torch.from_numpy(keys_of(g[0, 8:8 + length].numpy()) == tie_key)].any()


@pytest.mark.parametrize("length", [777, 30001])
def test_extremes_zero_rows_distinct_rows_and_nans(length):
    gen = torch.Generator().manual_seed(74)
    rank = length // 3
    rows = lay_out([(length, rank)] * 3 + [(length, length - 3)])
    n = rows[-1][0] + rows[-1][1]
    w, teacher, source, gw = buffers(gen, 1, n)
    g = torch.zeros((1, gw))
    # row 0: all zero.  row 1: distinct values.  rows 2, 3: two NaNs (either sign) among distinct values
    distinct = (torch.randperm(length, generator=gen).float() + 1.0) * 1e-6 * torch.where(torch.rand(length, generator=gen) < 0.5, -1.0, 1.0)
    for r in (1, 2, 3):
        g[0, rows[r][0]:rows[r][0] + length] = distinct.roll(r)
    nan_at = [rows[r][0] + o for r in (2, 3) for o in (5, length - 2)]
    g[0, nan_at[0]], g[0, nan_at[1]], g[0, nan_at[2]], g[0, nan_at[3]] = float("nan"), -float("nan"), float("nan"), -float("nan")
    gamma, w1, _, restored, masks = check_petal(g, w, teacher, source, rows, n, 1, 0.9)
    m = masks[0]
    counts = [int(m[s:s + l].sum()) for s, l, _ in rows]
    assert counts[0] == 0 and gamma[0, 0] == 0, "an all-zero gradient restored something"
    assert counts[1] == rank, "a row of distinct values restores exactly `rank` elements"
    assert counts[2] == rank and counts[3] == length - 3          # rank length - 3: the largest finite value is the threshold
    assert not m[nan_at].any(), "a NaN was restored"
    assert gamma[0, 3] < 0x7F800000


def test_clustered_exponents_one_million_values_in_one_binade():
    """Every key shares its exponent: the first digit's histogram takes all of them in 8 of its bins."""
    gen = torch.Generator().manual_seed(75)
    length = 1 << 20
    rows = [(0, length, math.floor(0.03 * length))]
    w, teacher, source, gw = buffers(gen, 1, length)
    g = torch.zeros((1, gw))
    g[0, :length] = 1.0 + torch.rand(length, generator=gen)
    g[0, :length] *= torch.where(torch.rand(length, generator=gen) < 0.5, -1.0, 1.0)
    assert ((g[0, :length].abs() >= 1) & (g[0, :length].abs() < 2)).all()
    _, _, _, restored, _ = check_petal(g, w, teacher, source, rows, length, 1, 0.999)
    assert 0 < int(restored[0]) <= rows[0][2]


def test_teacher_edge_values_of_alpha():
    gen = torch.Generator().manual_seed(76)
    rows = lay_out([(515, 100), (9000, 1800)])
    n = rows[-1][0] + rows[-1][1]
    w, teacher, source, gw = buffers(gen, 2, n)
    teacher[0, 3], teacher[1, 7] = -0.0, 0.0
    g = torch.randn((2, gw), generator=gen)
    _, w1, t1, restored, _ = check_petal(g, w, teacher, source, rows, n, 2, 1.0)
    assert torch.equal(bits(t1), bits(teacher)), "alpha = 1 moved the teacher"
    assert restored.tolist() == [1900, 1900]
    _, _, t1, _, _ = check_petal(g, w, teacher, source, rows, n, 2, 0.0)
    assert torch.equal(t1[:, :n], w[:, :n]), "alpha = 0: the teacher is the student"


def test_g_replicas_equal_g_single_calls_and_a_rerun():
    gen = torch.Generator().manual_seed(77)
    b = boundary()
    rows = lay_out([(300, 60), (b + 5000, 2000), (5, 1), (3 * b, b)])
    n = rows[-1][0] + rows[-1][1]
    G = 3
    w, teacher, source, gw = buffers(gen, G, n)
    g = torch.randn((G, gw), generator=gen) * torch.logspace(-6, 0, gw)
    a = run_petal(g, w, teacher, source, rows, n, G, 0.9)
    again = run_petal(g, w, teacher, source, rows, n, G, 0.9)
    for x, y in zip(a, again):
        assert np.array_equal(np.asarray(x), np.asarray(y)), "two runs of the same call differ"
    for s in range(G):
        one = run_petal(g[s:s + 1], w[s:s + 1], teacher[s:s + 1], source, rows, n, 1, 0.9)
        assert np.array_equal(one[0][0], a[0][s]) and torch.equal(bits(one[1][0]), bits(a[1][s]))
        assert torch.equal(bits(one[2][0]), bits(a[2][s])) and int(one[3][0]) == int(a[3][s])
    assert (a[3] > 0).all()


# ----------------------------------------------------------------------------- 2. the plugin against a PETAL restatement
def petal_cfg(model_cfg, axes, quantile=0.2, alpha=0.9, **kw):
    cfg = cotta_cfg(model_cfg, axes, alpha=alpha, **kw)
    del cfg["method"]["cotta"]
    cfg["method"]["name"] = "petal_tta"
    cfg["method"]["petal"] = {"mirror_axes": list(axes), "alpha": alpha, "quantile": quantile}
    return cfg


def rule_mask(grad, quantile):
    """The restore mask of one tensor from its own gradient: fp32 by the keys, float64 (the restatement's second run) by |g|."""
    flat = grad.detach().reshape(-1)
    k = keys_of(flat.numpy()) if flat.dtype == torch.float32 else flat.abs().numpy()
    rank = math.floor(quantile * k.shape[0])
    return torch.from_numpy(k < np.partition(k, rank)[rank])


def petal_reference(model, xs, train_cfg, steps, masks, layout, alpha=0.9, quantile=0.2, episodic=True, softmax=False):
    """``test_hip_cotta.cotta_reference`` with the restore mask of every tensor taken from its own gradient by the rule.  Per
    volume the per-step losses, the restored counts, the masks (per step, {name: mask}) and the final eval logits."""
    import oracle
    from oracle.tta import select_params
    (refs, _) = layout
    source = copy.deepcopy(model.state_dict())
    teacher = copy.deepcopy(model)
    for p in teacher.parameters():
        p.requires_grad_(False)
    teacher.train()
    named = select_params(model, "all")
    opt, out = None, []
    for x in xs:
        if episodic or opt is None:
            model.load_state_dict(source)
            teacher.load_state_dict(source)
            opt = oracle.adam.build_optimizer(named, train_cfg)
        losses, counts, decisions = [], [], []
        model.train()
        for _ in range(steps):
            target = teacher_target(teacher, x, masks, softmax)
            opt.zero_grad()
            loss = consistency_loss(model(x), target, softmax)[0]
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            with torch.no_grad():
                student, teach = dict(model.named_parameters()), dict(teacher.named_parameters())
                step_masks = {}
                for name, off, numel in refs:
                    teach[name].mul_(alpha).add_(student[name], alpha=1.0 - alpha)
                    m = rule_mask(student[name].grad, quantile).view(student[name].shape)
                    student[name][m] = source[name].to(student[name].dtype)[m]
                    step_masks[name] = m
                counts.append(sum(int(m.sum()) for m in step_masks.values()))
                decisions.append(step_masks)
        model.eval()
        with torch.no_grad():
            out.append({"logits": model(x), "losses": losses, "restored": counts, "masks": decisions})
    return out, teacher


def run_both(model_cfg, cfg, vols, axes, float64=True, seed=42, softmax=False):
    from multimodal_tta_amd.config import get_config
    from multimodal_tta_amd.memo import view_masks
    from multimodal_tta_amd.registry import get_plugin
    masks = view_masks(axes)
    ref, hip = build_pair(model_cfg, seed=seed)
    plug = get_plugin("petal_tta")(cfg).setup(hip, "cuda")
    c = cfg["method"]["petal"]
    args = dict(alpha=c["alpha"], quantile=c["quantile"], episodic=bool(get_config(cfg, "method.episodic", True)), softmax=softmax)
    steps = cfg["method"]["steps"]
    xs = [v[0] for v in vols]
    o64 = None
    if float64:
        o64, _ = petal_reference(copy.deepcopy(ref).double(), [x.double() for x in xs], cfg["training"], steps, masks,
                                 layout_of(plug), **args)
    out_ref, _ = petal_reference(ref, xs, cfg["training"], steps, masks, layout_of(plug), **args)
    results = []
    for x in xs:
        r = plug.adapt_volume(x.cuda())
        results.append({"logits": plug.logits(r).cpu(), "losses": r["losses"].cpu().clone(), "restored": r["restored"].cpu().clone()})
    if float64:
        for k, (a, b) in enumerate(zip(out_ref, o64)):
            differ = [sum(int((ma[name] != mb[name]).sum()) for name in ma) for ma, mb in zip(a["masks"], b["masks"])]
            print(f"volume {k}: restore decisions on which the fp32 and the float64 restatement disagree, per step: {differ}; "
                  f"restored: device {results[k]['restored'].tolist()}, fp32 {a['restored']}, float64 {b['restored']}")
    return plug, results, out_ref, o64


def test_petal_matches_the_restatement():
    axes = ["h", "w"]
    cfg = petal_cfg(SMALL, axes, steps=3, group=1)
    x, y = volume(0)
    plug, res, out_ref, o64 = run_both(SMALL, cfg, [(x, y)], axes)
    assert res[0]["losses"].shape == (3,) and res[0]["restored"].shape == (3,)
    check_against_reference(res[0]["logits"], res[0]["losses"], out_ref[0], o64[0], y)
    n_train = plug.rt.arena.n_train
    assert all(0 < int(v) <= 0.2 * n_train for v in res[0]["restored"])
    ar = plug.rt.arena
    assert not torch.equal(plug.teacher[0], ar.source[:n_train]) and not torch.equal(plug.teacher[0], ar.params_all[0, :n_train])


def test_petal_bf16_tracks_the_restatement():
    axes = ["h", "w"]
    cfg = petal_cfg(SMALL, axes, steps=3, group=1, precision="bf16")
    x, y = volume(5)
    plug, res, out_ref, _ = run_both(SMALL, cfg, [(x, y)], axes, float64=False)
    check_against_reference(res[0]["logits"], res[0]["losses"], out_ref[0], None, y, bf16=True)


def test_petal_deepfusion_matches_the_restatement():
    import oracle
    from multimodal_tta_amd.memo import view_masks
    from multimodal_tta_amd.models import MultimodalUNetDeepFusion
    from multimodal_tta_amd.registry import get_plugin
    axes = ["w"]
    mcfg = dict(name="unet_multimodal_deepfusion", num_modalities=4, num_classes=3, spatial_dims=3,
                channels=[4, 8, 16, 32, 64], strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)
    cfg = petal_cfg(mcfg, axes, steps=2, group=1)
    torch.manual_seed(42)
    ref = oracle.MultimodalUNetDeepFusion(mcfg)
    hip = MultimodalUNetDeepFusion(mcfg)
    hip.load_state_dict(ref.state_dict())
    x, y = volume(2)
    plug = get_plugin("petal_tta")(cfg).setup(hip, "cuda")
    assert plug.group == 1
    o64, _ = petal_reference(copy.deepcopy(ref).double(), [x.double()], cfg["training"], 2, view_masks(axes), layout_of(plug))
    out_ref, _ = petal_reference(ref, [x], cfg["training"], 2, view_masks(axes), layout_of(plug))
    res = plug.adapt_volume(x.cuda())
    assert (res["restored"] > 0).all()
    check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref[0], o64[0], y)


# ----------------------------------------------------------------------------- stage by stage
def test_petal_steps_match_the_rule_on_the_device_gradient(monkeypatch):
    """Three eager steps, read around the pass after the optimizer: on the gradient the backward left in the arena, the
    pre-update weights, the teacher and the source, the post-step weights and ``restored`` must be exactly what the NumPy
    rule gives, and the teacher exactly what ``mmtta_cotta_update_sets`` makes of the same two spans (its arithmetic is the
    specification: the compiler fuses a t + (b w) in its 16-byte path, so a host restatement is an ulp off in places)."""
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.petal import rank_rows
    from multimodal_tta_amd.registry import get_plugin
    cfg = petal_cfg(SMALL, ["h", "w"], steps=3, lr=1e-3, group=1, use_graph=False)
    _, hip = build_pair(SMALL)
    plug = get_plugin("petal_tta")(cfg).setup(hip, "cuda")
    ar = plug.rt.arena
    nt = ar.n_train
    rows = rank_rows(ar.refs, 0.2)
    assert rows == [(r.offset, r.numel, math.floor(0.2 * r.numel)) for r in sorted(ar.refs, key=lambda r: r.offset) if r.trainable]
    assert plug.table.rows == rows and {ops.magnitude_select_class(r[1]) for r in rows} == {0, 1}
    source = ar.source[:nt].cpu()
    update, seen = ops.petal_update_sets, []

    def spy_update(w, teacher, src, g, gamma, table, n, sets, alpha, partial, restored):
        assert (n, sets, alpha) == (nt, 1, 0.9) and g is ar.grads_all and w is ar.params_all
        w0, t0, g0 = w[0, :nt].cpu(), teacher[0].cpu(), g[0, :nt].cpu()
        wc, tc = w[:1, :nt].clone(), teacher[:1].clone()
        ops.cotta_update_sets(wc, tc, src, nt, 1, alpha, 0.0, 0, ar.step, torch.zeros(1, dtype=torch.int32, device="cuda"),
                              torch.empty(ops.cotta_update_partials(nt, 1), dtype=torch.int64, device="cuda"),
                              torch.empty(1, dtype=torch.int64, device="cuda"))
        update(w, teacher, src, g, gamma, table, n, sets, alpha, partial, restored)
        torch.cuda.synchronize()
        want_gamma, mask = rank_restore(g0.numpy(), rows)
        assert gamma[0].cpu().numpy().view(np.uint32).tolist() == want_gamma.tolist()
        mask = torch.from_numpy(mask)
        assert torch.equal(bits(w[0, :nt].cpu()), bits(torch.where(mask, source, w0))), "the restored set is not the rule's"
        assert torch.equal(bits(teacher[0].cpu()), bits(tc[0].cpu())), "the teacher is not mmtta_cotta_update_sets' average"
        ema = 0.9 * t0.double() + (1.0 - 0.9) * w0.double()
        assert ((teacher[0].cpu().double() - ema).abs() <= 2.0 ** -22 * torch.maximum(t0.abs(), w0.abs()).double()).all()
        assert int(restored[0]) == int(mask.sum())
        seen.append(int(mask.sum()))

    monkeypatch.setattr(ops, "petal_update_sets", spy_update)
    res = plug.adapt_volume(volume(0)[0].cuda())
    assert len(seen) == 3 and res["restored"].tolist() == seen and all(v > 0 for v in seen)
    assert not torch.equal(ar.params_all[0, :nt].cpu(), source)


# ----------------------------------------------------------------------------- bit for bit
def test_quantile_zero_is_cotta_without_restore():
    from multimodal_tta_amd.registry import get_plugin
    x = volume(0)[0].cuda()
    out = {}
    for name, cfg in (("petal_tta", petal_cfg(SMALL, ["h", "w"], quantile=0, steps=3, lr=1e-3, group=1)),
                      ("cotta_tta", cotta_cfg(SMALL, ["h", "w"], steps=3, lr=1e-3, group=1, restore_p=0.0))):
        _, hip = build_pair(SMALL)
        plug = get_plugin(name)(cfg).setup(hip, "cuda")
        r = plug.adapt_volume(x)
        out[name] = (plug.logits(r).cpu(), r["losses"].cpu(), plug.teacher.cpu(), r["restored"].cpu())
    for a, b in zip(out["petal_tta"], out["cotta_tta"]):
        assert torch.equal(a, b)
    assert out["petal_tta"][3].tolist() == [0, 0, 0]


def test_without_views_the_first_gradient_is_zero_and_nothing_is_restored():
    from multimodal_tta_amd.registry import get_plugin
    cfg = petal_cfg(SMALL, [], steps=2, lr=1e-3, group=1)
    _, hip = build_pair(SMALL)
    plug = get_plugin("petal_tta")(cfg).setup(hip, "cuda")
    r = plug.adapt_volume(volume(3)[0].cuda())
    assert int(r["restored"][0]) == 0          # the target equals the logits: a gradient of exactly zero, no key below gamma = 0


def test_petal_group_equals_one_volume_at_a_time_and_graph_equals_eager():
    from multimodal_tta_amd.registry import get_plugin
    G = 2
    vols = [volume(i)[0] for i in range(G)]
    runs = {}
    for group, use_graph in ((G, True), (1, True), (G, False)):
        cfg = petal_cfg(SMALL, ["w"], steps=3, lr=1e-3, group=group, tune_volumes=4, use_graph=use_graph)
        _, hip = build_pair(SMALL)
        plug = get_plugin("petal_tta")(cfg).setup(hip, "cuda")
        if group == G:
            r = plug.adapt_volume(torch.cat(vols).cuda())
            assert r["restored"].shape == (3, G)
            runs[(group, use_graph)] = (plug.logits(r).cpu(), r["losses"].cpu(), r["restored"].cpu(), plug.teacher.cpu())
        else:
            zs, ls, rs, ts = [], [], [], []
            for v in vols:
                r = plug.adapt_volume(v.cuda())
                zs.append(plug.logits(r).cpu())
                ls.append(r["losses"].cpu())
                rs.append(r["restored"].cpu())
                ts.append(plug.teacher.cpu())
            runs[(group, use_graph)] = (torch.cat(zs), torch.stack(ls, 1), torch.stack(rs, 1), torch.cat(ts))
    assert (runs[(G, True)][2] > 0).all()
    for a, b in zip(runs[(G, True)], runs[(1, True)]):
        assert torch.equal(a, b), "grouped run differs from one volume at a time"
    for a, b in zip(runs[(G, True)], runs[(G, False)]):
        assert torch.equal(a, b), "graph replay differs from eager launches"


# ----------------------------------------------------------------------------- continual, refusals, end to end
def test_episodic_false_carries_student_and_teacher_and_keeps_restoring():
    from multimodal_tta_amd.registry import get_plugin
    cfg = petal_cfg(SMALL, ["w"], steps=2, lr=1e-3, group=1, episodic=False)
    _, hip = build_pair(SMALL)
    plug = get_plugin("petal_tta")(cfg).setup(hip, "cuda")
    ar = plug.rt.arena
    nt = ar.n_train
    states = []
    for i in range(3):
        before = (ar.params_all[0, :nt].clone(), plug.teacher[0].clone())
        r = plug.adapt_volume(volume(i)[0].cuda())
        assert (r["restored"] > 0).all(), f"volume {i}: a step restored nothing"
        states.append(before)
    src = ar.source[:nt]
    assert torch.equal(states[0][0], src) and torch.equal(states[0][1], src)
    for w, t in states[1:]:          # the next volume started from what the one before left
        assert not torch.equal(w, src) and not torch.equal(t, src)
    held = torch.zeros(nt, dtype=torch.bool, device=src.device)
    for r in ar.refs:
        if r.trainable:
            held[r.offset:r.offset + r.numel] = bits(ar.params_all[0, r.offset:r.offset + r.numel]) == bits(src[r.offset:r.offset + r.numel])
    share = float(held.float().mean())
    print(f"share of the trainable span at its source bits after 3 volumes: {share:.3f}")
    assert 0.0 < share < 1.0
    assert int(ar.step) == 6, "the optimizer's step counter did not run on"


def test_batchnorm_models_are_refused():
    from multimodal_tta_amd.registry import get_plugin
    _, hip = build_pair(BATCH)
    with pytest.raises(NotImplementedError, match="model.norm"):
        get_plugin("petal_tta")(petal_cfg(BATCH, ["w"], steps=1, group=1)).setup(hip, "cuda")


def test_seg_tta_eval_with_tta_petal():
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_petal", "method.steps=2", "method.episodic=false"])
    cfg["model"] = dict(SMALL)
    cfg["dataset"]["synthetic"]["num_volumes"] = 2
    cfg["dataset"]["synthetic"]["shape"] = [32, 32, 32]
    _, hip = build_pair(SMALL)
    loader = get_dataset_builder("brats")(cfg).get_loader("test")
    strat = get_evaluation_strategy("seg_tta_eval")(cfg)
    m = strat.evaluate_epoch(hip, loader, torch.device("cuda"))
    assert type(strat.plugin).__name__ == "FisherRestoreTTA" and strat.plugin.views == 4 and strat.plugin.quantile == 0.03
    assert {"et_dc", "tc_dc", "wt_dc", "avg_dc", "loss"} <= set(m)
    assert 0.0 <= m["avg_dc"] <= 1.0
