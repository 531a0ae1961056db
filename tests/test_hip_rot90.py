"""Quarter-turn (rot90) views on the GPU: the staging kernels against ``torch.rot90`` / the intensity restatement, the
marginal-entropy loss and the ensemble against float64 torch restatements (views brought to the volume's frame with flip,
then transpose), the tiled loss kernel against the mirror kernel bit for bit, the rejection of non-square planes, and
``memo_tta`` / ``cotta_tta`` with ``rot90: {k: [1, 2, 3]}`` against their restatements, grouped and under graph capture.

The loops of the restatements are those of tests/test_hip_memo.py and tests/test_hip_cotta.py with the two places that know
what a view is (``memo_views``, ``marginal_log``) replaced by the code-aware forms below; every tolerance is the
corresponding mirror test's, through that test's own checking function."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_hip_cotta as tc
import test_hip_intensity as ti
import test_hip_memo as tm
from test_hip_tta import SMALL, build_pair, volume

pytestmark = pytest.mark.gpu

ROT = [0, 18, 3, 17]          # identity and torch.rot90(k = 1, 2, 3) in the (H, W) plane (tests/test_rot90_host.py derives them)
SQUARE8 = [0, 2, 18, 16, 3, 1, 17, 19]          # mirror_axes: [h], k: [1, 2, 3]
CODES = {2: [[0, 18], [0, 21]], 4: [ROT, [0, 2, 18, 16], [0, 20, 7, 5]], 8: [SQUARE8, [0, 23, 4, 16, 17, 22, 3, 20]]}


# ----------------------------------------------------------------------------- a view and its inverse, in torch
def to_view(t, code, d):
    """t with (D, H, W) at dimensions (d, d + 1, d + 2): the view with code ``code`` - H and W transposed where bit 4 is set,
    THEN mirrored along W, H, D of the result where bits 0, 1, 2 are set."""
    y = t.transpose(d + 1, d + 2) if code & 16 else t
    dims = [dim for bit, dim in ((4, d), (2, d + 1), (1, d + 2)) if code & bit]
    return torch.flip(y, dims) if dims else y


def to_frame(t, code, d):
    """The inverse: flip, then transpose."""
    dims = [dim for bit, dim in ((4, d), (2, d + 1), (1, d + 2)) if code & bit]
    y = torch.flip(t, dims) if dims else t
    return y.transpose(d + 1, d + 2) if code & 16 else y


def test_the_restated_views_are_torch_rot90():
    x = torch.randn(2, 3, 4, 6, 6)
    for k, code in ((1, 18), (2, 3), (3, 17)):
        assert torch.equal(to_view(x, code, 2), torch.rot90(x, k, dims=(3, 4)))
    for code in list(range(8)) + list(range(16, 24)):
        assert torch.equal(to_frame(to_view(x, code, 2), code, 2), x)


def marginal_log(z, codes, softmax):
    """tests/test_hip_memo.py::marginal_log for view codes: z [G*V,R,D,H,W], view v of volume g at item g*V+v in its own
    frame -> log pbar (and log qbar for the sigmoid head) [G,R,D,H,W] in the volumes' frame."""
    V = len(codes)
    G = z.shape[0] // V
    zs = z.reshape(G, V, *z.shape[1:])
    u = torch.stack([to_frame(zs[:, v], c, 2) for v, c in enumerate(codes)], 1)
    if softmax:
        return torch.logsumexp(F.log_softmax(u, dim=2), 1) - math.log(V), None
    return torch.logsumexp(F.logsigmoid(u), 1) - math.log(V), torch.logsumexp(F.logsigmoid(-u), 1) - math.log(V)


def memo_views(x, codes):
    """x [G,C,D,H,W] -> [G*V,C,D,H,W], item g*V+v = view v of volume g."""
    return torch.stack([to_view(x, c, 2) for c in codes], 1).reshape(-1, *x.shape[1:])


@pytest.fixture
def restated(monkeypatch):
    """The mirror tests' restatements, reading view codes."""
    for mod in (tm, tc):
        monkeypatch.setattr(mod, "marginal_log", marginal_log)
        monkeypatch.setattr(mod, "memo_views", memo_views)


# ----------------------------------------------------------------------------- 1. staging
def device_rows(base, C):
    from multimodal_tta_amd import ops
    G, D, H, W, _ = base.shape
    x = ops.new_cl(G, D, H, W, C, "cuda", ldc=4, dtype=base.dtype)
    (x if x._base is None else x._base).copy_(base)
    return x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [1, 2, 4])
@pytest.mark.parametrize("shape", [(5, 24, 24), (3, 16, 16), (2, 7, 7)])
def test_mirror_views_with_turned_codes_is_bit_exact(dtype, C, shape):
    from multimodal_tta_amd import ops
    G, (D, H, W) = 2, shape
    gen = torch.Generator().manual_seed(11 + C + D)
    for codes in (ROT, SQUARE8, [0, 16], [0, 23, 20, 6]):
        V = len(codes)
        base = torch.randn((G, D, H, W, 4), generator=gen).to(dtype)          # pad lanes carry values too
        x = device_rows(base, C)
        y = ops.new_cl(G * V, D, H, W, C, "cuda", ldc=4, dtype=dtype)
        yb = y if y._base is None else y._base
        yb.fill_(float("nan"))
        ops.mirror_views(x, y, codes)
        torch.cuda.synchronize()
        got = yb.cpu()
        for g in range(G):
            for v, c in enumerate(codes):
                assert torch.equal(ti.bits(got[g * V + v]), ti.bits(to_view(base[g], c, 0))), (codes, g, v)
            if codes is ROT:          # ... which for the quarter turns is torch.rot90
                for k in (1, 2, 3):
                    assert torch.equal(ti.bits(got[g * V + k]), ti.bits(torch.rot90(base[g], k, dims=(1, 2)))), (g, k)


def views_restated(base, C, codes, table, seed, ordinals, dtype=torch.float32):
    """tests/test_hip_intensity.py::views_restated for view codes: transformed in the volume's frame (the noise field is
    indexed there), then turned and mirrored."""
    G, V = base.shape[0], len(codes)
    nvox = base[0, ..., 0].numel()
    out = []
    for g in range(G):
        item = base[g].to(dtype)
        lo, hi = item.reshape(-1, 4).amin(0), item.reshape(-1, 4).amax(0)
        for v, c in enumerate(codes):
            noisy = v > 0 and bool((table[g, v, :, 3] > 0).any())
            noise = ti.noise_restated(nvox, seed, ordinals[g], v) if noisy else None
            t = item if v == 0 else ti.transform_restated(item, C, table[g, v], lo, hi, noise)
            out.append(to_view(t, c, 0))
    return torch.stack(out)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(5, 24, 24), (3, 16, 16)])
def test_augment_views_with_turned_codes(dtype, shape):
    """Three readings of one launch with the codes of the rotation group.  (a) identity rows: ``mirror_views``' bits.  (b)
    scale and shift only: x * a + b, two roundings, bit for bit against torch (the exact case of
    tests/test_hip_intensity.py).  (c) everything on: view v is, bit for bit, what the mirror-group launch writes for view v
    under the same table - the same row at the same frame voxel, noise included - moved to its turned place; and it sits
    within that file's bound (1e-5 of the largest value, bf16: 2^-7) of the restatement."""
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.intensity import view_parameters
    G, C, (D, H, W), ordinals = 2, 4, shape, [5, 9]
    base = ti.make_base(G, D, H, W, C, dtype, 19 + D, pad=3.5)
    # (a)
    got, _ = ti.run_kernels(base, C, ROT, ti.identity_table(G, 4, C), 0, ordinals)
    y = ops.new_cl(G * 4, D, H, W, C, "cuda", ldc=4, dtype=dtype)
    yb = y if y._base is None else y._base
    ops.mirror_views(device_rows(base, C), y, ROT)
    torch.cuda.synchronize()
    assert torch.equal(ti.bits(got), ti.bits(yb.cpu()))
    # (b)
    rng = np.random.default_rng(3)
    table = ti.identity_table(G, 4, C)
    table[:, 1:, :, 1] = rng.uniform(0.9, 1.1, (G, 3, C))
    table[:, 1:, :, 2] = rng.uniform(-0.1, 0.1, (G, 3, C))
    got, _ = ti.run_kernels(base, C, ROT, table, 0, ordinals)
    x32 = base.float()
    for g in range(G):
        for v, code in enumerate(ROT):
            want = x32[g].clone()
            if v > 0:
                for c in range(C):
                    want[..., c] = x32[g, ..., c] * torch.tensor(table[g, v, c, 1]) + torch.tensor(table[g, v, c, 2])
            want = to_view(want, code, 0).to(dtype)
            assert torch.equal(ti.bits(got[g * 4 + v][..., :C]), ti.bits(want[..., :C])), (g, v)
            assert torch.equal(ti.bits(got[g * 4 + v][..., C:]), ti.bits(to_view(base[g], code, 0)[..., C:]))          # the pad moves
    # (c)
    cfg = ti.spec([], copies=4, per_channel=True, seed=8, **ti.ALL_ON)
    table = view_parameters(cfg, ordinals, C)
    got, _ = ti.run_kernels(base, C, ROT, table, cfg.seed, ordinals)
    mirrored, _ = ti.run_kernels(base, C, [0, 2, 1, 3], table, cfg.seed, ordinals)
    for g in range(G):
        for v, (code, m) in enumerate(zip(ROT, [0, 2, 1, 3])):
            assert torch.equal(ti.bits(got[g * 4 + v]), ti.bits(to_view(to_frame(mirrored[g * 4 + v], m, 0), code, 0))), (g, v)
    want = views_restated(base, C, ROT, table, cfg.seed, ordinals)
    tol = (2.0 ** -7 if dtype == torch.bfloat16 else 1e-5) * want[..., :C].abs().max().item()
    assert (got[..., :C].float() - want[..., :C]).abs().max().item() <= tol


# ----------------------------------------------------------------------------- 2. the loss against float64
SHAPES = [(5, 24, 24), (3, 16, 16), (4, 7, 7)]          # edge tiles, whole tiles, less than a tile


@pytest.mark.parametrize("softmax,R,generic", tm.HEADS)
@pytest.mark.parametrize("V", [2, 4, 8])
@pytest.mark.parametrize("G", [1, 3])
def test_memo_loss_with_turned_views_matches_float64(restated, softmax, R, generic, V, G):
    """tests/test_hip_memo.py::check_loss, bounds and all (loss 1e-5 relative, fp32 gradient 2e-5 of its maximum, bf16
    gradient = the fp32 one rounded, within 1 ulp of bf16), on the tiled fast path (fp32 and bf16 gradients), the generic
    Bernoulli path and the categorical path."""
    for i, codes in enumerate(CODES[V]):
        for shape in SHAPES[i % 2:i % 2 + 2]:
            gen = torch.Generator().manual_seed(200 + 7 * R + V + G + shape[1])
            z = torch.randn((G * V, R, *shape), generator=gen) * 3.0          # independent logits per view
            tm.check_loss(z, codes, softmax, generic)


@pytest.mark.parametrize("softmax,R,generic", tm.HEADS)
def test_memo_loss_with_turned_views_is_finite_on_saturated_logits(restated, softmax, R, generic):
    gen = torch.Generator().manual_seed(300 + R)
    G, V = 2, 4
    z = tm.SATURATED[torch.randint(0, len(tm.SATURATED), (G * V, R, 5, 24, 24), generator=gen)]
    z[:, :, 0, 0, :] = 1e4 if not softmax else 0.0
    z[:, :, 0, 1, :] = -1e4 if not softmax else 0.0
    tm.check_loss(z, ROT, softmax, generic)


@pytest.mark.parametrize("softmax,R,generic,dtype", [(False, 3, False, torch.float32), (False, 3, False, torch.bfloat16),
                                                     (False, 3, True, torch.float32), (True, 4, False, torch.float32)])
def test_g_volumes_equal_g_single_volume_calls(softmax, R, generic, dtype):
    gen = torch.Generator().manual_seed(5)
    G, V = 3, 4
    z = torch.randn((G * V, R, 9, 24, 24), generator=gen) * 3.0
    loss, g = tm.run_loss(tm.stage(z, generic), ROT, softmax, dtype)
    for k in range(G):
        one = tm.run_loss(tm.stage(z[k * V:(k + 1) * V], generic), ROT, softmax, dtype)
        assert torch.equal(one[0], loss[k:k + 1]) and torch.equal(one[1], g[k * V:(k + 1) * V])


# ----------------------------------------------------------------------------- 3. the tiled kernel against the mirror kernel
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("R", [1, 3, 4])
@pytest.mark.parametrize("shape", [(5, 24, 24), (3, 16, 16), (2, 40, 40)])
def test_tiled_loss_has_the_mirror_kernels_gradient_bits(dtype, R, shape):
    """Logits z for the codes [0, 2, 1, 3] (the mirror kernel) and z' for [0, 18, 3, 17] (the tiled kernel) with the same
    frame-aligned rows in every view, z'_v = view_c'v(frame_cv(z_v)): every voxel then sees the same numbers in the same
    order v = 0..V-1, so the gradients brought back to the frame are the same bits; the losses sum the same terms in fp64 in
    another order and agree to 1e-12 relative."""
    G, mirrors = 2, [0, 2, 1, 3]
    gen = torch.Generator().manual_seed(41 + R + shape[1])
    z = torch.randn((G * 4, R, *shape), generator=gen) * 3.0
    z2 = torch.stack([to_view(to_frame(z[i], mirrors[i % 4], 1), ROT[i % 4], 1) for i in range(G * 4)])
    loss_a, g_a = tm.run_loss(tm.stage(z, False), mirrors, False, dtype)
    loss_b, g_b = tm.run_loss(tm.stage(z2, False), ROT, False, dtype)
    assert torch.isfinite(g_a).all() and g_a.abs().max().item() > 0
    for i in range(G * 4):
        fa, fb = to_frame(g_a[i], mirrors[i % 4], 1), to_frame(g_b[i], ROT[i % 4], 1)
        assert torch.equal(fa.contiguous().view(torch.int32), fb.contiguous().view(torch.int32)), i
    for a, b in zip(loss_a.tolist(), loss_b.tolist()):
        print(f"loss: mirror kernel {a!r}, tiled kernel {b!r}")
        assert abs(a - b) <= 1e-12 * abs(a)


# ----------------------------------------------------------------------------- 4. the ensemble
@pytest.mark.parametrize("softmax,R,generic", tm.HEADS)
@pytest.mark.parametrize("V", [2, 4, 8])
def test_memo_ensemble_with_turned_views_matches_float64(softmax, R, generic, V):
    """tests/test_hip_memo.py::test_memo_ensemble_matches_float64 with view codes: 2e-5 of max|result| inside the clamp,
    sign and clamp outside; the tiled gather (dense 16-byte rows), the generic path and the categorical head."""
    gen = torch.Generator().manual_seed(400 + R + V)
    G = 2
    for codes, shape in zip(CODES[V], SHAPES):
        for saturated in (False, True):
            if saturated:
                z = tm.SATURATED[torch.randint(0, len(tm.SATURATED), (G * V, R, *shape), generator=gen)]
            else:
                z = torch.randn((G * V, R, *shape), generator=gen) * 3.0
            lp, lq = marginal_log(z.double(), codes, softmax)
            ref = lp if softmax else lp - lq
            got = tm.run_ensemble(tm.stage(z, generic), codes, softmax)
            assert torch.isfinite(got).all()
            inside = ref.abs() < tm.CLAMP if not softmax else torch.ones_like(ref, dtype=torch.bool)
            scale = ref[inside].abs().max().item()
            err = (got.double() - ref)[inside].abs().max().item()
            print(f"ensemble {codes} saturated={saturated}: {err / scale:.2e} of max|result|")
            assert err <= 2e-5 * scale
            assert (got[~inside].abs() <= tm.CLAMP * (1 + 1e-6)).all() and (got[~inside].sign() == ref[~inside].sign()).all()


# ----------------------------------------------------------------------------- 5. non-square planes
def test_non_square_planes_are_rejected_at_the_entry_points_and_the_plugins():
    from multimodal_tta_amd import _lib, ops
    from multimodal_tta_amd.registry import get_plugin
    lib = _lib.load()
    z = ops.new_cl(2, 4, 6, 8, 3, "cuda", ldc=4, zero=True)
    g = ops.new_cl(2, 4, 6, 8, 3, "cuda", ldc=4, zero=True)
    out = ops.new_cl(1, 4, 6, 8, 3, "cuda", ldc=4, zero=True)
    partial = torch.zeros(ops.memo_partials(z, 2), dtype=torch.float64, device="cuda")
    loss = torch.zeros(1, device="cuda")
    for call in (lambda: ops.memo_loss_items(z, g, [0, 18], partial, loss), lambda: ops.memo_ensemble(z, out, [0, 17]),
                 lambda: ops.mirror_views(out, z, [0, 16])):
        with pytest.raises(ops.MmttaError, match=r"h = 6, w = 8"):
            call()
        assert b"view_axes[1]" in lib.mmtta_last_error()
    ops.memo_loss_items(z, g, [0, 3], partial, loss)          # the half turn is a pair of mirrors: any plane
    torch.cuda.synchronize()
    x, _ = volume(0, shape=(16, 32, 48))
    for method, make in (("memo", tm.memo_cfg), ("cotta", tc.cotta_cfg)):
        cfg = make(SMALL, [], steps=1, group=1)
        cfg["method"][method]["rot90"] = {"k": [1, 2, 3]}
        _, hip = build_pair(SMALL)
        plug = get_plugin(f"{method}_tta")(cfg).setup(hip, "cuda")
        with pytest.raises(ValueError, match=rf"method\.{method}\.rot90.*H = 32, W = 48"):
            plug.adapt_volume(x.cuda())
        cfg["method"][method]["rot90"] = {"k": [2]}
        _, hip = build_pair(SMALL)
        plug = get_plugin(f"{method}_tta")(cfg).setup(hip, "cuda")
        assert plug.view_axes == [0, 3]
        assert torch.isfinite(plug.logits(plug.adapt_volume(x.cuda()))).all()


# ----------------------------------------------------------------------------- 6. the plugins against their restatements
def rot_cfg(make, axes, k, **kw):
    cfg = make(SMALL, axes, **kw)
    cfg["method"][cfg["method"]["name"][:-4]]["rot90"] = {"k": list(k)}
    return cfg


@pytest.mark.parametrize("axes,k,ensemble", [([], [1, 2, 3], False), (["h"], [1, 2, 3], True), (["d"], [3], False)])
def test_memo_with_turned_views_matches_the_restatement(restated, axes, k, ensemble):
    """tests/test_hip_memo.py's MEMO restatement and bounds (``check_against_reference``), graph capture on."""
    from multimodal_tta_amd.registry import get_plugin
    cfg = rot_cfg(tm.memo_cfg, axes, k, steps=3, ensemble=ensemble, group=1, use_graph=True)
    ref, hip = build_pair(SMALL)
    ref0 = copy.deepcopy(ref)
    x, y = volume(0)
    plug = get_plugin("memo_tta")(cfg).setup(hip, "cuda")
    codes = plug.view_axes
    assert plug.views == (1 << len(axes)) * (1 + len(k)) and any(c & 16 for c in codes) and not plug.rt.fused_layers
    out_ref = tm.memo_reference(ref, x, cfg["training"], 3, codes, ensemble=ensemble)
    res = plug.adapt_volume(x.cuda())
    assert res["losses"].shape == (3,)
    staged = plug.rt.pool.cl("x_views", plug.views, 32, 32, 32, 4, ldc=4, zero=True, dtype=torch.float32)
    assert torch.equal(staged.permute(0, 4, 1, 2, 3).cpu(), memo_views(x, codes))
    tm.check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref, ref0, x, y, cfg, codes, ensemble=ensemble)


def test_memo_with_turned_views_bf16_tracks_the_restatement(restated):
    from multimodal_tta_amd.registry import get_plugin
    cfg = rot_cfg(tm.memo_cfg, [], [1, 2, 3], steps=3, group=1, precision="bf16")
    ref, hip = build_pair(SMALL)
    x, y = volume(5)
    out_ref = tm.memo_reference(ref, x, cfg["training"], 3, ROT)
    plug = get_plugin("memo_tta")(cfg).setup(hip, "cuda")
    res = plug.adapt_volume(x.cuda())
    tm.check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref, None, x, y, cfg, ROT, bf16=True)


def test_cotta_with_turned_views_matches_the_restatement(restated):
    """tests/test_hip_cotta.py's CoTTA restatement and bounds, graph capture on."""
    from multimodal_tta_amd.registry import get_plugin
    cfg = rot_cfg(tc.cotta_cfg, [], [1, 2, 3], steps=3, group=1, use_graph=True)
    ref, hip = build_pair(SMALL)
    x, y = volume(0)
    plug = get_plugin("cotta_tta")(cfg).setup(hip, "cuda")
    assert plug.views == 4 and plug.view_axes == ROT
    args = dict(alpha=0.9, restore_p=0.2, seed=0)
    o64, _ = tc.cotta_reference(copy.deepcopy(ref).double(), [x.double()], cfg["training"], 3, ROT, tc.layout_of(plug), **args)
    out_ref, _ = tc.cotta_reference(ref, [x], cfg["training"], 3, ROT, tc.layout_of(plug), **args)
    res = plug.adapt_volume(x.cuda())
    tc.check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref[0], o64[0], y)
    n_train = plug.rt.arena.n_train
    for t in range(3):
        assert int(res["restored"][t]) == int(tc.restore_mask(n_train, 0, t + 1, 0, 0.2).sum())


def test_memo_deepfusion_takes_turned_views_at_group_1(restated):
    import oracle
    from multimodal_tta_amd.models import MultimodalUNetDeepFusion
    from multimodal_tta_amd.registry import get_plugin
    mcfg = dict(name="unet_multimodal_deepfusion", num_modalities=4, num_classes=3, spatial_dims=3,
                channels=[4, 8, 16, 32, 64], strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)
    cfg = tm.memo_cfg(mcfg, [], steps=3, group=2)
    cfg["method"]["memo"]["rot90"] = {"k": [1]}
    torch.manual_seed(42)
    ref = oracle.MultimodalUNetDeepFusion(mcfg)
    hip = MultimodalUNetDeepFusion(mcfg)
    hip.load_state_dict(ref.state_dict())
    ref0 = copy.deepcopy(ref)
    x, y = volume(2)
    out_ref = tm.memo_reference(ref, x, cfg["training"], 3, [0, 18])
    with pytest.warns(UserWarning, match="method.group = 2 -> 1"):
        plug = get_plugin("memo_tta")(cfg).setup(hip, "cuda")
    assert plug.group == 1 and plug.view_axes == [0, 18]
    res = plug.adapt_volume(x.cuda())
    tm.check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref, ref0, x, y, cfg, [0, 18])


# ----------------------------------------------------------------------------- 7. bit for bit
@pytest.mark.parametrize("method", ["memo", "cotta"])
def test_a_group_of_two_equals_one_volume_at_a_time_and_graph_equals_eager(method):
    """Same ``tune_volumes``: a group of 2 volumes, the volumes one at a time, and the group without graph capture."""
    from multimodal_tta_amd.registry import get_plugin
    make = tm.memo_cfg if method == "memo" else tc.cotta_cfg
    G = 2
    vols = [volume(i)[0] for i in range(G)]
    runs = {}
    for group, use_graph in ((G, True), (1, True), (G, False)):
        cfg = rot_cfg(make, [], [1, 2, 3], steps=3, lr=1e-3, group=group, tune_volumes=8, use_graph=use_graph)
        _, hip = build_pair(SMALL)
        plug = get_plugin(f"{method}_tta")(cfg).setup(hip, "cuda")
        assert plug.view_axes == ROT
        if group == G:
            r = plug.adapt_volume(torch.cat(vols).cuda())
            runs[(group, use_graph)] = (plug.logits(r).cpu(), r["losses"].cpu())
        else:
            zs, ls = [], []
            for v in vols:
                r = plug.adapt_volume(v.cuda())
                zs.append(plug.logits(r).cpu())
                ls.append(r["losses"].cpu())
            runs[(group, use_graph)] = (torch.cat(zs), torch.stack(ls, 1))
    for a, b in zip(runs[(G, True)], runs[(1, True)]):
        assert torch.equal(a, b), "grouped run differs from one volume at a time"
    for a, b in zip(runs[(G, True)], runs[(G, False)]):
        assert torch.equal(a, b), "graph replay differs from eager launches"


@pytest.mark.parametrize("method", ["memo", "cotta"])
def test_the_default_block_is_the_block_absent_bit_for_bit(method):
    from multimodal_tta_amd.registry import get_plugin
    make = tm.memo_cfg if method == "memo" else tc.cotta_cfg
    x = volume(0)[0].cuda()
    out = []
    for block in (None, {"k": []}):
        cfg = make(SMALL, ["h", "w"], steps=2, lr=1e-3, group=1)
        if block is not None:
            cfg["method"][method]["rot90"] = block
        _, hip = build_pair(SMALL)
        plug = get_plugin(f"{method}_tta")(cfg).setup(hip, "cuda")
        r = plug.adapt_volume(x)
        out.append((plug.logits(r).cpu(), r["losses"].cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
