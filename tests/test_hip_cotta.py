"""CoTTA adaptation (``cotta_tta``) on the GPU: the consistency loss against a float64 torch restatement, the teacher /
restore pass against the NumPy Philox restatement of tests/test_cotta_host.py, the plugin against a CoTTA restatement on
the oracle networks (deep-copied teacher, flipped views, the same restore mask mapped through ``Arena.refs``), and the
bitwise properties (graph replay = eager, grouped = one volume at a time, the returned logits = a plain eval forward of
the adapted replica)."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_cotta_host import restore_mask
from test_hip_memo import (BATCH, CLAMP, HEADS, SATURATED, SECOND_TRIP, check_second_trip, grad_buffer, marginal_log, memo_views,
                           second_trip_logits, stage)
from test_hip_tta import SMALL, build_pair, root_cfg, volume

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- float64 restatements
def consistency_loss(z, t, softmax):
    """Per-item consistency loss [N] of the logits z against the target t (logit(pbar), softmax head: log pbar); t carries
    no gradient and is held inside +-CLAMP as the ensemble holds its output."""
    t = t.detach()
    if softmax:
        return (-(t.exp() * F.log_softmax(z, 1)).sum(1)).flatten(1).mean(1)
    t = t.clamp(-CLAMP, CLAMP)
    return (-(torch.sigmoid(t) * F.logsigmoid(z) + torch.sigmoid(-t) * F.logsigmoid(-z))).flatten(1).mean(1)


def loss_reference(z, t, softmax):
    z = z.double().detach().requires_grad_(True)
    loss = consistency_loss(z, t.double(), softmax)
    loss.sum().backward()
    return loss.detach(), z.grad


def run_loss(z_cl, t_cl, softmax, dtype=torch.float32):
    from multimodal_tta_amd import ops
    g = grad_buffer(z_cl, dtype)
    partial = torch.empty(ops.consistency_partials(z_cl), dtype=torch.float64, device="cuda")
    loss = torch.full((z_cl.shape[0],), 123.0, device="cuda")
    ops.consistency_loss_items(z_cl, t_cl, g, partial, loss, softmax=softmax)
    torch.cuda.synchronize()
    return loss.cpu(), ops.from_cl(g.float()).cpu()


def make_target(logits, softmax):
    """What the teacher hands over: its logits (sigmoid head) or the fp32 log softmax of them (softmax head)."""
    return F.log_softmax(logits.double(), 1).float() if softmax else logits


def check_loss(z, t, softmax, generic):
    l_ref, g_ref = loss_reference(z, t, softmax)
    assert torch.isfinite(l_ref).all() and torch.isfinite(g_ref).all()
    z_cl, t_cl = stage(z, generic), stage(t, generic)
    for dtype in ((torch.float32, torch.bfloat16) if (not softmax and not generic) else (torch.float32,)):
        loss, g = run_loss(z_cl, t_cl, softmax, dtype)
        assert torch.isfinite(loss).all() and torch.isfinite(g).all()
        for a, b in zip(loss.tolist(), l_ref.tolist()):
            print(f"{dtype}: loss {a} vs {b}")
            assert abs(a - b) <= 1e-5 * abs(b), (a, b)
        gmax = g_ref.abs().max().item()
        if dtype == torch.float32:
            err = (g.double() - g_ref).abs().max().item()
            print(f"gradient error {err / gmax:.2e} of the maximum")
            assert err <= 2e-5 * gmax
        else:
            # the fp32 result rounded to bf16, bit-exact or 1 ulp of bf16 (2^-7 relative)
            g32 = run_loss(z_cl, t_cl, softmax, torch.float32)[1]
            want = g32.to(torch.bfloat16).float()
            assert ((g - want).abs() <= want.abs() * 2.0 ** -7).all()


# ----------------------------------------------------------------------------- 1. the consistency loss
@pytest.mark.parametrize("softmax,R,generic", HEADS)
@pytest.mark.parametrize("G", [1, 3])
def test_consistency_loss_matches_float64(softmax, R, generic, G):
    gen = torch.Generator().manual_seed(500 + 7 * R + G)
    z = torch.randn((G, R, 5, 6, 7), generator=gen) * 3.0
    t = make_target(torch.randn((G, R, 5, 6, 7), generator=gen) * 3.0, softmax)
    check_loss(z, t, softmax, generic)


@functools.lru_cache(maxsize=None)
def second_trip_consistency_reference(softmax):
    t = make_target(second_trip_logits(83), softmax)
    return (t,) + loss_reference(second_trip_logits(82), t, softmax)


@pytest.mark.parametrize("softmax,generic,dtype", SECOND_TRIP)
def test_consistency_loss_on_the_second_trip_of_the_walk(softmax, generic, dtype):
    """test_consistency_loss_matches_float64 at test_hip_memo.SECOND_TRIP_SHAPE: more voxels than one launch has threads, two
    items."""
    t, l_ref, g_ref = second_trip_consistency_reference(softmax)
    z_cl, t_cl = stage(second_trip_logits(82), generic), stage(t, generic)
    loss, g = run_loss(z_cl, t_cl, softmax, dtype)
    g32 = run_loss(z_cl, t_cl, softmax, torch.float32)[1] if dtype != torch.float32 else g
    check_second_trip(loss, g, g32, l_ref, g_ref, dtype)


@pytest.mark.parametrize("softmax,R,generic", HEADS)
@pytest.mark.parametrize("G", [1, 3])
def test_consistency_loss_is_finite_on_saturated_logits(softmax, R, generic, G):
    gen = torch.Generator().manual_seed(600 + R + G)
    shape = (G, R, 5, 6, 7)
    z = SATURATED[torch.randint(0, len(SATURATED), shape, generator=gen)]
    t = SATURATED[torch.randint(0, len(SATURATED), shape, generator=gen)]
    # rows saturated the same way and the opposite way on both inputs
    z[:, :, 0, 0, :], t[:, :, 0, 0, :] = 1e4, 1e4
    z[:, :, 0, 1, :], t[:, :, 0, 1, :] = -1e4, -1e4
    z[:, :, 0, 2, :], t[:, :, 0, 2, :] = 1e4, -1e4
    z[:, :, 0, 3, :], t[:, :, 0, 3, :] = -1e4, 1e4
    if softmax:
        z[:, 0, 0, 2, :], t[:, 1, 0, 2, :] = 2e4, 2e4          # a certain student against a teacher certain of another class
    check_loss(z, make_target(t, softmax), softmax, generic)


@pytest.mark.parametrize("softmax,R,generic,dtype", [(False, 3, False, torch.float32), (False, 3, False, torch.bfloat16),
                                                     (False, 3, True, torch.float32), (True, 4, False, torch.float32)])
def test_n_items_equal_n_single_item_calls(softmax, R, generic, dtype):
    gen = torch.Generator().manual_seed(6)
    N = 3
    z = torch.randn((N, R, 9, 8, 7), generator=gen) * 3.0
    t = make_target(torch.randn((N, R, 9, 8, 7), generator=gen) * 3.0, softmax)
    loss, g = run_loss(stage(z, generic), stage(t, generic), softmax, dtype)
    for k in range(N):
        one = run_loss(stage(z[k:k + 1], generic), stage(t[k:k + 1], generic), softmax, dtype)
        assert torch.equal(one[0], loss[k:k + 1]) and torch.equal(one[1], g[k:k + 1])


@pytest.mark.parametrize("softmax,R,generic", HEADS)
def test_own_logits_as_target_give_a_zero_gradient(softmax, R, generic):
    """target = the student's own logits: the gradient is exactly zero, saturated logits included.  (Softmax head: the
    target is the one-view ensemble of the same logits, the log softmax the teacher's path produces.)"""
    from multimodal_tta_amd import ops
    gen = torch.Generator().manual_seed(700 + R)
    z = torch.randn((2, R, 5, 6, 7), generator=gen) * 3.0
    z[1] = SATURATED[torch.randint(0, len(SATURATED), z[1].shape, generator=gen)]
    z_cl = stage(z, generic)
    t_cl = z_cl
    if softmax:
        n, d, h, w, r = z_cl.shape
        t_cl = ops.new_cl(n, d, h, w, r, "cuda", ldc=z_cl.stride(3))
        ops.memo_ensemble(z_cl, t_cl, [0], softmax=True)
    for dtype in ((torch.float32, torch.bfloat16) if (not softmax and not generic) else (torch.float32,)):
        loss, g = run_loss(z_cl, t_cl, softmax, dtype)
        assert torch.isfinite(loss).all() and torch.equal(g, torch.zeros_like(g))


# ----------------------------------------------------------------------------- 2. teacher EMA + stochastic restore
def bits(t):
    return t.contiguous().view(torch.int32)


def run_update(w, teacher, source, n, sets, alpha, p, seed, t, ordinals):
    from multimodal_tta_amd import ops
    w, teacher, source = w.cuda().clone(), teacher.cuda().clone(), source.cuda()
    step = torch.tensor([t], dtype=torch.int32, device="cuda")
    ords = torch.from_numpy(np.array(ordinals, dtype=np.uint32).view(np.int32)).cuda()
    partial = torch.full((ops.cotta_update_partials(n, sets),), -7, dtype=torch.int64, device="cuda")
    restored = torch.full((sets,), -7, dtype=torch.int64, device="cuda")
    ops.cotta_update_sets(w, teacher, source, n, sets, alpha, p, seed, step, ords, partial, restored)
    torch.cuda.synchronize()
    return w.cpu(), teacher.cpu(), restored.cpu()


def check_update(w0, t0, source, n, sets, alpha, p, seed, t, ordinals):
    w1, t1, restored = run_update(w0, t0, source, n, sets, alpha, p, seed, t, ordinals)
    for s in range(w0.shape[0]):
        mask = torch.from_numpy(restore_mask(n, seed, t, ordinals[s], p)) if s < sets else torch.zeros(n, dtype=torch.bool)
        want = torch.where(mask, source[:n], w0[s, :n])
        assert torch.equal(bits(w1[s, :n]), bits(want)), f"set {s}: the restored positions differ from the Philox mask"
        assert torch.equal(bits(w1[s, n:]), bits(w0[s, n:])) and torch.equal(bits(t1[s, n:]), bits(t0[s, n:])), "written past n"
        if s >= sets:
            assert torch.equal(bits(t1[s]), bits(t0[s]))
            continue
        assert int(restored[s]) == int(mask.sum()), (s, int(restored[s]), int(mask.sum()))
        ref = alpha * t0[s, :n].double() + (1.0 - alpha) * w0[s, :n].double()
        bound = 2.0 ** -22 * torch.maximum(t0[s, :n].abs(), w0[s, :n].abs()).double()
        assert ((t1[s, :n].double() - ref).abs() <= bound).all()
    return w1, t1, restored


@pytest.mark.parametrize("seed", [0, 0x9E3779B97F4A7C15])
def test_update_restores_the_philox_mask_and_averages_the_teacher(seed):
    gen = torch.Generator().manual_seed(31)
    n, G = 1003, 3                                   # no multiple of 4: the last three elements go one by one
    w = torch.randn((G + 1, 1008), generator=gen)
    teacher = torch.randn((G + 1, 1004), generator=gen)
    source = torch.randn(1008, generator=gen)
    ordinals = [5, 0, 4000000000]
    drawn = []
    for t in (1, 2):
        w1, _, restored = check_update(w, teacher, source, n, G, 0.9, 0.2, seed, t, ordinals)
        assert (restored > 100).all()
        drawn.append(w1)
    assert not torch.equal(drawn[0], drawn[1]), "the step does not enter the draw"


def test_update_covers_a_span_wider_than_its_grid():
    gen = torch.Generator().manual_seed(32)
    n = 4 * 4096 * 256 + 4 * 1000 + 2               # more quads than threads in flight: the grid-stride loop and the tail
    width = (n + 3) // 4 * 4
    w = torch.randn((1, width), generator=gen)
    teacher = torch.randn((1, width), generator=gen)
    source = torch.randn(width, generator=gen)
    _, _, restored = check_update(w, teacher, source, n, 1, 0.999, 0.01, 3, 7, [2])
    assert abs(int(restored[0]) - 0.01 * n) <= 5 * (0.01 * 0.99 * n) ** 0.5


def test_update_edge_values_of_alpha_and_p():
    gen = torch.Generator().manual_seed(33)
    n = 515
    w = torch.randn((2, 516), generator=gen)
    teacher = torch.randn((2, 516), generator=gen)
    teacher[0, 3], teacher[1, 7] = -0.0, 0.0
    source = torch.randn(516, generator=gen)
    w1, t1, restored = check_update(w, teacher, source, n, 2, 0.5, 0.0, 1, 1, [0, 1])
    assert torch.equal(bits(w1), bits(w)) and restored.tolist() == [0, 0], "p = 0 restored something"
    w1, t1, restored = check_update(w, teacher, source, n, 2, 1.0, 0.3, 1, 1, [0, 1])
    assert torch.equal(bits(t1), bits(teacher)), "alpha = 1 moved the teacher"
    assert (restored > 0).all()
    w1, t1, _ = check_update(w, teacher, source, n, 2, 0.0, 0.0, 1, 1, [0, 1])
    assert torch.equal(t1[:, :n], w[:, :n]), "alpha = 0: the teacher is the student"


# ----------------------------------------------------------------------------- the plugin against a CoTTA restatement
def cotta_cfg(model_cfg, axes, steps=3, lr=None, alpha=0.9, restore_p=0.2, seed=0, **method):
    """``lr=None``: the configured learning rate (the reference's)."""
    from multimodal_tta_amd.config import compose
    cfg = root_cfg(model_cfg, steps=steps, lr=1e-3 if lr is None else lr, **method)
    if lr is None:
        cfg["training"]["optimizers"]["adam"]["lr"] = compose(overrides=["task=brats", "model=unet"])["training"]["optimizers"]["adam"]["lr"]
    cfg["method"]["name"] = "cotta_tta"
    cfg["method"]["cotta"] = {"mirror_axes": list(axes), "alpha": alpha, "restore_p": restore_p, "seed": seed}
    return cfg


def layout_of(plug):
    ar = plug.rt.arena
    return [(r.name, r.offset, r.numel) for r in ar.refs if r.trainable], ar.n_train


def teacher_target(teacher, x, masks, softmax):
    """logit(pbar) resp. log pbar of the teacher's train-mode predictions over the mirrored views, no gradient."""
    with torch.no_grad():
        lp, lq = marginal_log(teacher(memo_views(x, masks)), masks, softmax)
        return lp if softmax else (lp - lq).clamp(-CLAMP, CLAMP)


def cotta_reference(model, xs, train_cfg, steps, masks, layout, alpha=0.9, restore_p=0.2, seed=0, ordinals=None,
                    episodic=True, softmax=False, missing=()):
    """CoTTA over the mirror views with torch autograd on the volumes ``xs`` served one after another: per volume the
    per-step losses and the final eval logits of the student."""
    import oracle
    from oracle.tta import apply_modality_mask, modality_mask, select_params
    (refs, n_train) = layout
    ordinals = list(range(len(xs))) if ordinals is None else ordinals
    source = copy.deepcopy(model.state_dict())
    teacher = copy.deepcopy(model)
    for p in teacher.parameters():
        p.requires_grad_(False)
    teacher.train()
    named = select_params(model, "all")
    opt, t, out = None, 0, []
    for x, ordinal in zip(xs, ordinals):
        if episodic or opt is None:
            model.load_state_dict(source)
            teacher.load_state_dict(source)
            opt, t = oracle.adam.build_optimizer(named, train_cfg), 0
        x = apply_modality_mask(x, modality_mask(x.shape[1], missing, 0.0, None))
        losses = []
        model.train()
        for _ in range(steps):
            target = teacher_target(teacher, x, masks, softmax)
            opt.zero_grad()
            loss = consistency_loss(model(x), target, softmax)[0]
            loss.backward()
            opt.step()
            t += 1
            losses.append(float(loss.detach()))
            mask = torch.from_numpy(restore_mask(n_train, seed, t, ordinal, restore_p))
            with torch.no_grad():
                student, teach = dict(model.named_parameters()), dict(teacher.named_parameters())
                for name, off, numel in refs:
                    teach[name].mul_(alpha).add_(student[name], alpha=1.0 - alpha)
                    m = mask[off:off + numel].view(student[name].shape)
                    student[name][m] = source[name].to(student[name].dtype)[m]
        model.eval()
        with torch.no_grad():
            out.append({"logits": model(x), "losses": losses})
    return out, teacher


def check_against_reference(z_hip, losses, out_ref, o64, y, softmax=False, bf16=False):
    """Tent's bounds, as tests/test_hip_memo.py::check_against_reference applies them.  fp32, against a
    float64 run of the restatement (``o64``): per-step loss 1e-4 relative, final logits within max(2e-3 of max|logits|, 3x
    the fp32 restatement's own distance from that run), mask voxels differing only where the float64 logit (softmax head: the
    float64 top-2 margin) lies within that bound of the threshold, Dice 1e-3.  bf16, against the fp32 restatement: loss 1e-2,
    logits 3e-2 of max|logits|, masks 1e-2, Dice 2e-2, and the bf16 path must have been taken."""
    import oracle
    steps = len(out_ref["losses"])
    losses = losses.cpu().reshape(-1).tolist()

    def masks_of(z):
        if softmax:
            return F.one_hot(z.argmax(1), z.shape[1]).permute(0, 4, 1, 2, 3)
        return torch.sigmoid(z) >= 0.5

    def dice(m):
        return oracle.binary_dice_iou(m.to(torch.uint8), (y > 0.5).to(torch.uint8))[0]

    z_ref = out_ref["logits"]
    if bf16:
        for t, (a, b) in enumerate(zip(losses, out_ref["losses"])):
            assert abs(a - b) <= 1e-2 * abs(b), f"step {t}: loss {a} vs reference {b}"
        err = (z_hip - z_ref).abs().max().item() / z_ref.abs().max().item()
        mism = (masks_of(z_hip) != masks_of(z_ref)).float().mean().item()
        ddice = (dice(masks_of(z_hip)) - dice(masks_of(z_ref))).abs().max().item()
        print(f"bf16: losses {losses}; logits {err:.2e}, masks {mism:.2e}, Dice {ddice:.2e}")
        assert err > 1e-6, "bf16 path not taken"
        assert err <= 3e-2 and mism <= 1e-2 and ddice <= 2e-2, (err, mism, ddice)
        return
    for t in range(steps):
        a, b, c = losses[t], out_ref["losses"][t], o64["losses"][t]
        print(f"step {t}: loss {a}, fp32 restatement {b}, float64 {c}")
        assert abs(a - c) <= 1e-4 * abs(c) + 1e-6, f"step {t}: loss {a}, fp32 {b}, fp64 {c}"
    z64 = o64["logits"]
    scale = z64.abs().max().item()
    e_ref = (z_ref.double() - z64).abs().max().item() / scale
    e_hip = (z_hip.double() - z64).abs().max().item() / scale
    bound = max(2e-3, 3.0 * e_ref)
    print(f"losses {losses}; logits {e_hip:.2e} (fp32 restatement {e_ref:.2e})")
    assert e_hip <= bound, f"HIP vs fp64 CoTTA {e_hip:.3e}; fp32 CoTTA vs fp64 CoTTA {e_ref:.3e}"
    m_hip, m_ref, m64 = masks_of(z_hip), masks_of(z_ref), masks_of(z64)
    if softmax:
        top2 = z64.topk(2, dim=1).values
        near = ((top2[:, 0] - top2[:, 1]) <= bound * scale).unsqueeze(1)
    else:
        near = z64.abs() <= bound * scale
    assert not torch.any((m_hip != m64) & ~near), "a mask voxel differs away from the threshold"
    d64 = dice(m64)
    dd_hip, dd_ref = (dice(m_hip) - d64).abs().max().item(), (dice(m_ref) - d64).abs().max().item()
    print(f"Dice {dd_hip:.2e} (fp32 restatement {dd_ref:.2e}), mask voxels differing {(m_hip != m64).float().mean().item():.2e}")
    assert dd_hip <= 1e-3, (dd_hip, dd_ref)


def run_both(model_cfg, cfg, vols, axes, float64=True, seed=42, softmax=False, **kw):
    """The plugin and the restatement (fp32, and float64 on request) on the volumes ``vols`` served one at a time."""
    from multimodal_tta_amd.config import get_config
    from multimodal_tta_amd.memo import view_masks
    from multimodal_tta_amd.registry import get_plugin
    masks = view_masks(axes)
    ref, hip = build_pair(model_cfg, seed=seed)
    plug = get_plugin("cotta_tta")(cfg).setup(hip, "cuda")
    c = cfg["method"]["cotta"]
    args = dict(alpha=c["alpha"], restore_p=c["restore_p"], seed=c["seed"],
                episodic=bool(get_config(cfg, "method.episodic", True)), softmax=softmax, **kw)
    steps = cfg["method"]["steps"]
    xs = [v[0] for v in vols]
    o64 = None
    if float64:
        o64, _ = cotta_reference(copy.deepcopy(ref).double(), [x.double() for x in xs], cfg["training"], steps, masks,
                                 layout_of(plug), **args)
    out_ref, _ = cotta_reference(ref, xs, cfg["training"], steps, masks, layout_of(plug), **args)
    results = []
    for x in xs:
        r = plug.adapt_volume(x.cuda())
        results.append({"logits": plug.logits(r).cpu(), "losses": r["losses"].cpu().clone(), "restored": r["restored"].cpu().clone()})
    return plug, results, out_ref, o64


@pytest.mark.parametrize("axes", [["h", "w"], []])
def test_cotta_matches_the_restatement(axes):
    cfg = cotta_cfg(SMALL, axes, steps=3, group=1)
    x, y = volume(0)
    plug, res, out_ref, o64 = run_both(SMALL, cfg, [(x, y)], axes)
    assert res[0]["losses"].shape == (3,) and res[0]["restored"].shape == (3,)
    check_against_reference(res[0]["logits"], res[0]["losses"], out_ref[0], o64[0], y)
    n_train = plug.rt.arena.n_train
    for t in range(3):          # the restored counts are the mask's
        assert int(res[0]["restored"][t]) == int(restore_mask(n_train, 0, t + 1, 0, 0.2).sum())
    ar = plug.rt.arena
    assert not torch.equal(plug.teacher[0], ar.source[:n_train]) and not torch.equal(plug.teacher[0], ar.params_all[0, :n_train])


def test_cotta_bf16_tracks_the_restatement():
    axes = ["h", "w"]
    cfg = cotta_cfg(SMALL, axes, steps=3, group=1, precision="bf16")
    x, y = volume(5)
    plug, res, out_ref, _ = run_both(SMALL, cfg, [(x, y)], axes, float64=False)
    check_against_reference(res[0]["logits"], res[0]["losses"], out_ref[0], None, y, bf16=True)


def test_cotta_softmax_head_matches_the_restatement():
    axes = ["h", "w"]
    mcfg = dict(SMALL, num_classes=4)
    cfg = cotta_cfg(mcfg, axes, steps=3, group=1)
    cfg["training"]["criterion"]["softmax"] = True
    cfg["training"]["criterion"]["sigmoid"] = False
    x, y = volume(1, R=4)
    plug, res, out_ref, o64 = run_both(mcfg, cfg, [(x, y)], axes, softmax=True)
    assert plug.softmax
    check_against_reference(res[0]["logits"], res[0]["losses"], out_ref[0], o64[0], y, softmax=True)


def test_cotta_missing_modality_masks_then_mirrors():
    axes = ["w"]
    mcfg = dict(SMALL, in_channels=2, num_classes=1)
    cfg = cotta_cfg(mcfg, axes, steps=2, group=1, missing_modalities=[1])
    x, y = volume(2, shape=(16, 48, 48), C=2, R=1)
    plug, res, out_ref, o64 = run_both(mcfg, cfg, [(x, y)], axes, seed=7, missing=[1])
    check_against_reference(res[0]["logits"], res[0]["losses"], out_ref[0], o64[0], y)


def test_cotta_deepfusion_matches_the_restatement():
    import oracle
    from multimodal_tta_amd.memo import view_masks
    from multimodal_tta_amd.models import MultimodalUNetDeepFusion
    from multimodal_tta_amd.registry import get_plugin
    axes = ["w"]
    mcfg = dict(name="unet_multimodal_deepfusion", num_modalities=4, num_classes=3, spatial_dims=3,
                channels=[4, 8, 16, 32, 64], strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)
    cfg = cotta_cfg(mcfg, axes, steps=2, group=2)
    torch.manual_seed(42)
    ref = oracle.MultimodalUNetDeepFusion(mcfg)
    hip = MultimodalUNetDeepFusion(mcfg)
    hip.load_state_dict(ref.state_dict())
    x, y = volume(2)
    with pytest.warns(UserWarning, match="method.group = 2 -> 1"):
        plug = get_plugin("cotta_tta")(cfg).setup(hip, "cuda")
    assert plug.group == 1
    o64, _ = cotta_reference(copy.deepcopy(ref).double(), [x.double()], cfg["training"], 2, view_masks(axes), layout_of(plug))
    out_ref, _ = cotta_reference(ref, [x], cfg["training"], 2, view_masks(axes), layout_of(plug))
    res = plug.adapt_volume(x.cuda())
    check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref[0], o64[0], y)


# ----------------------------------------------------------------------------- one step, stage by stage
def test_one_cotta_step_matches_torch_stage_by_stage(monkeypatch):
    """One eager step of the plugin read at every stage against torch on the same weights: the teacher's target and the
    student's logits (5e-4 of their maximum), the loss (1e-5 relative against the restatement on the recorded tensors, 1e-4
    against torch end to end), every parameter's gradient (2e-3 of its tensor's maximum) - the whole-network bounds of
    DESIGN.md section 6 - then the teacher after the step and the restored set."""
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.memo import view_masks
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_unet import feeds_norm
    axes = ["h", "w"]
    masks = view_masks(axes)
    cfg = cotta_cfg(SMALL, axes, steps=1, lr=1e-3, seed=11, group=1, use_graph=False)
    ref, hip = build_pair(SMALL)
    x, _ = volume(0)
    plug = get_plugin("cotta_tta")(cfg).setup(hip, "cuda")
    assert plug.views == len(masks) and not plug.rt.fused_layers
    rec = {}
    ensemble, loss_items, step, update = ops.memo_ensemble, ops.consistency_loss_items, plug.optimizer_step, ops.cotta_update_sets
    ar = plug.rt.arena
    nt = ar.n_train

    def spy_ensemble(zv, out, view_axes, softmax=False):
        ensemble(zv, out, view_axes, softmax=softmax)
        rec["axes"], rec["arena_at_teacher"] = list(view_axes), ar.params_all[0, :nt].cpu()

    def spy_loss(logits, target, dlogits, partial, loss, softmax=False):
        loss_items(logits, target, dlogits, partial, loss, softmax=softmax)
        rec["z"], rec["target"], rec["loss"] = ops.from_cl(logits).cpu(), ops.from_cl(target).cpu(), loss.cpu().clone()

    def spy_step(volumes=1, fused=False):
        rec["g"] = ar.grads_all[0, :nt].cpu()
        step(volumes, fused=fused)

    def spy_update(w, teacher, source, n, sets, *args):
        rec["w"], rec["teacher0"], rec["n"], rec["sets"] = w[0, :nt].cpu(), teacher[0].cpu(), n, sets
        update(w, teacher, source, n, sets, *args)

    monkeypatch.setattr(ops, "memo_ensemble", spy_ensemble)
    monkeypatch.setattr(ops, "consistency_loss_items", spy_loss)
    monkeypatch.setattr(plug, "optimizer_step", spy_step)
    monkeypatch.setattr(ops, "cotta_update_sets", spy_update)
    res = plug.adapt_volume(x.cuda(), ordinals=[9])
    source = ar.source[:nt].cpu()
    assert rec["axes"] == masks and rec["n"] == nt and rec["sets"] == 1
    assert torch.equal(rec["arena_at_teacher"], source), "the teacher's forward did not run on the teacher (= source at step 1)"
    ref.train()
    target = teacher_target(ref, x, masks, False)
    z = ref(x)
    loss = consistency_loss(z, target, False)[0]
    loss.backward()
    assert (rec["target"] - target).abs().max().item() <= 5e-4 * target.abs().max().item()
    assert (rec["z"] - z.detach()).abs().max().item() <= 5e-4 * z.abs().max().item()
    own = consistency_loss(rec["z"].double(), rec["target"].double(), False)[0].item()
    print(f"loss {rec['loss'].item()}, restatement on the recorded tensors {own}, torch end to end {loss.item()}")
    assert abs(rec["loss"].item() - own) <= 1e-5 * abs(own)
    assert abs(rec["loss"].item() - loss.item()) <= 1e-4 * abs(loss.item())
    named = dict(ref.named_parameters())
    for r in ar.refs:
        if r.trainable:
            want = named[r.name].grad.reshape(-1)
            got = rec["g"][r.offset:r.offset + r.numel]
            if feeds_norm(ref, r.name):
                wscale = named[r.name[:-len("bias")] + "weight"].grad.abs().max().item()
                assert got.abs().max().item() <= 2e-3 * wscale and want.abs().max().item() <= 2e-3 * wscale, r.name
                continue
            assert (got - want).abs().max().item() <= 2e-3 * want.abs().max().item(), r.name
    # the teacher after the step: alpha teacher + (1 - alpha) student-after-its-step, on the recorded spans
    assert torch.equal(rec["teacher0"], source) and not torch.equal(rec["w"], source)
    ema = 0.9 * rec["teacher0"].double() + (1.0 - 0.9) * rec["w"].double()
    bound = 2.0 ** -22 * torch.maximum(rec["teacher0"].abs(), rec["w"].abs()).double()
    assert ((plug.teacher[0].cpu().double() - ema).abs() <= bound).all()
    # the restored set: the Philox mask of (seed 11, step 1, ordinal 9), source bits there, the stepped student elsewhere
    mask = torch.from_numpy(restore_mask(nt, 11, 1, 9, 0.2))
    final = ar.params_all[0, :nt].cpu()
    assert torch.equal(bits(final), bits(torch.where(mask, source, rec["w"])))
    assert int(res["restored"][0]) == int(mask.sum()) and 0.15 * nt < int(mask.sum()) < 0.25 * nt


# ----------------------------------------------------------------------------- bit for bit
def test_cotta_group_equals_one_volume_at_a_time_and_graph_equals_eager():
    from multimodal_tta_amd.registry import get_plugin
    G = 3
    vols = [volume(i)[0] for i in range(G)]
    ordinals = [10, 11, 4]
    runs = {}
    for group, use_graph in ((G, True), (1, True), (G, False)):
        cfg = cotta_cfg(SMALL, ["w"], steps=3, lr=1e-3, group=group, tune_volumes=4, use_graph=use_graph)
        _, hip = build_pair(SMALL)
        plug = get_plugin("cotta_tta")(cfg).setup(hip, "cuda")
        if group == G:
            r = plug.adapt_volume(torch.cat(vols).cuda(), ordinals=ordinals)
            assert r["restored"].shape == (3, G)
            runs[(group, use_graph)] = (plug.logits(r).cpu(), r["losses"].cpu(), r["restored"].cpu(), plug.teacher.cpu())
        else:
            zs, ls, rs, ts = [], [], [], []
            for v, o in zip(vols, ordinals):
                r = plug.adapt_volume(v.cuda(), ordinals=[o])
                zs.append(plug.logits(r).cpu())
                ls.append(r["losses"].cpu())
                rs.append(r["restored"].cpu())
                ts.append(plug.teacher.cpu())
            runs[(group, use_graph)] = (torch.cat(zs), torch.stack(ls, 1), torch.stack(rs, 1), torch.cat(ts))
    assert (runs[(G, True)][2] > 0).all() and len({int(v) for v in runs[(G, True)][2][0]}) == G, "the volumes share a draw"
    for a, b in zip(runs[(G, True)], runs[(1, True)]):
        assert torch.equal(a, b), "grouped run differs from one volume at a time"
    for a, b in zip(runs[(G, True)], runs[(G, False)]):
        assert torch.equal(a, b), "graph replay differs from eager launches"


def test_default_ordinals_count_the_volumes_served():
    from multimodal_tta_amd.registry import get_plugin
    cfg = cotta_cfg(SMALL, [], steps=1, lr=1e-3, group=1)
    _, hip = build_pair(SMALL)
    plug = get_plugin("cotta_tta")(cfg).setup(hip, "cuda")
    x = volume(0)[0].cuda()
    nt = plug.rt.arena.n_train
    counts = [int(plug.adapt_volume(x)["restored"][0]) for _ in range(3)] + [int(plug.adapt_volume(x, ordinals=[1])["restored"][0])]
    assert counts == [int(restore_mask(nt, 0, 1, o, 0.2).sum()) for o in (0, 1, 2, 1)]
    with pytest.raises(ValueError, match="ordinals"):
        plug.adapt_volume(x, ordinals=[1, 2])


@pytest.mark.parametrize("group", [1, 2])
def test_returned_logits_are_the_plain_eval_forward_of_the_adapted_replica(group):
    from multimodal_tta_amd.registry import get_plugin
    cfg = cotta_cfg(SMALL, ["h", "w"], steps=2, lr=1e-3, group=group)
    _, hip = build_pair(SMALL)
    plug = get_plugin("cotta_tta")(cfg).setup(hip, "cuda")
    xs = torch.cat([volume(i)[0] for i in range(group)]).cuda()
    z = plug.logits(plug.adapt_volume(xs)).clone()
    rt = plug.rt
    source = rt.arena.source.clone()
    assert not torch.equal(rt.arena.params_all[0], source), "nothing adapted"
    for g in range(group):
        # replica g's adapted STUDENT weights as the one weight set of a plain eval forward
        _, twin = build_pair(SMALL)
        twin.configure_training(None, plug.no_decay_keys, plug.treat_1d)          # the plugin's arena layout
        twin.cuda()
        rt2 = twin.runtime(torch.device("cuda"))
        assert rt2.arena.total == rt.arena.total
        rt2.arena.params.copy_(rt.arena.params_all[g])
        twin.eval()
        with torch.no_grad():
            want = twin(xs[g:g + 1])
        assert torch.equal(z[g:g + 1], want)


# ----------------------------------------------------------------------------- continual and degenerate settings
def test_episodic_false_carries_teacher_and_student_to_the_next_volume():
    """Two volumes, student and teacher persisting: both against the restatement run over both, so the second volume's first
    target comes from the teacher the first volume left.  The learning rate is 1e-3 so that two steps move the prediction
    visibly: the second volume's first loss must differ from an episodic run's by more than 2e-4 relative - twice the 1e-4
    either loss is held to, the least difference the two checks together can tell apart."""
    axes = ["w"]
    vols = [volume(0), volume(1)]
    cfg = cotta_cfg(SMALL, axes, steps=2, lr=1e-3, group=1, episodic=False)
    plug, res, out_ref, o64 = run_both(SMALL, cfg, vols, axes)
    for k in range(2):
        check_against_reference(res[k]["logits"], res[k]["losses"], out_ref[k], o64[k], vols[k][1])
    # the step counter ran on: the second volume's draws are those of steps 3 and 4
    nt = plug.rt.arena.n_train
    assert [int(v) for v in res[1]["restored"]] == [int(restore_mask(nt, 0, t, 1, 0.2).sum()) for t in (3, 4)]
    cfg = cotta_cfg(SMALL, axes, steps=2, lr=1e-3, group=1, episodic=True)
    _, res_ep, ref_ep, _ = run_both(SMALL, cfg, vols, axes, float64=False)
    assert torch.equal(res_ep[0]["losses"], res[0]["losses"]), "the first volume does not depend on `episodic`"
    a, b = float(res[1]["losses"][0]), float(res_ep[1]["losses"][0])
    ra, rb = out_ref[1]["losses"][0], ref_ep[1]["losses"][0]
    print(f"second volume, first loss: continual {a} (restatement {ra}), episodic {b} (restatement {rb})")
    assert abs(b - rb) <= 1e-4 * abs(rb) + 1e-6
    assert abs(a - b) > 2e-4 * abs(b) and abs(ra - rb) > 2e-4 * abs(rb), "the teacher of the first volume did not reach the second"


def test_alpha_one_and_no_restore_is_self_training_against_the_frozen_source():
    cfg = cotta_cfg(SMALL, [], steps=3, group=1, alpha=1.0, restore_p=0.0)
    x, y = volume(3)
    plug, res, out_ref, o64 = run_both(SMALL, cfg, [(x, y)], [])
    ar = plug.rt.arena
    assert torch.equal(bits(plug.teacher[0]), bits(ar.source[:ar.n_train])), "alpha = 1 moved the teacher"
    assert res[0]["restored"].tolist() == [0, 0, 0]
    check_against_reference(res[0]["logits"], res[0]["losses"], out_ref[0], o64[0], y)


def test_alpha_one_keeps_the_teacher_after_every_step(monkeypatch):
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.registry import get_plugin
    cfg = cotta_cfg(SMALL, [], steps=3, lr=1e-3, group=1, alpha=1.0, restore_p=0.0, use_graph=False)
    _, hip = build_pair(SMALL)
    plug = get_plugin("cotta_tta")(cfg).setup(hip, "cuda")
    ar = plug.rt.arena
    update, seen = ops.cotta_update_sets, []

    def spy_update(w, teacher, *args):
        update(w, teacher, *args)
        seen.append(torch.equal(bits(teacher[0]), bits(ar.source[:ar.n_train])))

    monkeypatch.setattr(ops, "cotta_update_sets", spy_update)
    plug.adapt_volume(volume(3)[0].cuda())
    assert seen == [True, True, True]


def test_batchnorm_models_are_refused():
    from multimodal_tta_amd.registry import get_plugin
    _, hip = build_pair(BATCH)
    with pytest.raises(NotImplementedError, match="model.norm"):
        get_plugin("cotta_tta")(cotta_cfg(BATCH, ["w"], steps=1, group=1)).setup(hip, "cuda")


# ----------------------------------------------------------------------------- end to end
def test_seg_tta_eval_with_tta_cotta():
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_cotta", "method.steps=2", "method.episodic=false"])
    cfg["model"] = dict(SMALL)
    cfg["dataset"]["synthetic"]["num_volumes"] = 2
    cfg["dataset"]["synthetic"]["shape"] = [32, 32, 32]
    _, hip = build_pair(SMALL)
    loader = get_dataset_builder("brats")(cfg).get_loader("test")
    strat = get_evaluation_strategy("seg_tta_eval")(cfg)
    m = strat.evaluate_epoch(hip, loader, torch.device("cuda"))
    assert type(strat.plugin).__name__ == "MeanTeacherTTA" and strat.plugin.views == 4
    assert {"et_dc", "tc_dc", "wt_dc", "avg_dc", "loss"} <= set(m)
    assert 0.0 <= m["avg_dc"] <= 1.0
