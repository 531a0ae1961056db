"""Per-volume norm parameter sets (``mmtta_norm_sets``, ``method.norm_sets``): a group of volumes adapts a model whose norm
layers carry parameters - BatchNorm3d (affines + running statistics), GroupNorm, affine InstanceNorm3d - each volume with
its own affines, Adam state and running statistics.

Like tests/test_hip_groups.py, every check is BITWISE: the ``_sets`` entry points against one plain call per set, the
per-item affine descriptor (``mmtta_norm_on_load.per_item``) against the plain [C] one item by item, and end to end a group
of volumes through the plugin against the same volumes one at a time."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_hip_conv import cl, ref_module  # noqa: E402
from test_hip_groups import _sets  # noqa: E402

# (kind, groups, training)
KINDS = [("BATCH", 1, True), ("BATCH", 1, False), ("GROUP", 2, True), ("GROUP", 2, False), ("INSTANCE", 1, True),
         ("INSTANCE", 1, False)]

C = 16
AFF_STRIDE = 52          # elements between the replicas of the affines (an arena replica stride: not C, multiple of 4)
G_OFF, B_OFF = 4, 28     # gamma / beta inside a replica
ST_STRIDE = 40           # elements between running-statistics replicas
RM_OFF, RV_OFF = 0, 20


def _replicas(sets, seed, c=C):
    """Affines [sets, AFF_STRIDE] and running statistics [sets, ST_STRIDE], different in every set."""
    gen = torch.Generator().manual_seed(seed)
    P = torch.zeros(sets, AFF_STRIDE)
    P[:, G_OFF:G_OFF + c] = 1.0 + 0.5 * torch.randn(sets, c, generator=gen)
    P[:, B_OFF:B_OFF + c] = 0.3 * torch.randn(sets, c, generator=gen)
    S = torch.zeros(sets, ST_STRIDE)
    S[:, RM_OFF:RM_OFF + c] = 0.2 * torch.randn(sets, c, generator=gen)
    S[:, RV_OFF:RV_OFF + c] = 0.5 + torch.rand(sets, c, generator=gen)
    return P.cuda(), S.cuda()


def _chain(kind, groups, training, y, dT, part, rows, P, S, sets=None):
    """finalize -> combine (a consumer) -> bwd_reduce -> bwd_finalize -> bwd_apply over a batch; ``sets`` None: the plain
    entry points with set 0's parameters.  Returns every intermediate."""
    from multimodal_tta_amd import ops

    k = ops.NORM_KINDS[kind]
    n, d, h, w, c = y.shape
    dev = y.device
    mean, rstd, scale, shift = (torch.full((n * c,), float("nan"), device=dev) for _ in range(4))
    gi, bi = (torch.full((n * c,), float("nan"), device=dev) for _ in range(2))
    scratch = torch.zeros(n * c * 2, dtype=torch.float64, device=dev)
    gam, bet = P[0, G_OFF:G_OFF + c], P[0, B_OFF:B_OFF + c]
    rm, rv = S[0, RM_OFF:RM_OFF + c], S[0, RV_OFF:RV_OFF + c]
    use_batch = training or k != ops.NORM_BATCH
    if sets is None:
        ops.norm_stats_finalize(k, groups, part, rows, n, c, d * h * w, 1e-5, use_batch, rm, rv, 0.1, mean, rstd, scratch,
                                gam, bet, scale, shift)
        nl = ops.NL(mean, rstd, gam, bet, True, scale, shift)
    else:
        ops.norm_stats_finalize_sets(k, groups, part, rows, n, c, d * h * w, 1e-5, use_batch, rm, rv, 0.1, mean, rstd, scratch,
                                     sets, gam, bet, scale, shift, gi, bi)
        nl = ops.NL(mean, rstd, gi, bi, True, scale, shift, per_item=True)
    # a consumer that combines from gamma / beta itself (no precombined form) and one that reads scale / shift
    raw = ops.NL(nl.mean, nl.rstd, nl.gamma, nl.beta, True, None, None, per_item=nl.per_item)
    out_raw = ops.new_cl(n, d, h, w, c, dev)
    ops.combine(y, raw, None, None, out_raw)
    out_pre = ops.new_cl(n, d, h, w, c, dev)
    ops.combine(y, nl, None, None, out_pre)
    brows = ops.reduce_rows_per_n(y)
    bpart = torch.zeros(n * brows * 2 * c, device=dev)
    ops.norm_bwd_reduce(dT, y, nl, bpart)
    m1, m2 = (torch.full((n * c,), float("nan"), device=dev) for _ in range(2))
    DG = torch.full_like(P, float("nan"))
    scratch.zero_()
    args = (k, groups, bpart, brows, n, c, d * h * w, gam, use_batch, m1, m2, DG[0, G_OFF:G_OFF + c], DG[0, B_OFF:B_OFF + c],
            False, scratch)
    if sets is None:
        ops.norm_bwd_finalize(*args)
    else:
        ops.norm_bwd_finalize_sets(*args, sets)
    dy = ops.new_cl(n, d, h, w, c, dev)
    ops.norm_bwd_apply(dT, y, nl, m1, m2, dy)
    torch.cuda.synchronize()
    return dict(mean=mean.view(n, c), rstd=rstd.view(n, c), scale=scale.view(n, c), shift=shift.view(n, c),
                combine_raw=out_raw.clone(), combine=out_pre.clone(), m1=m1.view(n, c), m2=m2.view(n, c), dy=dy.clone(),
                dgamma=DG[:, G_OFF:G_OFF + c].clone(), dbeta=DG[:, B_OFF:B_OFF + c].clone(),
                running_mean=S[:, RM_OFF:RM_OFF + c].clone(), running_var=S[:, RV_OFF:RV_OFF + c].clone(),
                gamma_items=gi.view(n, c), beta_items=bi.view(n, c))


# items_per_set > 1 matters for BatchNorm only (the other statistics are per item).  C = 16 takes the 8-channel combine /
# backward-apply kernels, C = 12 the generic elementwise ones
@pytest.mark.parametrize("c", [C, 12])
@pytest.mark.parametrize("kind,groups,training,ips", [k + (1,) for k in KINDS] + [("BATCH", 1, True, 2), ("BATCH", 1, False, 2)])
def test_norm_sets_chain_equals_one_plain_call_per_set(kind, groups, training, ips, c):
    """G = 3 sets (different gamma / beta / running statistics at non-trivial replica strides) through the ``_sets`` chain ==
    each set through the plain chain with N = items_per_set, bit for bit."""
    from multimodal_tta_amd import ops

    C = c
    G = 3
    N = G * ips
    torch.manual_seed(11)
    shape = (4, 6, 8)
    y = cl(torch.randn(N, C, *shape) * 1.5 + 0.25)
    dT = cl(torch.randn(N, C, *shape))
    rows = ops.reduce_rows_per_n(y)
    part = torch.zeros(N * rows * 2 * C, device="cuda")
    ops.channel_stats(y, part)
    P0, S0 = _replicas(G, 3, C)
    P, S = P0.clone(), S0.clone()
    together = _chain(kind, groups, training, y, dT, part, rows, P, S,
                      sets=ops.norm_sets(ips, AFF_STRIDE, ST_STRIDE))
    for q in range(G):
        it = slice(q * ips, (q + 1) * ips)
        Pq, Sq = P0[q:q + 1].clone(), S0[q:q + 1].clone()
        alone = _chain(kind, groups, training, y[it], dT[it], part.view(N, -1)[it].reshape(-1), rows, Pq, Sq)
        for name in ("mean", "rstd", "scale", "shift", "combine_raw", "combine", "m1", "m2", "dy"):
            assert torch.equal(alone[name], together[name][it]), f"{name} of set {q}"
        for name in ("dgamma", "dbeta", "running_mean", "running_var"):
            assert torch.equal(alone[name][0], together[name][q]), f"{name} of set {q}"
        assert torch.equal(together["gamma_items"][it], P0[q, G_OFF:G_OFF + C].expand(ips, C))
        assert torch.equal(together["beta_items"][it], P0[q, B_OFF:B_OFF + C].expand(ips, C))
    if kind == "BATCH" and training:
        assert not torch.equal(together["running_mean"], S0[:, RM_OFF:RM_OFF + C].cuda())     # the EMA update happened


def test_one_launch_norm_backward_honours_per_item_affines():
    """mmtta_norm_bwd_small (instance statistics, frozen affines) with per-item gamma / beta == the item alone."""
    from multimodal_tta_amd import ops

    G, c = 3, 32
    torch.manual_seed(2)
    y = cl(torch.randn(G, c, 4, 4, 4))
    dT = cl(torch.randn(G, c, 4, 4, 4))
    mean = torch.randn(G * c, device="cuda") * 0.1
    rstd = torch.rand(G * c, device="cuda") + 0.5
    gi = torch.randn(G * c, device="cuda")
    bi = torch.randn(G * c, device="cuda")
    nl = ops.NL(mean, rstd, gi, bi, True, per_item=True)
    assert ops.norm_bwd_small_ok(dT, y, nl, dT)
    dy = ops.new_cl(G, 4, 4, 4, c, "cuda")
    ops.norm_bwd_small(dT, y, nl, 64, dy)
    for g in range(G):
        s = slice(g * c, (g + 1) * c)
        one = ops.new_cl(1, 4, 4, 4, c, "cuda")
        ops.norm_bwd_small(dT[g:g + 1], y[g:g + 1], ops.NL(mean[s], rstd[s], gi[s], bi[s], True), 64, one)
        torch.cuda.synchronize()
        assert torch.equal(one[0], dy[g]), f"item {g}"


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("cin,cout,k,stride,shape", [(16, 32, 3, 1, (8, 8, 8)), (32, 32, 3, 1, (8, 8, 16)),
                                                     (16, 16, 1, 1, (4, 6, 8)), (32, 64, 3, 2, (8, 8, 16))])
def test_conv_reading_per_item_affine_x_norm_equals_item_by_item(cin, cout, k, stride, shape, dtype):
    """mmtta_conv_run_sets / mmtta_conv_wgrad_sets whose input carries a per-item-affine norm-on-load (with its precombined
    scale / shift) == the same convolution item by item with that item's plain [C] affines."""
    from multimodal_tta_amd import ops

    G = 3
    torch.manual_seed(7 + cin + cout)
    dt = ops.PRECISIONS[dtype]
    mods = [ref_module(cin, cout, k, stride, False) for _ in range(G)]
    wshape, wnum = tuple(mods[0].weight.shape), mods[0].weight.numel()
    wpad, bpad = (wnum + 3) // 4 * 4, (cout + 3) // 4 * 4
    W = torch.zeros(G, wpad, device="cuda")
    Bv = torch.zeros(G, bpad, device="cuda")
    for g, m in enumerate(mods):
        W[g, :wnum] = m.weight.detach().reshape(-1).cuda()
        Bv[g, :cout] = m.bias.detach().cuda()
    x_cl = cl(torch.randn(G, cin, *shape))
    mean = torch.randn(G * cin, device="cuda") * 0.1
    rstd = torch.rand(G * cin, device="cuda") + 0.5
    gi = torch.randn(G * cin, device="cuda")
    bi = torch.randn(G * cin, device="cuda") * 0.2
    scale = rstd * gi
    shift = bi - mean * scale

    def run(items, precombined):
        n = len(items)
        op = ops.ConvOp(cin, cout, k, stride, False, "cuda", dtype=dt, n_sets=n)
        for j, g in enumerate(items):
            op.pack(W[g, :wnum].view(wshape), j)
        Bl = torch.stack([Bv[g] for g in items]).contiguous()
        _sets(op, 1, 1, wpad, 0, bpad, 0, on=n > 1)
        if n > 1:
            xin = x_cl
            nl = ops.NL(mean, rstd, gi, bi, True, scale if precombined else None, shift if precombined else None,
                        per_item=True)
        else:
            g = items[0]
            s = slice(g * cin, (g + 1) * cin)
            xin = x_cl[g:g + 1]
            nl = ops.NL(mean[s], rstd[s], gi[s], bi[s], True, scale[s] if precombined else None,
                        shift[s] if precombined else None)
        n_, do, ho, wo, _ = op.out_shape(xin)
        y = ops.new_cl(n_, do, ho, wo, cout, "cuda")
        op.forward(xin, nl, Bl[0, :cout], y)
        gen = torch.Generator().manual_seed(99)
        gy_all = torch.randn(G, cout, do, ho, wo, generator=gen)
        gy = cl(gy_all if n > 1 else gy_all[items[0]:items[0] + 1])
        dw = torch.full((n, wpad), float("nan"), device="cuda")
        db = torch.full((n, bpad), float("nan"), device="cuda")
        op.wgrad(xin, nl, gy, dw[0, :wnum].view(wshape), db[0, :cout])
        torch.cuda.synchronize()
        return y.clone(), dw[:, :wnum].clone(), db[:, :cout].clone()

    together = run(list(range(G)), True)
    for g in range(G):
        alone = run([g], True)
        for name, a, b in zip(("forward", "weight gradient", "bias gradient"), alone, together):
            assert torch.equal(a[0], b[g]), f"{name} of item {g}"
    # per-item affines reach the convolution kernels through the precombined form only: without it the call is refused
    with pytest.raises(ops.MmttaError, match="precombined scale / shift"):
        run(list(range(G)), False)


# ---------------------------------------------------------------------------------------------------------- end to end
SMALL = dict(name="unet", in_channels=4, num_classes=3, spatial_dims=3, channels=[4, 8, 16, 32, 64],
             strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)
BATCH = dict(SMALL, norm="BATCH")
GROUPN = dict(SMALL, num_classes=4, channels=[8, 8, 16, 32, 64], norm=["GROUP", {"num_groups": 2}])
AFFINE_IN = dict(SMALL, norm=["INSTANCE", {"affine": True}])


def _bn_state(plug, g):
    return [tuple(t.clone() if t is not None else None for t in trip) for trip in plug.rt.replica_buffers(g)]


@pytest.mark.parametrize("model_cfg,params", [(BATCH, "norm_affine"), (BATCH, "all"), (GROUPN, "all"),
                                              (AFFINE_IN, "norm_affine")])
def test_norm_sets_group_equals_one_volume_at_a_time(model_cfg, params):
    """`group: 3, norm_sets: true` on a model with norm parameters: no fall-back, no warning; the losses of every step, the
    final logits and each volume's running statistics / num_batches_tracked == a `group: 1` run over the same volumes, bit
    for bit, graph replay included; a partial group (2 of 3) as well."""
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import build_pair, root_cfg, volume

    G = 3
    xs = [volume(i, (32, 32, 32))[0] for i in range(G)]
    outs, bn = {}, {}
    for group in (1, G):
        cfg = root_cfg(model_cfg, steps=3, lr=1e-3, group=group, tune_volumes=4, norm_sets=True, params=params)
        _, hip = build_pair(model_cfg)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            plug = get_plugin("entmin_tta")(cfg).setup(hip, "cuda")
        assert plug.group == group and plug.rt.group == group
        if group == 1:
            outs[1], bn[1] = [], []
            for x in xs:
                r = plug.adapt_volume(x.cuda())
                outs[1].append((r["losses"].clone(), plug.logits(r).clone()))
                bn[1].append(_bn_state(plug, 0))
        else:
            for rep in range(2):              # second pass: graph replay, episodic reset of every replica
                r = plug.adapt_volume(torch.cat(xs).cuda())
                outs[G] = (r["losses"].clone(), plug.logits(r).clone())
                bn[G] = [_bn_state(plug, g) for g in range(G)]
            r2 = plug.adapt_volume(torch.cat(xs[:2]).cuda())
            part = (r2["losses"].clone(), plug.logits(r2).clone())
            bn_part = [_bn_state(plug, g) for g in range(2)]
        torch.cuda.synchronize()
    for g in range(G):
        assert torch.equal(outs[1][g][0], outs[G][0][:, g]), f"losses of volume {g}"
        assert torch.equal(outs[1][g][1][0], outs[G][1][g]), f"logits of volume {g}"
        assert len(bn[1][g]) == len(bn[G][g])
        for a, b in zip(bn[1][g], bn[G][g]):
            for ta, tb in zip(a, b):
                assert (ta is None and tb is None) or torch.equal(ta, tb), f"running statistics of volume {g}"
    for g in range(2):
        assert torch.equal(outs[1][g][0], part[0][:, g]) and torch.equal(outs[1][g][1][0], part[1][g]), f"partial group, volume {g}"
        for a, b in zip(bn[1][g], bn_part[g]):
            for ta, tb in zip(a, b):
                assert (ta is None and tb is None) or torch.equal(ta, tb), f"partial group, running statistics of volume {g}"
    if model_cfg is BATCH:
        assert len(bn[1][0]) > 0 and int(bn[1][0][0][2]) == 3       # num_batches_tracked: one per adaptation step


def test_norm_sets_batchnorm_norm_affine_matches_oracle():
    """The grouped BatchNorm Tent-style run (norm affines adapt, the forward updates the running statistics) stays within the
    tolerance logits_close applies against oracle.adapt_volume, for every volume of the group."""
    import copy

    import oracle
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import build_pair, logits_close, root_cfg, volume

    G = 3
    cfg = root_cfg(BATCH, steps=3, lr=1e-3, group=G, norm_sets=True, params="norm_affine")
    ref, hip = build_pair(BATCH)
    plug = get_plugin("entmin_tta")(cfg).setup(hip, "cuda")
    xs = [volume(i)[0] for i in range(G)]
    r = plug.adapt_volume(torch.cat(xs).cuda())
    z = plug.logits(r).cpu()
    for g in range(G):
        src = copy.deepcopy(ref)
        out_ref = oracle.adapt_volume(copy.deepcopy(ref), xs[g], cfg["training"], steps=3, params="norm_affine")
        logits_close(z[g:g + 1], out_ref, src, xs[g], cfg["training"], steps=3, params="norm_affine")


def test_norm_affine_runtime_packs_one_image_per_frozen_convolution():
    """`params: norm_affine`: every convolution is frozen and identical in every replica - the runtime packs ONE image per
    convolution (both orientations), once, and none on the per-step packer."""
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import build_pair, root_cfg, volume

    G = 3
    cfg = root_cfg(BATCH, steps=2, lr=1e-3, group=G, norm_sets=True, params="norm_affine")
    _, hip = build_pair(BATCH)
    plug = get_plugin("entmin_tta")(cfg).setup(hip, "cuda")
    plug.adapt_volume(torch.cat([volume(i)[0] for i in range(G)]).cuda())
    rt = plug.rt
    ops_ = {id(c.op): c for c in rt.convs}
    assert all(c.frozen for c in rt.convs)
    assert rt._packer is None
    images = [it[2].data_ptr() for it in rt._packer_frozen.items]
    expected = sum(1 + (1 if c.op.need_dgrad else 0) for c in ops_.values())
    assert len(images) == expected and len(set(images)) == expected
    for c in ops_.values():
        assert c.op.sets_grouped[0].packed_outer == 0 and c.op.sets_grouped[0].weight_outer == 0


def test_seg_tta_eval_lanes_times_group_with_norm_sets():
    """seg_tta_eval with 2 lanes x group 3 on a BatchNorm model (norm_sets): the same per-volume table and metrics as one
    lane adapting one volume at a time (5 volumes: a partial last group)."""
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    from multimodal_tta_amd.models import UNet
    from test_hip_tta import root_cfg

    results = []
    for lanes, group in ((1, 1), (2, 3)):
        cfg = root_cfg(BATCH, steps=2, lr=1e-3, group=group, lanes=lanes, tune_volumes=6, norm_sets=True,
                       params="norm_affine")
        cfg["dataset"]["synthetic"]["num_volumes"] = 5
        cfg["dataset"]["synthetic"]["shape"] = [32, 32, 32]
        torch.manual_seed(42)
        hip = UNet(BATCH)
        loader = get_dataset_builder("brats")(cfg).get_loader("test")
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message="method.group")
            strat = get_evaluation_strategy("seg_tta_eval")(cfg)
            m = strat.evaluate_epoch(hip, loader, torch.device("cuda"))
        assert strat.group == group and strat.lanes == lanes
        results.append((m, strat.last_table.clone()))
    assert results[0][1].shape[0] == 5
    assert torch.equal(results[1][1], results[0][1]), "per-volume table differs from the one-volume-at-a-time run"
    assert results[1][0] == results[0][0]


def test_deepfusion_batchnorm_with_norm_sets_falls_back_with_a_reason():
    """Grouped norm parameters are not built for the deep-fusion encoder families: such a model falls back to group 1 and
    the warning names why."""
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_model, get_plugin

    cfg = compose(overrides=["task=brats", "model=unet_multimodal_deepfusion"])
    mcfg = dict(name="unet_multimodal_deepfusion", num_modalities=4, num_classes=3, spatial_dims=3, channels=[4, 8, 16, 32, 64],
                strides=[2, 2, 2, 2], num_res_units=2, norm="BATCH", act="RELU", dropout=0.0)
    cfg["model"] = mcfg
    cfg["method"]["group"] = 2
    cfg["method"]["norm_sets"] = True
    cfg["method"]["steps"] = 1
    model = get_model(mcfg["name"])(mcfg)
    with pytest.warns(UserWarning, match="method.group = 2 -> 1: .*parameter-free"):
        plug = get_plugin("entmin_tta")(cfg).setup(model, "cuda")
    assert plug.group == 1 and plug.rt.group == 1


@pytest.mark.parametrize("model_cfg,params,group,norm_sets", [(BATCH, "norm_affine", 3, True), (SMALL, ["model.2."], 1, False)])
def test_frozen_images_follow_weights_loaded_after_setup(model_cfg, params, group, norm_sets):
    """Frozen convolutions are not repacked on every step: weights loaded into the model afterwards (load_state_dict writes
    through the nn.Parameters, not through the arena's own tensors) must still reach their packed images - the facade's
    forward then equals a fresh model holding those weights, bit for bit, and so does the next adapted volume."""
    from multimodal_tta_amd.models import UNet
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import build_pair, root_cfg, volume

    cfg = root_cfg(model_cfg, steps=2, lr=1e-3, group=group, tune_volumes=4, norm_sets=norm_sets, params=params)
    _, hip = build_pair(model_cfg)
    plug = get_plugin("entmin_tta")(cfg).setup(hip, "cuda")
    x = volume(0)[0].cuda()
    plug.adapt_volume(x)                                    # packers built, frozen images packed from the old weights
    assert plug.rt._packer_frozen is not None
    _, other = build_pair(model_cfg, seed=7)
    new_state = {k: v.clone() for k, v in other.state_dict().items()}
    hip.load_state_dict(new_state)
    rt = plug.rt
    assert hip.runtime(torch.device("cuda", torch.cuda.current_device())) is rt      # the runtime stays cached
    fresh = UNet(model_cfg)
    fresh.load_state_dict(new_state)
    hip.eval()
    fresh.eval()
    with torch.no_grad():
        z = hip(x)
        z_ref = fresh(x)
    torch.cuda.synchronize()
    assert torch.equal(z, z_ref), "the facade's forward ran on stale packed images of the frozen convolutions"
    # the next volume: a plugin whose source weights are the new ones adapts exactly like a fresh plugin on them
    plug.rt.arena.snapshot_source()
    plug.rt.snapshot_buffers()
    r = plug.adapt_volume(x)
    _, hip2 = build_pair(model_cfg, seed=7)
    plug2 = get_plugin("entmin_tta")(cfg).setup(hip2, "cuda")
    r2 = plug2.adapt_volume(x)
    torch.cuda.synchronize()
    assert torch.equal(plug.logits(r), plug2.logits(r2)) and torch.equal(r["losses"], r2["losses"])
