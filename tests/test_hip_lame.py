"""LAME output refinement on the GPU: ``mmtta_lame_refine`` (tiled and generic route) against the float64 restatement of
``lame_reference.py``, the exact flip count, the bitwise properties (N items = N calls, two runs, inputs untouched, pad lanes)
and the plugin ``lame_tta`` (= ``ops.lame_refine`` on ``entmin_tta``'s logits, bit for bit).

Tolerance of the comparisons: |got - ref| <= 1e-5 + 1e-5 |ref| for weight <= 1.  For weight < 2 the map is a contraction (the
derivative of tanh(l / 2) is <= 1/2 and sum_j w_ij <= 1), so rounding does not accumulate over the iterations; the fp32 run of
the restatement sits at 9e-7 of the float64 run (``test_lame_host.py``), which leaves a factor of ten.  One case at weight 4
with T = 2 is held to the same bound; beyond that non-contractive settings are not compared.

Shapes are the smallest at which a tile can go wrong, not the workload's: exactly one 4 x 8 x 32 tile, one voxel more in every
axis, (9, 10, 35), (1, 5, 70) and (3, 17, 4).  Every case runs N = 2 different volumes."""
import functools

import numpy as np
import pytest
import torch

from lame_reference import decision_gap, flipped, lame

pytestmark = pytest.mark.gpu

TILE = (4, 8, 32)          # csrc/lame.hip: LAME_TD, LAME_TH, LAME_TW
SHAPES = [TILE, (5, 9, 33), (9, 10, 35), (1, 5, 70), (3, 17, 4)]
N = 2


def within(got, ref):
    err = np.abs(got.astype(np.float64) - ref)
    bound = 1e-5 + 1e-5 * np.abs(ref)
    return bool((err <= bound).all()), float((err / bound).max())


# ----------------------------------------------------------------------------- inputs and the shared references
@functools.lru_cache(maxsize=None)
def inputs(shape, R, C, seed, bf16):
    """Logits ~ N(0, 3^2) and inputs ~ N(0, 1) of N different volumes, fp32; with ``bf16`` the inputs are bf16-representable
    (the restatement starts from the rounded values)."""
    rng = np.random.default_rng(seed)
    l0 = rng.normal(0.0, 3.0, (N,) + tuple(shape) + (R,)).astype(np.float32)
    x = rng.normal(0.0, 1.0, (N,) + tuple(shape) + (C,)).astype(np.float32)
    if bf16:
        x = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    l0.setflags(write=False)
    x.setflags(write=False)
    return l0, x


@functools.lru_cache(maxsize=None)
def reference(shape, R, C, seed, bf16, conn, lam, sigma, T, softmax, present):
    """The float64 restatement of every item, computed once per case and shared (never written)."""
    l0, x = inputs(shape, R, C, seed, bf16)
    ref = np.stack([lame(l0[n], x[n], conn, lam, sigma, T, softmax, present=present) for n in range(N)])
    ref.setflags(write=False)
    return ref


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


def run(l0, x, conn, lam, sigma, T, softmax, present=None, xdtype=torch.float32, ldc=None, owns=True):
    """One call on fresh buffers -> (out [N,D,H,W,R], flipped [N], the tensors for further checks)."""
    from multimodal_tta_amd import ops
    zl, zl_base = device_cl(l0, ldc=ldc, owns=owns)
    out, out_base = device_cl(np.zeros_like(l0), ldc=ldc, owns=owns)
    work, work_base = device_cl(np.zeros_like(l0), ldc=ldc, owns=owns)
    xd, xd_base = device_cl(x, dtype=xdtype) if x is not None else (None, None)
    fl = torch.full((l0.shape[0],), -7, dtype=torch.int64, device="cuda")
    ops.lame_refine(zl, xd, out, work, fl, connectivity=conn, weight=lam, sigma=sigma, iterations=T, present=present,
                    softmax=softmax)
    torch.cuda.synchronize()
    keep = dict(l0=zl_base, out=out_base, work=work_base, x=xd_base)
    return out.cpu().numpy(), fl.cpu().numpy(), keep


# ----------------------------------------------------------------------------- the cases
def _cases():
    """A covering set over heads x connectivity x T (18 combinations) with sigma, the input storage, R and C cycling at
    co-prime periods; ``test_the_cases_cover_what_they_should`` checks what it covers."""
    out = []
    i = 0
    for softmax in (False, True):
        for conn in (6, 18, 26):
            for T in (1, 2, 7):
                sigma = (1.0, 0.0, 1.0, 1.0)[i % 4]
                bf16 = bool((i // 2) % 2)
                R = (3, 1, 4)[(i + i // 3) % 3]
                C = (4, 1, 2)[(i + i // 9) % 3]
                out.append((softmax, conn, sigma, bf16, T, R, C))
                i += 1
    return out


CASES = _cases()


def test_the_cases_cover_what_they_should():
    for softmax in (False, True):
        mine = [c for c in CASES if c[0] == softmax]
        assert {c[1] for c in mine} == {6, 18, 26} and {c[4] for c in mine} == {1, 2, 7}
        assert {c[2] for c in mine} == {0.0, 1.0} and {c[5] for c in mine} == {1, 3, 4}
        aff = [c for c in mine if c[2] > 0]
        assert {c[3] for c in aff} == {False, True} and {c[6] for c in aff} == {1, 2, 4}
        assert {c[1] for c in aff} == {6, 18, 26} and {c[4] for c in aff} == {1, 2, 7}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("softmax,conn,sigma,bf16,T,R,C", CASES)
def test_tiled_kernel_matches_the_float64_restatement(softmax, conn, sigma, bf16, T, R, C, shape):
    l0, x = inputs(shape, R, C, 100 + R + C, bf16)
    ref = reference(shape, R, C, 100 + R + C, bf16, conn, 1.0, sigma, T, softmax, None)
    got, fl, keep = run(l0, x, conn, 1.0, sigma, T, softmax, xdtype=torch.bfloat16 if bf16 else torch.float32)
    ok, worst = within(got, ref)
    print(f"worst error / bound = {worst:.3f}")
    assert ok, f"worst error / bound = {worst:.3f}"
    assert (fl >= 0).all() and (fl <= np.prod(shape) * (1 if softmax else R)).all()
    # the views own their pad lanes: rows are whole 16-byte stores, pad lanes zero - in `out` and, from T = 2 on, in `work`
    if R < 4:
        assert (keep["out"][..., R:] == 0).all(), "pad lanes of `out` are not zero"
        pad_work = keep["work"][..., R:]
        assert (pad_work == 0).all() if T >= 2 else torch.isnan(pad_work).all(), "pad lanes of `work`"


@pytest.mark.parametrize("shape", [(5, 9, 33), (3, 17, 4)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("softmax", [False, True])
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("conn,T,sigma", [(26, 7, 1.0), (18, 2, 1.0), (6, 1, 0.0)])
def test_generic_kernel_matches_the_float64_restatement(conn, T, sigma, bf16, softmax, shape):
    """R = 5, C = 6: rows of 8 elements, past the tiled route."""
    R, C = 5, 6
    l0, x = inputs(shape, R, C, 7, bf16)
    ref = reference(shape, R, C, 7, bf16, conn, 1.0, sigma, T, softmax, None)
    got, fl, keep = run(l0, x, conn, 1.0, sigma, T, softmax, xdtype=torch.bfloat16 if bf16 else torch.float32)
    ok, worst = within(got, ref)
    assert ok, f"worst error / bound = {worst:.3f}"
    assert torch.isnan(keep["out"][..., R:]).all(), "the generic route leaves pad lanes as they are"


@pytest.mark.parametrize("softmax", [False, True])
def test_generic_kernel_takes_thin_rows_the_tiled_route_cannot(softmax):
    """R = 3 in rows of 3 floats (no pad): not 16-byte rows, so the generic kernel runs - and agrees with the tiled one
    within the tolerance of either."""
    shape, R, C = (5, 9, 33), 3, 4
    l0, x = inputs(shape, R, C, 100 + R + C, False)
    ref = reference(shape, R, C, 100 + R + C, False, 26, 1.0, 1.0, 2, softmax, None)
    got, _, _ = run(l0, x, 26, 1.0, 1.0, 2, softmax, ldc=3)
    ok, worst = within(got, ref)
    assert ok, f"worst error / bound = {worst:.3f}"


@pytest.mark.parametrize("softmax", [False, True])
def test_pad_lanes_of_views_that_do_not_own_them_are_preserved(softmax):
    shape, R, C = (5, 9, 33), 3, 4
    l0, x = inputs(shape, R, C, 100 + R + C, False)
    ref = reference(shape, R, C, 100 + R + C, False, 26, 1.0, 1.0, 2, softmax, None)
    got, _, keep = run(l0, x, 26, 1.0, 1.0, 2, softmax, owns=False)
    assert within(got, ref)[0]
    assert torch.isnan(keep["out"][..., R:]).all() and torch.isnan(keep["work"][..., R:]).all(), "a pad lane was written"


@pytest.mark.parametrize("softmax", [False, True])
@pytest.mark.parametrize("bf16", [False, True])
def test_a_masked_out_channel_does_not_enter_the_affinity(bf16, softmax):
    """Channel 2 holds large values; the mask leaves it out.  The result equals the restatement without that channel and
    differs from the restatement with it."""
    shape, R, C = (9, 10, 35), 3, 4
    l0, x = inputs(shape, R, C, 31, bf16)
    x = x.copy()
    x[..., 2] *= 64.0          # (a power of two: still bf16-representable)
    present = (True, True, False, True)
    masked = np.stack([lame(l0[n], x[n], 26, 1.0, 1.0, 7, softmax, present=present) for n in range(N)])
    unmasked = np.stack([lame(l0[n], x[n], 26, 1.0, 1.0, 7, softmax) for n in range(N)])
    assert np.abs(masked - unmasked).max() > 1e-2, "the large channel makes no difference: the case shows nothing"
    got, fl, _ = run(l0, x, 26, 1.0, 1.0, 7, softmax, present=present, xdtype=torch.bfloat16 if bf16 else torch.float32)
    ok, worst = within(got, masked)
    assert ok, f"worst error / bound = {worst:.3f}"
    assert not within(got, unmasked)[0]


@pytest.mark.parametrize("softmax", [False, True])
def test_weight_four_with_two_iterations(softmax):
    shape, R, C = (9, 10, 35), 3, 4
    l0, x = inputs(shape, R, C, 100 + R + C, False)
    ref = reference(shape, R, C, 100 + R + C, False, 26, 4.0, 1.0, 2, softmax, None)
    got, _, _ = run(l0, x, 26, 4.0, 1.0, 2, softmax)
    ok, worst = within(got, ref)
    assert ok, f"worst error / bound = {worst:.3f}"


# ----------------------------------------------------------------------------- flipped
# Seeds chosen with the float64 restatement alone (conn 26, weight 1, sigma 1, T = 7, R = 3, C = 4): no final sigmoid logit within
# 1e-4 of 0, no softmax top-2 gap within 1e-4, and a count > 0.  The test asserts all three again.
FLIP_SEEDS = {(False, (4, 8, 32)): 1001, (False, (5, 9, 33)): 1000, (False, (9, 10, 35)): 1001, (False, (1, 5, 70)): 1000,
              (False, (3, 17, 4)): 1000, (True, (4, 8, 32)): 1000, (True, (5, 9, 33)): 1000, (True, (9, 10, 35)): 1000,
              (True, (1, 5, 70)): 1005, (True, (3, 17, 4)): 1004}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("softmax", [False, True])
def test_flipped_equals_the_restatement_exactly(softmax, shape):
    R, C = 3, 4
    seed = FLIP_SEEDS[(softmax, shape)]
    l0, x = inputs(shape, R, C, seed, False)
    ref = reference(shape, R, C, seed, False, 26, 1.0, 1.0, 7, softmax, None)
    assert min(decision_gap(ref[n], softmax) for n in range(N)) > 1e-4, "an element sits on its decision boundary"
    assert min(decision_gap(l0[n].astype(np.float64), softmax) for n in range(N)) > 0.0
    want = [flipped(l0[n], ref[n], softmax) for n in range(N)]
    assert sum(want) > 0, "nothing flips: the case shows nothing"
    got, fl, _ = run(l0, x, 26, 1.0, 1.0, 7, softmax)
    assert within(got, ref)[0]
    print("flipped:", fl.tolist())
    assert fl.tolist() == want


@pytest.mark.parametrize("softmax,seed", [(False, 2005), (True, 2002)])
def test_flipped_on_the_generic_route(softmax, seed):
    """R = 5, C = 6 at (5, 9, 33); the seeds were chosen like FLIP_SEEDS."""
    shape, R, C = (5, 9, 33), 5, 6
    l0, x = inputs(shape, R, C, seed, False)
    ref = reference(shape, R, C, seed, False, 26, 1.0, 1.0, 7, softmax, None)
    assert min(decision_gap(ref[n], softmax) for n in range(N)) > 1e-4, "an element sits on its decision boundary"
    want = [flipped(l0[n], ref[n], softmax) for n in range(N)]
    assert sum(want) > 0, "nothing flips: the case shows nothing"
    got, fl, _ = run(l0, x, 26, 1.0, 1.0, 7, softmax)
    assert within(got, ref)[0]
    assert fl.tolist() == want


# ----------------------------------------------------------------------------- bitwise properties
@pytest.mark.parametrize("R,C,bf16", [(3, 4, True), (5, 6, False)], ids=["tiled", "generic"])
@pytest.mark.parametrize("softmax", [False, True])
def test_items_equal_calls_runs_repeat_and_inputs_stay(softmax, R, C, bf16):
    shape = (5, 9, 33)
    l0, x = inputs(shape, R, C, 5, bf16)
    xd = torch.bfloat16 if bf16 else torch.float32
    both, fl_both, keep = run(l0, x, 26, 1.0, 1.0, 7, softmax, xdtype=xd)
    # the inputs, pad lanes included, hold the bits they held
    _, l0_base_again = device_cl(l0)
    _, x_base_again = device_cl(x, dtype=xd)
    bits = lambda t: t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    assert torch.equal(bits(keep["l0"]), bits(l0_base_again)), "`logits0` was written"
    assert torch.equal(bits(keep["x"]), bits(x_base_again)), "`x` was written"
    again, fl_again, _ = run(l0, x, 26, 1.0, 1.0, 7, softmax, xdtype=xd)
    assert np.array_equal(both.view(np.int32), again.view(np.int32)) and np.array_equal(fl_both, fl_again), "two runs differ"
    for n in range(N):
        one, fl_one, _ = run(l0[n:n + 1], x[n:n + 1], 26, 1.0, 1.0, 7, softmax, xdtype=xd)
        assert np.array_equal(one.view(np.int32), both[n:n + 1].view(np.int32)), f"item {n} differs from a call of its own"
        assert fl_one[0] == fl_both[n]


def test_sigma_zero_reads_no_input_and_parity_lands_in_out():
    shape, R = (5, 9, 33), 3
    l0, x = inputs(shape, R, 4, 100 + R + 4, False)
    for T in (1, 2, 3):
        a, fa, _ = run(l0, None, 18, 1.0, 0.0, T, False)
        b, fb, _ = run(l0, x, 18, 1.0, 0.0, T, False)
        assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(fa, fb)
        ref = reference(shape, R, 4, 100 + R + 4, False, 18, 1.0, 0.0, T, False, None)
        assert within(a, ref)[0], f"T = {T}: the result is not in `out`"


def test_ops_lame_refine_refuses_bad_arguments_on_the_device():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.ops import MmttaError
    l0, x = inputs(TILE, 3, 4, 1, False)
    zl, _ = device_cl(l0)
    out, _ = device_cl(l0)
    work, _ = device_cl(l0)
    xd, _ = device_cl(x)
    fl = torch.zeros(N, dtype=torch.int64, device="cuda")
    kw = dict(connectivity=26, weight=1.0, sigma=1.0, iterations=2)
    with pytest.raises(MmttaError, match="aliased"):
        ops.lame_refine(zl, xd, zl, work, fl, **kw)
    with pytest.raises(MmttaError, match="aliased"):
        ops.lame_refine(zl, xd, out, out, fl, **kw)
    with pytest.raises(MmttaError, match="sigma > 0"):
        ops.lame_refine(zl, None, out, work, fl, **kw)
    with pytest.raises(MmttaError, match="channel_mask"):
        ops.lame_refine(zl, xd, out, work, fl, present=[False] * 4, **kw)
    with pytest.raises(MmttaError, match="present"):
        ops.lame_refine(zl, xd, out, work, fl, present=[True] * 3, **kw)
    with pytest.raises(MmttaError, match="flipped"):
        ops.lame_refine(zl, xd, out, work, fl[:1], **kw)
    with pytest.raises(MmttaError, match="connectivity"):
        ops.lame_refine(zl, xd, out, work, fl, **dict(kw, connectivity=8))


# ----------------------------------------------------------------------------- the plugin
def lame_cfg(model_cfg, steps, iterations=5, weight=1.0, sigma=1.0, connectivity=26, name="lame_tta", **method):
    from test_hip_tta import root_cfg
    cfg = root_cfg(model_cfg, steps=steps, lr=1e-3, **method)
    cfg["method"]["name"] = name
    cfg["method"]["lame"] = {"iterations": iterations, "weight": weight, "sigma": sigma, "connectivity": connectivity}
    return cfg


def plugin_run(name, cfg, xs, model_cfg=None):
    """Adapt the volumes ``xs`` (one call each) with a fresh plugin -> (plugin, [logits_cl clone], [result])."""
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import SMALL, build_pair
    _, hip = build_pair(model_cfg or SMALL)
    plug = get_plugin(name)(cfg).setup(hip, "cuda")
    outs, results = [], []
    for x in xs:
        r = plug.adapt_volume(x.cuda())
        torch.cuda.synchronize()
        outs.append(r["logits_cl"].clone())
        results.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()})
    return plug, outs, results


def refine_like_the_plugin(plug, logits_cl, x, cfg, present=None, softmax=False):
    """``ops.lame_refine`` on ``logits_cl`` with the volume staged by ``plug``'s runtime (its storage, its row width)."""
    from multimodal_tta_amd import ops
    lm = cfg["method"]["lame"]
    x_cl = plug.rt.stage_input(x.cuda().float())
    n, d, h, w, r = logits_cl.shape
    ldc = (r + 3) // 4 * 4
    src = ops.new_cl(n, d, h, w, r, "cuda", ldc=ldc, zero=True)
    src.copy_(logits_cl)
    out = ops.new_cl(n, d, h, w, r, "cuda", ldc=ldc, zero=True)
    work = ops.new_cl(n, d, h, w, r, "cuda", ldc=ldc, zero=True)
    fl = torch.zeros(n, dtype=torch.int64, device="cuda")
    ops.lame_refine(src, x_cl, out, work, fl, connectivity=lm["connectivity"], weight=lm["weight"], sigma=lm["sigma"],
                    iterations=lm["iterations"], present=present, softmax=softmax)
    torch.cuda.synchronize()
    return out, fl


def test_zero_iterations_is_entmin_bit_for_bit():
    from test_hip_tta import SMALL, volume
    xs = [volume(0)[0], volume(1)[0]]
    cfg = lame_cfg(SMALL, steps=2, iterations=0, group=1)
    _, ent, ent_res = plugin_run("entmin_tta", cfg, xs)
    _, lam, lam_res = plugin_run("lame_tta", cfg, xs)
    for a, b, ra, rb in zip(ent, lam, ent_res, lam_res):
        assert torch.equal(a, b) and torch.equal(ra["losses"], rb["losses"])
        assert rb["flipped"].tolist() == [0]


@pytest.mark.parametrize("steps,precision", [(0, "fp32"), (2, "bf16")])
def test_plugin_equals_the_refinement_of_the_entmin_logits(steps, precision):
    """``steps: 0`` is pure LAME on the source model, ``steps: 2`` Tent followed by the refinement - in bf16 precision on a
    U-Net of the shipped width (at 32^3), whose staged volume, the affinity input, is bf16 with 8-byte voxels."""
    from test_hip_tta import SMALL, volume
    mcfg = dict(SMALL, channels=[32, 64, 128, 256, 512]) if precision == "bf16" else SMALL
    x = volume(2)[0]
    cfg = lame_cfg(mcfg, steps=steps, iterations=5, group=1, precision=precision)
    ent_plug, ent, _ = plugin_run("entmin_tta", cfg, [x], model_cfg=mcfg)
    lam_plug, lam, res = plugin_run("lame_tta", cfg, [x], model_cfg=mcfg)
    assert (lam_plug.rt.input_dtype() == torch.bfloat16) == (precision == "bf16")
    want, fl = refine_like_the_plugin(ent_plug, ent[0], x, cfg)
    assert torch.equal(lam[0], want), "the plugin's logits are not the refinement of entmin_tta's"
    assert torch.equal(res[0]["flipped"], fl) and int(fl.sum()) > 0
    assert not torch.equal(lam[0], ent[0])
    assert len(res[0]["losses"]) == steps


def test_plugin_group_equals_one_at_a_time_and_graph_equals_eager():
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import SMALL, build_pair, volume
    G = 3
    vols = [volume(i)[0] for i in range(G)]
    runs = {}
    for group, use_graph in ((G, True), (1, True), (G, False)):
        cfg = lame_cfg(SMALL, steps=2, iterations=4, group=group, tune_volumes=4, use_graph=use_graph)
        _, hip = build_pair(SMALL)
        plug = get_plugin("lame_tta")(cfg).setup(hip, "cuda")
        if group == G:
            r = plug.adapt_volume(torch.cat(vols).cuda())
            runs[(group, use_graph)] = (plug.logits(r).cpu(), r["flipped"].cpu(), r["losses"].cpu())
        else:
            rs = []
            for v in vols:          # (the results are views of the plugin's buffers: read before the next volume)
                r = plug.adapt_volume(v.cuda())
                rs.append((plug.logits(r).cpu(), r["flipped"].cpu().clone(), r["losses"].cpu().clone()))
            runs[(group, use_graph)] = (torch.cat([r[0] for r in rs]), torch.cat([r[1] for r in rs]),
                                        torch.stack([r[2] for r in rs], 1))
    assert (runs[(G, True)][1] > 0).all(), "the refinement is not in the run"
    for a, b in zip(runs[(G, True)], runs[(1, True)]):
        assert torch.equal(a, b), "grouped run differs from one volume at a time"
    for a, b in zip(runs[(G, True)], runs[(G, False)]):
        assert torch.equal(a, b), "graph replay differs from eager launches"


def test_plugin_masks_the_missing_modality_out_of_the_affinity():
    from test_hip_tta import SMALL, volume
    x = volume(3)[0]
    cfg = lame_cfg(SMALL, steps=2, iterations=5, group=1, missing_modalities=[1])
    ent_plug, ent, _ = plugin_run("entmin_tta", cfg, [x])
    _, lam, res = plugin_run("lame_tta", cfg, [x])
    masked, fl = refine_like_the_plugin(ent_plug, ent[0], x, cfg, present=[True, False, True, True])
    unmasked, _ = refine_like_the_plugin(ent_plug, ent[0], x, cfg)
    assert torch.equal(lam[0], masked) and torch.equal(res[0]["flipped"], fl)
    assert not torch.equal(masked, unmasked), "the staged volume does not hold the absent channel: the case shows nothing"


def test_plugin_on_the_softmax_head_and_the_deep_fusion_network():
    """The softmax head (R = 4), and the deep-fusion net, whose staged [n,D,H,W,M] volume is the affinity input."""
    import oracle
    from multimodal_tta_amd.models import MultimodalUNetDeepFusion
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import SMALL, volume
    mcfg = dict(SMALL, num_classes=4)
    cfg = lame_cfg(mcfg, steps=1, iterations=3, group=1)
    cfg["training"]["criterion"]["softmax"] = True
    cfg["training"]["criterion"]["sigmoid"] = False
    x = volume(1, R=4)[0]
    ent_plug, ent, _ = plugin_run("entmin_tta", cfg, [x], model_cfg=mcfg)
    lam_plug, lam, res = plugin_run("lame_tta", cfg, [x], model_cfg=mcfg)
    assert lam_plug.softmax
    want, fl = refine_like_the_plugin(ent_plug, ent[0], x, cfg, softmax=True)
    assert torch.equal(lam[0], want) and torch.equal(res[0]["flipped"], fl)

    dcfg = dict(name="unet_multimodal_deepfusion", num_modalities=4, num_classes=3, spatial_dims=3,
                channels=[4, 8, 16, 32, 64], strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)
    cfg = lame_cfg(dcfg, steps=1, iterations=3, group=1)
    x = volume(1)[0]
    got = {}
    for name in ("entmin_tta", "lame_tta"):
        torch.manual_seed(42)
        ref = oracle.MultimodalUNetDeepFusion(dcfg)
        hip = MultimodalUNetDeepFusion(dcfg)
        hip.load_state_dict(ref.state_dict())
        plug = get_plugin(name)(cfg).setup(hip, "cuda")
        r = plug.adapt_volume(x.cuda())
        torch.cuda.synchronize()
        got[name] = (plug, r["logits_cl"].clone(), r)
    want, fl = refine_like_the_plugin(got["entmin_tta"][0], got["entmin_tta"][1], x, cfg)
    assert torch.equal(got["lame_tta"][1], want) and torch.equal(got["lame_tta"][2]["flipped"], fl)


def test_seg_tta_eval_scores_the_refined_logits():
    """One pass of the evaluator over two synthetic volumes: its Dice is the Dice of the plugin's refined logits - and not the
    Dice of the logits before the refinement."""
    import oracle
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy, get_plugin
    from test_hip_tta import SMALL, build_pair
    cfg = lame_cfg(SMALL, steps=1, iterations=3, weight=4.0, group=1, lanes=1)
    cfg["dataset"]["synthetic"]["num_volumes"] = 2
    cfg["dataset"]["synthetic"]["shape"] = [32, 32, 32]
    loader = get_dataset_builder("brats")(cfg).get_loader("test")
    _, hip = build_pair(SMALL)
    strat = get_evaluation_strategy("seg_tta_eval")(cfg)
    got = strat.evaluate_epoch(hip, loader, torch.device("cuda"))
    assert type(strat.plugin).__name__ == "LaplacianRefinedTTA"

    def recomputed(name):
        _, model = build_pair(SMALL)
        plug = get_plugin(name)(cfg).setup(model, "cuda")
        acc = oracle.RegionAccumulator(["ET", "TC", "WT"])
        flips = 0
        for batch in loader:
            x, y = strat.check_batch(batch, torch.device("cuda"))
            for i in range(x.size(0)):
                r = plug.adapt_volume(x[i:i + 1])
                z = plug.logits(r).cpu()
                flips += int(r["flipped"].sum()) if "flipped" in r else 0
                pred, gt = oracle.masks_from_logits(z, y[i:i + 1].cpu(), 0.5)
                d, io, v = oracle.binary_dice_iou(pred, gt)
                acc.add(d, io, v, [list(batch["domain"])[i]])
        return acc.metrics(), flips

    want, flips = recomputed("lame_tta")
    assert flips > 0
    keys = [k for k in want if k != "loss"]          # (the recomputation books no loss: every Dice / IoU key, overall and per domain)
    assert {"et_dc", "tc_dc", "wt_dc", "avg_dc", "miou"} <= set(keys)
    for k in keys:
        assert got[k] == want[k], (k, got[k], want[k])
    before, _ = recomputed("entmin_tta")
    assert any(before[k] != want[k] for k in keys), "the refinement changed no Dice: the case shows nothing"
