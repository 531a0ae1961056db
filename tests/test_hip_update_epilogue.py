"""The optimizer step in the epilogue of the transposed-read weight gradient (MMTTA_OPT_WGRAD_EPILOGUE_UPDATE, option 19:
wgrad_tr_upd_kernel) against the two launches it replaces - the weight-gradient kernel that writes its slab and
wgrad_update27_kernel that reads it back - on the same tensors in the same process: mmtta_conv_wgrad_update_sets from
identical starting state with option 19 at 1 and at 0.  A launch that plans one slab per set has the complete gradient of a
block in one workgroup, which then runs the same optim_update and the same image rounding on the same one-slab sums:
weights, moments, the bias and its moments and the bytes of both images are compared with torch.equal.

MMTTA_OPT_WGRAD_WORKGROUPS is 1 for these calls (and what it was afterwards), so that layers this small plan one slab.
Shapes are the smallest at which the form can go wrong: stride 1 (one column block per workgroup; tile 4 x 8 x 8 of dy) on
one tile, on two tiles that one workgroup walks, and on 5 x 9 x 10 where every border mask is live, with one, two and
three blocks on either channel side.

The stride-2 forms - paired column blocks (8^3 -> 4^3) under transform and raw staging, and the transposed convolution
(4^3 -> 8^3), whose module input is the dense operand - were built, passed these same cases, and measured slower than their
two launches (profiles/update_epilogue_ab.md): they are not part of the library.  Their cases stay, as calls that the query
declines and that must run the two launches under both settings.
"""
import ctypes as C

import pytest
import torch

import conv_geometry as cg
from test_hip_conv import cl_bf16

GPU = pytest.mark.gpu
OPT, OPT_RAW, WGRAD_WORKGROUPS = 19, 16, 4

# name: (cin, cout, stride, transposed, extents of x)
S1_SHAPES = [(4, 8, 8), (8, 8, 8), (5, 9, 10)]
FORMS = {
    "s1-32-32": (32, 32, 1, False, S1_SHAPES),
    "s1-64-32": (64, 32, 1, False, S1_SHAPES),
    "s1-32-96": (32, 96, 1, False, S1_SHAPES),
    "s2-32-64": (32, 64, 2, False, [(8, 8, 8)]),
    "convT-64-32": (64, 32, 2, True, [(4, 4, 4)]),
}
BUILT = ("s1-32-32", "s1-64-32", "s1-32-96")
CASES = [(f, s) for f, v in FORMS.items() for s in v[4]]
BATCHES = {"1-item": (1, 1), "3-sets-of-1": (3, 3), "1-set-of-2": (2, 1)}      # (batch items, parameter sets)
# optimizer, decay (SGD: with momentum / without, which keeps no first moment)
OPTIMS = [("adam", True), ("adam", False), ("adamw", True), ("adamw", False), ("sgd", True), ("sgd", False)]


class _Ctl:
    use_sets = True


def _layout(cin, cout):
    wnum = cin * cout * 27
    boff = (wnum + 3) // 4 * 4
    return wnum, boff, boff + (cout + 3) // 4 * 4


def _state(cin, cout, Q, seed):
    """Starting weights, bias and (non-zero: step 0 must not read them) moments of Q sets, on the CPU."""
    wnum, boff, total = _layout(cin, cout)
    g = torch.Generator().manual_seed(seed)
    P, M, V = torch.zeros(Q, total), torch.zeros(Q, total), torch.zeros(Q, total)
    P[:, :wnum] = 0.05 * torch.randn(Q, wnum, generator=g)
    P[:, boff:boff + cout] = 0.05 * torch.randn(Q, cout, generator=g)
    M[:, :wnum] = 1e-3 * torch.randn(Q, wnum, generator=g)
    V[:, :wnum] = 1e-6 * torch.rand(Q, wnum, generator=g)
    M[:, boff:boff + cout] = 1e-3 * torch.randn(Q, cout, generator=g)
    V[:, boff:boff + cout] = 1e-6 * torch.rand(Q, cout, generator=g)
    return P, M, V


def _operands(cin, cout, stride, transposed, shape, n, seed):
    c = cg.case("epi", cin, cout, 3, stride, transposed, (n,) + tuple(shape))
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    x = rnd(n, cin, *shape) * 1.5 + 0.25
    gy = rnd(n, cout, *cg.out_dhw(c))
    x[rnd(*x.shape) > 1.2] = -0.0
    gy[rnd(*gy.shape) > 1.2] = -0.0
    return cl_bf16(x), cl_bf16(gy), (rnd(n * cin).abs() + 0.5).cuda(), (rnd(n * cin) * 0.3).cuda()


def _update(cin, cout, stride, transposed, x, gy, nl, state, Q, opt, decay, bias, step0, want):
    """One mmtta_conv_wgrad_update_sets under the options as they are: everything it writes.  `want`: what the query must
    say first (None: not asked)."""
    from multimodal_tta_amd import _lib, ops
    wnum, boff, total = _layout(cin, cout)
    wshape = (cin, cout, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3)
    spec = ops.OptimSpec(name=opt, lr=1e-2, weight_decay=5e-2, momentum=0.9 if (opt == "sgd" and decay) else 0.0)
    op = ops.ConvOp(cin, cout, 3, stride, transposed, "cuda", dtype=ops.BF16, n_sets=Q)
    op.need_dgrad = True
    if Q > 1:
        op.set_param_sets(1, 1, total, 0, total, 0, _Ctl())
    assert op.plain_bf16_images()
    P, M, V = (t.cuda() for t in state)
    G = torch.zeros(Q, total, device="cuda")
    for q in range(Q):
        op.pack(P[q, :wnum].view(wshape), q)
    step = torch.full((1,), step0, dtype=torch.int32, device="cuda")
    bias_here = bias and not transposed            # (a transposed layer's bias gradient goes to b_grad)
    sl = slice(boff, boff + cout)
    target = op.update_target(spec, P[0, :wnum], M[0, :wnum], V[0, :wnum], P[0, sl] if bias_here else None,
                              M[0, sl] if bias_here else None, V[0, sl] if bias_here else None,
                              G[0, sl] if (bias and transposed) else None, decay, decay, step)
    if want is not None:
        tx, tdy = ops.desc_cl(x), ops.desc_cl(gy)
        sets = op._sets(op.d_fwd)
        got = int(_lib.load().mmtta_conv_wgrad_updates_in_epilogue(C.byref(op.d_fwd), C.byref(tx), C.byref(nl.struct()) if nl is not None else None,
                                                                    C.byref(tdy), C.byref(sets) if sets is not None else None))
        assert got == want, f"mmtta_conv_wgrad_updates_in_epilogue says {got}"
    # the slabs ([sets][27][CGp][CDp] floats at the head of the workspace) are written by the two launches only
    plan = op.wgrad_plan(x, gy)
    assert plan["nsl"] == 1 and plan["pre_chunks"] == 0, plan
    slab_bytes = Q * 27 * plan["CGp"] * plan["CDp"] * 4
    ws = ops.Workspace.get(max(slab_bytes, 1), x.device).view(-1)
    ws[:slab_bytes] = 0x5A
    op.wgrad_update(x, nl, gy, target)
    torch.cuda.synchronize()
    assert int(step) == step0, "the step counter is read, not advanced"
    if want is not None:
        untouched = bool((ops.Workspace.get(slab_bytes, x.device).view(-1)[:slab_bytes] == 0x5A).all())
        assert untouched == bool(want), "the slab is written exactly when the update is not in the epilogue"
    return dict(P=P, M=M, V=V, b_grad=G, fwd=op.packed_fwd, dgrad=op.packed_dgrad)


def _compare(form, shape, batch, eligible=True, raws=(3,)):
    from multimodal_tta_amd import ops
    if not ops.fused_update_enabled():
        pytest.fail("MMTTA_FUSED_UPDATE=0 is set: the fused entry point is switched off")
    cin, cout, stride, transposed = form
    n, Q = batch
    seed = 977 + 13 * cin + cout + 5 * n + Q + sum(shape)
    x, gy, sc, sh = _operands(cin, cout, stride, transposed, shape, n, seed)
    state = _state(cin, cout, Q, seed + 1)
    wnum, boff, total = _layout(cin, cout)
    before = cg.current_options(cg.GEOMETRY_KEYS + (OPT, OPT_RAW))
    for raw in raws:
        for nl in (None, ops.NL(sc, sc, relu=True, scale=sc, shift=sh)):
            for opt, decay in OPTIMS:
                for bias in (True, False):
                    for step0 in (0, 3):
                        got = {}
                        for on in (1, 0):
                            with cg.pinned({WGRAD_WORKGROUPS: 1, OPT: on, OPT_RAW: raw}):
                                got[on] = _update(cin, cout, stride, transposed, x, gy, nl, state, Q, opt, decay, bias, step0,
                                                  1 if (on and eligible) else 0)
                        what = (f"{cin} -> {cout} stride {stride}{' transposed' if transposed else ''} {shape} x{n} in {Q} sets, {opt}, "
                                f"decay {decay}, bias {bias}, step {step0}, {'norm-on-load x' if nl is not None else 'identity x'}, option 16 = {raw}")
                        assert not torch.equal(got[0]["P"][:, :wnum].cpu(), state[0][:, :wnum]), f"{what}: the step moved no weight"
                        for k in got[0]:
                            a, b = got[1][k], got[0][k]
                            assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {k}"
                            if a.dtype.is_floating_point:
                                assert torch.isfinite(b).all(), f"{what}: {k} of the two launches is not finite"
                            assert torch.equal(a, b), f"{what}: {k} differs between the update in the epilogue and the two launches"
    assert cg.current_options(cg.GEOMETRY_KEYS + (OPT, OPT_RAW)) == before


@GPU
@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("form,shape", CASES, ids=[f"{f}-{'x'.join(map(str, s))}" for f, s in CASES])
def test_update_in_the_epilogue_equals_the_two_launches(form, shape, batch):
    """Every form x optimizer kind x decay x bias x step 0 (reads no moments) and 3 x identity / real norm-on-load on x; the
    stride-2 forms (declined: see above) under raw (option 16 = 3: dy raw, an identity x raw too) and transform (0) staging."""
    raws = (3, 0) if FORMS[form][2] == 2 else (3,)
    _compare(FORMS[form][:4], shape, BATCHES[batch], eligible=form in BUILT, raws=raws)


@GPU
def test_a_declined_layer_takes_the_two_launches():
    """Cg = 40: a partial group of 8 in the second 32-row block.  The query says no under both settings, and the call gives
    what it gives with the option off."""
    _compare((40, 32, 1, False), (4, 8, 8), BATCHES["3-sets-of-1"], eligible=False)


@GPU
def test_unet_adaptation_is_the_same_with_and_without():
    """A three-level U-Net (32, 64, 128) on 16^3, two volumes side by side, two entropy-minimisation steps, option 19 on
    against off: the losses of every step and the final logits, bit for bit.  The launch geometry is the one tuned for many
    volumes in flight (one workgroup per block, one slab), under which the 32 -> 32 stride-1 convolutions of the model
    update in their epilogue."""
    from multimodal_tta_amd import _lib
    from multimodal_tta_amd._lib import BF16, CONV_FWD, ConvDesc, ParamSets
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_tta import SMALL, build_pair, root_cfg, volume

    model = dict(SMALL, channels=[32, 64, 128], strides=[2, 2])
    xs = torch.cat([volume(i, (16, 16, 16))[0] for i in range(2)]).cuda()
    res = {}
    for on in (1, 0):
        with cg.pinned({OPT: on}):
            cfg = root_cfg(model, steps=2, lr=1e-3, precision="bf16", group=2, tune_volumes=512, use_graph=False)
            _, hip = build_pair(model)
            plug = get_plugin("entmin_tta")(cfg).setup(hip, "cuda")
            assert plug.rt.fused_layers
            assert cg.current_options((WGRAD_WORKGROUPS,)) == {WGRAD_WORKGROUPS: 1}
            d = ConvDesc(CONV_FWD, 3, 1, 32, 32, BF16)
            x, dy = cg._fake_tensor(_lib, 1 << 30, 2, 32, (8, 8, 8), True), cg._fake_tensor(_lib, 1 << 40, 2, 32, (8, 8, 8), True)
            sets = ParamSets(1, 1, 1 << 20, 0, 1 << 20, 0, 1 << 10, 0)
            assert int(_lib.load().mmtta_conv_wgrad_updates_in_epilogue(C.byref(d), C.byref(x), None, C.byref(dy), C.byref(sets))) == on
            r = plug.adapt_volume(xs)
            z = plug.logits(r)
            torch.cuda.synchronize()
            res[on] = (r["losses"].clone(), z.clone())
    assert torch.isfinite(res[0][0]).all() and torch.isfinite(res[0][1]).all()
    assert torch.equal(res[1][0], res[0][0]), "losses differ"
    assert torch.equal(res[1][1], res[0][1]), "logits differ"
