"""The fused weight update (``mmtta_conv_wgrad_update_sets``): the 27-tap slab reduction steps the optimizer and repacks
both bf16 images in one pass.  Every check is BITWISE against the separate passes it replaces - the weight gradient
(``mmtta_conv_wgrad_sets``), the arena optimizer (``mmtta_optim_step_sets``) and the batched repack
(``mmtta_conv_pack_batched``) - per layer kind, optimizer, step, and group size, and end to end through the adaptation
plugin with ``MMTTA_FUSED_UPDATE=0`` against the default, each in a process of its own (the switch is read once)."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_hip_conv import cl, ref_module  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# (cin, cout, stride, transposed, (d, h, w))
KINDS = [
    (32, 48, 1, False, (8, 8, 16)),      # conv k3 s1 (ragged 48-column image)
    (32, 64, 2, False, (8, 8, 16)),      # conv k3 s2
    (64, 32, 2, True, (4, 4, 8)),        # ConvTranspose3d k3 s2 (its bias stays with the arena optimizer)
    (20, 48, 1, False, (8, 8, 8)),       # reduced side (cin) not a multiple of 8: a partial cg tile, zero-filled image columns
    (40, 20, 2, True, (4, 4, 8)),        # ConvTranspose3d with a ragged reduced side (cout = 20)
]
OPTS = [("adam", True), ("adam", False), ("adamw", True), ("sgd", True), ("sgd", False)]
GROUPS = [(1, 1), (8, 8), (8, 3)]        # (replicas G, volumes B): B < G updates B replicas


def _sets(op, total, on):
    class Ctl:
        use_sets = on
    op.set_param_sets(1, 1, total, 0, total, 0, Ctl())


@pytest.mark.parametrize("G,B", GROUPS)
@pytest.mark.parametrize("opt,decay", OPTS)
@pytest.mark.parametrize("cin,cout,stride,transposed,shape", KINDS)
def test_fused_update_equals_separate_passes(cin, cout, stride, transposed, shape, opt, decay, G, B):
    from multimodal_tta_amd import ops

    if not ops.fused_update_enabled():
        pytest.fail("MMTTA_FUSED_UPDATE=0 is set: the fused entry point is switched off")
    torch.manual_seed(11 + cin + cout + G + B)
    d, h, w = shape
    mod = ref_module(cin, cout, 3, stride, transposed)
    wshape, wnum = tuple(mod.weight.shape), mod.weight.numel()
    boff = (wnum + 3) // 4 * 4
    total = boff + (cout + 3) // 4 * 4
    spec = ops.OptimSpec(name=opt, lr=1e-2, weight_decay=5e-2, momentum=0.9 if opt == "sgd" else 0.0)
    P = torch.zeros(G, total, device="cuda")
    P[:, :wnum] = 0.05 * torch.randn(G, wnum, device="cuda")
    P[:, boff:boff + cout] = 0.05 * torch.randn(G, cout, device="cuda")
    M = torch.zeros(G, total, device="cuda")
    V = torch.zeros(G, total, device="cuda")
    M[:, :wnum] = 1e-3 * torch.randn(G, wnum, device="cuda")      # step 0 must not read these
    V[:, :wnum] = 1e-6 * torch.rand(G, wnum, device="cuda")
    x = cl(torch.randn(B, cin, d, h, w))
    on = G > 1

    def make_op():
        op = ops.ConvOp(cin, cout, 3, stride, transposed, "cuda", dtype=ops.BF16, n_sets=G)
        _sets(op, total, on)
        assert op.plain_bf16_images()
        return op

    # A: separate passes
    opA, PA, MA, VA, GA = make_op(), P.clone(), M.clone(), V.clone(), torch.zeros(G, total, device="cuda")
    stepA = torch.zeros(1, dtype=torch.int32, device="cuda")
    items = []
    for g in range(G):
        wv = PA[g, :wnum].view(wshape)
        items += [(opA.d_fwd, wv, opA.packed_image(False, g)), (opA.d_dgrad, wv, opA.packed_image(True, g))]
    packer = ops.BatchedPacker(items, "cuda")
    packer.run()
    # B: fused
    opB, PB, MB, VB, GB = make_op(), P.clone(), M.clone(), V.clone(), torch.zeros(G, total, device="cuda")
    stepB = torch.zeros(1, dtype=torch.int32, device="cuda")
    for g in range(G):
        opB.pack(PB[g, :wnum].view(wshape), g)
    bias_here = not transposed
    target = opB.update_target(spec, PB[0, :wnum], MB[0, :wnum], VB[0, :wnum],
                               PB[0, boff:boff + cout] if bias_here else None, MB[0, boff:boff + cout] if bias_here else None,
                               VB[0, boff:boff + cout] if bias_here else None, None if bias_here else GB[0, boff:boff + cout],
                               decay, decay, stepB)
    segs = [] if bias_here else [(boff, total - boff, decay)]
    table, total_left = ops.optim_segments_table(segs, "cuda") if segs else (torch.zeros(1, dtype=torch.int64, device="cuda"), 0)

    for t in range(3):
        gy = cl(torch.randn(B, cout, *opA.out_shape(torch.empty(1, d, h, w, 1))[1:4]))
        opA.wgrad(x, None, gy, GA[0, :wnum].view(wshape), GA[0, boff:boff + cout])
        ops.optim_step_sets(spec, PA, GA, MA, VA, total, total if decay else 0, B, stepA)
        packer.run()
        opB.wgrad_update(x, None, gy, target)
        ops.optim_step_segments(spec, PB, GB, MB, VB, table, len(segs), total_left, B, stepB)
        torch.cuda.synchronize()
        where = f"step {t}"
        assert int(stepA) == int(stepB) == t + 1, where
        assert torch.equal(PA, PB), f"weights / bias, {where}"
        assert torch.equal(MA, MB), f"first moments, {where}"
        if opt != "sgd":
            assert torch.equal(VA, VB), f"second moments, {where}"
        assert torch.equal(opA.packed_fwd, opB.packed_fwd), f"forward images, {where}"
        assert torch.equal(opA.packed_dgrad, opB.packed_dgrad), f"input-gradient images, {where}"
    assert not torch.equal(PA, P), "the step moved no weight"


CHILD = r"""
import json, sys, torch
sys.path.insert(0, sys.argv[1])
from multimodal_tta_amd.registry import get_plugin
from test_hip_tta import build_pair, root_cfg, volume
from test_hip_groups import WIDE
use_graph = sys.argv[2] == "1"
xs = [volume(i, (32, 32, 32))[0] for i in range(3)]
cfg = root_cfg(WIDE, steps=3, lr=1e-3, precision="bf16", group=3, tune_volumes=4, use_graph=use_graph)
_, hip = build_pair(WIDE)
plug = get_plugin("entmin_tta")(cfg).setup(hip, "cuda")
r = plug.adapt_volume(torch.cat(xs).cuda())                 # (graphs on: warm-up + capture)
r = plug.adapt_volume(torch.cat(xs).cuda())                 # (graphs on: replay after the episodic reset)
z = plug.logits(r)
ar = plug.rt.arena
torch.cuda.synchronize()
out = {"params": ar.params_all.cpu(), "m": ar.exp_avg_all.cpu(), "v": ar.exp_avg_sq_all.cpu(), "step": ar.step.cpu(),
       "logits": z.cpu(), "losses": r["losses"].cpu(), "counts": (z > 0).sum(dim=(2, 3, 4)).cpu()}
torch.save(out, sys.argv[3])
print(json.dumps({"fused_layers": len(plug.rt.fused_layers)}))
"""


@pytest.mark.parametrize("use_graph", [False, True])
def test_adapt_volume_fused_equals_separate_passes(tmp_path, use_graph):
    """A grouped U-Net adaptation (3 volumes, 3 steps): the default against MMTTA_FUSED_UPDATE=0, each in its own process -
    weights, both moments, the step counter, losses, logits and mask counts bit for bit."""
    res, info = {}, {}
    for flag in ("1", "0"):
        env = dict(os.environ, MMTTA_FUSED_UPDATE=flag)
        path = str(tmp_path / f"out{flag}.pt")
        p = subprocess.run([sys.executable, "-c", CHILD, HERE, "1" if use_graph else "0", path], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        info[flag] = json.loads(p.stdout.strip().splitlines()[-1])
        res[flag] = torch.load(path)
    assert info["1"]["fused_layers"] > 0 and info["0"]["fused_layers"] == 0, info
    for k in ("params", "m", "v", "step", "losses", "logits", "counts"):
        assert torch.equal(res["1"][k], res["0"][k]), f"{k} differs between the fused update and the separate passes"


def test_load_state_dict_between_volumes_is_picked_up():
    """Weights written from outside the step (load_state_dict) reach the fused layers' images before the next forward."""
    from multimodal_tta_amd.models import UNet
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_groups import WIDE
    from test_hip_tta import build_pair, root_cfg, volume

    x = volume(0, (32, 32, 32))[0].cuda()
    cfg = root_cfg(WIDE, steps=2, lr=1e-3, precision="bf16", episodic=False)
    _, hip = build_pair(WIDE)
    plug = get_plugin("entmin_tta")(cfg).setup(hip, "cuda")
    assert plug.rt.fused_layers
    plug.adapt_volume(x)
    torch.manual_seed(7)
    other = UNet(WIDE)
    hip.load_state_dict(other.state_dict())
    z = plug.logits(plug.adapt_volume(x, steps=0)).clone()
    _, hip2 = build_pair(WIDE)
    hip2.load_state_dict(other.state_dict())
    plug2 = get_plugin("entmin_tta")(cfg).setup(hip2, "cuda")
    z2 = plug2.logits(plug2.adapt_volume(x, steps=0))
    torch.cuda.synchronize()
    assert torch.equal(z, z2)


def test_facade_backward_after_setup_gives_plain_gradients():
    """The fused update belongs to the adaptation step only: after a plugin set the model up, the nn.Module facade's backward
    leaves the weights alone and returns the gradients a model without the fused update returns, bit for bit."""
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_groups import WIDE
    from test_hip_tta import build_pair, root_cfg, volume

    x = volume(0, (32, 32, 32))[0].cuda()
    cfg = root_cfg(WIDE, steps=1, lr=1e-3, precision="bf16", group=1)
    grads = {}
    for fused in (True, False):
        _, hip = build_pair(WIDE)
        plug = get_plugin("entmin_tta")(cfg)
        plug.fused_update = fused
        plug.setup(hip, "cuda")
        assert bool(plug.rt.fused_layers) == fused
        hip.train()
        before = [p.detach().clone() for p in hip.parameters()]
        for _ in range(2):                        # the second backward sees the first one's (unchanged) weights
            for p in hip.parameters():
                p.grad = None
            loss = torch.sigmoid(hip(x).float()).square().mean()
            loss.backward()
        torch.cuda.synchronize()
        for b, p in zip(before, hip.parameters()):
            assert torch.equal(b, p.detach()), "the facade backward moved a weight"
        grads[fused] = [p.grad.clone() for p in hip.parameters() if p.grad is not None]
    assert len(grads[True]) == len(grads[False]) > 0
    assert any(bool(g.abs().sum() > 0) for g in grads[True])
    for a, b in zip(grads[True], grads[False]):
        assert torch.equal(a, b)


def test_supervised_trainer_keeps_the_separate_passes():
    """The supervised trainer steps the optimizer over the whole arena: setting it up turns the fused update off."""
    from multimodal_tta_amd.registry import get_plugin
    from multimodal_tta_amd.trainer import SupervisedSegStep
    from test_hip_groups import WIDE
    from test_hip_tta import build_pair, root_cfg

    cfg = root_cfg(WIDE, steps=1, lr=1e-3, precision="bf16", group=1)
    _, hip = build_pair(WIDE)
    plug = get_plugin("entmin_tta")(cfg).setup(hip, "cuda")
    assert plug.rt.fused_layers
    tr = SupervisedSegStep(cfg).setup(hip, "cuda")
    assert not tr.rt.fused_layers and tr.rt.leftover is None
