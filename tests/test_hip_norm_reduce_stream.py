"""The streamed form of the two-stage channel reduction (csrc/pointwise.hip: channel_reduce_stream_kernel) writes, bit for
bit, the partial rows of the kernel it replaces.

tests/golden/norm_reduce_rows.npz holds `part` of every case of tests/golden/make_norm_reduce_rows.py as the commit before
the streamed form wrote it (one workgroup per row, one voxel quad per trip).  The inputs are rebuilt from the same seeds;
any re-scheduling of the first stage has to keep, per (row, channel), the voxels of a lane, their order, the order of the
lane partials and the contraction of every product-sum.  The cases that the streamed form does not take (rows of exactly
3 channels, a W-slice of a wider tensor) are in the same file and must not move either.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_norm_reduce_rows", os.path.join(GOLDEN, "make_norm_reduce_rows.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()
CASES = GEN.cases()


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "norm_reduce_rows.npz")) as f:
        return {k: f[k] for k in f.files}


def test_fixture_holds_every_case(golden):
    assert sorted(golden) == sorted(c.name for c in CASES)


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c.name for c in CASES])
def test_partial_rows_are_bit_identical(golden, index):
    case = CASES[index]
    got = GEN.run_case(case, index)
    want = torch.from_numpy(golden[case.name])
    assert got.shape == want.shape
    assert not bool(torch.isnan(got).any()), "a (row, sum, channel) was left unwritten"
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        r, s, c = (int(v) for v in bad[0])
        pytest.fail(f"{case.name}: {len(bad)} of {got.numel()} values differ, first at row {r} sum {s} channel {c}: "
                    f"{got[r, s, c].item():.9g} vs {want[r, s, c].item():.9g}")


def test_norm_layer_backward_end_to_end():
    """engine.NormLayer.backward (reduce -> finalize -> apply, bf16-stored activation and gradients) on 16^3 x 32 channels
    against fp32 torch autograd, with the tolerance of test_hip_pointwise.test_norm_forward_backward (rel 2e-4, abs 2e-6):
    as it stands for the fp32 sums m1 / m2 that the reduce pass feeds the apply pass; for dx, which this path stores as
    bf16, plus the one rounding of that store (the unit roundoff of bf16, 8 significand bits: 2^-8 relative)."""
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.engine import NormLayer, Pool

    gen = torch.Generator().manual_seed(5)
    n, c, d, h, w = 2, 32, 16, 16, 16
    y = (torch.randn((n, c, d, h, w), generator=gen) * 1.7 + 0.3).to(torch.bfloat16).float().requires_grad_(True)
    gout = torch.randn((n, c, d, h, w), generator=gen).to(torch.bfloat16).float()
    F.relu(F.instance_norm(y, eps=1e-5)).backward(gout)

    def cl16(t):
        out = ops.new_cl(n, d, h, w, c, "cuda", ldc=ops.row_pad(c, torch.bfloat16), dtype=torch.bfloat16)
        out.copy_(t.detach().permute(0, 2, 3, 4, 1))
        return out

    y16, g16 = cl16(y), cl16(gout)
    rows = ops.reduce_rows_per_n(y16)
    part = torch.empty(n * rows * 2 * c, device="cuda")
    ops.channel_stats(y16, part)
    mean, rstd = torch.empty(n * c, device="cuda"), torch.empty(n * c, device="cuda")
    scratch = torch.empty(n * c * 2, dtype=torch.float64, device="cuda")
    ops.norm_stats_finalize(ops.NORM_INSTANCE, 1, part, rows, n, c, d * h * w, 1e-5, True, None, None, 0.1, mean, rstd, scratch)
    nl = ops.NL(mean, rstd, None, None, relu=True)
    layer = NormLayer("INSTANCE", c)
    assert d * h * w > ops.small_norm_backward_max(), "the case must take the three-pass backward"
    dy = torch.empty_like(g16)
    pool = Pool(torch.device("cuda"))
    layer.backward(pool, "t", g16, y16, nl, dy, training=True)
    torch.cuda.synchronize()
    # what the reduce pass feeds the apply pass (fp32, no storage rounding): mean dz and mean dz * xhat per (item, channel)
    yd = y.detach().double()
    xhat = (yd - yd.mean((2, 3, 4), keepdim=True)) / (yd.var((2, 3, 4), unbiased=False, keepdim=True) + 1e-5).sqrt()
    dz = gout.double() * (xhat > 0)
    for name, ref_m in (("m1", dz.mean((2, 3, 4))), ("m2", (dz * xhat).mean((2, 3, 4)))):
        got_m = pool.flat(("t", name), n * c).cpu().double().view(n, c)
        err_m, scale_m = (got_m - ref_m).abs().max().item(), ref_m.abs().max().item()
        print(f"{name}: max|err| = {err_m:.3e}, max|ref| = {scale_m:.3e}")
        assert err_m <= 2e-4 * scale_m + 2e-6
    got = dy.float().permute(0, 4, 1, 2, 3).cpu().double()
    ref = y.grad.double()
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    bound = (2e-4 + 2.0 ** -8) * scale + 2e-6
    print(f"norm backward dx: max|err| = {err:.3e}, max|ref| = {scale:.3e}, bound {bound:.3e}")
    assert err <= bound
