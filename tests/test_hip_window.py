"""Sliding-window adaptation (``window_tta``) on the GPU: the crop against torch's pad-and-slice bit for bit, the loss and its
gradient against float64 autograd of the restatement (``window_reference.py``), the blend against float64 and bit for bit where
one window covers a voxel, the plugin against the restatement on the oracle networks, and the bitwise properties (roi = the
volume is Tent, grouped = one volume at a time, graph replay = eager, ``steps: 0`` = the blend of plain eval forwards)."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import window_reference as wr
from test_hip_tta import SMALL, build_pair, root_cfg, volume

pytestmark = pytest.mark.gpu

VOLUME = (7, 9, 11)
# roi 4 x 5 x 6: 3 x 3 x 3 = 27 windows, up to 27 meet at a voxel (the clipped last start sits one voxel behind its
# neighbour); 8 x 9 x 12: one window that reaches one voxel past the volume along D and W (front pad (r - n) // 2 = 0: the
# origin stays 0); 12 x 9 x 16: one window with front pads of 2 - the origin is negative along D and W
ROIS = [(4, 5, 6), (8, 9, 12), (12, 9, 16)]


def package_grid(extents, roi, **spec):
    from multimodal_tta_amd.window import WindowSpec, window_grid
    return window_grid(extents, WindowSpec(tuple(roi), **spec))


def device_grid(grid):
    """The grid's origins (int32 [W_n * 3]) and tables (fp32, D | H | W) on the device, as Runtime.stage_windows uploads them."""
    origins = torch.tensor(grid.origins, dtype=torch.int32).reshape(-1).cuda()
    tables = torch.from_numpy(np.concatenate([t.reshape(-1) for t in grid.tables])).cuda()
    return origins, tables


def weights64(grid):
    """a [W_n, rd, rh, rw]: the fp32 tables the kernels read, multiplied in float64."""
    return wr.window_weights([torch.from_numpy(t).double() for t in grid.tables])


def weights32(grid):
    """... and multiplied in fp32, (d * h) * w, as the kernels do."""
    return wr.window_weights([torch.from_numpy(t) for t in grid.tables])


# ----------------------------------------------------------------------------- 1. the crop
def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def filled_rows(G, D, H, W, C, ldc, dtype, gen):
    """A staged input whose every lane (pad lanes too) carries a value, with NaN, -0 and both infinities in every channel."""
    from multimodal_tta_amd import ops
    x = ops.new_cl(G, D, H, W, C, "cuda", ldc=ldc, dtype=dtype)
    base = x if x._base is None else x._base
    host = torch.randn(base.shape, generator=gen)
    host[:, 0, 0, 0, :] = float("nan")
    host[:, 0, 0, 1, :] = -0.0
    host[:, 0, 0, 2, :] = float("-inf")
    host[:, D - 1, H - 1, W - 1, :] = float("inf")
    base.copy_(host.to(dtype))
    return x, base


def check_crop(G, C, ldc, dtype, roi, gen, pad_value=-2.5):
    from multimodal_tta_amd import ops
    D, H, W = VOLUME
    grid = package_grid(VOLUME, roi, pad_value=pad_value)
    ref = wr.grid(VOLUME, roi, pad_value=pad_value)
    assert list(grid.origins) == ref.origins
    x, base = filled_rows(G, D, H, W, C, ldc, dtype, gen)
    y = ops.new_cl(G * grid.windows, *roi, C, "cuda", ldc=ldc, dtype=dtype)
    ybase = y if y._base is None else y._base
    ybase.fill_(float("nan"))
    origins, _ = device_grid(grid)
    ops.window_views(x, y, grid, origins, pad_value)
    torch.cuda.synchronize()
    want = wr.crop(base.cpu()[..., :C].permute(0, 4, 1, 2, 3), ref).permute(0, 2, 3, 4, 1).contiguous()      # pad-and-slice
    got = ybase.cpu()
    assert torch.equal(bits(got[..., :C].contiguous()), bits(want)), (G, C, ldc, dtype, roi)
    assert (bits(got[..., C:].contiguous()) == 0).all(), "a pad lane is not +0"
    assert torch.isnan(want).any() and (roi == ROIS[0] or (want == pad_value).any())      # the cases are what they claim to be


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("G", [1, 3])
def test_window_views_are_bit_exact_against_pad_and_slice(dtype, C, G):
    """Dense rows of 4 lanes: kept values bit for bit (NaN, -0, both infinities), the pad value outside the volume, pad lanes
    +0 over an output that held NaN."""
    gen = torch.Generator().manual_seed(41 + C + G)
    for roi in ROIS:
        check_crop(G, C, 4, dtype, roi, gen)
    check_crop(G, C, 4, dtype, ROIS[2], gen, pad_value=0.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,ldc", [(3, 3), (5, 8), (6, 6)])
def test_window_views_on_the_generic_path(dtype, C, ldc):
    gen = torch.Generator().manual_seed(67 + C)
    for G in (1, 3):
        for roi in ROIS:
            check_crop(G, C, ldc, dtype, roi, gen)


# ----------------------------------------------------------------------------- 2. the loss against float64
def stage(z, generic):
    from multimodal_tta_amd import ops
    n, r, d, h, w = z.shape
    ldc = (r + 3) // 4 * 4 if not generic else (r if r % 4 else r + 1)
    return ops.to_cl(z.cuda(), ldc=ldc)


def grad_buffer(z_cl, dtype):
    from multimodal_tta_amd import ops
    n, d, h, w, r = z_cl.shape
    g = ops.new_cl(n, d, h, w, r, "cuda", ldc=z_cl.stride(3) if dtype == torch.float32 else 4, dtype=dtype)
    (g if g._base is None else g._base).fill_(float("nan"))
    return g


def run_loss(z_cl, grid, softmax, dtype=torch.float32):
    from multimodal_tta_amd import ops
    g = grad_buffer(z_cl, dtype)
    G = z_cl.shape[0] // grid.windows
    origins, tables = device_grid(grid)
    partial = torch.full((ops.window_partials(z_cl),), float("nan"), dtype=torch.float64, device="cuda")
    loss = torch.full((G,), 123.0, device="cuda")
    ops.window_entropy_items(z_cl, g, grid, origins, tables, partial, loss, softmax=softmax)
    torch.cuda.synchronize()
    return loss.cpu(), ops.from_cl(g.float()).cpu()


# (softmax, R, generic layout): sigmoid R in {1, 3, 4} and softmax R in {2, 5}, dense and odd rows
HEADS = [(False, 1, False), (False, 3, False), (False, 4, False), (False, 3, True), (False, 4, True), (False, 1, True),
         (True, 2, False), (True, 5, False), (True, 2, True), (True, 5, True)]
SATURATED = torch.tensor([0.0, 20.0, -20.0, 90.0, -90.0, 1e4, -1e4])


def check_values(loss, g, g32, l_ref, g_ref, dtype, what=""):
    """test_hip_memo.py's bounds: the loss 1e-5 relative, the fp32 gradient 2e-5 of its maximum, a bf16 gradient the fp32 one
    rounded (2^-7 relative)."""
    assert torch.isfinite(loss).all() and torch.isfinite(g).all()
    for a, b in zip(loss.tolist(), l_ref.tolist()):
        print(f"{what}{dtype}: loss {a} vs {b}")
        assert abs(a - b) <= 1e-5 * abs(b), (a, b)
    gmax = g_ref.abs().max().item()
    if dtype == torch.float32:
        err = (g.double() - g_ref).abs().max().item()
        print(f"{what}gradient error {err / gmax:.2e} of the maximum")
        assert err <= 2e-5 * gmax
    else:
        want = g32.to(torch.bfloat16).float()
        assert ((g - want).abs() <= want.abs() * 2.0 ** -7).all()


def check_loss(z, grid, softmax, generic):
    voxels = grid.extents[0] * grid.extents[1] * grid.extents[2]
    l_ref, g_ref = wr.loss_reference(z, weights64(grid), voxels, softmax)
    assert torch.isfinite(l_ref).all() and torch.isfinite(g_ref).all()
    outside = ~wr.inside(wr.grid(grid.extents, grid.roi))
    z_cl = stage(z, generic)
    g32 = None
    for dtype in ((torch.float32, torch.bfloat16) if (not softmax and not generic) else (torch.float32,)):
        loss, g = run_loss(z_cl, grid, softmax, dtype)
        check_values(loss, g, g32, l_ref, g_ref, dtype, f"{grid.roi} ")
        g32 = g
        gw = g.reshape(-1, grid.windows, *g.shape[1:])
        assert (gw[:, outside.unsqueeze(1).expand(-1, g.shape[1], -1, -1, -1)] == 0).all(), "a pad voxel has a gradient"


@pytest.mark.parametrize("softmax,R,generic", HEADS)
@pytest.mark.parametrize("roi", ROIS)
@pytest.mark.parametrize("G", [1, 2])
def test_window_loss_matches_float64(softmax, R, generic, roi, G):
    gen = torch.Generator().manual_seed(700 + 7 * R + G + roi[0])
    grid = package_grid(VOLUME, roi)
    z = torch.randn((G * grid.windows, R, *roi), generator=gen) * 3.0
    check_loss(z, grid, softmax, generic)
    check_loss(z, package_grid(VOLUME, roi, mode="constant"), softmax, generic)


@pytest.mark.parametrize("softmax,R,generic", HEADS)
def test_window_loss_is_finite_on_saturated_logits(softmax, R, generic):
    """Logits drawn from {0, +-20, +-90, +-1e4}: the loss and every gradient are finite, the loss within 1e-5 of float64, the pad
    voxels' gradient 0.  (The gradient's bound is not asked here: where every logit is saturated the largest float64 gradient
    is 20 sigma(-20) = 4e-8 before the scale, and the any-stride Bernoulli path forms sigma (1 - sigma) by subtraction, as the
    entropy objective does on that path - 0 from |z| = 17 on.)"""
    gen = torch.Generator().manual_seed(800 + R)
    for roi in ROIS[:2]:
        grid = package_grid(VOLUME, roi)
        z = SATURATED[torch.randint(0, len(SATURATED), (2 * grid.windows, R, *roi), generator=gen)]
        z[:, :, 0, 0, :] = 1e4 if not softmax else 0.0
        z[:, :, 0, 1, :] = -1e4 if not softmax else 0.0
        if softmax:
            z[:, 0, 0, 0, :] = 1e4
            z[:, 1, 0, 1, :] = -1e4
        l_ref, g_ref = wr.loss_reference(z, weights64(grid), VOLUME[0] * VOLUME[1] * VOLUME[2], softmax)
        outside = ~wr.inside(wr.grid(VOLUME, roi))
        z_cl = stage(z, generic)
        for dtype in ((torch.float32, torch.bfloat16) if (not softmax and not generic) else (torch.float32,)):
            loss, g = run_loss(z_cl, grid, softmax, dtype)
            assert torch.isfinite(loss).all() and torch.isfinite(g).all()
            for a, b in zip(loss.tolist(), l_ref.tolist()):
                print(f"{roi} {dtype}: loss {a} vs {b}; gradient {(g.double() - g_ref).abs().max().item():.2e} off at a maximum of "
                      f"{g_ref.abs().max().item():.2e}")
                assert abs(a - b) <= 1e-5 * abs(b), (a, b)
            gw = g.reshape(-1, grid.windows, *g.shape[1:])
            assert (gw[:, outside.unsqueeze(1).expand(-1, g.shape[1], -1, -1, -1)] == 0).all()


# The second trip of the voxel walk: at most 2048 workgroups of 256 threads per item, the rest in a grid-stride loop; 81^3 is
# the smallest cube with more voxels (531 441) than that (524 288).  The two items are the two windows of an 81 x 81 x 90 volume.
SECOND_TRIP_VOLUME, SECOND_TRIP_ROI = (81, 81, 90), (81, 81, 81)
SECOND_TRIP = [pytest.param(False, False, torch.float32, id="bernoulli-fast-fp32"),
               pytest.param(False, False, torch.bfloat16, id="bernoulli-fast-bf16"),
               pytest.param(False, True, torch.float32, id="bernoulli-generic"),
               pytest.param(True, False, torch.float32, id="categorical")]


@functools.lru_cache(maxsize=None)
def second_trip_logits():
    return torch.randn((2, 3, *SECOND_TRIP_ROI), generator=torch.Generator().manual_seed(81)) * 3.0


@functools.lru_cache(maxsize=None)
def second_trip_reference(softmax):
    grid = package_grid(SECOND_TRIP_VOLUME, SECOND_TRIP_ROI)
    return wr.loss_reference(second_trip_logits(), weights64(grid), 81 * 81 * 90, softmax)


@pytest.mark.parametrize("softmax,generic,dtype", SECOND_TRIP)
def test_window_loss_on_the_second_trip_of_the_walk(softmax, generic, dtype):
    grid = package_grid(SECOND_TRIP_VOLUME, SECOND_TRIP_ROI)
    assert grid.windows == 2 and grid.origins == ((0, 0, 0), (0, 0, 9))
    l_ref, g_ref = second_trip_reference(softmax)
    z_cl = stage(second_trip_logits(), generic)
    loss, g = run_loss(z_cl, grid, softmax, dtype)
    g32 = run_loss(z_cl, grid, softmax, torch.float32)[1] if dtype != torch.float32 else None
    check_values(loss, g, g32, l_ref, g_ref, dtype)


@pytest.mark.parametrize("softmax,R,generic,dtype", [(False, 3, False, torch.float32), (False, 3, False, torch.bfloat16),
                                                     (False, 3, True, torch.float32), (True, 5, False, torch.float32)])
def test_g_volumes_equal_g_single_volume_calls(softmax, R, generic, dtype):
    gen = torch.Generator().manual_seed(5)
    G, roi = 3, ROIS[0]
    grid = package_grid(VOLUME, roi)
    V = grid.windows
    z = torch.randn((G * V, R, *roi), generator=gen) * 3.0
    loss, g = run_loss(stage(z, generic), grid, softmax, dtype)
    for k in range(G):
        loss1, g1 = run_loss(stage(z[k * V:(k + 1) * V], generic), grid, softmax, dtype)
        assert torch.equal(loss1, loss[k:k + 1]) and torch.equal(g1, g[k * V:(k + 1) * V])


@pytest.mark.parametrize("softmax,R,generic", HEADS)
def test_one_window_is_the_entropy_objective(softmax, R, generic):
    """roi = the volume: one window with a = 1 everywhere, against mmtta_entropy_loss_items on the same logits - the loss within
    1e-6 relative, the gradient within 2e-6 of its maximum (test_one_view_is_the_entropy_objective's bounds).  (As with one
    view there, the entry point hands this grid to the entropy objective's own kernels.)"""
    from multimodal_tta_amd import ops
    gen = torch.Generator().manual_seed(11 + R)
    N, shape = 3, (5, 6, 7)
    grid = package_grid(shape, shape)
    assert grid.windows == 1 and all((t == 1).all() for t in grid.tables)
    z = torch.randn((N, R, *shape), generator=gen) * 3.0
    z_cl = stage(z, generic)
    loss, g = run_loss(z_cl, grid, softmax)
    g0 = grad_buffer(z_cl, torch.float32)
    partial = torch.empty(ops.entropy_partials_items(z_cl), dtype=torch.float64, device="cuda")
    loss0 = torch.empty(N, device="cuda")
    ops.entropy_loss_items(z_cl, g0, partial, loss0, softmax=softmax)
    torch.cuda.synchronize()
    g0, loss0 = ops.from_cl(g0).cpu(), loss0.cpu()
    gmax = g0.abs().max().item()
    print(f"one window vs entropy_loss_items: loss {((loss - loss0).abs() / loss0.abs()).max().item():.2e}, "
          f"gradient {(g - g0).abs().max().item() / gmax:.2e} of its maximum")
    assert ((loss - loss0).abs() <= 1e-6 * loss0.abs()).all(), (loss, loss0)
    assert (g - g0).abs().max().item() <= 2e-6 * gmax


# ----------------------------------------------------------------------------- 3. the blend
def run_blend(z, grid, generic=False):
    from multimodal_tta_amd import ops
    z_cl = stage(z, generic)
    G, R = z.shape[0] // grid.windows, z.shape[1]
    out = ops.new_cl(G, *grid.extents, R, "cuda", ldc=z_cl.stride(3))
    base = out if out._base is None else out._base
    base.fill_(float("nan"))
    origins, tables = device_grid(grid)
    ops.window_blend(z_cl, out, grid, origins, tables)
    torch.cuda.synchronize()
    if R <= 4 and not generic:          # dense 16-byte rows: the row's pad lanes are the output's to write
        assert (base[..., R:] == 0).all(), "a pad lane of the blend is not 0"
    return ops.from_cl(out).cpu()


@pytest.mark.parametrize("R,generic", [(1, False), (3, False), (4, False), (3, True), (5, False), (1, True)])
@pytest.mark.parametrize("roi", ROIS)
@pytest.mark.parametrize("G", [1, 2])
def test_window_blend_matches_float64(R, generic, roi, G):
    """Within (K + 4) * 2^-23 * max|z| of float64, K = the most windows that meet at a voxel (the fma chain's bound with a factor
    2); bit-equal to the window's own logit wherever one window covers the voxel."""
    gen = torch.Generator().manual_seed(900 + R + G + roi[0])
    for mode in ("gaussian", "constant"):
        grid = package_grid(VOLUME, roi, mode=mode)
        ref = wr.grid(VOLUME, roi, mode=mode)
        z = torch.randn((G * grid.windows, R, *roi), generator=gen) * 3.0
        got = run_blend(z, grid, generic)
        want = wr.blend(z.double(), ref, weights64(grid))
        cover = wr.covering(ref)
        K = int(cover.max())
        err = (got.double() - want).abs().max().item()
        print(f"roi {roi} {mode}: K = {K}, blend error {err:.2e} against the bound {(K + 4) * 2.0 ** -23 * z.abs().max().item():.2e}")
        assert got.shape == (G, R, *VOLUME) and err <= (K + 4) * 2.0 ** -23 * z.abs().max().item()
        alone = (cover == 1).expand(G, R, -1, -1, -1)
        assert torch.equal(got[alone], wr.blend(z, ref, weights32(grid))[alone])


def test_an_exact_tiling_returns_every_window_bit_for_bit():
    """Overlap 0 and extents that are multiples of the roi: every voxel has one window, a = 1, the blend is a copy."""
    extents, roi = (8, 10, 12), (4, 5, 6)
    grid = package_grid(extents, roi, overlap=0.0)
    ref = wr.grid(extents, roi, overlap=0.0)
    assert grid.windows == 8 and int(wr.covering(ref).max()) == 1 and all((t == 1).all() for t in grid.tables)
    z = torch.randn((2 * 8, 3, *roi), generator=torch.Generator().manual_seed(12)) * 3.0
    z[0, :, 0, 0, 0] = torch.tensor([float("inf"), float("-inf"), 3e38])
    got = run_blend(z, grid)
    want = torch.zeros((2, 3, *extents))
    for g in range(2):
        for w, o in enumerate(grid.origins):
            want[g, :, o[0]:o[0] + 4, o[1]:o[1] + 5, o[2]:o[2] + 6] = z[g * 8 + w]
    assert torch.equal(bits(got), bits(want))


# ----------------------------------------------------------------------------- 4. the plugin against the restatement
ROI = [32, 32, 32]
TWO_AXES = (48, 40, 32)          # D [0, 16], H [0, 8] (the second start clipped): 4 windows
PADDED = (24, 40, 32)            # D padded 4 / 4, H [0, 8]: 2 windows


def window_cfg(model_cfg, steps=3, lr=None, block=None, **method):
    """``lr=None``: the configured learning rate (the reference's)."""
    from multimodal_tta_amd.config import compose
    cfg = root_cfg(model_cfg, steps=steps, lr=1e-3 if lr is None else lr, **method)
    if lr is None:
        cfg["training"]["optimizers"]["adam"]["lr"] = compose(overrides=["task=brats", "model=unet"])["training"]["optimizers"]["adam"]["lr"]
    cfg["method"]["name"] = "window_tta"
    cfg["method"]["window"] = dict({"roi": list(ROI)}, **(block or {}))
    return cfg


def check_against_reference(z_hip, losses, out_ref, ref0, x, y, cfg, softmax=False, bf16=False, roi=ROI, **kw):
    """fp32, against a float64 run of the restatement: per-step loss 1e-4 relative + 1e-6, final logits within max(2e-3 of
    max|logits|, 3x the fp32 restatement's own distance from that run) (test_hip_tta.logits_close's rule), thresholded masks
    differing on a share <= 1e-4.  bf16, against the fp32 restatement: test_memo_bf16_tracks_the_restatement's bounds - loss
    1e-2, logits 3e-2 of max|logits|, masks 1e-2, Dice 2e-2, and the bf16 path must have been taken."""
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
    assert z_hip.shape == z_ref.shape == (1, z_ref.shape[1], *x.shape[2:])
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
    o64 = wr.window_reference(copy.deepcopy(ref0).double(), x.double(), cfg["training"], steps, roi, softmax=softmax, **kw)
    for t in range(steps):
        a, b, c = losses[t], out_ref["losses"][t], o64["losses"][t]
        print(f"step {t}: loss {a}, fp32 restatement {b}, float64 {c}")
        assert abs(a - c) <= 1e-4 * abs(c) + 1e-6, f"step {t}: loss {a}, fp32 {b}, fp64 {c}"
    z64 = o64["logits"]
    scale = z64.abs().max().item()
    e_ref = (z_ref.double() - z64).abs().max().item() / scale
    e_hip = (z_hip.double() - z64).abs().max().item() / scale
    print(f"losses {losses}; logits {e_hip:.2e} (fp32 restatement {e_ref:.2e})")
    assert e_hip <= max(2e-3, 3.0 * e_ref), f"HIP vs fp64 restatement {e_hip:.3e}; fp32 restatement vs fp64 {e_ref:.3e}"
    m_hip, m_ref, m64 = masks_of(z_hip), masks_of(z_ref), masks_of(z64)
    share, share_ref = (m_hip != m64).float().mean().item(), (m_ref != m64).float().mean().item()
    print(f"mask voxels differing from float64: {share:.2e} (fp32 restatement {share_ref:.2e})")
    assert share <= 1e-4, (share, share_ref)


@pytest.mark.parametrize("shape,windows,index", [(TWO_AXES, 4, 0), (PADDED, 2, 1)], ids=["48x40x32", "24x40x32"])
def test_window_tta_matches_the_restatement(shape, windows, index):
    from multimodal_tta_amd.registry import get_plugin
    cfg = window_cfg(SMALL, steps=3, group=1)
    ref, hip = build_pair(SMALL)
    ref0 = copy.deepcopy(ref)
    x, y = volume(index, shape=shape)
    plug = get_plugin("window_tta")(cfg).setup(hip, "cuda")
    out_ref = wr.window_reference(ref, x, cfg["training"], 3, ROI)
    res = plug.adapt_volume(x.cuda())
    assert res["windows"] == windows == out_ref["windows"] and res["losses"].shape == (3,)
    assert tuple(res["logits_cl"].shape) == (1, *shape, 3)
    assert plug.rt.views == 1 and not plug.rt.use_sets
    check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref, ref0, x, y, cfg)


def test_window_tta_softmax_head_matches_the_restatement():
    from multimodal_tta_amd.registry import get_plugin
    mcfg = dict(SMALL, num_classes=4)
    cfg = window_cfg(mcfg, steps=3, group=1)
    cfg["training"]["criterion"]["softmax"] = True
    cfg["training"]["criterion"]["sigmoid"] = False
    ref, hip = build_pair(mcfg)
    ref0 = copy.deepcopy(ref)
    x, y = volume(1, shape=TWO_AXES, R=4)
    plug = get_plugin("window_tta")(cfg).setup(hip, "cuda")
    assert plug.softmax
    out_ref = wr.window_reference(ref, x, cfg["training"], 3, ROI, softmax=True)
    res = plug.adapt_volume(x.cuda())
    check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref, ref0, x, y, cfg, softmax=True)


def test_window_tta_with_a_missing_modality():
    from multimodal_tta_amd.registry import get_plugin
    cfg = window_cfg(SMALL, steps=3, group=1, missing_modalities=[1])
    ref, hip = build_pair(SMALL)
    ref0 = copy.deepcopy(ref)
    x, y = volume(3, shape=PADDED)
    plug = get_plugin("window_tta")(cfg).setup(hip, "cuda")
    out_ref = wr.window_reference(ref, x, cfg["training"], 3, ROI, missing=(1,))
    res = plug.adapt_volume(x.cuda())
    check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref, ref0, x, y, cfg, missing=(1,))


DEEP = dict(name="unet_multimodal_deepfusion", num_modalities=4, num_classes=3, spatial_dims=3,
            channels=[4, 8, 16, 32, 64], strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)
# the network's factor is 16, but torch's InstanceNorm refuses the single bottleneck voxel of a 16^3 input in train mode: 32^3
# is the smallest roi the restatement can run
DEEP_ROI, DEEP_VOLUME = [32, 32, 32], (40, 32, 32)


def test_window_tta_deepfusion_matches_the_restatement():
    import oracle
    from multimodal_tta_amd.models import MultimodalUNetDeepFusion
    from multimodal_tta_amd.registry import get_plugin
    cfg = window_cfg(DEEP, steps=3, group=1, block={"roi": DEEP_ROI})
    torch.manual_seed(42)
    ref = oracle.MultimodalUNetDeepFusion(DEEP)
    hip = MultimodalUNetDeepFusion(DEEP)
    hip.load_state_dict(ref.state_dict())
    ref0 = copy.deepcopy(ref)
    # (volume 0: on the CPU the fp32 restatement's thresholded masks equal the float64 ones there, as on the U-Net's two
    # volumes above; this untrained network's logits sit close to 0, and on volume 2 fp32 alone already differs on 3e-5)
    x, y = volume(0, shape=DEEP_VOLUME)
    out_ref = wr.window_reference(ref, x, cfg["training"], 3, DEEP_ROI)
    plug = get_plugin("window_tta")(cfg).setup(hip, "cuda")
    res = plug.adapt_volume(x.cuda())
    assert res["windows"] == 2
    check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref, ref0, x, y, cfg, roi=DEEP_ROI)
    with pytest.raises(NotImplementedError, match="group 1 only"):
        get_plugin("window_tta")(window_cfg(DEEP, steps=1, group=2, block={"roi": DEEP_ROI})).setup(hip, "cuda")


def test_window_tta_bf16_tracks_the_restatement():
    from multimodal_tta_amd.registry import get_plugin
    cfg = window_cfg(SMALL, steps=3, group=1, precision="bf16")
    ref, hip = build_pair(SMALL)
    x, y = volume(5, shape=TWO_AXES)
    out_ref = wr.window_reference(ref, x, cfg["training"], 3, ROI)
    plug = get_plugin("window_tta")(cfg).setup(hip, "cuda")
    res = plug.adapt_volume(x.cuda())
    check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref, None, x, y, cfg, bf16=True)


# ----------------------------------------------------------------------------- 5. bit for bit
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_roi_equal_to_the_volume_is_bitwise_entmin(precision):
    """One window, a = 1: the plugin runs entmin_tta's own staging, step and final forward - its loss kernel, its fused update."""
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_groups import WIDE
    model_cfg = SMALL if precision == "fp32" else WIDE          # (wide enough for the fused weight update)
    for G in (1, 3):
        xs = torch.cat([volume(i)[0] for i in range(G)]).cuda()
        out = {}
        for name in ("entmin_tta", "window_tta"):
            cfg = window_cfg(model_cfg, steps=3, lr=1e-3, group=G, tune_volumes=4, precision=precision)
            cfg["method"]["name"] = name
            _, hip = build_pair(model_cfg)
            plug = get_plugin(name)(cfg).setup(hip, "cuda")
            assert plug.views == 1 and hip.views == 1
            res = plug.adapt_volume(xs)
            out[name] = (plug.logits(res).cpu(), res["losses"].cpu(), len(plug.rt.fused_layers))
            if name == "window_tta":
                assert res["windows"] == 1
        assert out["entmin_tta"][2] == out["window_tta"][2], "the fused update was not kept"
        if precision == "bf16":
            assert out["window_tta"][2] > 0
        for a, b in zip(out["entmin_tta"][:2], out["window_tta"][:2]):
            assert torch.equal(a, b)


def test_window_group_equals_one_volume_at_a_time_and_graph_equals_eager():
    from multimodal_tta_amd.registry import get_plugin
    G = 2
    vols = [volume(i, shape=TWO_AXES)[0] for i in range(G)]
    runs = {}
    for group, use_graph in ((G, True), (1, True), (G, False)):
        cfg = window_cfg(SMALL, steps=3, lr=1e-3, group=group, tune_volumes=8, use_graph=use_graph)
        _, hip = build_pair(SMALL)
        plug = get_plugin("window_tta")(cfg).setup(hip, "cuda")
        assert plug.group == group
        if group == G:
            r = plug.adapt_volume(torch.cat(vols).cuda())
            assert r["losses"].shape == (3, G) and r["windows"] == 4 and tuple(r["logits_cl"].shape) == (G, *TWO_AXES, 3)
            runs[(group, use_graph)] = [plug.logits(r).cpu(), r["losses"].cpu()]
        else:
            zs, ls = [], []
            for v in vols:
                r = plug.adapt_volume(v.cuda())
                zs.append(plug.logits(r).cpu())          # (the logits live in a pool buffer the next call writes again)
                ls.append(r["losses"].cpu().clone())
            runs[(group, use_graph)] = [torch.cat(zs), torch.stack(ls, 1)]
    for a, b in zip(runs[(G, True)], runs[(1, True)]):
        assert torch.equal(a, b), "grouped run differs from one volume at a time"
    for a, b in zip(runs[(G, True)], runs[(G, False)]):
        assert torch.equal(a, b), "graph replay differs from eager launches"


def test_volumes_of_different_shapes_keep_their_own_graphs():
    """A captured step carries its grid (extents, counts): a second shape captures its own, and the first shape's replay
    afterwards still gives what a fresh plugin gives."""
    from multimodal_tta_amd.registry import get_plugin
    cfg = window_cfg(SMALL, steps=2, lr=1e-3, group=1, tune_volumes=4)
    xa, xb = volume(0, shape=TWO_AXES)[0].cuda(), volume(1, shape=(40, 48, 32))[0].cuda()          # 4 windows each
    _, hip = build_pair(SMALL)
    plug = get_plugin("window_tta")(cfg).setup(hip, "cuda")
    first = plug.logits(plug.adapt_volume(xa)).cpu()
    other = plug.logits(plug.adapt_volume(xb)).cpu()
    again = plug.logits(plug.adapt_volume(xa)).cpu()
    assert torch.equal(first, again) and len(plug._graph_sets) == 2
    _, hip = build_pair(SMALL)
    fresh = get_plugin("window_tta")(cfg).setup(hip, "cuda")
    assert torch.equal(other, fresh.logits(fresh.adapt_volume(xb)).cpu())


def blend_fma(z, grid):
    """The kernel's order on the host, one volume: z fp32 [W_n, R, rd, rh, rw] -> [R, D, H, W], out = fma(a_w, z_w, out) from 0 in
    ascending window order, a = (A_d * A_h) * A_w in fp32.  The fma is the float64 sum of the exact product (48 bits) rounded
    to fp32."""
    a = weights32(grid)
    out = torch.zeros((z.shape[1], *grid.extents), dtype=torch.float32)
    for w, o in enumerate(grid.origins):
        lo = [max(o[k], 0) for k in range(3)]
        hi = [min(o[k] + grid.roi[k], grid.extents[k]) for k in range(3)]
        src = tuple(slice(lo[k] - o[k], hi[k] - o[k]) for k in range(3))
        dst = (slice(None),) + tuple(slice(lo[k], hi[k]) for k in range(3))
        out[dst] = (out[dst].double() + a[w][src].double() * z[(w, slice(None)) + src].double()).float()
    return out


@pytest.mark.parametrize("mode", ["gaussian", "constant"])
@pytest.mark.parametrize("shape", [TWO_AXES, PADDED], ids=["48x40x32", "24x40x32"])
def test_zero_steps_is_the_blend_of_plain_eval_forwards(mode, shape):
    """``steps: 0`` is sliding-window inference of the source model: bit for bit the model's own eval forward of the
    torch-cropped windows, blended on the host with the plugin's tables in the kernel's order."""
    from multimodal_tta_amd.registry import get_plugin
    cfg = window_cfg(SMALL, steps=0, lr=1e-3, group=1, block={"mode": mode, "pad_value": 0.25})
    _, hip = build_pair(SMALL)
    plug = get_plugin("window_tta")(cfg).setup(hip, "cuda")
    x, _ = volume(4, shape=shape)
    res = plug.adapt_volume(x.cuda())
    got = plug.logits(res).cpu()
    assert res["losses"].numel() == 0 and plug.rt.views == 1
    grid = plug.rt.window_grid
    hip.eval()
    with torch.no_grad():
        z = hip(wr.crop(x, wr.grid(shape, ROI, mode=mode, pad_value=0.25)).cuda()).cpu()
    assert torch.equal(got[0], blend_fma(z, grid))


def test_windows_do_not_stick_to_the_runtime_or_the_model():
    """After a windowed volume the runtime carries one item per volume again, and the model adapts under entmin_tta as before."""
    from multimodal_tta_amd.registry import get_plugin
    _, hip = build_pair(SMALL)
    plug = get_plugin("window_tta")(window_cfg(SMALL, steps=1, lr=1e-3, group=2)).setup(hip, "cuda")
    xs = torch.cat([volume(i, shape=PADDED)[0] for i in range(2)]).cuda()
    assert plug.adapt_volume(xs)["windows"] == 2
    assert plug.rt.views == 1 and not plug.rt.use_sets and hip.views == 1
    cfg = window_cfg(SMALL, steps=1, lr=1e-3, group=2)
    cfg["method"]["name"] = "entmin_tta"
    plug = get_plugin("entmin_tta")(cfg).setup(hip, "cuda")
    assert hip.views == 1 and plug.rt.views == 1
    assert plug.adapt_volume(torch.cat([volume(i)[0] for i in range(2)]).cuda())["losses"].shape == (1, 2)


# ----------------------------------------------------------------------------- 6. end to end
def test_seg_tta_eval_with_tta_window(monkeypatch):
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy
    from multimodal_tta_amd.window import SlidingWindowTTA
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_window", "method.steps=2", "method.window.roi=[32,32,32]"])
    cfg["model"] = dict(SMALL)
    cfg["dataset"]["synthetic"]["num_volumes"] = 2
    cfg["dataset"]["synthetic"]["shape"] = list(TWO_AXES)
    seen = []
    adapt = SlidingWindowTTA.adapt_volume

    def spy(self, x, steps=None):
        res = adapt(self, x, steps)
        seen.append((tuple(x.shape), tuple(res["logits_cl"].shape), res["windows"]))
        return res

    monkeypatch.setattr(SlidingWindowTTA, "adapt_volume", spy)
    _, hip = build_pair(SMALL)
    loader = get_dataset_builder("brats")(cfg).get_loader("test")
    strat = get_evaluation_strategy("seg_tta_eval")(cfg)
    m = strat.evaluate_epoch(hip, loader, torch.device("cuda"))
    assert type(strat.plugin).__name__ == "SlidingWindowTTA"
    assert seen == [((1, 4, *TWO_AXES), (1, *TWO_AXES, 3), 4)] * 2
    assert {"et_dc", "tc_dc", "wt_dc", "avg_dc", "loss"} <= set(m)
    assert all(0.0 <= m[k] <= 1.0 for k in ("et_dc", "tc_dc", "wt_dc", "avg_dc"))


# ----------------------------------------------------------------------------- 7. refusals
def test_window_tta_refuses_by_name_before_any_launch():
    from multimodal_tta_amd.registry import get_plugin
    cfg = window_cfg(SMALL, steps=1, group=1)
    cfg["method"]["moddrop"] = {"enabled": True, "p": 0.5, "seed": 0}
    with pytest.raises(NotImplementedError, match=r"method\.moddrop\.enabled"):
        get_plugin("window_tta")(cfg)
    batch = dict(SMALL, norm="BATCH")
    _, hip = build_pair(batch)
    with pytest.raises(NotImplementedError, match="running"):
        get_plugin("window_tta")(window_cfg(batch, steps=1, group=1)).setup(hip, "cuda")
    _, hip = build_pair(SMALL)
    with pytest.raises(ValueError, match=r"\(32, 24, 32\) is not divisible by 16"):
        get_plugin("window_tta")(window_cfg(SMALL, steps=1, group=1, block={"roi": [32, 24, 32]})).setup(hip, "cuda")
    plug = get_plugin("window_tta")(window_cfg(SMALL, steps=1, group=1)).setup(hip, "cuda")
    with pytest.raises(ValueError, match="method.group = 1"):
        plug.adapt_volume(torch.cat([volume(0, shape=PADDED)[0], volume(1, shape=PADDED)[0]]).cuda())
    with pytest.raises(ValueError, match=r"method\.window\.roi.*45 windows"):
        plug.adapt_volume(torch.zeros((1, 4, 96, 64, 64), device="cuda"))
