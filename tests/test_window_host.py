"""Host half of sliding-window adaptation (``window_tta``, ``mmtta_window_views`` / ``mmtta_window_partials`` /
``mmtta_window_entropy_items`` / ``mmtta_window_blend``): the plugin's registration and config, every refusal that needs no
device, the window grid on hand-computed cases, the weight tables' properties (partition of unity, a = 1 where one window is
alone, a = 0 on pad) and the entry points' argument checks (none touches a device).  The GPU half is ``test_hip_window.py``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import window_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE, STEP = 0x7F0000000000, 1 << 32          # device-looking addresses that are never dereferenced
INVALID, UNSUPPORTED = -1, -2

# (extents, roi, overlap, windows, the most windows that meet at a voxel)
GRIDS = [((32, 32, 32), (32, 32, 32), 0.5, 1, 1),
         ((48, 40, 32), (32, 32, 32), 0.5, 4, 4),
         ((24, 40, 32), (32, 32, 32), 0.5, 2, 2),
         ((7, 9, 11), (8, 9, 12), 0.5, 1, 1),
         ((7, 9, 11), (12, 9, 16), 0.5, 1, 1),
         ((64, 32, 96), (32, 32, 32), 0.0, 6, 1),
         ((40, 40, 40), (32, 32, 32), 0.5, 8, 8),
         ((155, 48, 40), (128, 48, 32), 0.5, 4, 4)]


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from multimodal_tta_amd import _lib as _l
    return _l, _l.load()


def _cfg(**window):
    from multimodal_tta_amd.config import compose
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_window"])
    cfg["method"]["window"] = dict({"roi": [32, 32, 32]}, **window)
    return cfg


# ----------------------------------------------------------------------------- registration and config
def test_window_tta_is_registered_and_composes():
    import multimodal_tta_amd  # noqa: F401
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin, list_plugins
    from multimodal_tta_amd.tta import EntropyMinimizationTTA
    assert "window_tta" in list_plugins()
    cfg = compose(overrides=["method=tta_window"])
    assert cfg["method"]["name"] == "window_tta" and cfg["method"]["group"] == 1
    assert dict(cfg["method"]["window"]) == {"roi": [128, 128, 128], "overlap": 0.5, "mode": "gaussian", "sigma_scale": 0.125,
                                             "floor": 1e-3, "pad_value": 0.0}
    entmin = compose(overrides=["method=tta_entmin"])["method"]
    assert set(cfg["method"].keys()) - {"window"} == set(entmin.keys())          # every other key is tta_entmin.yaml's
    plug = get_plugin("window_tta")(cfg)
    assert isinstance(plug, EntropyMinimizationTTA) and plug.views == 1 and plug.fused_update
    assert plug.window.roi == (128, 128, 128) and plug.window.mode == "gaussian" and plug.window.floor == 1e-3
    plug = get_plugin("window_tta")(compose(overrides=["method=tta_window", "method.window.roi=[64,96,32]",
                                                       "method.window.mode=constant", "method.window.overlap=0.25"]))
    assert plug.window.roi == (64, 96, 32) and plug.window.mode == "constant" and plug.window.overlap == 0.25


@pytest.mark.parametrize("block,match", [
    (None, r"method\.window = None"),
    ({"overlap": 0.5}, r"method\.window\.roi = None"),
    ({"roi": [32, 32]}, r"method\.window\.roi = \[32, 32\]"),
    ({"roi": [32, 32, 0]}, r"method\.window\.roi"),
    ({"roi": [32, 32, 32.0]}, r"method\.window\.roi"),
    ({"roi": "32"}, r"method\.window\.roi"),
    ({"roi": [32, 32, 32], "overlap": 1.0}, r"method\.window\.overlap = 1\.0"),
    ({"roi": [32, 32, 32], "overlap": -0.1}, r"method\.window\.overlap"),
    ({"roi": [32, 32, 32], "overlap": "half"}, r"method\.window\.overlap"),
    ({"roi": [32, 32, 32], "mode": "cosine"}, r"method\.window\.mode = 'cosine'"),
    ({"roi": [32, 32, 32], "sigma_scale": 0.0}, r"method\.window\.sigma_scale"),
    ({"roi": [32, 32, 32], "floor": 0.0}, r"method\.window\.floor"),
    ({"roi": [32, 32, 32], "floor": 2.0}, r"method\.window\.floor"),
    ({"roi": [32, 32, 32], "pad_value": float("nan")}, r"method\.window\.pad_value"),
    ({"roi": [32, 32, 32], "padding": "reflect"}, r"method\.window\.padding: unknown key"),
])
def test_the_window_block_is_checked(block, match):
    from multimodal_tta_amd.registry import get_plugin
    cfg = _cfg()
    cfg["method"]["window"] = block
    with pytest.raises(ValueError, match=match):
        get_plugin("window_tta")(cfg)


def test_moddrop_is_refused_by_name():
    from multimodal_tta_amd.registry import get_plugin
    cfg = _cfg()
    cfg["method"]["moddrop"] = {"enabled": True, "p": 0.5, "seed": 0}
    with pytest.raises(NotImplementedError, match=r"method\.moddrop\.enabled.*window_tta"):
        get_plugin("window_tta")(cfg)


# ----------------------------------------------------------------------------- the grid
@pytest.mark.parametrize("n,r,overlap,want", [
    (32, 32, 0.5, [0]),                    # n = r: one window whatever the overlap
    (32, 32, 0.0, [0]),
    (24, 32, 0.5, [-4]),                   # n < r: pad 8 split 4 / 4
    (27, 32, 0.5, [-2]),                   # pad 5 split 2 / 3
    (40, 32, 0.5, [0, 8]),                 # interval 16, the second start clipped to n - r
    (155, 128, 0.5, [0, 27]),
    (64, 32, 0.0, [0, 32]),                # overlap 0: an exact tiling
    (70, 32, 0.0, [0, 32, 38]),
    (96, 32, 0.5, [0, 16, 32, 48, 64]),
    (160, 128, 0.5, [0, 32]),
    (33, 32, 0.99, [0, 1]),                # int(32 * 0.01) = 0: the interval is held at 1
])
def test_window_starts_on_hand_computed_cases(n, r, overlap, want):
    from multimodal_tta_amd.window import window_starts
    assert window_starts(n, r, overlap) == want
    assert wr.axis_starts(n, r, overlap) == want


def test_the_grid_is_the_product_of_the_start_lists_with_w_fastest():
    from multimodal_tta_amd.window import WindowSpec, window_grid
    g = window_grid((48, 40, 24), WindowSpec((32, 32, 32)))
    assert g.starts == ((0, 16), (0, 8), (-4,)) and g.windows == 4
    assert g.origins == ((0, 0, -4), (0, 8, -4), (16, 0, -4), (16, 8, -4))
    g = window_grid((160, 192, 160), WindowSpec((128, 128, 128)))          # the full BraTS volume: 8 windows
    assert g.windows == 8 and g.origins[1] == (0, 0, 32) and g.origins[2] == (0, 64, 0) and g.origins[4] == (32, 0, 0)
    assert [t.shape for t in g.tables] == [(2, 128)] * 3 and all(t.dtype == np.float32 for t in g.tables)


def test_more_than_32_windows_are_refused_with_the_keys_and_the_count():
    from multimodal_tta_amd.window import WindowSpec, window_grid
    assert window_grid((64, 64, 128), WindowSpec((32, 32, 32), overlap=0.0)).windows == 16
    assert window_grid((96, 64, 32), WindowSpec((32, 32, 32))).windows == 15
    with pytest.raises(ValueError, match=r"method\.window\.roi.*method\.window\.overlap.*45 windows \(5 x 3 x 3\)"):
        window_grid((96, 64, 64), WindowSpec((32, 32, 32)))
    with pytest.raises(ValueError, match=r"48 windows \(4 x 3 x 4\)"):
        window_grid((7, 9, 11), WindowSpec((4, 5, 6), overlap=0.6))          # intervals 1, 2, 2


def test_axis_weights_are_the_clamped_gaussian_or_one():
    from multimodal_tta_amd.window import axis_weights
    w = axis_weights(32, "gaussian", 0.125, 1e-3)
    assert w.dtype == np.float64 and w.shape == (32,)
    assert w[0] == pytest.approx(max(np.exp(-(15.5 ** 2) / (2 * 16.0)), 1e-3)) and w[0] == 1e-3          # exp(-7.5) < the floor
    assert w[15] == pytest.approx(np.exp(-0.25 / 32.0)) and np.array_equal(w, w[::-1]) and w.max() < 1.0
    assert np.array_equal(axis_weights(5, "constant"), np.ones(5))
    for r in (4, 5, 32, 128):
        assert np.allclose(axis_weights(r, "gaussian", 0.125, 1e-3), wr.axis_weight(r, "gaussian", 0.125, 1e-3).numpy(), rtol=1e-15)


# ----------------------------------------------------------------------------- the tables
def _package_grid(extents, roi, overlap, mode="gaussian"):
    from multimodal_tta_amd.window import WindowSpec, window_grid
    return window_grid(extents, WindowSpec(tuple(roi), overlap=overlap, mode=mode))


def _weights32(g):
    """a [W_n, rd, rh, rw] in fp32 the way the kernels form it: (A_d * A_h) * A_w, each product rounded."""
    return wr.window_weights([torch.from_numpy(t) for t in g.tables])


@pytest.mark.parametrize("mode", ["gaussian", "constant"])
@pytest.mark.parametrize("extents,roi,overlap,windows,meet", GRIDS)
def test_the_tables_are_a_partition_of_unity(extents, roi, overlap, windows, meet, mode):
    """sum_w a_w(v) = 1 within 8 * 2^-24 at every voxel of the volume (each a is a product of three fp32 roundings and at most
    8 windows meet at a voxel), a = 1 exactly where one window alone sees the voxel, a = 0 on every pad voxel, and the tables
    are the restatement's float64 ones rounded to fp32."""
    g = _package_grid(extents, roi, overlap, mode)
    ref = wr.grid(extents, roi, overlap=overlap, mode=mode)
    assert g.windows == windows == ref.windows and list(g.origins) == ref.origins
    cover = wr.covering(ref)
    assert cover.min().item() >= 1 and cover.max().item() == meet <= 8          # no voxel of the volume is left out
    for t, t64 in zip(g.tables, ref.tables):
        assert np.array_equal(t, t64.numpy().astype(np.float32))
    a = _weights32(g)
    assert a.dtype == torch.float32
    ins = wr.inside(ref)
    assert (a[~ins] == 0).all() and (a[ins] > 0).all()
    total = wr.blend(torch.ones((g.windows, 1, *roi), dtype=torch.float64), ref, a.double())[0, 0]
    print(f"{extents} roi {roi} {mode}: {windows} windows, {meet} meet, |sum a - 1| <= {(total - 1).abs().max().item():.2e}")
    assert (total - 1).abs().max().item() <= 8 * 2.0 ** -24
    alone = wr.blend(torch.ones((g.windows, 1, *roi), dtype=torch.float64), ref,
                     torch.where(a == 1.0, 1.0, 0.0).double())[0, 0]          # 1 where a window holds the voxel with a == 1
    assert torch.equal(alone[cover == 1], torch.ones_like(alone[cover == 1])), "a != 1 where one window covers the voxel"


@pytest.mark.parametrize("extents,roi,overlap,windows,meet", GRIDS)
def test_blending_the_crops_gives_the_volume_back(extents, roi, overlap, windows, meet):
    g = _package_grid(extents, roi, overlap)
    ref = wr.grid(extents, roi, overlap=overlap, pad_value=7.0)
    x = torch.randn((2, 3, *extents), generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 4.0
    xv = wr.crop(x, ref)
    assert xv.shape == (2 * windows, 3, *roi)
    ins = wr.inside(ref)
    assert (xv.reshape(2, windows, 3, *roi).permute(0, 2, 1, 3, 4, 5)[:, :, ~ins] == 7.0).all()          # the pad value, outside only
    back = wr.blend(xv, ref, _weights32(g).double())
    err = (back - x).abs().max().item()
    print(f"{extents} roi {roi}: blend(crop(x)) - x = {err:.2e} at max|x| = {x.abs().max().item():.2f}")
    assert err <= 8 * 2.0 ** -24 * x.abs().max().item()


def test_the_restated_loss_counts_every_voxel_of_the_volume_once():
    """With the same logit at every window voxel the loss is the entropy of that logit: the weights of a voxel sum to 1 and
    the pad voxels weigh 0."""
    ref = wr.grid((7, 9, 11), (4, 5, 6))
    z = torch.full((2 * ref.windows, 3, 4, 5, 6), 0.7, dtype=torch.float64)
    p = torch.sigmoid(torch.tensor(0.7, dtype=torch.float64))
    h = -(p * p.log() + (1 - p) * (1 - p).log())
    loss, grad = wr.loss_reference(z, ref.weights, 7 * 9 * 11, softmax=False)
    assert torch.allclose(loss, h.expand(2), rtol=1e-12)
    ref = wr.grid((7, 9, 11), (12, 9, 16))
    z = torch.full((ref.windows, 3, 12, 9, 16), 0.7, dtype=torch.float64)
    loss, grad = wr.loss_reference(z, ref.weights, 7 * 9 * 11, softmax=False)
    assert torch.allclose(loss, h.expand(1), rtol=1e-12) and (grad[0, :, ~wr.inside(ref)[0]] == 0).all()


# ----------------------------------------------------------------------------- the entry points
def _rows(_l, slot=0, n=4, c=3, d=4, h=6, w=10, ptr=True, dtype=None, ldc=4, flags=None):
    return _l.Tensor((FAKE + slot * STEP) if ptr is True else ptr, n, c, d, h, w, d * h * w * ldc, 1, h * w * ldc, w * ldc, ldc,
                     _l.F32 if dtype is None else dtype, _l.TENSOR_OWNS_PAD if flags is None else flags)


def _grid(_l, extent=(6, 6, 10), count=(2, 1, 1)):
    return _l.WindowGrid((ctypes.c_int32 * 3)(*extent), (ctypes.c_int32 * 3)(*count))


def test_the_window_symbols_are_declared_exported_and_typed():
    _l, lib = _lib()
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmtta.h")).read(), flags=re.S)
    for name in ("mmtta_window_views", "mmtta_window_entropy_items", "mmtta_window_blend"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    assert re.search(r"\bint64_t\s+mmtta_window_partials\s*\(", code) and "mmtta_window_grid" in code
    names = {"mmtta_window_views", "mmtta_window_partials", "mmtta_window_entropy_items", "mmtta_window_blend"}
    assert names <= set(_l.exported_names())
    for name in names:
        assert getattr(ctypes.CDLL(_l.LIB_PATH), name) is not None
    assert lib.mmtta_window_partials.restype is ctypes.c_int64 and ctypes.sizeof(_l.WindowGrid) == 24
    assert lib.mmtta_abi_version() == 2          # additive: the version stays
    from multimodal_tta_amd import ops
    assert all(callable(getattr(ops, n)) for n in ("window_views", "window_partials", "window_entropy_items", "window_blend"))
    from multimodal_tta_amd.build import SOURCES
    assert "window.hip" in SOURCES


def test_window_partials_answers_on_the_host():
    """The workgroups of ONE item (256 (voxel, region) pairs each, at most 2048) x items."""
    _l, lib = _lib()
    count = lambda **kw: lib.mmtta_window_partials(ctypes.byref(_rows(_l, **kw)))
    assert count(n=4, c=3, d=5, h=6, w=7) == 3 * 4
    assert count(n=8, c=3, d=128, h=128, w=128) == 2048 * 8
    assert lib.mmtta_window_partials(None) == -1 and count(d=0) == -1 and count(n=0) == -1


def test_the_window_entry_points_reject_bad_arguments_without_a_gpu():
    _l, lib = _lib()
    err = lambda: lib.mmtta_last_error()
    host = (ctypes.c_int32 * 6)(0, 0, 0, 2, 0, 0)
    x, y = _rows(_l, 0, n=2, d=6), _rows(_l, 1, n=4)
    views = lambda x=x, y=y, g=None, host=host, dev=FAKE + 9 * STEP: lib.mmtta_window_views(
        ctypes.byref(x), ctypes.byref(y), ctypes.byref(_grid(_l) if g is None else g), host, dev, 0.0, None)
    assert views(dev=None) == INVALID and b"null argument" in err()
    assert views(host=None) == INVALID and b"null argument" in err()
    assert views(g=_grid(_l, count=(33, 1, 1))) == INVALID and b"33 starts" in err()
    assert views(g=_grid(_l, count=(8, 8, 1))) == INVALID and b"64 windows" in err()
    assert views(g=_grid(_l, count=(3, 1, 1))) == INVALID and b"no multiple" in err()
    assert views(g=_grid(_l, extent=(7, 6, 10))) == INVALID and b"not those of `x`" in err()
    assert views(y=_rows(_l, 1, n=4, c=2)) == INVALID and b"shape mismatch" in err()
    assert views(y=_rows(_l, 1, n=4, dtype=_l.BF16)) == INVALID and b"shape mismatch" in err()
    for bad in ((0, 0, 0, 6, 0, 0), (0, 0, 0, -4, 0, 0), (0, 6, 0, 2, 0, 0), (0, 0, -10, 2, 0, 0)):
        assert views(host=(ctypes.c_int32 * 6)(*bad)) == INVALID and b"misses the volume" in err(), bad
    assert views(y=_rows(_l, 0, n=4)) == INVALID and b"overlaps" in err()

    z, g = _rows(_l, 0), _rows(_l, 1)
    loss = lambda z=z, g=g, grid=None, tables=FAKE + 4 * STEP, partial=FAKE + 5 * STEP, out=FAKE + 6 * STEP, softmax=0: \
        lib.mmtta_window_entropy_items(ctypes.byref(z), softmax, ctypes.byref(_grid(_l) if grid is None else grid), tables,
                                       ctypes.byref(g), partial, out, None)
    for kw in ({"tables": None}, {"partial": None}, {"out": None}, {"z": _rows(_l, 0, ptr=None)}):
        assert loss(**kw) == INVALID and b"null argument" in err(), kw
    assert loss(g=_rows(_l, 1, d=8)) == INVALID and b"shape mismatch" in err()
    assert loss(grid=_grid(_l, count=(3, 1, 1))) == INVALID and b"no multiple" in err()
    assert loss(z=_rows(_l, 0, dtype=_l.BF16)) == UNSUPPORTED and b"fp32-stored" in err()
    assert loss(g=_rows(_l, 1, dtype=_l.BF16, ldc=4, flags=0, c=3)) == UNSUPPORTED and b"bf16" in err()          # a pad it does not own
    assert loss(z=_rows(_l, 0, c=17, ldc=20), g=_rows(_l, 1, c=17, ldc=20), softmax=1) == UNSUPPORTED and b"classes" in err()
    assert loss(z=_rows(_l, 0, n=2, d=2, h=2, w=600), g=_rows(_l, 1, n=2, d=2, h=2, w=600),
                grid=_grid(_l, extent=(2, 2, 700))) == UNSUPPORTED and b"above 512" in err()

    zb, ob = _rows(_l, 0, n=4), _rows(_l, 1, n=2, d=6)
    blend = lambda z=zb, o=ob, grid=None, origins=FAKE + 4 * STEP, tables=FAKE + 5 * STEP: lib.mmtta_window_blend(
        ctypes.byref(z), ctypes.byref(o), ctypes.byref(_grid(_l) if grid is None else grid), origins, tables, None)
    assert blend(origins=None) == INVALID and blend(tables=None) == INVALID and b"null argument" in err()
    assert blend(o=_rows(_l, 1, n=1, d=6)) == INVALID and b"shape mismatch" in err()
    assert blend(o=_rows(_l, 1, n=2, d=7)) == INVALID and b"not those of `out`" in err()
    assert blend(o=_rows(_l, 1, n=2, d=6, dtype=_l.BF16)) == UNSUPPORTED and b"fp32-stored" in err()
    assert blend(o=_rows(_l, 0, n=2, d=6)) == INVALID and b"overlaps" in err()
