"""MEMO adaptation (``memo_tta``, ``method=tta_memo``): the host-side half, no GPU needed.

The config composes and the plugin reads its keys; the views are enumerated as documented; the new entry points (mirrored
views, marginal-entropy loss, ensemble) refuse every bad argument with the documented code and a message before anything
reaches the device."""
import ctypes

import pytest

INVALID, UNSUPPORTED = -1, -2
FAKE = 4096          # a 16-byte aligned address that is never dereferenced: the checks fail first


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from multimodal_tta_amd import _lib
    return _lib, _lib.load()


def test_tta_memo_config_composes_and_the_plugin_reads_it():
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin

    cfg = compose(overrides=["task=brats", "dataset=brats", "model=unet", "method=tta_memo"])
    assert cfg["method"]["name"] == "memo_tta" and cfg["method"]["kind"] == "tta"
    assert list(cfg["method"]["memo"]["mirror_axes"]) == ["h", "w"] and cfg["method"]["memo"]["ensemble"] is False
    plug = get_plugin("memo_tta")(cfg)
    assert plug.mirror_axes == ["h", "w"] and plug.views == 4 and plug.ensemble is False
    assert plug.view_axes == [0, 2, 1, 3]                 # bit 0 = W, bit 1 = H; view 1 mirrors mirror_axes[0] = h
    assert plug.fused_update is False
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_memo", "method.memo.mirror_axes=[d]",
                             "method.memo.ensemble=true"])
    plug = get_plugin("memo_tta")(cfg)
    assert plug.views == 2 and plug.view_axes == [0, 4] and plug.ensemble is True


def test_tta_memo_carries_every_key_of_tta_entmin():
    from multimodal_tta_amd.config import compose
    ent = compose(overrides=["task=brats", "model=unet", "method=tta_entmin"])["method"]
    memo = compose(overrides=["task=brats", "model=unet", "method=tta_memo"])["method"]
    assert set(memo) == set(ent) | {"memo"}
    for k in ent:
        if k not in ("name", "group"):          # `group` ships smaller: every volume brings V views
            assert memo[k] == ent[k], k
    assert 1 <= memo["group"] <= ent["group"]


@pytest.mark.parametrize("axes,masks", [([], [0]), (["w"], [0, 1]), (["h"], [0, 2]), (["d"], [0, 4]),
                                        (["h", "w"], [0, 2, 1, 3]), (["w", "h"], [0, 1, 2, 3]),
                                        (["d", "h", "w"], [0, 4, 2, 6, 1, 5, 3, 7]), (["D", "W"], [0, 4, 1, 5])])
def test_view_enumeration(axes, masks):
    from multimodal_tta_amd.memo import parse_mirror_axes, view_masks
    got = view_masks(parse_mirror_axes(axes))
    assert got == masks and got[0] == 0 and len(got) == 2 ** len(axes) and len(set(got)) == len(got)
    for v, m in enumerate(got):          # view v mirrors axes[i] iff bit i of v is set; mask bit 0 = W, 1 = H, 2 = D
        want = sum({"d": 4, "h": 2, "w": 1}[a.lower()] for i, a in enumerate(axes) if (v >> i) & 1)
        assert m == want


@pytest.mark.parametrize("bad", [["x"], ["h", "h"], "hw", 3, ["d", "h", "w", "d"], [1], None])
def test_memo_plugin_rejects_bad_mirror_axes(bad):
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_memo"])
    cfg["method"]["memo"] = {"mirror_axes": bad, "ensemble": False}
    if bad is None:
        cfg["method"]["memo"] = {"mirror_axes": 0.5}
    with pytest.raises(ValueError, match="method.memo.mirror_axes"):
        get_plugin("memo_tta")(cfg)


def test_memo_plugin_rejects_a_bad_ensemble_flag_and_moddrop():
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_memo"])
    cfg["method"]["memo"]["ensemble"] = "maybe"
    with pytest.raises(ValueError, match="method.memo.ensemble"):
        get_plugin("memo_tta")(cfg)
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_memo"])
    cfg["method"]["moddrop"] = {"enabled": True, "p": 0.5, "seed": 0}
    with pytest.raises(NotImplementedError, match="method.moddrop.enabled"):
        get_plugin("memo_tta")(cfg)


def test_memo_is_a_registered_plugin():
    import multimodal_tta_amd  # noqa: F401
    from multimodal_tta_amd.registry import list_plugins
    assert {"memo_tta", "sar_tta", "entmin_tta"} <= set(list_plugins())


def test_the_library_exports_the_memo_entry_points():
    _l, lib = _lib()
    for name in ("mmtta_mirror_views", "mmtta_memo_partials", "mmtta_memo_loss_items", "mmtta_memo_ensemble"):
        assert hasattr(ctypes.CDLL(_l.LIB_PATH), name) and name in _l.exported_names()
    assert lib.mmtta_abi_version() == 2


def _tensor(_l, n=4, c=3, d=4, h=4, w=4, ptr=FAKE, dtype=None, ldc=4, flags=None):
    return _l.Tensor(ptr, n, c, d, h, w, d * h * w * ldc, 1, h * w * ldc, w * ldc, ldc, _l.F32 if dtype is None else dtype,
                     _l.TENSOR_OWNS_PAD if flags is None else flags)


def _axes(*masks):
    return (ctypes.c_int32 * len(masks))(*masks)


def _loss(lib, _l, z=None, g=None, softmax=0, views=2, axes=None, partial=FAKE, loss=FAKE):
    z = _tensor(_l) if z is None else z
    g = _tensor(_l) if g is None else g
    axes = _axes(0, 1, 2, 3, 4, 5, 6, 7) if axes is None else axes
    return lib.mmtta_memo_loss_items(ctypes.byref(z) if z != "null" else None, softmax, views, axes,
                                     ctypes.byref(g) if g != "null" else None, partial, loss, None)


def test_memo_loss_rejects_bad_arguments_without_a_gpu():
    _l, lib = _lib()
    for kw in ({"z": "null"}, {"g": "null"}, {"partial": None}, {"loss": None}, {"z": _tensor(_l, ptr=None)}):
        assert _loss(lib, _l, **kw) == INVALID
        assert b"null argument" in lib.mmtta_last_error()
    for v in (0, 3, 5, 16, -2):
        assert _loss(lib, _l, views=v) == INVALID
        assert b"views" in lib.mmtta_last_error()
    assert lib.mmtta_memo_loss_items(ctypes.byref(_tensor(_l)), 0, 2, None, ctypes.byref(_tensor(_l)), FAKE, FAKE, None) == INVALID
    assert b"view_axes" in lib.mmtta_last_error()
    assert _loss(lib, _l, axes=_axes(1, 0)) == INVALID and b"view 0" in lib.mmtta_last_error()
    assert _loss(lib, _l, axes=_axes(0, 8)) == INVALID and b"view_axes[1]" in lib.mmtta_last_error()
    assert _loss(lib, _l, z=_tensor(_l, n=6), g=_tensor(_l, n=6), views=4) == INVALID
    assert b"no multiple of views" in lib.mmtta_last_error()
    for bad in (_tensor(_l, n=2), _tensor(_l, c=2), _tensor(_l, d=5), _tensor(_l, h=3), _tensor(_l, w=2)):
        assert _loss(lib, _l, g=bad) == INVALID
        assert b"shape mismatch" in lib.mmtta_last_error()
    assert _loss(lib, _l, z=_tensor(_l, dtype=_l.BF16)) == UNSUPPORTED and b"fp32-stored" in lib.mmtta_last_error()
    assert _loss(lib, _l, softmax=1, g=_tensor(_l, dtype=_l.BF16)) == UNSUPPORTED
    assert _loss(lib, _l, g=_tensor(_l, dtype=_l.BF16, flags=0)) == UNSUPPORTED and b"own their pad" in lib.mmtta_last_error()
    assert _loss(lib, _l, softmax=1, z=_tensor(_l, c=17, ldc=20), g=_tensor(_l, c=17, ldc=20)) == UNSUPPORTED
    assert lib.mmtta_memo_partials(None, 2) == -1
    assert lib.mmtta_memo_partials(ctypes.byref(_tensor(_l)), 3) == -1
    assert lib.mmtta_memo_partials(ctypes.byref(_tensor(_l, n=6)), 4) == -1
    # one volume's block partials (4*4*4*3 elements -> 1 workgroup), per volume
    assert lib.mmtta_memo_partials(ctypes.byref(_tensor(_l, n=6)), 2) == 3
    assert lib.mmtta_memo_partials(ctypes.byref(_tensor(_l, n=8, d=16, h=16, w=16)), 4) == 2 * (16 ** 3 * 3 // 256)


def test_memo_ensemble_and_mirror_views_reject_bad_arguments_without_a_gpu():
    _l, lib = _lib()
    z, out, ax = _tensor(_l), _tensor(_l, n=2), _axes(0, 1)
    ens = lambda z=z, out=out, views=2, ax=ax, softmax=0: lib.mmtta_memo_ensemble(
        None if z is None else ctypes.byref(z), softmax, views, ax, None if out is None else ctypes.byref(out), None)
    mir = lambda x=out, y=z, views=2, ax=ax: lib.mmtta_mirror_views(
        None if x is None else ctypes.byref(x), None if y is None else ctypes.byref(y), views, ax, None)
    for fn in (ens, mir):
        for kw in ({"z": None}, {"out": None}) if fn is ens else ({"x": None}, {"y": None}):
            assert fn(**kw) == INVALID and b"null argument" in lib.mmtta_last_error()
        assert fn(views=3) == INVALID and b"views = 3" in lib.mmtta_last_error()
        assert fn(ax=None) == INVALID and b"view_axes" in lib.mmtta_last_error()
        assert fn(ax=_axes(2, 0)) == INVALID
    assert ens(out=_tensor(_l, n=4)) == INVALID and b"shape mismatch" in lib.mmtta_last_error()
    assert ens(out=_tensor(_l, n=2, w=5)) == INVALID and b"shape mismatch" in lib.mmtta_last_error()
    assert ens(z=_tensor(_l, n=3), out=_tensor(_l, n=1)) == INVALID and b"no multiple" in lib.mmtta_last_error()
    assert ens(out=_tensor(_l, n=2, dtype=_l.BF16)) == UNSUPPORTED
    assert mir(x=_tensor(_l, n=1)) == INVALID and b"shape mismatch" in lib.mmtta_last_error()
    assert mir(x=_tensor(_l, n=2, dtype=_l.BF16)) == INVALID and b"shape mismatch" in lib.mmtta_last_error()
    assert mir(y=_tensor(_l, flags=0)) == UNSUPPORTED and b"pad lanes" in lib.mmtta_last_error()
    assert mir(x=_tensor(_l, n=2, c=3, ldc=3)) == UNSUPPORTED and b"one width" in lib.mmtta_last_error()
    # gridDim.y carries the volume / output item: more than 65535 is refused, not launched
    big = 65536
    assert mir(x=_tensor(_l, n=big), y=_tensor(_l, n=2 * big)) == UNSUPPORTED and b"65535" in lib.mmtta_last_error()
    assert ens(z=_tensor(_l, n=2 * big), out=_tensor(_l, n=big)) == UNSUPPORTED and b"65535" in lib.mmtta_last_error()
    assert _loss(lib, _l, z=_tensor(_l, n=2 * big), g=_tensor(_l, n=2 * big)) == UNSUPPORTED and b"65535" in lib.mmtta_last_error()
