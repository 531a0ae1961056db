"""Quarter-turn (rot90) views of ``memo_tta`` / ``cotta_tta`` without a GPU: the ``rot90`` block, the view codes (derived
here from ``torch.rot90`` on a small tensor), the ordering of the views with mirrors and intensity copies, the rejected
combinations, the shipped YAML, and the argument checks of the C entry points."""
import ctypes

import numpy as np
import pytest
import torch

FAKE = 4096          # a 16-byte aligned address that is never dereferenced: the checks fail first
INVALID, UNSUPPORTED = -1, -2
VALID = list(range(8)) + list(range(16, 24))          # bit 3 (value 8) is not a code: it was invalid before and stays so


# ----------------------------------------------------------------------------- the code of a view, restated
def apply_code(x, code):
    """x [D,H,W,C] -> the view with code ``code``: bit 4 transposes H and W, then bits 0-2 mirror W, H, D of the result."""
    y = x.transpose(1, 2) if code & 16 else x
    dims = [dim for bit, dim in ((4, 0), (2, 1), (1, 2)) if code & bit]
    return torch.flip(y, dims) if dims else y


def code_of(fn, shape=(2, 3, 3, 2)):
    """The one valid code (0..7, 16..23) whose view of an all-distinct tensor equals fn(x)."""
    x = torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(shape)
    hits = [c for c in VALID if torch.equal(apply_code(x, c), fn(x))]
    assert len(hits) == 1, hits
    return hits[0]


def test_quarter_turn_codes_are_those_of_torch_rot90():
    from multimodal_tta_amd.memo import ROT90_CODES
    for k in (1, 2, 3):
        assert ROT90_CODES[k] == code_of(lambda x: torch.rot90(x, k, dims=(1, 2))), k
    assert set(ROT90_CODES) == {1, 2, 3}
    # the coordinate form of the contract: frame voxel (d, h, w) sits at view voxel (fd(d), fh(w), fw(h)) under bit 4
    D, H = 2, 3
    x = torch.arange(D * H * H, dtype=torch.float32).reshape(D, H, H, 1)
    for code in range(16, 24):
        y = apply_code(x, code)
        for d in range(D):
            for h in range(H):
                for w in range(H):
                    vd = D - 1 - d if code & 4 else d
                    vh = H - 1 - w if code & 2 else w
                    vw = H - 1 - h if code & 1 else h
                    assert y[vd, vh, vw, 0] == x[d, h, w, 0]


def test_mirror_after_rotation_composes_as_documented():
    from multimodal_tta_amd.memo import ROT90_CODES, rotated_code
    for k in (0, 1, 2, 3):
        r = ROT90_CODES[k] if k else 0
        for m in range(8):
            want = code_of(lambda x: apply_code(torch.rot90(x, k, dims=(1, 2)), m))
            assert rotated_code(r, m) == want == (r & 16) | ((r & 7) ^ m)


# ----------------------------------------------------------------------------- parsing
def test_parse_rot90_accepts_the_documented_values():
    from multimodal_tta_amd.memo import parse_rot90
    assert parse_rot90(None) == [] and parse_rot90({}) == [] and parse_rot90({"k": []}) == []
    assert parse_rot90({"k": [2]}) == [2] and parse_rot90({"k": [3, 1, 2]}) == [3, 1, 2] and parse_rot90({"k": (1,)}) == [1]


@pytest.mark.parametrize("bad", [{"k": 1}, {"k": "1"}, {"k": [0]}, {"k": [4]}, {"k": [1, 1]}, {"k": [True]}, {"k": [1.0]},
                                 {"k": [1], "axes": [1, 2]}, [1, 2, 3], 2, {"k": {"a": 1}}])
@pytest.mark.parametrize("method", ["memo", "cotta"])
def test_bad_rot90_blocks_name_their_key(bad, method):
    from multimodal_tta_amd.memo import parse_rot90
    with pytest.raises(ValueError, match=rf"method\.{method}\.rot90"):
        parse_rot90(bad, f"method.{method}.rot90")


# ----------------------------------------------------------------------------- the view set
def test_view_layout_orders_mirror_fastest_then_rotation_then_copy():
    from multimodal_tta_amd.intensity import parse_intensity, view_layout
    from multimodal_tta_amd.memo import view_masks
    assert view_layout([], 1, "method.memo.intensity", [1, 2, 3]) == [0, 18, 3, 17]          # the trainer's rotation group
    assert view_layout([], 1, "method.memo.intensity", [3, 1, 2]) == [0, 17, 18, 3]          # k in the listed order
    assert view_layout([], 1, "method.memo.intensity", [2]) == [0, 3]
    assert view_layout(["h"], 1, "method.memo.intensity", [1]) == [0, 2, 18, 16]
    assert view_layout(["w"], 2, "method.memo.intensity", [1]) == [0, 1, 18, 19] * 2
    eight = view_layout(["h"], 1, "method.memo.intensity", [1, 2, 3])
    assert eight == [0, 2, 18, 16, 3, 1, 17, 19] and len(set(eight)) == 8          # the square's symmetry group
    assert {c & 4 for c in eight} == {0}
    # every earlier call keeps its meaning: positional, keyword, no rotations
    for axes in ([], ["h"], ["h", "w"], ["d", "h", "w"]):
        assert view_layout(axes) == view_layout(axes, 1, "intensity", []) == view_masks(axes)
    assert view_layout(["h"], 2, "x") == [0, 2, 0, 2]
    spec = parse_intensity({"copies": 2, "scale": 0.1}, ["w"], "method.cotta.intensity", [1])
    assert spec.view_axes == [0, 1, 18, 19, 0, 1, 18, 19] and spec.views == 8
    assert parse_intensity(None, ["h", "w"]).view_axes == parse_intensity(None, ["h", "w"], "method.memo.intensity", []).view_axes == [0, 2, 1, 3]


def test_bad_view_counts_and_duplicate_views_are_rejected():
    from multimodal_tta_amd.intensity import parse_intensity, view_layout
    with pytest.raises(ValueError, match=r"method\.memo\.rot90.*V = 1 \* 3 \* 1 = 3"):
        view_layout([], 1, "method.memo.intensity", [1, 2])
    with pytest.raises(ValueError, match=r"method\.cotta\.rot90.*16 views"):
        view_layout(["h", "w"], 1, "method.cotta.intensity", [1, 2, 3])
    with pytest.raises(ValueError, match=r"method\.memo\.rot90.*16 views"):
        parse_intensity({"copies": 4, "scale": 0.1}, ["h"], "method.memo.intensity", [1])
    # [h, w] already holds the half turn (code 3): k: [2] repeats every view
    with pytest.raises(ValueError, match=r"method\.memo\.rot90.*same view \(code 3\)"):
        view_layout(["h", "w"], 1, "method.memo.intensity", [2])
    with pytest.raises(ValueError, match=r"method\.cotta\.rot90.*same view"):
        view_layout([], 2, "method.cotta.intensity", [1, 1, 2])          # (parse_rot90 refuses the repeat before this)
    assert view_layout(["h", "w"], 1, "method.cotta.intensity", [1]) == [0, 2, 1, 3, 18, 16, 19, 17]          # distinct: fine


@pytest.mark.parametrize("method", ["memo", "cotta"])
def test_plugins_read_the_block(method):
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin
    import multimodal_tta_amd  # noqa: F401
    cfg = compose(overrides=["task=brats", "model=unet", f"method=tta_{method}"])
    assert list(cfg["method"][method]["rot90"]["k"]) == []
    plug = get_plugin(f"{method}_tta")(cfg)
    assert plug.rot90 == [] and plug.views == 4 and plug.view_axes == [0, 2, 1, 3]          # the shipped views, as before
    del cfg["method"][method]["rot90"]
    assert get_plugin(f"{method}_tta")(cfg).view_axes == [0, 2, 1, 3]          # a config written before the block existed
    cfg["method"][method]["mirror_axes"] = []
    cfg["method"][method]["rot90"] = {"k": [1, 2, 3]}
    plug = get_plugin(f"{method}_tta")(cfg)
    assert plug.rot90 == [1, 2, 3] and plug.view_axes == [0, 18, 3, 17] and plug.views == 4
    if method == "memo":
        assert plug.fused_update is False
    cfg["method"][method]["rot90"] = {"k": [1, 2]}
    with pytest.raises(ValueError, match=rf"method\.{method}\.rot90"):
        get_plugin(f"{method}_tta")(cfg)
    cfg["method"][method]["rot90"] = {"k": [1]}
    cfg["method"]["moddrop"] = {"enabled": True, "p": 0.5, "seed": 0}
    with pytest.raises(NotImplementedError, match="moddrop"):
        get_plugin(f"{method}_tta")(cfg)


def test_non_square_planes_are_refused_with_key_and_extents():
    from multimodal_tta_amd.memo import check_square
    check_square([0, 3], 160, 192, "method.memo.rot90")          # a half turn needs no square
    check_square([0, 18, 3, 17], 144, 144, "method.memo.rot90")
    with pytest.raises(ValueError, match=r"method\.cotta\.rot90.*H = 160, W = 192"):
        check_square([0, 18, 3, 17], 160, 192, "method.cotta.rot90")


# ----------------------------------------------------------------------------- the entry points, without a GPU
def _lib():
    import __graft_entry__ as ge
    ge.build()
    from multimodal_tta_amd import _lib
    return _lib, _lib.load()


def _tensor(_l, n=4, c=3, d=4, h=4, w=4, ptr=FAKE, dtype=None, ldc=4):
    return _l.Tensor(ptr, n, c, d, h, w, d * h * w * ldc, 1, h * w * ldc, w * ldc, ldc, _l.F32 if dtype is None else dtype,
                     _l.TENSOR_OWNS_PAD)


def test_entry_points_reject_codes_outside_the_two_ranges_and_non_square_planes():
    """No launch is reached: every call below fails its argument checks (a square call with a valid code would launch)."""
    _l, lib = _lib()
    assert lib.mmtta_abi_version() == 2
    ax = lambda *m: (ctypes.c_int32 * len(m))(*m)
    z, g1, sq = _tensor(_l, h=4, w=6), _tensor(_l, n=2, h=4, w=6), _tensor(_l)
    ident = np.tile(np.array((1.0, 1.0, 0.0, 0.0), dtype=np.float32), 2 * 2 * 3)
    calls = {
        "loss": lambda t, o, a: lib.mmtta_memo_loss_items(ctypes.byref(t), 0, 2, a, ctypes.byref(t), FAKE, FAKE, None),
        "ensemble": lambda t, o, a: lib.mmtta_memo_ensemble(ctypes.byref(t), 0, 2, a, ctypes.byref(o), None),
        "mirror": lambda t, o, a: lib.mmtta_mirror_views(ctypes.byref(o), ctypes.byref(t), 2, a, None),
        "augment": lambda t, o, a: lib.mmtta_augment_views(ctypes.byref(o), ctypes.byref(t), 2, a,
                                                           ident.ctypes.data_as(ctypes.c_void_p), FAKE, FAKE, 0, FAKE, None),
    }
    for name, call in calls.items():
        for code in (16, 18, 17, 23):
            assert call(z, g1, ax(0, code)) == INVALID, (name, code)
            msg = lib.mmtta_last_error()
            assert b"h = 4" in msg and b"w = 6" in msg and b"view_axes[1]" in msg, (name, msg)
        for code in (8, 10, 15, 24, 32, -1, -8):
            assert call(sq, _tensor(_l, n=2), ax(0, code)) == INVALID and b"view_axes[1]" in lib.mmtta_last_error(), (name, code)
        assert call(sq, _tensor(_l, n=2), ax(18, 0)) == INVALID and b"view 0" in lib.mmtta_last_error()
