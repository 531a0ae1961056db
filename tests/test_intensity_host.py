"""Intensity-augmented views of ``memo_tta`` / ``cotta_tta`` (``multimodal_tta_amd/intensity.py``): the host-side half, no GPU
needed.

The package's host Philox reproduces the Random123 known answers; the parameter draws are deterministic, stay inside their
intervals, leave view 0 and absent channels alone and depend on the volume's ordinal, never on its slot; the layout of the
views; the validation of the ``intensity`` block; the shipped YAMLs compose to the off state; the new entry points refuse
bad arguments before anything reaches the device."""
import ctypes
import math

import numpy as np
import pytest

from test_cotta_host import philox4x32_10 as philox_restated

INVALID, UNSUPPORTED = -1, -2
FAKE = 4096          # a 16-byte aligned address that is never dereferenced: the checks fail first
IDENTITY = np.array([1, 1, 0, 0], dtype=np.float32)

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def spec(mirror_axes=("h",), **kw):
    from multimodal_tta_amd.intensity import parse_intensity
    return parse_intensity(kw, list(mirror_axes), "method.memo.intensity")


ALL_ON = dict(copies=2, scale=0.1, shift=0.1, gamma=0.3, noise_std=0.05)


# ----------------------------------------------------------------------------- the generator
@pytest.mark.parametrize("counter,key,want", KNOWN_ANSWERS)
def test_the_package_philox_reproduces_the_random123_known_answers(counter, key, want):
    from multimodal_tta_amd.intensity import philox4x32_10
    got = tuple(int(v) for v in philox4x32_10(counter, key))
    assert got == want, [hex(v) for v in got]


def test_the_package_philox_is_the_restatement_on_arrays():
    from multimodal_tta_amd.intensity import philox4x32_10
    rng = np.random.default_rng(3)
    ctr = [rng.integers(0, 1 << 32, size=257, dtype=np.uint64) for _ in range(3)] + [2]
    for a, b in zip(philox4x32_10(ctr, (7, 9)), philox_restated(ctr, (7, 9))):
        assert a.dtype == np.uint32 and np.array_equal(a, b)


# ----------------------------------------------------------------------------- the parameter draws
def restated_parameters(cfg, ordinal, view, channel):
    """(g, a, b, sigma) of one (volume, view, channel) from the issue's words: counter (c, v, ordinal, 2), c = 0 unless
    per_channel; u_j = (word_j >> 8) 2^-24; float64, rounded once."""
    w = philox_restated((channel if cfg.per_channel else 0, view, ordinal, 2), (cfg.seed & 0xFFFFFFFF, cfg.seed >> 32))
    u = [float(int(x) >> 8) * 2.0 ** -24 for x in w[:3]]
    return np.array([math.exp(cfg.gamma * (2 * u[0] - 1)), 1 + cfg.scale * (2 * u[1] - 1), cfg.shift * (2 * u[2] - 1),
                     cfg.noise_std], dtype=np.float64).astype(np.float32)


@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("seed", [0, 0x9E3779B97F4A7C15])
def test_view_parameters_are_the_specified_draws(per_channel, seed):
    from multimodal_tta_amd.intensity import view_parameters
    cfg = spec(per_channel=per_channel, seed=seed, **ALL_ON)
    ordinals = [5, 9, 2, (1 << 32) - 1]
    t = view_parameters(cfg, ordinals, 4)
    assert t.dtype == np.float32 and t.shape == (4, cfg.views, 4, 4) and t.flags["C_CONTIGUOUS"]
    assert np.array_equal(t, view_parameters(cfg, ordinals, 4)), "not deterministic"
    for b, o in enumerate(ordinals):
        for v in range(1, cfg.views):
            for c in range(4):
                assert np.array_equal(t[b, v, c], restated_parameters(cfg, o, v, c)), (b, v, c)
    # view 0 is the volume itself
    assert np.array_equal(t[:, 0], np.broadcast_to(IDENTITY, (4, 4, 4)))
    # one draw per view (the reference's whole-image transforms), or one per modality
    same = all(np.array_equal(t[:, :, 0], t[:, :, c]) for c in range(1, 4))
    assert same == (not per_channel)
    # every view v >= 1, every ordinal and every seed draws its own numbers
    rows = {tuple(t[b, v, 0]) for b in range(4) for v in range(1, cfg.views)}
    assert len(rows) == 4 * (cfg.views - 1)
    other = view_parameters(spec(per_channel=per_channel, seed=seed + 1, **ALL_ON), ordinals, 4)
    assert not np.any(np.all(other[:, 1:] == t[:, 1:], axis=-1))


def test_every_draw_lies_inside_its_interval():
    from multimodal_tta_amd.intensity import view_parameters
    cfg = spec(mirror_axes=(), copies=8, scale=0.1, shift=0.2, gamma=0.3, noise_std=0.05, per_channel=True)
    t = view_parameters(cfg, list(range(512)), 4)[:, 1:].astype(np.float64)
    f32 = lambda v: float(np.float32(v))          # the table is rounded once: the ends of an interval round with it
    g, a, b, s = (t[..., k] for k in range(4))
    assert f32(math.exp(-0.3)) <= g.min() and g.max() <= f32(math.exp(0.3))
    assert f32(0.9) <= a.min() and a.max() <= f32(1.1)
    assert f32(-0.2) <= b.min() and b.max() <= f32(0.2)
    assert np.all(s == f32(0.05))
    # and fills it: 14336 uniform draws each
    for x, lo, hi in ((np.log(g), -0.3, 0.3), (a, 0.9, 1.1), (b, -0.2, 0.2)):
        assert x.min() < lo + 0.01 * (hi - lo) and x.max() > hi - 0.01 * (hi - lo)
        assert abs(x.mean() - (lo + hi) / 2) <= 5 * (hi - lo) / math.sqrt(12 * x.size)


def test_a_zero_magnitude_draws_the_identity():
    from multimodal_tta_amd.intensity import view_parameters
    t = view_parameters(spec(copies=2, scale=0.1), [0, 1, 2], 3)
    assert np.all(t[..., 0] == 1) and np.all(t[..., 2] == 0) and np.all(t[..., 3] == 0) and not np.any(np.signbit(t[..., 2]))
    assert np.all(t[:, 1:, :, 1] != 1)


def test_absent_channels_carry_identity_rows():
    from multimodal_tta_amd.intensity import view_parameters
    cfg = spec(**ALL_ON)
    full = view_parameters(cfg, [4, 7], 4)
    t = view_parameters(cfg, [4, 7], 4, present=[True, False, True, False])
    assert np.array_equal(t[:, :, [1, 3]], np.broadcast_to(IDENTITY, (2, cfg.views, 2, 4)))
    assert np.array_equal(t[:, :, [0, 2]], full[:, :, [0, 2]])
    with pytest.raises(ValueError, match="modality mask"):
        view_parameters(cfg, [4], 4, present=[True, False])


def test_a_batch_equals_its_volumes_one_at_a_time():
    """The ordinal, not the slot, enters the draw."""
    from multimodal_tta_amd.intensity import view_parameters
    cfg = spec(per_channel=True, seed=11, **ALL_ON)
    ordinals = [5, 9, 2]
    batch = view_parameters(cfg, ordinals, 4)
    for b, o in enumerate(ordinals):
        assert np.array_equal(batch[b], view_parameters(cfg, [o], 4)[0])
    assert np.array_equal(view_parameters(cfg, [2, 5, 9], 4), batch[[2, 0, 1]])
    with pytest.raises(ValueError, match="ordinals"):
        view_parameters(cfg, [1 << 32], 4)


# ----------------------------------------------------------------------------- layout
def test_view_layout():
    from multimodal_tta_amd.intensity import view_layout
    from multimodal_tta_amd.memo import view_masks
    assert view_layout(["h"], 2) == [0, 2, 0, 2]
    assert view_layout([], 4) == [0, 0, 0, 0]
    assert view_layout(["h", "w"], 1) == view_masks(["h", "w"]) == [0, 2, 1, 3]
    assert view_layout(["h", "w"], 2) == [0, 2, 1, 3, 0, 2, 1, 3]
    assert view_layout(["d", "h", "w"], 1) == view_masks(["d", "h", "w"])
    for axes, copies in ((["d", "h", "w"], 2), (["h", "w"], 4), (["w"], 8)):
        with pytest.raises(ValueError, match="copies"):
            view_layout(axes, copies)


# ----------------------------------------------------------------------------- validation
def _cfg(method, **intensity):
    from multimodal_tta_amd.config import compose
    cfg = compose(overrides=["task=brats", "model=unet", f"method=tta_{method}"])
    for k, v in intensity.items():
        cfg["method"][method]["intensity"][k] = v
    return cfg


@pytest.mark.parametrize("method", ["memo", "cotta"])
@pytest.mark.parametrize("key,bad", [
    ("copies", {"copies": 2}),                                       # all four magnitudes 0: the views would be identical
    ("copies", {"copies": 4, "scale": 0.1}),                         # [h, w] x 4 = 16 views
    ("copies", {"copies": 3, "scale": 0.1}), ("copies", {"copies": 0}), ("copies", {"copies": 2.0, "scale": 0.1}),
    ("copies", {"copies": True}),
    ("scale", {"scale": -0.1}), ("scale", {"scale": float("nan")}), ("scale", {"scale": float("inf")}), ("scale", {"scale": 1.0}),
    ("scale", {"scale": 1.5}), ("scale", {"scale": "some"}),
    ("shift", {"shift": -1e-3}), ("shift", {"shift": float("inf")}), ("shift", {"shift": None}),
    ("gamma", {"gamma": -0.5}), ("gamma", {"gamma": float("nan")}), ("gamma", {"gamma": True}),
    ("noise_std", {"noise_std": -1.0}), ("noise_std", {"noise_std": float("-inf")}),
    ("per_channel", {"per_channel": 1}), ("per_channel", {"per_channel": "yes"}),
    ("seed", {"seed": -1}), ("seed", {"seed": 1 << 64}), ("seed", {"seed": 0.5}),
    ("strength", {"strength": 1.0}),                                 # an unknown key
])
def test_the_plugins_reject_a_bad_intensity_block(method, key, bad):
    from multimodal_tta_amd.registry import get_plugin
    cfg = _cfg(method)
    for k, v in bad.items():
        cfg["method"][method]["intensity"][k] = "often" if v is None else v
    with pytest.raises(ValueError, match=rf"method\.{method}\.intensity\.{key}"):
        get_plugin(f"{method}_tta")(cfg)


@pytest.mark.parametrize("method", ["memo", "cotta"])
def test_the_plugins_accept_the_ends_of_the_ranges(method):
    from multimodal_tta_amd.registry import get_plugin
    for kw in ({"scale": 0.999}, {"shift": 10.0}, {"gamma": 2.0}, {"noise_std": 1.0}, {"seed": (1 << 64) - 1, "shift": 0.1},
               {"copies": 2, "noise_std": 0.1}, {"copies": 2, "gamma": 0.1, "per_channel": True}):
        plug = get_plugin(f"{method}_tta")(_cfg(method, **kw))
        assert plug.intensity.active and plug.views == 4 * kw.get("copies", 1) and plug.view_axes == [0, 2, 1, 3] * kw.get("copies", 1)
    cfg = _cfg(method, copies=8, scale=0.1)
    cfg["method"][method]["mirror_axes"] = []
    plug = get_plugin(f"{method}_tta")(cfg)
    assert plug.views == 8 and plug.view_axes == [0] * 8
    cfg = _cfg(method, scale=0.1)
    cfg["method"][method]["intensity"] = "strong"
    with pytest.raises(ValueError, match=rf"method\.{method}\.intensity"):
        get_plugin(f"{method}_tta")(cfg)
    # modality dropout stays refused, with or without the block
    cfg = _cfg(method, scale=0.1)
    cfg["method"]["moddrop"] = {"enabled": True, "p": 0.5, "seed": 0}
    with pytest.raises(NotImplementedError, match="method.moddrop.enabled"):
        get_plugin(f"{method}_tta")(cfg)


def test_fused_update_stays_tied_to_one_view():
    from multimodal_tta_amd.registry import get_plugin
    cfg = _cfg("memo", scale=0.1)
    cfg["method"]["memo"]["mirror_axes"] = []
    assert get_plugin("memo_tta")(cfg).fused_update is True          # V = 1: view 0 alone, the method is entmin_tta
    cfg = _cfg("memo", scale=0.1, copies=2)
    cfg["method"]["memo"]["mirror_axes"] = []
    plug = get_plugin("memo_tta")(cfg)
    assert plug.views == 2 and plug.fused_update is False


# ----------------------------------------------------------------------------- defaults
@pytest.mark.parametrize("method", ["memo", "cotta"])
def test_the_shipped_yaml_composes_to_the_off_state(method):
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.intensity import IntensitySpec
    from multimodal_tta_amd.memo import view_masks
    from multimodal_tta_amd.registry import get_plugin
    cfg = compose(overrides=["task=brats", "dataset=brats", "model=unet", f"method=tta_{method}"])
    block = cfg["method"][method]["intensity"]
    assert dict(block) == dict(copies=1, scale=0.0, shift=0.0, gamma=0.0, noise_std=0.0, per_channel=False, seed=0)
    plug = get_plugin(f"{method}_tta")(cfg)
    assert plug.intensity == IntensitySpec(view_axes=view_masks(["h", "w"])) and not plug.intensity.active
    assert plug.views == 4 and plug.view_axes == [0, 2, 1, 3]
    # a config without the block (written before it existed) is the same plugin
    del cfg["method"][method]["intensity"]
    old = get_plugin(f"{method}_tta")(cfg)
    assert old.intensity == plug.intensity and old.view_axes == plug.view_axes


# ----------------------------------------------------------------------------- the entry points, without a GPU
def _lib():
    import __graft_entry__ as ge
    ge.build()
    from multimodal_tta_amd import _lib
    return _lib, _lib.load()


def _tensor(_l, n=2, c=3, d=4, h=4, w=4, ptr=FAKE, dtype=None, ldc=4, flags=None):
    return _l.Tensor(ptr, n, c, d, h, w, d * h * w * ldc, 1, h * w * ldc, w * ldc, ldc, _l.F32 if dtype is None else dtype,
                     _l.TENSOR_OWNS_PAD if flags is None else flags)


def test_the_library_exports_the_intensity_entry_points():
    _l, lib = _lib()
    for name in ("mmtta_intensity_range_partials", "mmtta_intensity_range", "mmtta_augment_views"):
        assert hasattr(ctypes.CDLL(_l.LIB_PATH), name) and name in _l.exported_names()
    assert lib.mmtta_abi_version() == 2


def test_intensity_range_rejects_bad_arguments_without_a_gpu():
    _l, lib = _lib()

    def call(x=None, partial=FAKE, out=FAKE):
        x = _tensor(_l) if x is None else x
        return lib.mmtta_intensity_range(None if x == "null" else ctypes.byref(x), partial, out, None)

    for kw in ({"x": "null"}, {"partial": None}, {"out": None}, {"x": _tensor(_l, ptr=None)}):
        assert call(**kw) == INVALID and b"null argument" in lib.mmtta_last_error()
    assert call(x=_tensor(_l, c=5, ldc=8)) == UNSUPPORTED and b"4 channels" in lib.mmtta_last_error()
    assert call(x=_tensor(_l, ptr=FAKE + 8)) == UNSUPPORTED and b"misaligned" in lib.mmtta_last_error()
    assert call(x=_tensor(_l, ptr=FAKE + 4, dtype=_l.BF16)) == UNSUPPORTED and b"misaligned" in lib.mmtta_last_error()
    assert call(x=_tensor(_l, dtype=7)) == UNSUPPORTED and b"fp32 or bf16" in lib.mmtta_last_error()
    assert call(x=_tensor(_l, n=65536)) == UNSUPPORTED and b"65535" in lib.mmtta_last_error()
    assert call(partial=FAKE + 4) == UNSUPPORTED and b"aligned" in lib.mmtta_last_error()
    assert lib.mmtta_intensity_range_partials(None) == -1 and b"null" in lib.mmtta_last_error()
    # one volume's block partials: 8 floats (4 lanes x (min, max)) per workgroup of 256 voxels, at most 2048 workgroups
    assert lib.mmtta_intensity_range_partials(ctypes.byref(_tensor(_l, n=5))) == 5 * 8
    assert lib.mmtta_intensity_range_partials(ctypes.byref(_tensor(_l, n=2, d=16, h=16, w=16))) == 2 * 16 * 8
    assert lib.mmtta_intensity_range_partials(ctypes.byref(_tensor(_l, n=1, d=128, h=128, w=128))) == 2048 * 8


def test_augment_views_rejects_bad_arguments_without_a_gpu():
    _l, lib = _lib()
    ident = np.tile(IDENTITY, 2 * 4 * 3)                               # [G = 2][V = 4][C = 3][4]
    keep = [ident]

    def call(x=None, y=None, views=4, axes=(0, 2, 1, 3), table_host=ident, table=FAKE, value_range=FAKE, seed=0, ordinals=FAKE):
        x = _tensor(_l) if x is None else x
        y = _tensor(_l, n=8) if y is None else y
        ref = lambda v: None if v == "null" else ctypes.byref(v)
        ax = None if axes is None else (ctypes.c_int32 * len(axes))(*axes)
        th = None if table_host is None else table_host.ctypes.data_as(ctypes.c_void_p)
        return lib.mmtta_augment_views(ref(x), ref(y), views, ax, th, table, value_range, seed, ordinals, None)

    for kw in ({"x": "null"}, {"y": "null"}, {"table_host": None}, {"table": None}, {"value_range": None}, {"ordinals": None},
               {"axes": None}, {"y": _tensor(_l, n=8, ptr=None)}):
        assert call(**kw) == INVALID and b"null argument" in lib.mmtta_last_error(), kw
    for v in (0, 3, 5, 16, -1):
        assert call(views=v) == INVALID and b"views" in lib.mmtta_last_error()
    assert call(axes=(1, 2, 1, 3)) == INVALID and b"view_axes[0]" in lib.mmtta_last_error()
    assert call(axes=(0, 8, 1, 3)) == INVALID and b"view_axes[1]" in lib.mmtta_last_error()
    assert call(y=_tensor(_l, n=6)) == INVALID and b"multiple" in lib.mmtta_last_error()
    for bad in (_tensor(_l, n=12), _tensor(_l, n=8, c=2), _tensor(_l, n=8, d=5), _tensor(_l, n=8, dtype=_l.BF16)):
        assert call(y=bad) == INVALID and b"shape mismatch" in lib.mmtta_last_error()
    assert call(y=_tensor(_l, n=8, flags=0)) == UNSUPPORTED and b"pad lanes" in lib.mmtta_last_error()
    assert call(x=_tensor(_l, c=5, ldc=8), y=_tensor(_l, n=8, c=5, ldc=8)) == UNSUPPORTED and b"4 channels" in lib.mmtta_last_error()
    assert call(x=_tensor(_l, ptr=FAKE + 8)) == UNSUPPORTED and b"misaligned" in lib.mmtta_last_error()
    assert call(table=FAKE + 4) == UNSUPPORTED and b"aligned" in lib.mmtta_last_error()
    # view 0's rows must be the identity, whatever the other rows hold (repeated masks are views like any other: the call
    # gets as far as the table)
    for g, c, k, val in ((0, 0, 1, 1.1), (1, 2, 2, 0.1), (1, 1, 0, 1.2), (0, 2, 3, 0.05)):
        t = ident.copy().reshape(2, 4, 3, 4)
        t[:, 1:] = (1.2, 0.9, 0.1, 0.05)
        t[g, 0, c, k] = val
        keep.append(t)
        assert call(table_host=t, axes=(0, 0, 2, 2)) == INVALID and b"view 0" in lib.mmtta_last_error()
