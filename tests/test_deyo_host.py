"""DeYO adaptation (``deyo_tta``, ``method=tta_deyo``): the host-side half, no GPU needed.

The config composes and the plugin reads and validates its keys; the permutation draw equals a Fisher-Yates restatement over
Philox4x32-10; the two new entry points (patch shuffle, PLPD-weighted entropy) refuse every bad argument with
MMTTA_ERR_INVALID and a message before anything reaches the device."""
import ctypes

import pytest

INVALID = -1
FAKE = 4096          # 16-byte aligned addresses that are never dereferenced: the checks fail first
FAR = 1 << 30


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from multimodal_tta_amd import _lib
    return _lib, _lib.load()


def _cfg(*extra):
    from multimodal_tta_amd.config import compose
    return compose(overrides=["task=brats", "model=unet", "method=tta_deyo", *extra])


def test_tta_deyo_config_composes_and_the_plugin_reads_it():
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin, list_plugins
    assert compose(overrides=["method=tta_deyo"])["method"]["name"] == "deyo_tta"
    cfg = _cfg()
    assert cfg["method"]["name"] == "deyo_tta" and cfg["method"]["kind"] == "tta"
    d = cfg["method"]["deyo"]
    assert d["e_margin"] == 0.5 and d["e_margin0"] == 0.4 and d["plpd_threshold"] == 0.2 and d["seed"] == 0
    assert list(d["patches"]) == [4, 4, 4]
    assert "deyo_tta" in list_plugins()
    plug = get_plugin("deyo_tta")(cfg)
    assert (plug.e_margin, plug.e_margin0, plug.plpd_threshold, plug.patches, plug.seed) == (0.5, 0.4, 0.2, [4, 4, 4], 0)
    assert plug.fused_update is True and plug.views == 1
    assert abs(plug.margin(3) - 0.5 * 0.6931471805599453) < 1e-12          # sigmoid head: K = 2
    assert abs(plug.margin(3, plug.e_margin0) - 0.4 * 0.6931471805599453) < 1e-12
    plug.softmax = True
    assert abs(plug.margin(4) - 0.5 * 1.3862943611198906) < 1e-12          # softmax head: K = R
    assert [k for k, _, _ in plug.records] == ["losses", "kept", "kept_entropy"]
    plug = get_plugin("deyo_tta")(_cfg("method.deyo.e_margin=0.8", "method.deyo.plpd_threshold=-1", "method.deyo.patches=[2,1,8]",
                                       "method.deyo.seed=18446744073709551615"))
    assert plug.e_margin == 0.8 and plug.plpd_threshold == -1.0 and plug.patches == [2, 1, 8] and plug.seed == (1 << 64) - 1


def test_tta_deyo_carries_every_key_of_tta_entmin():
    from multimodal_tta_amd.config import compose
    ent = compose(overrides=["task=brats", "model=unet", "method=tta_entmin"])["method"]
    deyo = _cfg()["method"]
    assert set(deyo) == set(ent) | {"deyo"}
    for k in ent:
        if k != "name":
            assert deyo[k] == ent[k], k


@pytest.mark.parametrize("key,value", [
    ("e_margin", 0.0), ("e_margin", -1.0), ("e_margin", float("nan")), ("e_margin", float("inf")), ("e_margin", True),
    ("e_margin0", 0.0), ("e_margin0", -0.4), ("e_margin0", float("nan")), ("e_margin0", float("inf")), ("e_margin0", "0.4"),
    ("plpd_threshold", 1.0), ("plpd_threshold", -1.5), ("plpd_threshold", float("nan")), ("plpd_threshold", float("inf")),
    ("plpd_threshold", False),
    ("seed", -1), ("seed", 1 << 64), ("seed", 1.5), ("seed", True),
    ("patches", [4, 4]), ("patches", [4, 4, 4, 4]), ("patches", [0, 4, 4]), ("patches", [17, 1, 1]), ("patches", [1, 1, 1]),
    ("patches", [2.0, 2, 2]), ("patches", [True, 2, 2]), ("patches", 4), ("patches", "444")])
def test_deyo_plugin_rejects_bad_hyper_parameters(key, value):
    from multimodal_tta_amd.registry import get_plugin
    cfg = _cfg()
    cfg["method"]["deyo"][key] = value
    with pytest.raises(ValueError, match=f"method.deyo.{key} "):
        get_plugin("deyo_tta")(cfg)


def test_deyo_plugin_refuses_modality_dropout_but_takes_missing_modalities():
    from multimodal_tta_amd.registry import get_plugin
    cfg = _cfg()
    cfg["method"]["moddrop"] = {"enabled": True, "p": 0.5, "seed": 0}
    with pytest.raises(NotImplementedError, match="method.moddrop.enabled"):
        get_plugin("deyo_tta")(cfg)
    cfg = _cfg()
    cfg["method"]["missing_modalities"] = [1]
    assert get_plugin("deyo_tta")(cfg).missing == [1]


# ----------------------------------------------------------------------------- the draw
def fisher_yates(seed, ordinal, P):
    """The restatement: from the identity, j = P-1 .. 1, u = word 0 of Philox4x32-10 at the counter (j, 0, ordinal, 3) under
    the key (seed & 0xffffffff, seed >> 32), k = (u (j + 1)) >> 32, swap."""
    from multimodal_tta_amd.intensity import philox4x32_10
    perm = list(range(P))
    for j in range(P - 1, 0, -1):
        u = int(philox4x32_10((j, 0, ordinal, 3), (seed & 0xFFFFFFFF, seed >> 32))[0])
        k = (u * (j + 1)) >> 32
        assert 0 <= k <= j
        perm[j], perm[k] = perm[k], perm[j]
    return perm


@pytest.mark.parametrize("seed,ordinal,P", [(0, 0, 64), (0, 1, 64), (7, 3, 2), (1 << 40 | 5, (2 << 24) + 9, 8), ((1 << 64) - 1, (1 << 32) - 1, 4096),
                                            (3, 0, 27)])
def test_the_permutation_draw_is_the_fisher_yates_restatement(seed, ordinal, P):
    from multimodal_tta_amd.deyo import draw_permutation
    perm = draw_permutation(seed, ordinal, P)
    assert perm == fisher_yates(seed, ordinal, P)
    assert sorted(perm) == list(range(P)), "no bijection"
    assert perm == draw_permutation(seed, ordinal, P), "equal (seed, ordinal) must draw the same permutation"


def test_the_draw_depends_on_ordinal_and_seed_and_keeps_to_its_own_counter_word():
    from multimodal_tta_amd.deyo import DRAW_STREAM, draw_permutation
    assert DRAW_STREAM == 3
    a, b = draw_permutation(0, 0, 64), draw_permutation(0, 1, 64)
    assert a != b, "ordinals 0 and 1 drew the same permutation of 64 patches"
    assert a != list(range(64)) and draw_permutation(1, 0, 64) != a
    assert draw_permutation(0, 5, 1) == [0]


def test_patch_table_holds_the_permutation_and_its_inverse_and_refuses_anything_else():
    import torch
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.ops import MmttaError
    perms = [[2, 0, 3, 1], [0, 1, 2, 3], [3, 2, 1, 0]]
    t = ops.patch_table(perms)
    assert t.dtype == torch.int32 and tuple(t.shape) == (3, 2, 4)
    for n, p in enumerate(perms):
        assert t[n, 0].tolist() == p
        assert [p[j] for j in t[n, 1].tolist()] == [0, 1, 2, 3], "row 1 is not the inverse"
        assert all(t[n, 1, p[j]] == j for j in range(4))
    for bad in ([[0, 0, 1, 2]], [[0, 1, 2, 4]], [[-1, 0, 1, 2]], [[0, 1, 2, 3], [0, 1, 2]]):
        with pytest.raises(MmttaError, match="no permutation"):
            ops.patch_table(bad)


# ----------------------------------------------------------------------------- entry points
def test_the_deyo_symbols_are_exported_and_typed():
    _l, lib = _lib()
    for name in ("mmtta_patch_shuffle", "mmtta_deyo_partials", "mmtta_deyo_loss_items"):
        assert name in _l.exported_names() and getattr(lib, name).argtypes is not None
    assert lib.mmtta_abi_version() == 2


def _tensor(_l, n=2, c=3, d=4, h=4, w=4, ptr=FAKE, dtype=None, ldc=4, flags=None):
    return _l.Tensor(ptr, n, c, d, h, w, d * h * w * ldc, 1, h * w * ldc, w * ldc, ldc, _l.F32 if dtype is None else dtype,
                     _l.TENSOR_OWNS_PAD if flags is None else flags)


def _grid(*g):
    return (ctypes.c_int32 * 3)(*g)


def _shuffle(lib, _l, x=None, y=None, grid=(2, 2, 1), table=FAKE):
    x = _tensor(_l) if x is None else x
    y = _tensor(_l, ptr=FAR) if y is None else y
    return lib.mmtta_patch_shuffle(ctypes.byref(x), ctypes.byref(y), None if grid is None else _grid(*grid), table, None)


def test_patch_shuffle_rejects_bad_arguments_without_a_gpu():
    _l, lib = _lib()
    for kw in ({"x": _tensor(_l, ptr=None)}, {"y": _tensor(_l, ptr=None)}, {"table": None}):
        assert _shuffle(lib, _l, **kw) == INVALID
        assert b"null argument" in lib.mmtta_last_error()
    assert lib.mmtta_patch_shuffle(None, None, _grid(2, 2, 1), FAKE, None) == INVALID
    assert _shuffle(lib, _l, grid=None) == INVALID
    assert b"null patch grid" in lib.mmtta_last_error()
    for bad in (_tensor(_l, n=3, ptr=FAR), _tensor(_l, c=2, ptr=FAR), _tensor(_l, d=8, ptr=FAR), _tensor(_l, h=2, ptr=FAR),
                _tensor(_l, w=8, ptr=FAR), _tensor(_l, ptr=FAR, dtype=_l.BF16)):
        assert _shuffle(lib, _l, y=bad) == INVALID
        assert b"shape mismatch" in lib.mmtta_last_error()
    for g in ((3, 1, 1), (1, 3, 1), (1, 1, 3), (8, 1, 1)):
        assert _shuffle(lib, _l, grid=g) == INVALID
        assert b"does not divide" in lib.mmtta_last_error()
    for g in ((0, 2, 2), (2, -1, 2), (2, 2, 0)):
        assert _shuffle(lib, _l, grid=g) == INVALID
        assert b"patch grid" in lib.mmtta_last_error()
    assert _shuffle(lib, _l, grid=(1, 1, 1)) == INVALID
    assert b"1 patches" in lib.mmtta_last_error()
    big = dict(d=32, h=32, w=32)
    assert _shuffle(lib, _l, x=_tensor(_l, **big), y=_tensor(_l, ptr=FAR, **big), grid=(32, 16, 16)) == INVALID
    assert b"patches" in lib.mmtta_last_error()
    # in place, and overlapping without being equal
    assert _shuffle(lib, _l, y=_tensor(_l)) == INVALID
    assert b"in-place" in lib.mmtta_last_error()
    assert _shuffle(lib, _l, y=_tensor(_l, ptr=FAKE + 4 * 4 * 4 * 4 * 4)) == INVALID
    assert b"in-place" in lib.mmtta_last_error()


def _loss(lib, _l, z=None, zs=None, g=None, grid=(2, 2, 1), table=FAKE, margin=0.3, margin0=0.25, thr=0.2, keep_out=FAKE,
          partial=FAKE, loss=FAKE, kept=FAKE, kept_entropy=FAKE, softmax=0):
    z = _tensor(_l) if z is None else z
    zs = _tensor(_l) if zs is None else zs
    g = _tensor(_l) if g is None else g
    return lib.mmtta_deyo_loss_items(ctypes.byref(z), ctypes.byref(zs), None if grid is None else _grid(*grid), table, softmax,
                                     margin, margin0, thr, keep_out, ctypes.byref(g), partial, loss, kept, kept_entropy, None)


def test_deyo_loss_rejects_bad_arguments_without_a_gpu():
    _l, lib = _lib()
    for m in (float("nan"), float("inf"), float("-inf"), 0.0, -0.5):
        assert _loss(lib, _l, margin=m) == INVALID
        assert b"margin must" in lib.mmtta_last_error()
        assert _loss(lib, _l, margin0=m) == INVALID
        assert b"margin0" in lib.mmtta_last_error()
    for t in (float("nan"), float("inf"), 1.0, 1.5, -1.25):
        assert _loss(lib, _l, thr=t) == INVALID
        assert b"plpd_threshold" in lib.mmtta_last_error()
    assert _loss(lib, _l, keep_out=None) == INVALID
    assert b"null mask output" in lib.mmtta_last_error()
    for kw in ({"partial": None}, {"loss": None}, {"kept": None}, {"kept_entropy": None}, {"table": None},
               {"z": _tensor(_l, ptr=None)}, {"zs": _tensor(_l, ptr=None)}, {"g": _tensor(_l, ptr=None)}):
        assert _loss(lib, _l, **kw) == INVALID
        assert b"null argument" in lib.mmtta_last_error()
    assert _loss(lib, _l, grid=None) == INVALID
    assert b"null patch grid" in lib.mmtta_last_error()
    for bad in (_tensor(_l, n=3), _tensor(_l, c=2), _tensor(_l, d=8), _tensor(_l, h=2), _tensor(_l, w=8)):
        assert _loss(lib, _l, g=bad) == INVALID
        assert b"shape mismatch" in lib.mmtta_last_error()
        assert _loss(lib, _l, zs=bad) == INVALID
        assert b"shape mismatch" in lib.mmtta_last_error()
    for g in ((3, 1, 1), (1, 3, 1), (1, 1, 3)):
        assert _loss(lib, _l, grid=g) == INVALID
        assert b"does not divide" in lib.mmtta_last_error()
    assert _loss(lib, _l, grid=(1, 1, 1)) == INVALID
    assert b"1 patches" in lib.mmtta_last_error()
    big = dict(d=32, h=32, w=32)
    assert _loss(lib, _l, z=_tensor(_l, **big), zs=_tensor(_l, **big), g=_tensor(_l, **big), grid=(32, 16, 16)) == INVALID
    assert b"patches" in lib.mmtta_last_error()
    # storages without a kernel: bf16-stored logits of either kind
    assert _loss(lib, _l, zs=_tensor(_l, dtype=_l.BF16)) == -2
    assert lib.mmtta_deyo_partials(None) == -1
    z = _tensor(_l, n=3, d=4, h=4, w=4)
    assert lib.mmtta_deyo_partials(ctypes.byref(z)) == 3 * 3 * 1
    assert 2 * lib.mmtta_deyo_partials(ctypes.byref(z)) == 3 * lib.mmtta_entropy_weighted_partials(ctypes.byref(z))
