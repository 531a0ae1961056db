"""CoTTA adaptation (``cotta_tta``, ``method=tta_cotta``): the host-side half, no GPU needed.

The config composes and the plugin reads and validates its keys; a NumPy restatement of Philox4x32-10 (the restore draw of
DESIGN.md section 7, which tests/test_hip_cotta.py holds the kernel to) reproduces the Random123 known-answer vectors and
draws the specified share; the new entry points refuse bad arguments before anything reaches the device."""
import ctypes
import math

import numpy as np
import pytest

INVALID, UNSUPPORTED = -1, -2
FAKE = 4096          # a 16-byte aligned address that is never dereferenced: the checks fail first

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85


# ----------------------------------------------------------------------------- the restore draw, restated
def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars), key: two -> the four output words (uint32 arrays)."""
    c = [np.asarray(v, dtype=np.uint64) & 0xFFFFFFFF for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)          # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(0xFFFFFFFF),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(0xFFFFFFFF)]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def restore_uniforms(n, seed, t, ordinal):
    """u_i for i in [0, n): word i & 3 of Philox at counter (i >> 2, t, ordinal, 0), key (seed lo, seed hi); fp32."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((q, t, ordinal, 0), (seed & 0xFFFFFFFF, seed >> 32))
    w = np.stack(words, 1).reshape(-1)[:n]
    return (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def restore_mask(n, seed, t, ordinal, p):
    return restore_uniforms(n, seed, t, ordinal) < np.float32(p)


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_restatement_reproduces_the_random123_known_answers(counter, key, want):
    got = tuple(int(v) for v in philox4x32_10(counter, key))
    assert got == want, [hex(v) for v in got]


def test_restore_draw_gives_the_specified_share():
    n, p = 1 << 20, 0.01
    share = float(restore_mask(n, 0, 1, 0, p).mean())
    sigma = math.sqrt(p * (1 - p) / n)
    print(f"share of u < {p}: {share:.6f}, {(share - p) / sigma:+.2f} sigma")
    assert abs(share - p) <= 5 * sigma
    u = restore_uniforms(4096, 7, 3, 5)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    # the counter words matter: another step, ordinal or seed draws other numbers
    for other in (restore_uniforms(4096, 7, 4, 5), restore_uniforms(4096, 7, 3, 6), restore_uniforms(4096, 8, 3, 5),
                  restore_uniforms(4096, 7 + (1 << 32), 3, 5)):
        assert (other != u).mean() > 0.99


# ----------------------------------------------------------------------------- config and plugin
def test_cotta_is_a_registered_plugin():
    import multimodal_tta_amd  # noqa: F401
    from multimodal_tta_amd.registry import get_plugin, list_plugins
    assert {"cotta_tta", "memo_tta", "sar_tta", "entmin_tta"} <= set(list_plugins())
    assert get_plugin("cotta_tta").__name__ == "MeanTeacherTTA"


def test_tta_cotta_config_composes_and_the_plugin_reads_it():
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin
    cfg = compose(overrides=["task=brats", "dataset=brats", "model=unet", "method=tta_cotta"])
    assert cfg["method"]["name"] == "cotta_tta" and cfg["method"]["kind"] == "tta"
    c = cfg["method"]["cotta"]
    assert list(c["mirror_axes"]) == ["h", "w"] and c["alpha"] == 0.999 and c["restore_p"] == 0.01 and c["seed"] == 0
    plug = get_plugin("cotta_tta")(cfg)
    assert plug.mirror_axes == ["h", "w"] and plug.views == 4 and plug.view_axes == [0, 2, 1, 3]
    assert plug.alpha == 0.999 and plug.restore_p == 0.01 and plug.seed == 0 and plug.fused_update is False
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_cotta", "method.cotta.mirror_axes=[]",
                             "method.cotta.alpha=1", "method.cotta.restore_p=0", "method.cotta.seed=12345678901234567890",
                             "method.episodic=false"])
    plug = get_plugin("cotta_tta")(cfg)
    assert plug.views == 1 and plug.view_axes == [0] and plug.alpha == 1.0 and plug.restore_p == 0.0
    assert plug.seed == 12345678901234567890 and plug.episodic is False


def test_tta_cotta_carries_every_key_of_tta_entmin():
    from multimodal_tta_amd.config import compose
    ent = compose(overrides=["task=brats", "model=unet", "method=tta_entmin"])["method"]
    cot = compose(overrides=["task=brats", "model=unet", "method=tta_cotta"])["method"]
    assert set(cot) == set(ent) | {"cotta"}
    for k in ent:
        if k not in ("name", "group"):          # `group` ships smaller: the teacher's forward carries V views per volume
            assert cot[k] == ent[k], k
    assert 1 <= cot["group"] <= ent["group"]


def _cfg(**cotta):
    from multimodal_tta_amd.config import compose
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_cotta"])
    for k, v in cotta.items():
        cfg["method"]["cotta"][k] = v
    return cfg


@pytest.mark.parametrize("key,bad", [("alpha", -0.1), ("alpha", 1.5), ("alpha", float("nan")), ("alpha", "high"), ("alpha", True),
                                     ("restore_p", -1e-3), ("restore_p", 1.0), ("restore_p", float("nan")), ("restore_p", None),
                                     ("seed", -1), ("seed", 1 << 64), ("seed", 0.5),
                                     ("mirror_axes", ["x"]), ("mirror_axes", ["h", "h"]), ("mirror_axes", "hw"), ("mirror_axes", 3)])
def test_cotta_plugin_rejects_bad_keys(key, bad):
    from multimodal_tta_amd.registry import get_plugin
    cfg = _cfg()
    if bad is None:
        cfg["method"]["cotta"][key] = "often"
    else:
        cfg["method"]["cotta"][key] = bad
    with pytest.raises(ValueError, match=f"method.cotta.{key}"):
        get_plugin("cotta_tta")(cfg)


def test_cotta_plugin_accepts_the_ends_of_the_ranges_and_rejects_moddrop():
    from multimodal_tta_amd.registry import get_plugin
    for kw in ({"alpha": 0.0}, {"alpha": 1.0}, {"restore_p": 0.0}, {"restore_p": 0.999}, {"seed": (1 << 64) - 1},
               {"mirror_axes": ["d", "h", "w"]}):
        get_plugin("cotta_tta")(_cfg(**kw))
    cfg = _cfg()
    cfg["method"]["moddrop"] = {"enabled": True, "p": 0.5, "seed": 0}
    with pytest.raises(NotImplementedError, match="method.moddrop.enabled"):
        get_plugin("cotta_tta")(cfg)


# ----------------------------------------------------------------------------- the entry points, without a GPU
def _lib():
    import __graft_entry__ as ge
    ge.build()
    from multimodal_tta_amd import _lib
    return _lib, _lib.load()


def _tensor(_l, n=2, c=3, d=4, h=4, w=4, ptr=FAKE, dtype=None, ldc=4, flags=None):
    return _l.Tensor(ptr, n, c, d, h, w, d * h * w * ldc, 1, h * w * ldc, w * ldc, ldc, _l.F32 if dtype is None else dtype,
                     _l.TENSOR_OWNS_PAD if flags is None else flags)


def test_the_library_exports_the_cotta_entry_points():
    _l, lib = _lib()
    for name in ("mmtta_consistency_partials", "mmtta_consistency_loss_items", "mmtta_cotta_update_partials",
                 "mmtta_cotta_update_sets"):
        assert hasattr(ctypes.CDLL(_l.LIB_PATH), name) and name in _l.exported_names()
    assert lib.mmtta_abi_version() == 2


def test_consistency_loss_rejects_bad_arguments_without_a_gpu():
    _l, lib = _lib()

    def call(z=None, t=None, g=None, softmax=0, partial=FAKE, loss=FAKE):
        z, t, g = (_tensor(_l) if v is None else v for v in (z, t, g))
        ref = lambda v: None if v == "null" else ctypes.byref(v)
        return lib.mmtta_consistency_loss_items(ref(z), ref(t), softmax, ref(g), partial, loss, None)

    for kw in ({"z": "null"}, {"t": "null"}, {"g": "null"}, {"partial": None}, {"loss": None}, {"t": _tensor(_l, ptr=None)}):
        assert call(**kw) == INVALID and b"null argument" in lib.mmtta_last_error()
    for bad in (_tensor(_l, n=3), _tensor(_l, c=2), _tensor(_l, d=5), _tensor(_l, h=3), _tensor(_l, w=2)):
        assert call(t=bad) == INVALID and b"shape mismatch" in lib.mmtta_last_error()
        assert call(g=bad) == INVALID and b"shape mismatch" in lib.mmtta_last_error()
    assert call(z=_tensor(_l, dtype=_l.BF16)) == UNSUPPORTED and b"fp32-stored" in lib.mmtta_last_error()
    assert call(t=_tensor(_l, dtype=_l.BF16)) == UNSUPPORTED and b"fp32-stored" in lib.mmtta_last_error()
    assert call(softmax=1, g=_tensor(_l, dtype=_l.BF16)) == UNSUPPORTED
    assert call(g=_tensor(_l, dtype=_l.BF16, flags=0)) == UNSUPPORTED and b"own their pad" in lib.mmtta_last_error()
    big = [_tensor(_l, c=17, ldc=20) for _ in range(3)]
    assert call(*big, softmax=1) == UNSUPPORTED and b"classes" in lib.mmtta_last_error()
    many = [_tensor(_l, n=65536) for _ in range(3)]
    assert call(*many) == UNSUPPORTED and b"65535" in lib.mmtta_last_error()
    assert lib.mmtta_consistency_partials(None) == -1
    # one item's block partials (4*4*4*3 elements -> 1 workgroup), per item
    assert lib.mmtta_consistency_partials(ctypes.byref(_tensor(_l, n=5))) == 5
    assert lib.mmtta_consistency_partials(ctypes.byref(_tensor(_l, n=2, d=16, h=16, w=16))) == 2 * (16 ** 3 * 3 // 256)


def test_cotta_update_rejects_bad_arguments_without_a_gpu():
    _l, lib = _lib()

    def call(w=FAKE, teacher=FAKE, source=FAKE, n=1000, sets=2, ws=1024, ts=1000, alpha=0.9, p=0.1, seed=0, step=FAKE,
             ordinals=FAKE, partial=FAKE, restored=FAKE):
        return lib.mmtta_cotta_update_sets(w, teacher, source, n, sets, ws, ts, alpha, p, seed, step, ordinals, partial,
                                           restored, None)

    for k in ("w", "teacher", "source", "step", "ordinals", "partial", "restored"):
        assert call(**{k: None}) == INVALID and b"null argument" in lib.mmtta_last_error()
    for a in (-0.5, 1.001, float("nan")):
        assert call(alpha=a) == INVALID and b"alpha" in lib.mmtta_last_error()
    for p in (-0.1, 1.0, float("nan")):
        assert call(p=p) == INVALID and b"restore_p" in lib.mmtta_last_error()
    assert call(sets=0) == INVALID and b"sets" in lib.mmtta_last_error()
    assert call(n=-1) == INVALID
    assert call(ws=1022) == INVALID and b"strides" in lib.mmtta_last_error()
    assert call(ts=996) == INVALID and b"strides" in lib.mmtta_last_error()
    assert call(w=FAKE + 4) == UNSUPPORTED and b"aligned" in lib.mmtta_last_error()
    assert lib.mmtta_cotta_update_partials(-1, 1) == -1 and lib.mmtta_cotta_update_partials(8, 0) == -1
    assert lib.mmtta_cotta_update_partials(1003, 3) == 3          # 251 quads -> 1 workgroup per set
    assert lib.mmtta_cotta_update_partials(1 << 30, 2) == 2 * 4096
