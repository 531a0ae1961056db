"""LAME output refinement (``lame_tta``, ``method=tta_lame``): the host-side half, no GPU needed.

The symbol is declared, exported and typed; ``mmtta_lame_refine`` refuses every bad argument with MMTTA_ERR_INVALID (or
_UNSUPPORTED) and a message naming it before anything reaches the device; the plugin is registered, its config composes and
every bad value raises a ValueError naming its key; the float64 restatement the GPU tests compare against
(``lame_reference.py``) is pinned by three hand-computed cases."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from lame_reference import decision_gap, flipped, lame, offsets, shift

INVALID, UNSUPPORTED = -1, -2
FAKE = 4096          # 16-byte aligned addresses that are never dereferenced: the checks fail first
STEP = 1 << 28       # distance between the fake buffers: far more than any tensor below spans
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from multimodal_tta_amd import _lib
    return _lib, _lib.load()


# ----------------------------------------------------------------------------- the entry point
def test_the_lame_symbol_is_declared_exported_and_typed():
    _l, lib = _lib()
    header = open(os.path.join(ROOT, "include", "mmtta.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+mmtta_lame_refine\s*\(", code), "include/mmtta.h does not declare mmtta_lame_refine"
    assert "mmtta_lame_refine" in _l.exported_names()
    fn = ctypes.CDLL(_l.LIB_PATH).mmtta_lame_refine          # AttributeError: not exported
    assert fn is not None
    assert len(lib.mmtta_lame_refine.argtypes) == 12 and lib.mmtta_lame_refine.restype is ctypes.c_int
    assert lib.mmtta_abi_version() == 2


def _tensor(_l, slot=0, n=2, c=3, d=4, h=5, w=6, ptr=True, dtype=None, ldc=4, flags=None):
    return _l.Tensor((FAKE + slot * STEP) if ptr is True else ptr, n, c, d, h, w, d * h * w * ldc, 1, h * w * ldc, w * ldc, ldc,
                     _l.F32 if dtype is None else dtype, _l.TENSOR_OWNS_PAD if flags is None else flags)


def _refine(lib, _l, l0=None, x=None, work=None, out=None, mask=0xF, softmax=0, conn=26, weight=1.0, sigma=1.0, iters=3,
            flipped_ptr=FAKE + 5 * STEP, **skip):
    l0 = _tensor(_l, 0) if l0 is None else l0
    x = _tensor(_l, 1, c=4) if x is None else x
    work = _tensor(_l, 2) if work is None else work
    out = _tensor(_l, 3) if out is None else out
    ref = lambda t, name: None if skip.get(name) else ctypes.byref(t)
    return lib.mmtta_lame_refine(ref(l0, "no_l0"), ref(x, "no_x"), mask, softmax, conn, weight, sigma, iters, ref(work, "no_work"),
                                 ref(out, "no_out"), flipped_ptr, None)


def _err(lib):
    return lib.mmtta_last_error()


def test_lame_refine_rejects_null_pointers_without_a_gpu():
    _l, lib = _lib()
    for kw, word in (({"no_l0": True}, b"logits0"), ({"l0": _tensor(_l, 0, ptr=None)}, b"logits0"),
                     ({"no_work": True}, b"work"), ({"work": _tensor(_l, 2, ptr=None)}, b"work"),
                     ({"no_out": True}, b"out"), ({"out": _tensor(_l, 3, ptr=None)}, b"out"),
                     ({"flipped_ptr": None}, b"flipped"),
                     ({"no_x": True}, b"`x`"), ({"x": _tensor(_l, 1, c=4, ptr=None)}, b"`x`")):
        assert _refine(lib, _l, **kw) == INVALID, kw
        assert b"null" in _err(lib) and word in _err(lib), (kw, _err(lib))


def test_lame_refine_rejects_bad_scalars_without_a_gpu():
    _l, lib = _lib()
    for conn in (0, 4, 7, 8, 27, -6):
        assert _refine(lib, _l, conn=conn) == INVALID
        assert b"connectivity" in _err(lib)
    for iters in (0, -1, 65, 1000):
        assert _refine(lib, _l, iters=iters) == INVALID
        assert b"iterations" in _err(lib)
    for weight in (0.0, -1.0, 16.5, float("nan"), float("inf"), float("-inf")):
        assert _refine(lib, _l, weight=weight) == INVALID
        assert b"weight" in _err(lib)
    for sigma in (-0.5, float("nan"), float("inf"), float("-inf")):
        assert _refine(lib, _l, sigma=sigma) == INVALID
        assert b"sigma" in _err(lib)
    for mask in (0, 0x10, 0xFFFFFFF0):          # no bit among the 4 channels of x
        assert _refine(lib, _l, mask=mask) == INVALID
        assert b"channel_mask" in _err(lib)
    assert _refine(lib, _l, x=_tensor(_l, 1, c=2), mask=0xC) == INVALID          # bits 2, 3 with 2 channels
    assert b"channel_mask" in _err(lib)


def test_lame_refine_rejects_mismatched_and_aliased_tensors_without_a_gpu():
    _l, lib = _lib()
    for bad in (dict(n=3), dict(c=2), dict(d=8), dict(h=2), dict(w=8)):
        assert _refine(lib, _l, work=_tensor(_l, 2, **bad)) == INVALID
        assert b"shape mismatch" in _err(lib) and b"work" in _err(lib)
        assert _refine(lib, _l, out=_tensor(_l, 3, **bad)) == INVALID
        assert b"shape mismatch" in _err(lib) and b"out" in _err(lib)
    for bad in (dict(n=3), dict(d=8), dict(h=2), dict(w=8)):
        assert _refine(lib, _l, x=_tensor(_l, 1, c=4, **bad)) == INVALID
        assert b"shape mismatch" in _err(lib) and b"`x`" in _err(lib)
    assert _refine(lib, _l, work=_tensor(_l, 2, ldc=8)) == INVALID
    assert b"row width" in _err(lib)
    assert _refine(lib, _l, out=_tensor(_l, 3, ldc=8)) == INVALID
    assert b"row width" in _err(lib)
    # aliased: equal, and overlapping without being equal
    for kw in ({"work": _tensor(_l, 0)}, {"out": _tensor(_l, 0)}, {"out": _tensor(_l, 2)},
               {"out": _tensor(_l, 0, ptr=FAKE + 16 * 7)}, {"work": _tensor(_l, 3, ptr=FAKE + 3 * STEP + 4 * 5 * 6 * 16)}):
        assert _refine(lib, _l, **kw) == INVALID, kw
        assert b"aliased" in _err(lib)
    assert _refine(lib, _l, x=_tensor(_l, 3, c=4)) == INVALID
    assert b"aliased" in _err(lib) and b"`x`" in _err(lib)


def test_lame_refine_refuses_what_it_has_no_kernel_for_without_a_gpu():
    _l, lib = _lib()
    wide = dict(c=17, ldc=20)
    assert _refine(lib, _l, l0=_tensor(_l, 0, **wide), work=_tensor(_l, 2, **wide), out=_tensor(_l, 3, **wide)) == UNSUPPORTED
    assert b"regions" in _err(lib)
    assert _refine(lib, _l, x=_tensor(_l, 1, **wide), mask=1) == UNSUPPORTED
    assert b"channels" in _err(lib)
    assert _refine(lib, _l, out=_tensor(_l, 3, dtype=_l.BF16)) == UNSUPPORTED
    assert b"fp32" in _err(lib)
    big = dict(n=1, d=1024, h=1024, w=512)          # 2^29 voxels x 4 floats = 2^31 elements in one item
    far = lambda slot: _tensor(_l, ptr=FAKE + slot * (1 << 40), **big)
    assert _refine(lib, _l, l0=far(0), x=_tensor(_l, ptr=FAKE + (1 << 42), c=4, **big), work=far(1), out=far(2)) == UNSUPPORTED
    assert b"2^31" in _err(lib)


def test_ops_lame_refine_checks_its_arguments_before_the_library():
    import torch
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.ops import MmttaError
    cpu = torch.zeros(1, 2, 2, 2, 3)
    with pytest.raises(MmttaError, match="flipped"):
        ops.lame_refine(cpu, None, cpu, cpu, torch.zeros(1, dtype=torch.int32), connectivity=26, weight=1.0, sigma=0.0,
                        iterations=1)


# ----------------------------------------------------------------------------- plugin and config
def _cfg(*extra):
    from multimodal_tta_amd.config import compose
    return compose(overrides=["task=brats", "model=unet", "method=tta_lame", *extra])


def test_lame_tta_is_registered_and_its_config_composes():
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin, list_plugins
    from multimodal_tta_amd.tta import EntropyMinimizationTTA
    assert "lame_tta" in list_plugins()
    assert compose(overrides=["method=tta_lame"])["method"]["name"] == "lame_tta"
    cfg = _cfg()
    assert cfg["method"]["name"] == "lame_tta" and cfg["method"]["kind"] == "tta"
    assert dict(cfg["method"]["lame"]) == {"iterations": 10, "weight": 1.0, "sigma": 1.0, "connectivity": 26}
    plug = get_plugin("lame_tta")(cfg)
    assert isinstance(plug, EntropyMinimizationTTA)
    assert (plug.iterations, plug.weight, plug.sigma, plug.connectivity) == (10, 1.0, 1.0, 26)
    assert plug.fused_update is True and plug.views == 1 and plug.records == EntropyMinimizationTTA.records
    plug = get_plugin("lame_tta")(_cfg("method.steps=0", "method.lame.iterations=0", "method.lame.weight=16",
                                       "method.lame.sigma=0", "method.lame.connectivity=6"))
    assert (plug.steps, plug.iterations, plug.weight, plug.sigma, plug.connectivity) == (0, 0, 16.0, 0.0, 6)
    # the block is optional: the defaults are the yaml's
    cfg = _cfg()
    del cfg["method"]["lame"]
    plug = get_plugin("lame_tta")(cfg)
    assert (plug.iterations, plug.weight, plug.sigma, plug.connectivity) == (10, 1.0, 1.0, 26)


def test_tta_lame_carries_every_key_of_tta_entmin():
    from multimodal_tta_amd.config import compose
    ent = compose(overrides=["task=brats", "model=unet", "method=tta_entmin"])["method"]
    lam = _cfg()["method"]
    assert set(lam) == set(ent) | {"lame"}
    for k in ent:
        if k != "name":
            assert lam[k] == ent[k], k


@pytest.mark.parametrize("key,value", [
    ("iterations", -1), ("iterations", 65), ("iterations", 2.0), ("iterations", True), ("iterations", "10"),
    ("weight", 0.0), ("weight", -1.0), ("weight", 16.5), ("weight", float("nan")), ("weight", float("inf")), ("weight", True),
    ("weight", "1"),
    ("sigma", -0.1), ("sigma", float("nan")), ("sigma", float("inf")), ("sigma", False), ("sigma", "1"),
    ("connectivity", 0), ("connectivity", 7), ("connectivity", 27), ("connectivity", 26.0), ("connectivity", True),
    ("connectivity", "26")])
def test_lame_plugin_rejects_bad_hyper_parameters(key, value):
    from multimodal_tta_amd.registry import get_plugin
    cfg = _cfg()
    cfg["method"]["lame"][key] = value
    with pytest.raises(ValueError, match=f"method.lame.{key} "):
        get_plugin("lame_tta")(cfg)


# ----------------------------------------------------------------------------- the restatement, pinned by hand
def test_the_neighbourhoods_and_the_shift():
    assert [len(offsets(c)) for c in (6, 18, 26)] == [6, 18, 26]
    assert set(offsets(6)) == {(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)}
    assert set(offsets(26)) - set(offsets(18)) == {(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)}
    a = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    s = shift(a, (1, -1, 0))
    assert s[0, 1, 2] == a[1, 0, 2] and s[1, 1, 2] == 0 and s[0, 0, 2] == 0 and s.shape == a.shape


def test_restatement_on_a_1x1x2_volume():
    """Two voxels: each has ONE neighbour (along W), whatever the connectivity; w = a / n."""
    la, lb, xa, xb, lam, sigma = 0.7, -1.3, 0.25, 1.0, 1.5, 0.8
    l0 = np.array([la, lb]).reshape(1, 1, 2, 1)
    x = np.array([xa, xb]).reshape(1, 1, 2, 1)
    a = math.exp(-(xa - xb) ** 2 / (2 * sigma ** 2))
    for conn in (6, 18, 26):
        a1, b1 = la + lam * a / conn * math.tanh(lb / 2), lb + lam * a / conn * math.tanh(la / 2)
        got = lame(l0, x, conn, lam, sigma, 1, False)
        assert np.allclose(got.reshape(-1), [a1, b1], rtol=0, atol=1e-15)
        a2, b2 = la + lam * a / conn * math.tanh(b1 / 2), lb + lam * a / conn * math.tanh(a1 / 2)          # Jacobi: both from l(1)
        got = lame(l0, x, conn, lam, sigma, 2, False)
        assert np.allclose(got.reshape(-1), [a2, b2], rtol=0, atol=1e-15)
        # sigma = 0: a = 1 and x is not read
        got = lame(l0, None, conn, lam, 0.0, 1, False)
        assert np.allclose(got.reshape(-1), [la + lam / conn * math.tanh(lb / 2), lb + lam / conn * math.tanh(la / 2)], atol=1e-15)
    # softmax head, R = 2: the neighbour's probabilities, no re-centring
    l0 = np.array([[0.2, -0.4], [1.0, 0.5]]).reshape(1, 1, 2, 2)
    pb = np.exp([1.0, 0.5]) / np.exp([1.0, 0.5]).sum()
    got = lame(l0, x, 6, lam, sigma, 1, True)
    assert np.allclose(got[0, 0, 0], np.array([0.2, -0.4]) + lam * a / 6 * pb, atol=1e-15)
    # a masked-out channel does not enter the affinity
    x2 = np.concatenate([x, 100.0 * x], -1)
    assert np.array_equal(lame(l0, x2, 6, lam, sigma, 2, True, present=[True, False]), lame(l0, x, 6, lam, sigma, 2, True))
    assert not np.array_equal(lame(l0, x2, 6, lam, sigma, 2, True), lame(l0, x, 6, lam, sigma, 2, True))


def test_restatement_on_a_uniform_volume_interior_and_corner():
    """Uniform logits and input: every affinity is 1.  An interior voxel has the full neighbourhood - its shift is
    lam * tanh(l / 2) -, a corner voxel 7 of 26 (3 of 6, 6 of 18) neighbours."""
    lval, lam = 1.1, 0.9
    l0 = np.full((5, 5, 5, 2), lval)
    x = np.full((5, 5, 5, 3), 0.37)
    t = math.tanh(lval / 2)
    for conn, corner, edge, face in ((26, 7, 11, 17), (18, 6, 9, 13), (6, 3, 4, 5)):
        got = lame(l0, x, conn, lam, 1.0, 1, False)
        assert abs(got[2, 2, 2, 0] - (lval + lam * t)) < 1e-15, "interior"
        assert abs(got[1, 3, 2, 1] - (lval + lam * t)) < 1e-15, "interior"
        for c in ((0, 0, 0), (4, 0, 4), (4, 4, 4)):
            assert abs(got[c][0] - (lval + lam * corner / conn * t)) < 1e-15, ("corner", conn)
        assert abs(got[0, 0, 2, 0] - (lval + lam * edge / conn * t)) < 1e-15, ("edge", conn)
        assert abs(got[0, 2, 2, 0] - (lval + lam * face / conn * t)) < 1e-15, ("face", conn)
    # softmax head: the interior shift of class k is lam * softmax(l)_k
    l0 = np.tile(np.array([0.3, -0.2, 1.0]), (5, 5, 5, 1))
    p = np.exp(l0[0, 0, 0]) / np.exp(l0[0, 0, 0]).sum()
    got = lame(l0, x, 26, lam, 1.0, 1, True)
    assert np.allclose(got[2, 2, 2], l0[0, 0, 0] + lam * p, atol=1e-15)
    assert np.allclose(got[0, 0, 0], l0[0, 0, 0] + lam * 7 / 26 * p, atol=1e-15)


def test_flip_count_and_decision_gap_of_the_restatement():
    l0 = np.array([[-0.1, 0.2], [0.3, -0.4]]).reshape(1, 1, 2, 2)
    l = np.array([[0.1, 0.2], [0.3, -0.5]]).reshape(1, 1, 2, 2)
    assert flipped(l0, l, False) == 1 and flipped(l0, l0, False) == 0
    assert flipped(l0, l, True) == 0          # arg max (1, 0) before and after
    assert flipped(l0, l[..., ::-1], True) == 2
    assert abs(decision_gap(l, False) - 0.1) < 1e-15 and abs(decision_gap(l, True) - 0.1) < 1e-15
    tie = np.array([1.0, 1.0, 0.0]).reshape(1, 1, 1, 3)
    assert flipped(tie, tie, True) == 0 and np.argmax(tie, -1).item() == 0          # the FIRST arg max


def test_fp32_arithmetic_of_the_restatement_sits_far_inside_the_gpu_tolerance():
    """The bound the GPU tests use, |got - ref| <= 1e-5 + 1e-5 |ref|, leaves a factor of ten over what fp32 arithmetic costs at
    weight 1: the fp32 run of this restatement against the float64 run."""
    rng = np.random.default_rng(0)
    l0 = rng.normal(0.0, 3.0, (9, 10, 35, 3))
    x = rng.normal(0.0, 1.0, (9, 10, 35, 4))
    l32 = lame(l0.astype(np.float32), x.astype(np.float32), 26, 1.0, 1.0, 10, False, dtype=np.float32)
    l64 = lame(l0.astype(np.float32), x.astype(np.float32), 26, 1.0, 1.0, 10, False)
    assert l32.dtype == np.float32
    err = np.abs(l32.astype(np.float64) - l64)
    assert err.max() <= 2e-6, err.max()
