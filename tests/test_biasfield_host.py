"""Host half of the bias-field adaptation (``biasfield_tta``, ``mmtta_bias_field_apply`` / ``mmtta_bias_field_grad``): the basis
and its tables, the config parser's refusals, the plugin's registration and refusals, the entry points' argument checks (none
touches a device) and the torch restatement against its own analytic gradient.  The GPU half is ``test_hip_biasfield.py``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import biasfield_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE, STEP = 0x7F0000000000, 1 << 32          # device-looking addresses that are never dereferenced
INVALID, UNSUPPORTED = -1, -2
NAMES = {"mmtta_bias_field_apply", "mmtta_bias_field_grad", "mmtta_bias_field_grad_partials"}


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from multimodal_tta_amd import _lib as _l
    return _l, _l.load()


def _err(lib):
    return lib.mmtta_last_error()


def _rows(_l, slot=0, n=2, c=3, d=4, h=6, w=10, ptr=True, dtype=None, ldc=4, flags=None):
    return _l.Tensor((FAKE + slot * STEP) if ptr is True else ptr, n, c, d, h, w, d * h * w * ldc, 1, h * w * ldc, w * ldc, ldc,
                     _l.F32 if dtype is None else dtype, _l.TENSOR_OWNS_PAD if flags is None else flags)


def _dy(_l, slot=2, n=2, c0=8, d=2, h=3, w=5, ldc=None, **kw):
    return _rows(_l, slot, n=n, c=c0, d=d, h=h, w=w, ldc=c0 if ldc is None else ldc, **kw)


# ----------------------------------------------------------------------------- the basis
def test_term_counts_and_order():
    from multimodal_tta_amd import biasfield
    assert [len(biasfield.field_terms(o)) for o in range(4)] == [1, 4, 10, 20]
    want = [(0, 0, 0),
            (0, 0, 1), (0, 1, 0), (1, 0, 0),
            (0, 0, 2), (0, 1, 1), (0, 2, 0), (1, 0, 1), (1, 1, 0), (2, 0, 0),
            (0, 0, 3), (0, 1, 2), (0, 2, 1), (0, 3, 0), (1, 0, 2), (1, 1, 1), (1, 2, 0), (2, 0, 1), (2, 1, 0), (3, 0, 0)]
    assert biasfield.field_terms(3) == want
    for o in range(4):
        t = biasfield.field_terms(o)
        assert t == want[:len(t)] == ref.terms(o), "an order's terms are the first K of the list"
        assert t == sorted(t, key=lambda e: (sum(e), e)) and all(sum(e) <= o for e in t)
    for bad in (4, -1, True, 2.0, "2"):
        with pytest.raises(ValueError, match="order"):
            biasfield.field_terms(bad)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 128, 512])
def test_tables_are_the_legendre_polynomials_at_the_voxel_centres(n):
    from multimodal_tta_amd import biasfield
    t64 = biasfield.legendre_tables64(n)
    centres = (2.0 * np.arange(n) + 1.0) / n - 1.0
    assert t64.shape == (4, n) and t64.dtype == np.float64
    for a in range(4):
        want = np.polynomial.legendre.legval(centres, [0.0] * a + [1.0])
        assert np.abs(t64[a] - want).max() <= 1e-14, a
    assert np.abs(t64).max() <= 1.0 and (np.abs(centres) < 1.0).all()
    if n == 1:
        assert t64[:, 0].tolist() == [1.0, 0.0, -0.5, 0.0]
    t32, = biasfield.legendre_tables((n,))
    assert t32.dtype == np.float32 and np.array_equal(t32, t64.astype(np.float32)), "rounded once"
    assert np.array_equal(t32, ref.legendre_tables((n,), torch.float32)[0].numpy()), "the test restatement's tables"


def test_evaluate_field_is_exp_of_the_polynomial():
    from multimodal_tta_amd import biasfield
    rng = np.random.default_rng(0)
    ext = (3, 4, 5)
    for order in range(4):
        K = len(biasfield.field_terms(order))
        coeff = 0.2 * rng.standard_normal((2, 3, K))
        got = biasfield.evaluate_field(coeff, ext)
        tables = [t.double() for t in ref.legendre_tables(ext, torch.float32)]
        want = torch.exp(ref.log_field(torch.from_numpy(coeff), tables, order)).numpy()
        assert got.shape == (2, 3, *ext) and np.abs(got - want).max() <= 1e-14
    assert np.array_equal(biasfield.evaluate_field(np.zeros((4, 10)), ext), np.ones((4, *ext)))
    one = biasfield.evaluate_field(torch.tensor([0.5]), ext)
    assert one.shape == ext and np.allclose(one, np.exp(0.5)), "term 0 is the global log-gain"
    with pytest.raises(ValueError, match="terms"):
        biasfield.evaluate_field(np.zeros((4, 5)), ext)


# ----------------------------------------------------------------------------- the entry points
def test_the_bias_field_symbols_are_declared_exported_and_typed():
    _l, lib = _lib()
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmtta.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mmtta_bias_field_apply\s*\(", code) and re.search(r"\bint\s+mmtta_bias_field_grad\s*\(", code)
    assert re.search(r"\bint64_t\s+mmtta_bias_field_grad_partials\s*\(", code)
    assert NAMES <= set(_l.exported_names())
    for name in NAMES:
        assert getattr(ctypes.CDLL(_l.LIB_PATH), name) is not None
    assert len(lib.mmtta_bias_field_apply.argtypes) == 11 and len(lib.mmtta_bias_field_grad.argtypes) == 21
    assert lib.mmtta_bias_field_grad_partials.restype is ctypes.c_int64
    assert lib.mmtta_abi_version() == 2
    from multimodal_tta_amd import ops
    assert ops.BIAS_ANCHORS == {"min": int(re.search(r"#define MMTTA_BIAS_ANCHOR_MIN (\d+)", code).group(1)),
                                "zero": int(re.search(r"#define MMTTA_BIAS_ANCHOR_ZERO (\d+)", code).group(1))}


def test_grad_partials_answers_on_the_host():
    """4 K fp64 sums per tile of 4 x 8 x 64 input voxels and item."""
    _l, lib = _lib()
    count = lambda order, **kw: lib.mmtta_bias_field_grad_partials(ctypes.byref(_rows(_l, **kw)), order)
    for order, K in enumerate((1, 4, 10, 20)):
        assert count(order, n=1, d=2, h=2, w=2) == 4 * K
        assert count(order, n=3, d=5, h=9, w=65) == 3 * (2 * 2 * 2) * 4 * K
        assert count(order, n=1, d=128, h=128, w=128) == 32 * 16 * 2 * 4 * K
    assert lib.mmtta_bias_field_grad_partials(None, 2) == -1
    assert count(2, n=0) == -1 and b"partials" in _err(lib)
    assert count(4) == -1 and b"order" in _err(lib)
    assert count(-1) == -1 and b"order" in _err(lib)


def _apply(lib, _l, x=None, y=None, order=2, anchor=0, theta=FAKE + 5 * STEP, **ptrs):
    x = _rows(_l, 0) if x is None else x
    y = _rows(_l, 1) if y is None else y
    ref_ = lambda t, name: None if ptrs.get(name) else ctypes.byref(t)
    slot = lambda name, k: None if ptrs.get(name) else FAKE + k * STEP
    return lib.mmtta_bias_field_apply(ref_(x, "no_x"), ref_(y, "no_y"), None if ptrs.get("no_theta") else theta, slot("no_range", 6),
                                      slot("no_tables_d", 7), slot("no_tables_h", 8), slot("no_tables_w", 9), order, anchor, 0xF, None)


def test_apply_rejects_bad_arguments_without_a_gpu():
    _l, lib = _lib()
    for kw, word in (({"no_x": True}, b"`x`"), ({"x": _rows(_l, 0, ptr=None)}, b"`x`"), ({"no_y": True}, b"`y`"),
                     ({"y": _rows(_l, 1, ptr=None)}, b"`y`"), ({"no_theta": True}, b"theta"), ({"no_range": True}, b"range"),
                     ({"no_tables_d": True}, b"tables_d"), ({"no_tables_h": True}, b"tables_h"), ({"no_tables_w": True}, b"tables_w")):
        assert _apply(lib, _l, **kw) == INVALID, kw
        assert b"null" in _err(lib) and word in _err(lib), (kw, _err(lib))
    for bad in (dict(n=3), dict(c=2), dict(d=8), dict(h=2), dict(w=8)):
        assert _apply(lib, _l, y=_rows(_l, 1, **bad)) == INVALID and b"shape mismatch" in _err(lib)
    assert _apply(lib, _l, y=_rows(_l, 0)) == INVALID and b"must not be `x`" in _err(lib)
    assert _apply(lib, _l, order=-1) == INVALID and b"order" in _err(lib)
    assert _apply(lib, _l, anchor=2) == INVALID and b"anchor" in _err(lib)
    # what there is no kernel for
    assert _apply(lib, _l, order=4) == UNSUPPORTED and b"order = 4" in _err(lib)
    for axis in ("d", "h", "w"):
        big = {axis: 513}
        assert _apply(lib, _l, x=_rows(_l, 0, **big), y=_rows(_l, 1, **big)) == UNSUPPORTED and b"512" in _err(lib), axis
    assert _apply(lib, _l, x=_rows(_l, 0, dtype=_l.BF16)) == UNSUPPORTED and b"fp32" in _err(lib)
    assert _apply(lib, _l, x=_rows(_l, 0, c=5, ldc=8), y=_rows(_l, 1, c=5, ldc=8)) == UNSUPPORTED and b"channels" in _err(lib)
    assert _apply(lib, _l, y=_rows(_l, 1, ldc=8)) == UNSUPPORTED and b"4 lanes" in _err(lib)
    assert _apply(lib, _l, y=_rows(_l, 1, flags=0)) == UNSUPPORTED and b"pad lanes" in _err(lib)
    assert _apply(lib, _l, y=_rows(_l, 1, ptr=FAKE + STEP + 4)) == UNSUPPORTED and b"misaligned" in _err(lib)
    assert _apply(lib, _l, theta=FAKE + 5 * STEP + 4) == UNSUPPORTED and b"theta" in _err(lib)


def _grad(lib, _l, x=None, dys=None, n_branches=None, k=3, stride=2, weights=True, set_stride=0, order=2, anchor=0, lr=0.0,
          bounds=(0.7, 0.2), l2=0.0, state=True, theta=FAKE + 5 * STEP, **ptrs):
    x = _rows(_l, 0) if x is None else x
    dys = [_dy(_l, 2), _dy(_l, 3)] if dys is None else dys
    arr = (_l.InputNormBranch * max(len(dys), 1))()
    for r, d in enumerate(dys):
        arr[r] = _l.InputNormBranch(ctypes.pointer(d) if d is not None else None, (FAKE + (10 + r) * STEP) if weights else None,
                                    set_stride, k, stride)
    slot = lambda name, j: None if ptrs.get(name) else FAKE + j * STEP
    st = (lambda j: FAKE + j * STEP) if state else (lambda j: None)
    return lib.mmtta_bias_field_grad(None if ptrs.get("no_x") else ctypes.byref(x), None if ptrs.get("no_branches") else arr,
                                     len(dys) if n_branches is None else n_branches, None if ptrs.get("no_theta") else theta,
                                     slot("no_range", 6), slot("no_tables_d", 15), slot("no_tables_h", 16), slot("no_tables_w", 17),
                                     order, anchor, 0xF, slot("no_partial", 7), slot("no_grad", 8), st(12), st(13), st(14), lr,
                                     *bounds, l2, None)


def test_grad_rejects_null_pointers_without_a_gpu():
    _l, lib = _lib()
    for kw, word in (({"no_x": True}, b"`x`"), ({"x": _rows(_l, 0, ptr=None)}, b"`x`"), ({"no_branches": True}, b"branches"),
                     ({"no_theta": True}, b"theta"), ({"no_range": True}, b"range"), ({"no_partial": True}, b"partial"),
                     ({"no_grad": True}, b"`grad`"), ({"no_tables_d": True}, b"tables_d"), ({"no_tables_h": True}, b"tables_h"),
                     ({"no_tables_w": True}, b"tables_w"), ({"dys": [None]}, b"`dy`"), ({"dys": [_dy(_l, 2, ptr=None)]}, b"`dy`"),
                     ({"weights": False}, b"weight"), ({"state": False, "lr": 1e-2}, b"exp_avg")):
        assert _grad(lib, _l, **kw) == INVALID, kw
        assert b"null" in _err(lib) and word in _err(lib), (kw, _err(lib))


def test_grad_rejects_bad_branches_shapes_and_scalars_without_a_gpu():
    _l, lib = _lib()
    for count in (0, 3, -1):
        assert _grad(lib, _l, n_branches=count) == INVALID and b"n_branches" in _err(lib)
    for bad in (dict(n=3), dict(d=3), dict(h=2), dict(w=4)):          # dy against the outputs [2, 3, 5] of the input [4, 6, 10]
        assert _grad(lib, _l, dys=[_dy(_l, 2, **bad)]) == INVALID and b"shape mismatch" in _err(lib)
    assert _grad(lib, _l, dys=[_dy(_l, 2), _dy(_l, 3, c0=4)]) == INVALID and b"output channels" in _err(lib)
    assert _grad(lib, _l, dys=[_dy(_l, 2), _dy(_l, 3, dtype=_l.BF16)]) == INVALID and b"storage mismatch" in _err(lib)
    assert _grad(lib, _l, set_stride=-4) == INVALID and b"set stride" in _err(lib)
    for lr in (-1e-3, float("nan"), float("inf")):
        assert _grad(lib, _l, lr=lr) == INVALID and b"lr" in _err(lib)
    for l2 in (-1e-3, float("nan"), float("inf")):
        assert _grad(lib, _l, l2=l2) == INVALID and b"l2" in _err(lib)
    for bounds in ((0.0, 0.2), (0.7, -1.0), (0.7, float("nan"))):
        assert _grad(lib, _l, lr=1e-2, bounds=bounds) == INVALID and b"bounds" in _err(lib)
    assert _grad(lib, _l, order=-1) == INVALID and b"order" in _err(lib)
    assert _grad(lib, _l, anchor=-1) == INVALID and b"anchor" in _err(lib)


def test_grad_refuses_what_it_has_no_kernel_for_without_a_gpu():
    _l, lib = _lib()
    for k, stride in ((1, 2), (5, 2), (3, 1), (3, 3)):
        assert _grad(lib, _l, k=k, stride=stride) == UNSUPPORTED
        assert b"k = 3, stride 2" in _err(lib)
    for c0 in (6, 68, 2):
        assert _grad(lib, _l, dys=[_dy(_l, 2, c0=c0, ldc=(c0 + 3) // 4 * 4)]) == UNSUPPORTED and b"multiple of 4" in _err(lib)
    assert _grad(lib, _l, x=_rows(_l, 0, c=5, ldc=8)) == UNSUPPORTED and b"channels" in _err(lib)
    assert _grad(lib, _l, x=_rows(_l, 0, dtype=_l.BF16)) == UNSUPPORTED and b"fp32" in _err(lib)
    assert _grad(lib, _l, dys=[_dy(_l, 2, ptr=FAKE + 2 * STEP + 4)]) == UNSUPPORTED and b"misaligned" in _err(lib)
    assert _grad(lib, _l, theta=FAKE + 5 * STEP + 8) == UNSUPPORTED and b"theta" in _err(lib)
    assert _grad(lib, _l, order=4) == UNSUPPORTED and b"order = 4" in _err(lib)
    assert _grad(lib, _l, x=_rows(_l, 0, w=514), dys=[_dy(_l, 2, w=257)]) == UNSUPPORTED and b"512" in _err(lib)
    t = _dy(_l, 2)
    t.sc = 2
    assert _grad(lib, _l, dys=[t]) == UNSUPPORTED and b"channels-last" in _err(lib)


def test_ops_wrappers_check_their_tables_before_the_library():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.ops import MmttaError
    x = torch.zeros(1, 2, 2, 2, 4)
    with pytest.raises(MmttaError, match="theta must"):
        ops.bias_field_apply(x, x.clone(), torch.zeros(4), torch.zeros(8), (), 2)
    assert ops.BIAS_ROW == 20


# ----------------------------------------------------------------------------- plugin and config
def _cfg(*extra):
    from multimodal_tta_amd.config import compose
    return compose(overrides=["task=brats", "model=unet", "method=tta_biasfield", *extra])


DEFAULT_BLOCK = {"lr": 1e-2, "order": 2, "anchor": "min", "l2": 0.0, "bound": {"gain": 0.7, "field": 0.2}}


def test_biasfield_tta_is_registered_and_its_config_composes():
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin, list_plugins
    from multimodal_tta_amd.tta import EntropyMinimizationTTA
    assert "biasfield_tta" in list_plugins()
    assert compose(overrides=["method=tta_biasfield"])["method"]["name"] == "biasfield_tta"
    cfg = _cfg()
    assert cfg["method"]["name"] == "biasfield_tta" and cfg["method"]["kind"] == "tta"
    assert cfg["method"]["biasfield"] == DEFAULT_BLOCK
    plug = get_plugin("biasfield_tta")(cfg)
    assert isinstance(plug, EntropyMinimizationTTA) and type(plug).__name__ == "BiasFieldTTA"
    assert (plug.lr, plug.order, plug.anchor, plug.l2, plug.bounds) == (1e-2, 2, "min", 0.0, (0.7, 0.2))
    assert len(plug.terms) == 10 and [r[0] for r in plug.records] == ["losses"]
    plug = get_plugin("biasfield_tta")(_cfg("method.biasfield.lr=0", "method.biasfield.order=3", "method.biasfield.anchor=zero",
                                            "method.biasfield.l2=0.5", "method.biasfield.bound.gain=4",
                                            "method.biasfield.bound.field=1"))
    assert (plug.lr, plug.order, plug.anchor, plug.l2, plug.bounds) == (0.0, 3, "zero", 0.5, (4.0, 1.0))
    cfg = _cfg()
    del cfg["method"]["biasfield"]          # the block is optional: the defaults are the yaml's
    plug = get_plugin("biasfield_tta")(cfg)
    assert (plug.lr, plug.order, plug.anchor, plug.l2, plug.bounds) == (1e-2, 2, "min", 0.0, (0.7, 0.2))


def test_tta_biasfield_carries_every_key_of_tta_entmin():
    from multimodal_tta_amd.config import compose
    ent = compose(overrides=["task=brats", "model=unet", "method=tta_entmin"])["method"]
    bf = _cfg()["method"]
    assert set(bf) == set(ent) | {"biasfield"}
    for k in ent:
        if k != "name":
            assert bf[k] == ent[k], k
    text = open(os.path.join(ROOT, "configs", "method", "tta_biasfield.yaml")).read()
    assert "nobody has measured a Dice" in text


@pytest.mark.parametrize("key,value", [
    ("lr", -1e-3), ("lr", float("nan")), ("lr", float("inf")), ("lr", True), ("lr", "1e-2"),
    ("order", 4), ("order", -1), ("order", 1.0), ("order", True), ("order", "2"),
    ("anchor", "max"), ("anchor", 0), ("anchor", "MIN"), ("anchor", True),
    ("l2", -1e-3), ("l2", float("nan")), ("l2", float("inf")), ("l2", False), ("l2", "0"),
    ("bound.gain", 0.0), ("bound.gain", 4.5), ("bound.gain", float("nan")), ("bound.gain", True),
    ("bound.field", 0.0), ("bound.field", 1.5), ("bound.field", -0.2), ("bound.field", "0.2"),
    ("bound", 0.7), ("gamma", False), ("bound.log_scale", 0.7), ("bound.shift", 1.0)])
def test_biasfield_plugin_rejects_bad_hyper_parameters(key, value):
    """Out of range, of the wrong type or unknown: a ValueError that names the key - with ``lr: 0`` as well."""
    from multimodal_tta_amd.registry import get_plugin
    for lr in (None, 0.0):
        cfg = _cfg()
        node, parts = cfg["method"]["biasfield"], key.split(".")
        if lr is not None and key != "lr":
            node["lr"] = lr
        for p in parts[:-1]:
            node = node[p]
        node[parts[-1]] = value
        with pytest.raises(ValueError, match=re.escape(f"method.biasfield.{key} ")):
            get_plugin("biasfield_tta")(cfg)


def test_moddrop_and_the_deep_fusion_model_are_refused():
    from multimodal_tta_amd.models import MultimodalUNetDeepFusion
    from multimodal_tta_amd.registry import get_plugin
    with pytest.raises(NotImplementedError, match="method.moddrop.enabled"):
        get_plugin("biasfield_tta")(_cfg("method.moddrop.enabled=true", "method.moddrop.p=0.25"))
    dcfg = dict(name="unet_multimodal_deepfusion", num_modalities=4, num_classes=3, spatial_dims=3,
                channels=[4, 8, 16, 32, 64], strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)
    with pytest.raises(NotImplementedError, match="biasfield_tta.*MultimodalUNetDeepFusion"):
        get_plugin("biasfield_tta")(_cfg()).setup(MultimodalUNetDeepFusion(dcfg), "cuda")          # (refused before any device call)


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("anchor", ["min", "zero"])
def test_reference_gradient_is_the_analytic_one(anchor):
    """d x' / d theta_k = (x - a) exp(F) phi_k: the restatement's autograd against the closed form, in float64."""
    g = torch.Generator().manual_seed(5)
    order, ext = 3, (3, 4, 5)
    x = torch.randn(2, 3, *ext, generator=g, dtype=torch.float64)
    theta = 0.2 * torch.randn(2, 3, 20, generator=g, dtype=torch.float64)
    tables = ref.legendre_tables(ext)
    w = torch.randn(x.shape, generator=g, dtype=torch.float64)
    th = theta.clone().requires_grad_(True)
    (ref.apply_field(x, th, tables, order, anchor) * w).sum().backward()
    a = ref.anchors(x, anchor).reshape(2, 3, 1, 1, 1)
    want = torch.einsum("bcdhw,kdhw->bck", w * (x - a) * torch.exp(ref.log_field(theta, tables, order)), ref.basis(tables, order, x.dtype))
    assert torch.allclose(th.grad, want, rtol=1e-12, atol=1e-12)
    assert torch.equal(ref.apply_field(x, torch.zeros_like(theta), tables, order, anchor), (x - a) + a)
    if anchor == "min":
        xp = ref.apply_field(x, theta, tables, order, anchor)
        at_min = x == a
        assert at_min.sum() == 6 and torch.equal(xp[at_min], x[at_min]), "the anchor is a fixed point of the map"
