"""Host half of the input-normaliser adaptation (``innorm_tta``, ``mmtta_input_norm_apply`` / ``mmtta_input_norm_grad``): the
plugin's registration, config and refusals, the entry points' argument checks (none touches a device) and the torch
restatement's analytic derivatives against autograd.  The GPU half is ``test_hip_innorm.py``."""
import ctypes
import os
import re

import pytest
import torch

from innorm_reference import apply_map, channel_range, derivatives

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE, STEP = 0x7F0000000000, 1 << 32          # device-looking addresses that are never dereferenced
INVALID, UNSUPPORTED = -1, -2


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


# ----------------------------------------------------------------------------- the entry points
def test_the_input_norm_symbols_are_declared_exported_and_typed():
    _l, lib = _lib()
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmtta.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mmtta_input_norm_apply\s*\(", code) and re.search(r"\bint\s+mmtta_input_norm_grad\s*\(", code)
    assert re.search(r"\bint64_t\s+mmtta_input_norm_grad_partials\s*\(", code)
    names = {"mmtta_input_norm_apply", "mmtta_input_norm_grad", "mmtta_input_norm_grad_partials"}
    assert names <= set(_l.exported_names())
    for name in names:
        assert getattr(ctypes.CDLL(_l.LIB_PATH), name) is not None
    assert len(lib.mmtta_input_norm_apply.argtypes) == 7 and len(lib.mmtta_input_norm_grad.argtypes) == 17
    assert lib.mmtta_input_norm_grad_partials.restype is ctypes.c_int64
    assert lib.mmtta_abi_version() == 2
    assert ctypes.sizeof(_l.InputNormBranch) == 32


def test_grad_partials_answers_on_the_host():
    """12 fp64 sums per tile of 4 x 8 x 64 input voxels and item."""
    _l, lib = _lib()
    count = lambda **kw: lib.mmtta_input_norm_grad_partials(ctypes.byref(_rows(_l, **kw)))
    assert count(n=1, d=2, h=2, w=2) == 12
    assert count(n=2, d=4, h=8, w=64) == 2 * 12
    assert count(n=3, d=5, h=9, w=65) == 3 * (2 * 2 * 2) * 12
    assert count(n=1, d=128, h=128, w=128) == 32 * 16 * 2 * 12
    assert lib.mmtta_input_norm_grad_partials(None) == -1
    assert count(n=0) == -1 and b"partials" in _err(lib)


def _apply(lib, _l, x=None, y=None, **ptrs):
    x = _rows(_l, 0) if x is None else x
    y = _rows(_l, 1) if y is None else y
    ref = lambda t, name: None if ptrs.get(name) else ctypes.byref(t)
    slot = lambda name, k: None if ptrs.get(name) else FAKE + k * STEP
    return lib.mmtta_input_norm_apply(ref(x, "no_x"), ref(y, "no_y"), slot("no_theta", 5), slot("no_range", 6), 0xF, 0, None)


def test_apply_rejects_bad_arguments_without_a_gpu():
    _l, lib = _lib()
    for kw, word in (({"no_x": True}, b"`x`"), ({"x": _rows(_l, 0, ptr=None)}, b"`x`"), ({"no_y": True}, b"`y`"),
                     ({"y": _rows(_l, 1, ptr=None)}, b"`y`"), ({"no_theta": True}, b"theta"), ({"no_range": True}, b"range")):
        assert _apply(lib, _l, **kw) == INVALID, kw
        assert b"null" in _err(lib) and word in _err(lib), (kw, _err(lib))
    for bad in (dict(n=3), dict(c=2), dict(d=8), dict(h=2), dict(w=8)):
        assert _apply(lib, _l, y=_rows(_l, 1, **bad)) == INVALID and b"shape mismatch" in _err(lib)
    assert _apply(lib, _l, y=_rows(_l, 0)) == INVALID and b"must not be `x`" in _err(lib)
    # storages and layouts without a kernel
    assert _apply(lib, _l, x=_rows(_l, 0, dtype=_l.BF16)) == UNSUPPORTED and b"fp32" in _err(lib)
    assert _apply(lib, _l, x=_rows(_l, 0, c=5, ldc=8), y=_rows(_l, 1, c=5, ldc=8)) == UNSUPPORTED and b"channels" in _err(lib)
    assert _apply(lib, _l, y=_rows(_l, 1, ldc=8)) == UNSUPPORTED and b"4 lanes" in _err(lib)
    assert _apply(lib, _l, y=_rows(_l, 1, flags=0)) == UNSUPPORTED and b"pad lanes" in _err(lib)
    assert _apply(lib, _l, y=_rows(_l, 1, ptr=FAKE + STEP + 4)) == UNSUPPORTED and b"misaligned" in _err(lib)


def _grad(lib, _l, x=None, dys=None, n_branches=None, k=3, stride=2, weights=True, set_stride=0, lr=0.0, bounds=(0.7, 1.0, 0.7),
          state=True, **ptrs):
    x = _rows(_l, 0) if x is None else x
    dys = [_dy(_l, 2), _dy(_l, 3)] if dys is None else dys
    arr = (_l.InputNormBranch * max(len(dys), 1))()
    for r, d in enumerate(dys):
        arr[r] = _l.InputNormBranch(ctypes.pointer(d) if d is not None else None, (FAKE + (10 + r) * STEP) if weights else None,
                                    set_stride, k, stride)
    slot = lambda name, j: None if ptrs.get(name) else FAKE + j * STEP
    st = (lambda j: FAKE + j * STEP) if state else (lambda j: None)
    return lib.mmtta_input_norm_grad(None if ptrs.get("no_x") else ctypes.byref(x), None if ptrs.get("no_branches") else arr,
                                     len(dys) if n_branches is None else n_branches, slot("no_theta", 5), slot("no_range", 6), 0xF, 0,
                                     slot("no_partial", 7), slot("no_grad", 8), st(12), st(13), st(14), lr, *bounds, None)


def test_grad_rejects_null_pointers_without_a_gpu():
    _l, lib = _lib()
    for kw, word in (({"no_x": True}, b"`x`"), ({"x": _rows(_l, 0, ptr=None)}, b"`x`"), ({"no_branches": True}, b"branches"),
                     ({"no_theta": True}, b"theta"), ({"no_range": True}, b"range"), ({"no_partial": True}, b"partial"),
                     ({"no_grad": True}, b"`grad`"), ({"dys": [None]}, b"`dy`"), ({"dys": [_dy(_l, 2, ptr=None)]}, b"`dy`"),
                     ({"weights": False}, b"weight"), ({"state": False, "lr": 1e-2}, b"exp_avg")):
        assert _grad(lib, _l, **kw) == INVALID, kw
        assert b"null" in _err(lib) and word in _err(lib), (kw, _err(lib))


def test_grad_rejects_bad_branches_shapes_and_scalars_without_a_gpu():
    _l, lib = _lib()
    for count in (0, 3, -1):
        assert _grad(lib, _l, n_branches=count) == INVALID and b"n_branches" in _err(lib)
    # dy against the output extents of the input [4, 6, 10] -> [2, 3, 5]
    for bad in (dict(n=3), dict(d=3), dict(h=2), dict(w=4)):
        assert _grad(lib, _l, dys=[_dy(_l, 2, **bad)]) == INVALID and b"shape mismatch" in _err(lib)
    assert _grad(lib, _l, dys=[_dy(_l, 2), _dy(_l, 3, c0=4)]) == INVALID and b"output channels" in _err(lib)
    assert _grad(lib, _l, dys=[_dy(_l, 2), _dy(_l, 3, dtype=_l.BF16)]) == INVALID and b"storage mismatch" in _err(lib)
    assert _grad(lib, _l, set_stride=-4) == INVALID and b"set stride" in _err(lib)
    for lr in (-1e-3, float("nan"), float("inf")):
        assert _grad(lib, _l, lr=lr) == INVALID and b"lr" in _err(lib)
    for bounds in ((0.0, 1.0, 0.7), (0.7, -1.0, 0.7), (0.7, 1.0, float("nan"))):
        assert _grad(lib, _l, lr=1e-2, bounds=bounds) == INVALID and b"bounds" in _err(lib)


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
    t = _dy(_l, 2)
    t.sc = 2
    assert _grad(lib, _l, dys=[t]) == UNSUPPORTED and b"channels-last" in _err(lib)


def test_ops_wrappers_check_their_tables_before_the_library():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.ops import MmttaError
    x = torch.zeros(1, 2, 2, 2, 4)
    with pytest.raises(MmttaError, match="theta must"):
        ops.input_norm_apply(x, x.clone(), torch.zeros(4), torch.zeros(8))
    with pytest.raises(MmttaError, match="modality mask"):
        ops._keep_mask([True, False], 4)
    assert ops._keep_mask(None, 3) == 7 and ops._keep_mask([True, False, True, True], 4) == 0b1101


# ----------------------------------------------------------------------------- plugin and config
def _cfg(*extra):
    from multimodal_tta_amd.config import compose
    return compose(overrides=["task=brats", "model=unet", "method=tta_innorm", *extra])


def test_innorm_tta_is_registered_and_its_config_composes():
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin, list_plugins
    from multimodal_tta_amd.tta import EntropyMinimizationTTA
    assert "innorm_tta" in list_plugins()
    assert compose(overrides=["method=tta_innorm"])["method"]["name"] == "innorm_tta"
    cfg = _cfg()
    assert cfg["method"]["name"] == "innorm_tta" and cfg["method"]["kind"] == "tta"
    assert cfg["method"]["innorm"] == {"lr": 1e-2, "gamma": False, "bound": {"log_scale": 0.7, "shift": 1.0, "log_gamma": 0.7}}
    plug = get_plugin("innorm_tta")(cfg)
    assert isinstance(plug, EntropyMinimizationTTA) and type(plug).__name__ == "InputNormTTA"
    assert (plug.lr, plug.gamma, plug.bounds) == (1e-2, False, (0.7, 1.0, 0.7))
    assert [r[0] for r in plug.records] == ["losses"]
    plug = get_plugin("innorm_tta")(_cfg("method.innorm.lr=0", "method.innorm.gamma=true", "method.innorm.bound.log_scale=4",
                                         "method.innorm.bound.shift=16", "method.innorm.bound.log_gamma=2"))
    assert (plug.lr, plug.gamma, plug.bounds) == (0.0, True, (4.0, 16.0, 2.0))
    cfg = _cfg()
    del cfg["method"]["innorm"]          # the block is optional: the defaults are the yaml's
    plug = get_plugin("innorm_tta")(cfg)
    assert (plug.lr, plug.gamma, plug.bounds) == (1e-2, False, (0.7, 1.0, 0.7))


def test_tta_innorm_carries_every_key_of_tta_entmin():
    from multimodal_tta_amd.config import compose
    ent = compose(overrides=["task=brats", "model=unet", "method=tta_entmin"])["method"]
    inn = _cfg()["method"]
    assert set(inn) == set(ent) | {"innorm"}
    for k in ent:
        if k != "name":
            assert inn[k] == ent[k], k
    text = open(os.path.join(ROOT, "configs", "method", "tta_innorm.yaml")).read()
    assert "nobody has measured a Dice" in text


@pytest.mark.parametrize("key,value", [
    ("lr", -1e-3), ("lr", float("nan")), ("lr", float("inf")), ("lr", True), ("lr", "1e-2"),
    ("gamma", 1), ("gamma", "true"), ("gamma", 0.5),
    ("bound.log_scale", 0.0), ("bound.log_scale", 4.5), ("bound.log_scale", float("nan")), ("bound.log_scale", True),
    ("bound.shift", 0.0), ("bound.shift", 16.5), ("bound.shift", -1.0), ("bound.shift", "1"),
    ("bound.log_gamma", 0.0), ("bound.log_gamma", 2.5), ("bound.log_gamma", float("inf")), ("bound.log_gamma", False)])
def test_innorm_plugin_rejects_bad_hyper_parameters(key, value):
    from multimodal_tta_amd.registry import get_plugin
    cfg = _cfg()
    node, parts = cfg["method"]["innorm"], key.split(".")
    for p in parts[:-1]:
        node = node[p]
    node[parts[-1]] = value
    with pytest.raises(ValueError, match=f"method.innorm.{key} "):
        get_plugin("innorm_tta")(cfg)


def test_moddrop_and_the_deep_fusion_model_are_refused():
    from multimodal_tta_amd.models import MultimodalUNetDeepFusion
    from multimodal_tta_amd.registry import get_plugin
    with pytest.raises(NotImplementedError, match="method.moddrop.enabled"):
        get_plugin("innorm_tta")(_cfg("method.moddrop.enabled=true", "method.moddrop.p=0.25"))
    dcfg = dict(name="unet_multimodal_deepfusion", num_modalities=4, num_classes=3, spatial_dims=3,
                channels=[4, 8, 16, 32, 64], strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)
    with pytest.raises(NotImplementedError, match="MultimodalUNetDeepFusion"):
        get_plugin("innorm_tta")(_cfg()).setup(MultimodalUNetDeepFusion(dcfg), "cuda")          # (refused before any device call)


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("gamma", [False, True], ids=["affine", "gamma"])
def test_analytic_derivatives_agree_with_autograd_in_float64(gamma):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 3, 4, 5, generator=g, dtype=torch.float64)
    x[1, 2] = 0.25                                   # a constant channel: hi == lo, u = x, no gamma gradient
    lo, hi = channel_range(x)
    theta = 0.3 * torch.randn(2, 3, 3, generator=g, dtype=torch.float64)
    if not gamma:
        theta[..., 2] = 0
    w = torch.randn(x.shape, generator=g, dtype=torch.float64)
    th = theta.clone().requires_grad_(True)
    (apply_map(x, th, lo, hi, gamma) * w).sum().backward()
    d = derivatives(x, theta, lo, hi, gamma)
    want = torch.stack([(w * dk).flatten(2).sum(-1) for dk in d], -1)
    assert torch.allclose(th.grad, want, rtol=1e-12, atol=1e-12), (th.grad - want).abs().max()
    assert (want[1, 2, 2] == 0) and (gamma or (want[..., 2] == 0).all())
    # the voxel at the channel's minimum has t = 0: the value is lo and the gamma derivative 0, not nan
    assert torch.isfinite(th.grad).all() and torch.isfinite(apply_map(x, theta, lo, hi, gamma)).all()
    if not gamma:
        assert torch.equal(apply_map(x, torch.zeros_like(theta), lo, hi, False), x)
