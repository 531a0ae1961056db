"""SAR adaptation (``sar_tta``, ``method=tta_sar``): the host-side half, no GPU needed.

The config composes and the plugin reads its two hyper-parameters; the two new entry points (filtered entropy, SAM ascent)
refuse every bad argument with MMTTA_ERR_INVALID and a message before anything reaches the device."""
import ctypes

import pytest

INVALID = -1
FAKE = 4096          # a 16-byte aligned address that is never dereferenced: the checks fail first


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from multimodal_tta_amd import _lib
    return _lib, _lib.load()


def test_tta_sar_config_composes_and_the_plugin_reads_it():
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin

    cfg = compose(overrides=["task=brats", "dataset=brats", "model=unet", "method=tta_sar"])
    assert cfg["method"]["name"] == "sar_tta" and cfg["method"]["kind"] == "tta"
    assert cfg["method"]["sar"]["e_margin"] == 0.4 and cfg["method"]["sar"]["rho"] == 0.05
    plug = get_plugin("sar_tta")(cfg)
    assert plug.e_margin == 0.4 and plug.rho == 0.05
    assert abs(plug.margin(3) - 0.4 * 0.6931471805599453) < 1e-12          # sigmoid head: K = 2
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_sar", "method.sar.e_margin=0.25", "method.sar.rho=0.1"])
    plug = get_plugin("sar_tta")(cfg)
    assert plug.e_margin == 0.25 and plug.rho == 0.1
    plug.softmax = True
    assert abs(plug.margin(4) - 0.25 * 1.3862943611198906) < 1e-12         # softmax head: K = R


def test_tta_sar_carries_every_key_of_tta_entmin():
    from multimodal_tta_amd.config import compose
    ent = compose(overrides=["task=brats", "model=unet", "method=tta_entmin"])["method"]
    sar = compose(overrides=["task=brats", "model=unet", "method=tta_sar"])["method"]
    assert set(sar) == set(ent) | {"sar"}
    for k in ent:
        if k != "name":
            assert sar[k] == ent[k], k


@pytest.mark.parametrize("key,value", [("e_margin", 0.0), ("e_margin", -1.0), ("e_margin", float("nan")),
                                       ("rho", -0.1), ("rho", float("inf"))])
def test_sar_plugin_rejects_bad_hyper_parameters(key, value):
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_sar"])
    cfg["method"]["sar"][key] = value
    with pytest.raises(ValueError, match=key):
        get_plugin("sar_tta")(cfg)


def test_sar_is_a_registered_plugin():
    import multimodal_tta_amd  # noqa: F401
    from multimodal_tta_amd.registry import list_plugins
    assert "sar_tta" in list_plugins()
    assert "entmin_tta" in list_plugins()


def test_sar_setup_refuses_an_empty_parameter_selection():
    import torch
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_sar", "method.params=no_such_parameter"])
    model = torch.nn.Conv3d(1, 1, 1)
    with pytest.raises(ValueError, match="no trainable parameter"):
        get_plugin("sar_tta")(cfg).setup(model, "cpu")


def _tensor(_l, n=2, c=3, d=4, h=4, w=4, ptr=FAKE):
    ldc = 4
    return _l.Tensor(ptr, n, c, d, h, w, d * h * w * ldc, 1, h * w * ldc, w * ldc, ldc, _l.F32, _l.TENSOR_OWNS_PAD)


def _filtered(lib, _l, z=None, g=None, margin=0.3, keep_in=None, keep_out=FAKE, partial=FAKE, loss=FAKE, kept=FAKE):
    z = _tensor(_l) if z is None else z
    g = _tensor(_l) if g is None else g
    return lib.mmtta_entropy_filtered_items(ctypes.byref(z), 0, margin, keep_in, keep_out, ctypes.byref(g), partial, loss,
                                            kept, None)


def test_filtered_entropy_rejects_bad_arguments_without_a_gpu():
    _l, lib = _lib()
    for m in (float("nan"), float("inf"), float("-inf"), 0.0, -0.5):
        assert _filtered(lib, _l, margin=m) == INVALID
        assert b"margin" in lib.mmtta_last_error()
    assert _filtered(lib, _l, keep_out=None) == INVALID
    assert b"null mask output" in lib.mmtta_last_error()
    for kw in ({"partial": None}, {"loss": None}, {"kept": None}):
        assert _filtered(lib, _l, **kw) == INVALID
        assert b"null argument" in lib.mmtta_last_error()
    for bad in (_tensor(_l, n=3), _tensor(_l, c=2), _tensor(_l, d=5), _tensor(_l, h=3), _tensor(_l, w=2)):
        assert _filtered(lib, _l, g=bad) == INVALID
        assert b"shape mismatch" in lib.mmtta_last_error()
    assert lib.mmtta_entropy_filtered_partials(None) == -1
    assert lib.mmtta_entropy_filtered_partials(ctypes.byref(_tensor(_l, n=3, d=4, h=4, w=4))) == 2 * 3 * 1


def _ascent(lib, p=FAKE, g=FAKE, saved=FAKE, saved_stride=64, partial=FAKE, n=64, sets=2, replicas=3, stride=128, rho=0.05):
    return lib.mmtta_sam_ascent_sets(p, g, saved, saved_stride, partial, n, sets, replicas, stride, rho, None)


def test_sam_ascent_rejects_bad_arguments_without_a_gpu():
    _l, lib = _lib()
    for r in (float("nan"), float("inf"), -1e-3):
        assert _ascent(lib, rho=r) == INVALID
        assert b"rho" in lib.mmtta_last_error()
    for kw in ({"p": None}, {"g": None}, {"saved": None}, {"partial": None}):
        assert _ascent(lib, **kw) == INVALID
        assert b"null argument" in lib.mmtta_last_error()
    for kw in ({"n": 6}, {"stride": 130}, {"n": -4}):
        assert _ascent(lib, **kw) == INVALID
        assert b"multiples of 4" in lib.mmtta_last_error()
    for kw in ({"n": 256, "saved_stride": 256}, {"sets": 4}, {"sets": 0}):
        assert _ascent(lib, **kw) == INVALID
        assert b"do not fit" in lib.mmtta_last_error()
    for kw in ({"saved_stride": 60}, {"saved_stride": 66}):
        assert _ascent(lib, **kw) == INVALID
        assert b"saved_stride" in lib.mmtta_last_error()
    assert _ascent(lib, p=FAKE + 4) == INVALID
    assert b"16-byte" in lib.mmtta_last_error()
    assert lib.mmtta_sam_ascent_partials(64, 2) == 2
    assert lib.mmtta_sam_ascent_partials(-4, 1) == -1
