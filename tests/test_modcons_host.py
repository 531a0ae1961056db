"""Host half of the modality-consistency adaptation (``modcons_tta``, ``mmtta_modality_views`` / ``mmtta_modcons_partials`` /
``mmtta_modcons_loss_items``): the plugin's registration, config, views and refusals, the entry points' argument checks (none
touches a device) and the restatement's closed-form gradients against autograd.  The GPU half is ``test_hip_modcons.py``."""
import ctypes
import os
import re

import pytest
import torch

from modcons_reference import closed_form_grad, loss_reference, masked_views, modcons_terms

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


def _rows(_l, slot=0, n=4, c=3, d=4, h=6, w=10, ptr=True, dtype=None, ldc=4, flags=None):
    return _l.Tensor((FAKE + slot * STEP) if ptr is True else ptr, n, c, d, h, w, d * h * w * ldc, 1, h * w * ldc, w * ldc, ldc,
                     _l.F32 if dtype is None else dtype, _l.TENSOR_OWNS_PAD if flags is None else flags)


# ----------------------------------------------------------------------------- the entry points
def test_the_modcons_symbols_are_declared_exported_and_typed():
    _l, lib = _lib()
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmtta.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mmtta_modality_views\s*\(", code) and re.search(r"\bint\s+mmtta_modcons_loss_items\s*\(", code)
    assert re.search(r"\bint64_t\s+mmtta_modcons_partials\s*\(", code)
    names = {"mmtta_modality_views", "mmtta_modcons_partials", "mmtta_modcons_loss_items"}
    assert names <= set(_l.exported_names())
    for name in names:
        assert getattr(ctypes.CDLL(_l.LIB_PATH), name) is not None
    assert len(lib.mmtta_modality_views.argtypes) == 5 and len(lib.mmtta_modcons_loss_items.argtypes) == 14
    assert lib.mmtta_modcons_partials.restype is ctypes.c_int64
    assert lib.mmtta_abi_version() == 2
    from multimodal_tta_amd import ops
    assert callable(ops.modality_views) and callable(ops.modcons_partials) and callable(ops.modcons_loss_items)
    from multimodal_tta_amd.build import SOURCES
    assert "modcons.hip" in SOURCES


def test_modcons_partials_answers_on_the_host():
    """(1 + 2 (V - 1)) rows x the workgroups of ONE item (256 (voxel, region) pairs each, at most 2048) x volumes."""
    _l, lib = _lib()
    count = lambda views, **kw: lib.mmtta_modcons_partials(ctypes.byref(_rows(_l, **kw)), views)
    assert count(2, n=2, c=3, d=5, h=6, w=7) == 3 * 3 * 1                    # 630 pairs: 3 workgroups
    assert count(5, n=15, c=3, d=5, h=6, w=7) == 9 * 3 * 3
    assert count(8, n=8, c=1, d=1, h=1, w=1) == 15
    assert count(3, n=6, c=4, d=128, h=128, w=128) == 5 * 2048 * 2             # the cap
    assert count(2, n=2, c=3, d=81, h=81, w=81) == 3 * 2048
    assert lib.mmtta_modcons_partials(None, 2) == -1
    for views, n in ((1, 4), (9, 9), (0, 4), (3, 4), (2, 1)):
        assert count(views, n=n) == -1, (views, n)
    assert count(2, n=2, d=0) == -1


def _views(lib, _l, x=None, y=None, views=2, masks=None, no_masks=False):
    x = _rows(_l, 0, n=2) if x is None else x
    y = _rows(_l, 1, n=2 * views) if y is None else y
    masks = [0b111, 0b011, 0b101, 0b110, 0b001, 0b010, 0b100, 0b111][:max(views, 1)] if masks is None else masks
    arr = (ctypes.c_uint32 * max(len(masks), 1))(*masks)
    ref = lambda t: None if t == "null" else ctypes.byref(t)
    return lib.mmtta_modality_views(ref(x), ref(y), views, None if no_masks else arr, None)


def test_modality_views_rejects_bad_arguments_without_a_gpu():
    _l, lib = _lib()
    for kw in ({"x": "null"}, {"y": "null"}, {"no_masks": True}, {"x": _rows(_l, 0, n=2, ptr=None)},
               {"y": _rows(_l, 1, ptr=None)}):
        assert _views(lib, _l, **kw) == INVALID, kw
        assert b"null argument" in _err(lib)
    for views in (0, 9, -1):
        assert _views(lib, _l, views=views, y=_rows(_l, 1, n=4)) == INVALID and b"views =" in _err(lib)
    for bad in (dict(n=5), dict(c=2), dict(d=8), dict(h=2), dict(w=8), dict(dtype=_l.BF16)):
        assert _views(lib, _l, y=_rows(_l, 1, **bad)) == INVALID and b"shape mismatch" in _err(lib), bad
    assert _views(lib, _l, masks=[0b111, 0b1000]) == INVALID and b"outside the 3 channels" in _err(lib)
    assert _views(lib, _l, y=_rows(_l, 0, n=4)) == INVALID and b"overlaps" in _err(lib)
    t = _rows(_l, 1)
    t.sc = 2
    assert _views(lib, _l, y=t) == UNSUPPORTED and b"channels-last" in _err(lib)
    assert _views(lib, _l, x=_rows(_l, 0, n=2, c=33, ldc=36), y=_rows(_l, 1, c=33, ldc=36)) == UNSUPPORTED and b"channels" in _err(lib)
    big = dict(d=1024, h=1024, w=512)
    assert _views(lib, _l, x=_rows(_l, 0, n=2, **big), y=_rows(_l, 4, n=4, **big)) == UNSUPPORTED and b"2^31" in _err(lib)


def _loss(lib, _l, z=None, g=None, softmax=0, views=2, weight=1.0, entropy_weight=1.0, detach=1, **ptrs):
    z = _rows(_l, 0) if z is None else z
    g = _rows(_l, 1) if g is None else g
    ref = lambda t: None if t == "null" else ctypes.byref(t)
    slot = lambda name, k: None if ptrs.get(name) else FAKE + k * STEP
    return lib.mmtta_modcons_loss_items(ref(z), softmax, views, weight, entropy_weight, detach, ref(g), slot("no_partial", 4),
                                        slot("no_loss", 5), slot("no_entropy", 6), slot("no_consistency", 7),
                                        slot("no_view_kl", 8), slot("no_disagree", 9), None)


def test_modcons_loss_rejects_bad_arguments_without_a_gpu():
    _l, lib = _lib()
    for kw in ({"z": "null"}, {"g": "null"}, {"z": _rows(_l, 0, ptr=None)}, {"g": _rows(_l, 1, ptr=None)}, {"no_partial": True},
               {"no_loss": True}, {"no_entropy": True}, {"no_consistency": True}, {"no_view_kl": True}, {"no_disagree": True}):
        assert _loss(lib, _l, **kw) == INVALID, kw
        assert b"null argument" in _err(lib)
    for views in (1, 9, 0, -2):
        assert _loss(lib, _l, views=views) == INVALID and b"views =" in _err(lib)
    assert _loss(lib, _l, views=3) == INVALID and b"no multiple of views" in _err(lib)
    assert _loss(lib, _l, views=8) == INVALID and b"no multiple of views" in _err(lib)
    for bad in (dict(n=6), dict(c=2), dict(d=8), dict(h=2), dict(w=8)):
        assert _loss(lib, _l, g=_rows(_l, 1, **bad)) == INVALID and b"shape mismatch" in _err(lib), bad
    for kw in (dict(weight=-1.0), dict(weight=float("nan")), dict(entropy_weight=float("inf")), dict(entropy_weight=-0.5)):
        assert _loss(lib, _l, **kw) == INVALID and b"weight" in _err(lib), kw
    # dlogits on top of the logits, equal or shifted by one voxel row
    assert _loss(lib, _l, g=_rows(_l, 0)) == INVALID and b"overlaps" in _err(lib)
    assert _loss(lib, _l, g=_rows(_l, 0, ptr=FAKE + 16)) == INVALID and b"overlaps" in _err(lib)


def test_modcons_loss_refuses_what_it_has_no_kernel_for_without_a_gpu():
    _l, lib = _lib()
    assert _loss(lib, _l, z=_rows(_l, 0, dtype=_l.BF16)) == UNSUPPORTED and b"fp32-stored" in _err(lib)
    t = _rows(_l, 0)
    t.sc = 2
    assert _loss(lib, _l, z=t) == UNSUPPORTED and b"channels-last" in _err(lib)
    # a bf16 gradient off the fast path: rows of 8 lanes, rows that do not own their pad, the softmax head
    bf = dict(dtype=_l.BF16)
    assert _loss(lib, _l, z=_rows(_l, 0, c=5, ldc=8), g=_rows(_l, 1, c=5, ldc=8, **bf)) == UNSUPPORTED and b"bf16" in _err(lib)
    assert _loss(lib, _l, g=_rows(_l, 1, flags=0, **bf)) == UNSUPPORTED and b"bf16" in _err(lib)
    assert _loss(lib, _l, softmax=1, g=_rows(_l, 1, **bf)) == UNSUPPORTED and b"fp32-stored" in _err(lib)
    assert _loss(lib, _l, softmax=1, z=_rows(_l, 0, c=17, ldc=20), g=_rows(_l, 1, c=17, ldc=20)) == UNSUPPORTED
    assert b"classes" in _err(lib)
    big = dict(d=1024, h=1024, w=512)
    assert _loss(lib, _l, z=_rows(_l, 0, **big), g=_rows(_l, 2, **big)) == UNSUPPORTED and b"2^31" in _err(lib)
    # more volumes than gridDim.y carries (one voxel each)
    many = dict(n=2 * 65536, d=1, h=1, w=1)
    assert _loss(lib, _l, z=_rows(_l, 0, **many), g=_rows(_l, 1, **many)) == UNSUPPORTED and b"65535 volumes" in _err(lib)


def test_ops_wrappers_check_their_buffers_before_the_library():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.ops import MmttaError
    x = torch.zeros(1, 2, 2, 2, 4)
    with pytest.raises(MmttaError, match="keep_masks"):
        ops.modality_views(x, x.clone(), [1 << 32])
    with pytest.raises(MmttaError, match="CUDA"):
        ops.modality_views(x, x.clone(), [3, 1])


# ----------------------------------------------------------------------------- plugin and config
def _cfg(*extra):
    from multimodal_tta_amd.config import compose
    return compose(overrides=["task=brats", "model=unet", "method=tta_modcons", *extra])


def _plug(channels=4, **block):
    from multimodal_tta_amd.registry import get_plugin
    cfg = _cfg()
    missing = block.pop("missing", [])
    cfg["method"]["missing_modalities"] = missing
    for k, v in block.items():
        cfg["method"]["modcons"][k] = v
    cfg["model"]["in_channels"] = channels
    return get_plugin("modcons_tta")(cfg)


def test_modcons_tta_is_registered_and_its_config_composes():
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin, list_plugins
    from multimodal_tta_amd.tta import EntropyMinimizationTTA
    assert "modcons_tta" in list_plugins()
    assert compose(overrides=["method=tta_modcons"])["method"]["name"] == "modcons_tta"
    cfg = _cfg()
    assert cfg["method"]["name"] == "modcons_tta" and cfg["method"]["kind"] == "tta"
    assert cfg["method"]["modcons"] == {"subsets": "leave_one_out", "weight": 1.0, "entropy_weight": 1.0, "detach": True}
    plug = _plug()
    assert isinstance(plug, EntropyMinimizationTTA) and type(plug).__name__ == "ModalityConsistencyTTA"
    assert (plug.subsets, plug.weight, plug.entropy_weight, plug.detach) == ("leave_one_out", 1.0, 1.0, True)
    assert [r[0] for r in plug.records] == ["losses", "entropy", "consistency"]
    assert plug.views == 5 and plug.keep_masks == [0b1111, 0b1110, 0b1101, 0b1011, 0b0111] and plug.fused_update is False
    cfg = _cfg()
    del cfg["method"]["modcons"]          # the block is optional: the defaults are the yaml's
    plug = get_plugin("modcons_tta")(cfg)
    assert (plug.subsets, plug.weight, plug.entropy_weight, plug.detach) == ("leave_one_out", 1.0, 1.0, True)
    plug = get_plugin("modcons_tta")(_cfg("method.modcons.subsets=single", "method.modcons.weight=0.5",
                                          "method.modcons.entropy_weight=0", "method.modcons.detach=false"))
    assert (plug.subsets, plug.weight, plug.entropy_weight, plug.detach) == ("single", 0.5, 0.0, False)


def test_tta_modcons_carries_every_key_of_tta_entmin():
    from multimodal_tta_amd.config import compose
    ent = compose(overrides=["task=brats", "model=unet", "method=tta_entmin"])["method"]
    mc = _cfg()["method"]
    assert set(mc) == set(ent) | {"modcons"}
    for k in ent:
        if k not in ("name", "group"):          # `group` ships smaller: every volume brings V views
            assert mc[k] == ent[k], k
    assert 1 <= mc["group"] <= ent["group"]
    text = open(os.path.join(ROOT, "configs", "method", "tta_modcons.yaml")).read()
    assert "nobody has measured a Dice" in text


def test_the_views_of_the_named_and_the_explicit_subsets():
    from multimodal_tta_amd.modcons import keep_masks
    # leave-one-out with a missing modality on 4 channels: V = 4, view 0 = the present channels
    plug = _plug(missing=[1])
    assert plug.views == 4 and plug.keep_masks == [0b1101, 0b1100, 0b1001, 0b0101]
    # single on 2 channels (PET / CT): V = 3
    plug = _plug(channels=2, subsets="single")
    assert plug.views == 3 and plug.keep_masks == [0b11, 0b01, 0b10]
    # leave-one-out on 2 channels is single in the other order
    assert keep_masks("leave_one_out", 2) == [0b11, 0b10, 0b01]
    # an explicit list, intersected with the present set; the order inside a subset does not matter
    plug = _plug(subsets=[[0, 1], [3, 2], [1, 3]], missing=[1])
    assert plug.views == 4 and plug.keep_masks == [0b1101, 0b0001, 0b1100, 0b1000]
    assert keep_masks("single", 4) == [0b1111, 1, 2, 4, 8] and len(keep_masks("single", 7)) == 8
    # the channel count is the model's: without one in the config the views wait for setup (resolve)
    from multimodal_tta_amd.registry import get_plugin
    cfg = _cfg()
    cfg["model"]["in_channels"] = "auto"
    plug = get_plugin("modcons_tta")(cfg)
    assert plug.keep_masks is None
    assert plug.resolve(3) == [0b111, 0b110, 0b101, 0b011] and plug.views == 4 and plug.fused_update is False


@pytest.mark.parametrize("channels,block", [
    (4, dict(subsets=[[0, 1], []])),                      # an empty subset
    (4, dict(subsets=[[1]], missing=[1])),                # ... empty once intersected with the present set
    (4, dict(subsets=[[0, 1, 2, 3]])),                    # equal to view 0
    (4, dict(subsets=[[0, 2, 3]], missing=[1])),          # ... equal to view 0 among the present channels
    (4, dict(subsets=[[0, 1], [1, 0]])),                  # equal to another subset
    (4, dict(subsets=[[0], [0, 1]], missing=[1])),        # ... equal once intersected
    (4, dict(subsets=[[0, 4]])),                          # an index outside the channels
    (4, dict(subsets=[[-1]])),
    (4, dict(subsets=[])),                                # no subset: V = 1
    (4, dict(subsets="leave_one_out", missing=[0, 1, 2])),          # fewer than two present modalities
    (1, dict(subsets="single")),
    (8, dict(subsets="leave_one_out")),                   # V = 9
    (8, dict(subsets="single")),
    (4, dict(subsets=[[0], [1], [2], [3], [0, 1], [0, 2], [0, 3], [1, 2]])),
    (4, dict(subsets="pairs")), (4, dict(subsets=3)), (4, dict(subsets=[0, 1])), (4, dict(subsets=[[0.5]])),
    (4, dict(subsets=[[True]])), (4, dict(subsets={"a": 1}))])
def test_bad_subsets_are_refused_by_key_name(channels, block):
    with pytest.raises(ValueError, match="method.modcons.subsets"):
        _plug(channels, **block)


@pytest.mark.parametrize("key,value", [("weight", -1.0), ("weight", float("nan")), ("weight", True), ("weight", "1"),
                                       ("entropy_weight", float("inf")), ("entropy_weight", -0.1), ("entropy_weight", None),
                                       ("detach", 1), ("detach", "true")])
def test_modcons_plugin_rejects_bad_hyper_parameters(key, value):
    if key == "entropy_weight" and value is None:
        value = [1.0]
    with pytest.raises(ValueError, match=f"method.modcons.{key} "):
        _plug(**{key: value})


def test_weight_zero_is_one_view():
    plug = _plug(weight=0)
    assert plug.views == 1 and plug.keep_masks is None and plug.fused_update is True
    assert plug.resolve(4) is None and plug.views == 1
    # nothing of the block is resolved: subsets that do not fit the channels do not matter to Tent's step
    assert _plug(channels=1, weight=0.0).views == 1


def test_moddrop_the_deep_fusion_model_and_too_many_volumes_are_refused():
    from multimodal_tta_amd.models import MultimodalUNetDeepFusion
    from multimodal_tta_amd.registry import get_plugin
    with pytest.raises(NotImplementedError, match="method.moddrop.enabled"):
        get_plugin("modcons_tta")(_cfg("method.moddrop.enabled=true", "method.moddrop.p=0.25"))
    dcfg = dict(name="unet_multimodal_deepfusion", num_modalities=4, num_classes=3, spatial_dims=3,
                channels=[4, 8, 16, 32, 64], strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)
    with pytest.raises(NotImplementedError, match="MultimodalUNetDeepFusion.*deep-fusion"):
        get_plugin("modcons_tta")(_cfg()).setup(MultimodalUNetDeepFusion(dcfg), "cuda")          # (refused before any device call)
    plug = _plug()
    assert plug.group == 2
    with pytest.raises(NotImplementedError, match="method.group = 2"):
        plug.adapt_volume(torch.zeros(3, 4, 8, 8, 8))          # (refused before any device call)


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("softmax", [False, True], ids=["sigmoid", "softmax"])
@pytest.mark.parametrize("detach", [True, False], ids=["teacher", "both-sides"])
def test_closed_form_gradients_agree_with_autograd_in_float64(softmax, detach):
    g = torch.Generator().manual_seed(5 + softmax)
    for V, G in ((2, 1), (3, 2), (5, 2)):
        z = 3.0 * torch.randn(G * V, 4, 3, 4, 5, generator=g, dtype=torch.float64)
        ref = loss_reference(z, V, softmax, weight=0.7, entropy_weight=1.3, detach=detach)
        got = closed_form_grad(z, V, softmax, weight=0.7, entropy_weight=1.3, detach=detach)
        assert torch.allclose(got, ref["grad"], rtol=1e-11, atol=1e-14), (got - ref["grad"]).abs().max()
        assert (ref["view_kl"] >= 0).all() and torch.allclose(ref["consistency"], ref["view_kl"].mean(1))
        assert torch.allclose(ref["loss"], 1.3 * ref["entropy"] + 0.7 * ref["consistency"])


def test_the_restatement_on_identical_views_and_its_masked_copy():
    g = torch.Generator().manual_seed(9)
    z = 3.0 * torch.randn(1, 3, 3, 4, 5, generator=g, dtype=torch.float64).repeat(3, 1, 1, 1, 1)
    for softmax in (False, True):
        entropy, view_kl, disagree = modcons_terms(z, 3, softmax)
        assert (view_kl == 0).all() and (disagree == 0).all() and entropy.item() > 0
        assert (closed_form_grad(z, 3, softmax, detach=False)[1:] == 0).all()
    x = torch.randn(2, 3, 2, 2, 2, generator=g)
    x[0, 1, 0, 0, 0], x[1, 1, 0, 0, 1] = float("nan"), -0.0
    xv = masked_views(x, [0b111, 0b101])
    assert xv.shape == (4, 3, 2, 2, 2)
    assert torch.equal(xv[0::2].view(torch.int32), x.view(torch.int32))
    assert (xv[1::2, 1].view(torch.int32) == 0).all() and torch.equal(xv[1::2, 0], x[:, 0]) and torch.equal(xv[1::2, 2], x[:, 2])
