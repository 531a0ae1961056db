"""LeakyReLU / no activation on the host side, without a GPU: the containers build MONAI's ADN blocks (and the oracle's
state_dict keys) from every form of `act`, unsupported activations still raise, and the C ABI refuses a bad activation
code or slope before anything is launched."""
import ctypes
import math

import pytest
import torch

SMALL = dict(in_channels=4, num_classes=3, spatial_dims=3, channels=[4, 8, 16, 32, 64], strides=[2, 2, 2, 2],
             num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)
DF = dict(name="unet_multimodal_deepfusion", num_modalities=4, num_classes=3, spatial_dims=3, channels=[4, 8, 16, 32, 64],
          strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)


def _acts(model):
    return [m for m in model.modules() if isinstance(m, (torch.nn.ReLU, torch.nn.LeakyReLU, torch.nn.PReLU))]


@pytest.mark.parametrize("act,slope", [("LEAKYRELU", 0.01), ("leakyrelu", 0.01), (("LEAKYRELU", {"negative_slope": 0.2}), 0.2),
                                       (["LEAKYRELU", {"negative_slope": -0.3, "inplace": True}], -0.3)])
def test_containers_build_leaky_relu_with_the_requested_slope(act, slope):
    from multimodal_tta_amd.models import UNet
    m = UNet(dict(SMALL, act=act))
    acts = _acts(m)
    assert acts and all(type(a) is torch.nn.LeakyReLU and a.negative_slope == slope for a in acts)


def test_config_compose_selects_leaky_relu():
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.models import UNet
    cfg = compose(overrides=["task=brats", "model=unet", "model.act=LEAKYRELU"])
    m = UNet(cfg["model"])
    assert _acts(m) and all(type(a) is torch.nn.LeakyReLU and a.negative_slope == 0.01 for a in _acts(m))


def test_act_none_builds_no_activation():
    """MONAI's ADN with act=None: norm (and dropout) only.  (Through a model config `act: null` means the default RELU, as in
    the reference's config reader.)"""
    import oracle
    from multimodal_tta_amd.models.containers import ADN, Convolution
    adn = ADN(8, "NDA", None, "INSTANCE", 0.0)
    assert [n for n, _ in adn.named_children()] == ["N", "D"]
    conv = Convolution(4, 8, act=None, norm="BATCH", dropout=0.0)
    ref = oracle.Convolution(3, 4, 8, act=None, norm="BATCH", dropout=0.0)
    assert not hasattr(conv.adn, "A")
    assert list(ref.state_dict()) == list(conv.state_dict())


@pytest.mark.parametrize("act", ["LEAKYRELU", ("LEAKYRELU", {"negative_slope": 0.2})])
@pytest.mark.parametrize("res", [0, 2])
def test_state_dict_keys_equal_the_oracle(act, res):
    import oracle
    from multimodal_tta_amd.models import MultimodalUNetDeepFusion, UNet
    cfg = dict(SMALL, act=act, num_res_units=res)
    assert list(oracle.UNet(cfg).state_dict()) == list(UNet(cfg).state_dict())
    dcfg = dict(DF, act=act, num_res_units=res)
    assert list(oracle.MultimodalUNetDeepFusion(dcfg).state_dict()) == list(MultimodalUNetDeepFusion(dcfg).state_dict())


@pytest.mark.parametrize("act", ["PRELU", "GELU", "ELU", ("SWISH", {})])
def test_other_activations_still_raise(act):
    from multimodal_tta_amd.models import UNet
    with pytest.raises(NotImplementedError, match="LEAKYRELU"):
        UNet(dict(SMALL, act=act))


def test_norm_on_load_act_fields():
    from multimodal_tta_amd import _lib, ops
    s = _lib.norm_on_load(relu=True)
    assert s.relu == _lib.ACT_RELU and ctypes.sizeof(s) == 64 and _lib.NormOnLoadAct.negative_slope.offset == 56
    s = ops.NL(None, None, act=ops.ACT_LEAKY_RELU, negative_slope=0.2).struct()
    assert s.relu == 2 and abs(s.negative_slope - 0.2) < 1e-7
    assert ops.NL(None, None, relu=False).struct().relu == 0 and ops.NL(None, None).struct().relu == 1
    assert ctypes.sizeof(_lib.ConvEpilogue) == 72


def test_abi_rejects_a_bad_activation_code_or_slope():
    from multimodal_tta_amd import _lib
    lib = _lib.load()
    for bad in (_lib.norm_on_load(act=3), _lib.norm_on_load(act=_lib.ACT_LEAKY_RELU, negative_slope=math.nan),
                _lib.norm_on_load(act=_lib.ACT_LEAKY_RELU, negative_slope=math.inf)):
        # the descriptors are checked before the (null) tensors are looked at
        assert lib.mmtta_combine(None, ctypes.byref(bad), None, None, None, None) == -1
        assert b"activation" in lib.mmtta_last_error() or b"slope" in lib.mmtta_last_error()
        assert lib.mmtta_norm_bwd_reduce(None, None, ctypes.byref(bad), None, None) == -1
        assert lib.mmtta_norm_bwd_apply(None, None, ctypes.byref(bad), None, None, None, None) == -1
        assert lib.mmtta_norm_bwd_small(None, None, ctypes.byref(bad), 1, None, None) == -1
        assert lib.mmtta_conv_wgrad(None, None, ctypes.byref(bad), None, None, None, 0, None, 0, None) == -1
        assert lib.mmtta_conv_run(None, None, ctypes.byref(bad), None, None, None, None, 0, None, None, 0, None) == -1
    ok = _lib.norm_on_load(act=_lib.ACT_LEAKY_RELU, negative_slope=0.2)
    assert lib.mmtta_combine(None, ctypes.byref(ok), None, None, None, None) == -1
    assert b"null tensor" in lib.mmtta_last_error()
