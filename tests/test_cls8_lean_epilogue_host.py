"""Host side of MMTTA_OPT_CLS8_LEAN_EPILOGUE (option 21): the option, the query mmtta_conv_cls8_lean_epilogue on made-up
descriptors - the eligible calls, another route, the options it stands on, a transform on the input, fp32 storage, a LeakyReLU
add, channel counts that are no multiple of 8 - and the resource figures of igemm_cls8_lean_kernel in the built library beside
its twin igemm_cls8_pipe_kernel.  Nothing here launches a kernel."""
import ctypes as C
import importlib.util
import os

import conv_geometry as cg

OPT, OPT_PIPE, OPT_RAW, OPT_CLS_MIN = 21, 20, 16, 12
ROUTE_CLS_FUSED = 15
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, Y, A, P = 1 << 30, 1 << 40, 1 << 41, 1 << 21
COARSE, FINE = (8, 8, 8), (16, 16, 16)


_t, _query = cg.fake, cg.query


def _lean(*a, **k):
    return _query("mmtta_conv_cls8_lean_epilogue", *a, **k)


def _pipelined(*a, **k):
    return _query("mmtta_conv_cls8_pipelined", *a, **k)


def _route(*a, **k):
    return _query("mmtta_conv_route", *a, **k)


def test_option_21_defaults_to_on_and_restores():
    from multimodal_tta_amd import ops
    assert cg.current_options((OPT,)) == {OPT: 1}
    with cg.pinned({OPT: 0}):
        assert cg.current_options((OPT,)) == {OPT: 0}
    with cg.pinned({OPT: 2}):
        assert cg.current_options((OPT,)) == {OPT: 0}, "bit 1 is reserved: nothing reads it"
    with cg.pinned({OPT: 3}):
        assert cg.current_options((OPT,)) == {OPT: 1}
    assert ops.set_option(OPT, 1) == 1


def test_the_symbol_is_declared_exported_and_typed():
    from multimodal_tta_amd import _lib
    header = open(os.path.join(ROOT, "include", "mmtta.h")).read()
    assert "mmtta_conv_cls8_lean_epilogue(" in header and "#define MMTTA_OPT_CLS8_LEAN_EPILOGUE 21" in header
    assert "mmtta_conv_cls8_lean_epilogue" in _lib.exported_names()
    fn = _lib.load().mmtta_conv_cls8_lean_epilogue
    assert len(fn.argtypes) == 7 and list(fn.argtypes) == list(_lib.load().mmtta_conv_cls8_pipelined.argtypes)
    assert _lib.load().mmtta_abi_version() == 2


def test_the_query_names_the_eligible_calls_only():
    from multimodal_tta_amd import _lib
    from multimodal_tta_amd._lib import BF16, CONV_DGRAD, CONV_FWD, CONVT_FWD, F32, ConvDesc, NormOnLoad
    convt = ConvDesc(CONVT_FWD, 3, 2, 128, 32, BF16)
    dgrad = ConvDesc(CONV_DGRAD, 3, 2, 32, 64, BF16)
    with cg.pinned({OPT_CLS_MIN: 1, OPT: 1, OPT_PIPE: 1, OPT_RAW: 3}):
        ok = (convt, _t(X, 128, COARSE), _t(Y, 32, FINE))
        # eligible: both forms, with a fused add, accumulate and statistics rows, under a norm-on-load that does nothing
        assert _route(*ok) == ROUTE_CLS_FUSED and _lean(*ok) == 1
        assert _lean(*ok, add=_t(A, 32, FINE), accumulate=1, stats=P) == 1
        assert _lean(*ok, x_nl=NormOnLoad()) == 1
        dg = (dgrad, _t(X, 64, COARSE), _t(Y, 32, FINE))
        assert _route(*dg) == ROUTE_CLS_FUSED and _lean(*dg) == 1 and _lean(*dg, accumulate=1) == 1
        odd = (dgrad, _t(X, 64, COARSE), _t(Y, 32, (15, 15, 15)))
        assert _route(*odd) == ROUTE_CLS_FUSED and _lean(*odd) == 1, "an odd extent is the kernel's business: its border tiles"
        assert _lean(ConvDesc(CONVT_FWD, 3, 2, 40, 24, BF16), _t(X, 40, COARSE), _t(Y, 24, FINE)) == 1, "partial stage, partial column block"
        # channel counts in groups of 4: the pipelined kernel, not the lean epilogue
        c36 = (ConvDesc(CONVT_FWD, 3, 2, 128, 36, BF16), _t(X, 128, COARSE), _t(Y, 36, FINE))
        assert _route(*c36) == ROUTE_CLS_FUSED and _pipelined(*c36) == 1 and _lean(*c36) == 0, "y.c % 8"
        assert _lean(*c36, add=_t(A, 36, FINE)) == 0
        # another route
        s1 = (ConvDesc(CONV_FWD, 3, 1, 64, 64, BF16), _t(X, 64, FINE), _t(Y, 64, FINE))
        assert _route(*s1) != ROUTE_CLS_FUSED and _lean(*s1) == 0, "a stride-1 layer"
        s2 = (ConvDesc(CONV_FWD, 3, 2, 32, 64, BF16), _t(X, 32, FINE), _t(Y, 64, COARSE))
        assert _route(*s2) != ROUTE_CLS_FUSED and _lean(*s2) == 0, "the stride-2 forward"
        with cg.pinned({OPT_CLS_MIN: 1 << 20}):
            assert _route(*ok) != ROUTE_CLS_FUSED and _lean(*ok) == 0, "the per-class launches of the same call"
        # a transform present, or operands the raw stage does not take
        assert _lean(*ok, x_nl=NormOnLoad(mean=P, rstd=P)) == 0, "norm-on-load with mean"
        assert _lean(*ok, x_nl=NormOnLoad(scale=P, shift=P)) == 0, "norm-on-load with scale"
        assert _lean(*ok, x_nl=_lib.norm_on_load(relu=True)) == 0, "activation-only norm-on-load"
        leaky = _lib.norm_on_load(act=_lib.ACT_LEAKY_RELU, negative_slope=0.1)
        assert _lean(*ok, x_nl=leaky) == 0
        assert _lean(*ok, add=_t(A, 32, FINE), add_nl=leaky) == 0, "LeakyReLU on the fused add: the instantiation without these kernels"
        fp = (convt, _t(X, 128, COARSE, bf=False), _t(Y, 32, FINE, bf=False))
        assert _route(*fp) == ROUTE_CLS_FUSED and _lean(*fp) == 0, "fp32-stored tensors"
        f32 = ConvDesc(CONVT_FWD, 3, 2, 128, 32, F32)
        assert _lean(f32, _t(X, 128, COARSE, bf=False), _t(Y, 32, FINE, bf=False)) == 0, "fp32 precision"
        # the options
        with cg.pinned({OPT: 0}):
            assert _lean(*ok) == 0 and _lean(*dg) == 0 and _route(*ok) == ROUTE_CLS_FUSED and _pipelined(*ok) == 1, "option 21 = 0"
        with cg.pinned({OPT: 2}):
            assert _lean(*ok) == 0, "bit 1 alone"
        with cg.pinned({OPT_PIPE: 0}):
            assert _lean(*ok) == 0 and _lean(*dg) == 0 and _route(*ok) == ROUTE_CLS_FUSED, "option 20 = 0"
        for bits, want in ((0, 0), (2, 0), (1, 1)):
            with cg.pinned({OPT_RAW: bits}):
                assert _lean(*ok) == want, f"option 16 = {bits}"
        assert _lean(ConvDesc(CONVT_FWD, 5, 2, 128, 32, BF16), _t(X, 128, COARSE), _t(Y, 32, FINE)) < 0, "an invalid call is an error"


def test_plans_do_not_depend_on_the_option():
    from multimodal_tta_amd import _lib
    from multimodal_tta_amd._lib import BF16, CONVT_FWD, ConvDesc
    d, x, y = ConvDesc(CONVT_FWD, 3, 2, 128, 32, BF16), _t(X, 128, COARSE), _t(Y, 32, FINE)
    plans = []
    for bit in (0, 1):
        with cg.pinned({OPT_CLS_MIN: 1, OPT: bit}):
            p = _lib.ConvPlan()
            assert int(_lib.load().mmtta_conv_plan(C.byref(d), C.byref(x), C.byref(y), C.byref(p))) == 0
            plans.append((p.tiles, p.launches, p.ksplit, p.stats_rows, p.config, p.workspace_bytes))
    assert plans[0] == plans[1] and plans[0][4] == ROUTE_CLS_FUSED


def test_the_new_kernel_spills_no_more_than_its_twin():
    """igemm_cls8_lean_kernel<16, true> beside igemm_cls8_pipe_kernel<16, true>: one of it, none in the LeakyReLU translation
    unit, inside 256 registers, no more scratch bytes and no more spilled VGPRs (the lean epilogue itself spills nothing; what
    spills does so in the border tiles' epilogue, which is the twin's)."""
    from multimodal_tta_amd import _lib
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    table = kr.figures(_lib.LIB_PATH)
    lean = [fig for name, fig in table.items() if "igemm_cls8_lean_kernel" in name]
    twin = [fig for name, fig in table.items() if name.startswith("_ZN5mmtta22igemm_cls8_pipe_kernelILi16ELb1EEE")]
    assert len(lean) == 1 and len(twin) == 1, (lean, twin)
    assert [name for name in table if "igemm_cls8_lean_kernel" in name][0].startswith("_ZN5mmtta22igemm_cls8_lean_kernelILi16ELb1EEE")
    assert not any("igemm_cls8_lean_kernel" in name and "leaky" in name for name in table), "none in the LeakyReLU translation unit"
    print("lean", lean[0], "twin", twin[0])
    assert lean[0]["lds"] == twin[0]["lds"] == 0          # dynamic LDS only: the launcher asks for box + two images
    assert lean[0]["vgpr"] + lean[0]["agpr"] <= 256
    assert lean[0]["scratch"] <= twin[0]["scratch"], (lean[0], twin[0])
    assert lean[0]["vgpr_spill"] <= twin[0]["vgpr_spill"], (lean[0], twin[0])
