"""Host side of MMTTA_OPT_THIN_LEAN (option 18): the option, the query mmtta_conv_thin_lean on made-up descriptors, plans and
routes that do not depend on the option, and the resource figures of the lean kernels in the built library.  Nothing here
launches a kernel."""
import ctypes as C
import importlib.util
import os

import conv_geometry as cg

OPT = 18
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, Y, A, P = 1 << 30, 1 << 40, 1 << 41, 1 << 21


_t, _query = cg.fake, cg.query


def _lean(*a, **k):
    return _query("mmtta_conv_thin_lean", *a, **k)


def test_option_18_defaults_to_both_bits_and_restores():
    from multimodal_tta_amd import ops
    assert cg.current_options((OPT,)) == {OPT: 3}
    with cg.pinned({OPT: 0}):
        assert cg.current_options((OPT,)) == {OPT: 0}
    with cg.pinned({OPT: 7}):
        assert cg.current_options((OPT,)) == {OPT: 3}, "two bits"
    assert ops.set_option(OPT, 3) == 3


def test_the_symbol_is_declared_exported_and_typed():
    from multimodal_tta_amd import _lib
    header = open(os.path.join(ROOT, "include", "mmtta.h")).read()
    assert "mmtta_conv_thin_lean(" in header and "#define MMTTA_OPT_THIN_LEAN 18" in header
    assert "mmtta_conv_thin_lean" in _lib.exported_names()
    assert len(_lib.load().mmtta_conv_thin_lean.argtypes) == len(_lib._SIGNATURES["mmtta_conv_route"][1])


def test_query_names_the_eligible_calls_only():
    from multimodal_tta_amd import _lib
    from multimodal_tta_amd._lib import BF16, CONV_FWD, CONVT_DGRAD, CONVT_FWD, F32, ConvDesc, NormOnLoad
    fine, coarse = (15, 15, 31), (8, 8, 16)
    leaky = _lib.norm_on_load(act=_lib.ACT_LEAKY_RELU, negative_slope=0.1)
    with cg.pinned({OPT: 3}):
        # ---- bit 0: thin-K at stride 2, bf16-stored on both sides
        for K in (2, 3, 4):
            d = ConvDesc(CONV_FWD, 3, 2, K, 32, BF16)
            assert _lean(d, _t(X, K, fine), _t(Y, 32, coarse)) == 1
            assert _lean(d, _t(X, K, fine), _t(Y, 32, coarse), add=_t(A, 32, coarse), stats=P) == 1
            assert _lean(d, _t(X, K, fine), _t(Y, 32, coarse), x_nl=NormOnLoad(scale=P, shift=P), stats=P) == 1, "a norm-on-load on x"
        d4 = ConvDesc(CONV_FWD, 3, 2, 4, 32, BF16)
        x4, y32 = _t(X, 4, fine), _t(Y, 32, coarse)
        for K in (1, 2, 3, 4):
            assert _lean(ConvDesc(CONV_FWD, 3, 2, K, 64, BF16), _t(X, K, fine), _t(Y, 64, coarse), stats=P) == 1, "64 columns"
        dT = ConvDesc(CONVT_DGRAD, 3, 2, 64, 3, BF16)
        assert _lean(dT, _t(X, 3, (16, 16, 32)), _t(Y, 64, coarse)) == 1, "the 64-column form"
        # not lean
        assert _lean(d4, x4, y32, accumulate=1) == 0, "accumulate"
        assert _lean(d4, x4, _t(Y, 32, coarse, bf=False)) == 0, "fp32-stored y"
        assert _lean(d4, _t(X, 4, fine, bf=False), y32) == 0, "fp32-stored x"
        assert _lean(d4, x4, y32, add=_t(A, 32, coarse), add_nl=leaky) == 0, "LeakyReLU on the add"
        assert _lean(d4, x4, y32, x_nl=leaky) == 0, "LeakyReLU on x"
        assert _lean(d4, x4, _t(Y + 8, 32, coarse)) == 0, "y off its 16-byte rows"
        assert _lean(ConvDesc(CONV_FWD, 3, 1, 4, 32, BF16), _t(X, 4, coarse), y32) == 0, "stride 1"
        assert _lean(ConvDesc(CONV_FWD, 3, 2, 4, 32, F32), _t(X, 4, fine, bf=False), _t(Y, 32, coarse, bf=False)) == 0, "fp32 precision"
        assert _lean(ConvDesc(CONV_FWD, 3, 2, 32, 64, BF16), _t(X, 32, fine), _t(Y, 64, coarse)) == 0, "the implicit GEMM"
        # ---- bit 1: the gather-GEMM up-convolution from a bf16-stored input without a transform
        for K in (32, 64):
            for R in (1, 2, 3, 4):
                dU = ConvDesc(CONVT_FWD, 3, 2, K, R, BF16)
                xu, yu = _t(X, K, coarse), _t(Y, R, (16, 16, 32), bf=False)
                assert _lean(dU, xu, yu, stats=P) == 2
                assert _lean(dU, xu, yu, add=_t(A, R, (16, 16, 32), bf=False)) == 2
                assert _lean(dU, xu, yu, x_nl=NormOnLoad()) == 2, "a norm-on-load that does nothing"
                assert _lean(dU, xu, yu, x_nl=NormOnLoad(scale=P, shift=P)) == 0, "norm-on-load with scale"
                assert _lean(dU, xu, yu, x_nl=NormOnLoad(mean=P, rstd=P)) == 0, "norm-on-load with mean"
                assert _lean(dU, _t(X, K, coarse, bf=False), yu) == 0, "fp32-stored x"
                assert _lean(dU, xu, yu, add=_t(A, R, (16, 16, 32), bf=False), add_nl=leaky) == 0, "LeakyReLU on the add"
        assert _lean(ConvDesc(CONV_FWD, 3, 1, 3, 3, BF16), _t(X, 3, coarse, bf=False), _t(Y, 3, coarse, bf=False)) == 0, "the head pair"
        # ---- the bits
        dU = ConvDesc(CONVT_FWD, 3, 2, 64, 3, BF16)
        xu, yu = _t(X, 64, coarse), _t(Y, 3, (16, 16, 32), bf=False)
        for bits, thin, up in ((0, 0, 0), (1, 1, 0), (2, 0, 2), (3, 1, 2)):
            with cg.pinned({OPT: bits}):
                assert _lean(d4, x4, y32) == thin and _lean(dU, xu, yu) == up, f"option 18 = {bits}"
        assert _lean(ConvDesc(CONV_FWD, 5, 2, 4, 32, BF16), x4, y32) < 0, "an invalid call is an error"


def test_plans_and_routes_do_not_depend_on_the_option():
    from multimodal_tta_amd import _lib
    from multimodal_tta_amd._lib import BF16, CONV_FWD, CONVT_DGRAD, CONVT_FWD, ConvDesc
    calls = [(ConvDesc(CONV_FWD, 3, 2, K, 32, BF16), _t(X, K, (15, 17, 31)), _t(Y, 32, (8, 9, 16))) for K in (2, 3, 4)]
    calls.append((ConvDesc(CONVT_DGRAD, 3, 2, 64, 3, BF16), _t(X, 3, (16, 18, 32)), _t(Y, 64, (8, 9, 16))))
    calls += [(ConvDesc(CONVT_FWD, 3, 2, K, 3, BF16), _t(X, K, (8, 9, 16)), _t(Y, 3, (16, 18, 32), bf=False)) for K in (32, 64)]
    seen = set()
    for desc, x, y in calls:
        got = []
        for bits in (0, 3):
            with cg.pinned({OPT: bits}):
                plan = _lib.ConvPlan()
                assert int(_lib.load().mmtta_conv_plan(C.byref(desc), C.byref(x), C.byref(y), C.byref(plan))) == 0
                got.append((bytes(plan), _query("mmtta_conv_route", desc, x, y, stats=P)))
        assert got[0] == got[1] and got[0][1] >= 0
        seen.add(got[0][1])
    assert seen == {6, 13}


def test_the_lean_kernels_use_no_scratch_and_spill_no_vector_registers():
    from multimodal_tta_amd import _lib
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    lean = {k: v for k, v in kr.figures(_lib.LIB_PATH).items() if "chan_mfma_lean_kernel" in k or "upconv8_lean_kernel" in k}
    assert len(lean) == 14 + 8, sorted(lean)      # K = 1 .. 4 x 32 / 64 columns x with / without a transform, less K = 1 into 32
    for name, fig in lean.items():
        assert fig["scratch"] == 0 and fig["vgpr_spill"] == 0, (name, fig)
