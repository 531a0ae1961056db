"""Host side of MMTTA_OPT_WGRAD_EPILOGUE_UPDATE (option 19): the option, the query mmtta_conv_wgrad_updates_in_epilogue on
made-up descriptors - the six layers of the headline U-Net whose weight gradient plans one slab per set at 24 volumes in
flight, and every reason to decline - plans that do not depend on the option, and the resource figures of
wgrad_tr_upd_kernel in the built library beside its twin.  Nothing here launches a kernel.

Of the six one-slab layers the three stride-1 convolutions are taken.  The stride-2 forms (both 128 -> 256 convolutions and
the 768 -> 128 transposed convolution) were built and measured slower than their two launches
(profiles/update_epilogue_ab.md), so they are not part of the library and the query must say 0 for them."""
import ctypes as C
import importlib.util
import os
import re

import conv_geometry as cg

OPT = 19
WGRAD_WORKGROUPS = 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, Y, P = 1 << 30, 1 << 40, 1 << 21

# (cin, cout, stride, transposed, x extent, dy extent, taken, workgroups per slab):
# 4 x 128^3 through channels (32, 64, 128, 256, 512) - the 16^3 and 8^3 levels
HEADLINE = [
    (512, 512, 1, False, (8, 8, 8), (8, 8, 8), 1, 16 * 16),
    (256, 512, 1, False, (8, 8, 8), (8, 8, 8), 1, 8 * 16),
    (256, 256, 1, False, (8, 8, 8), (8, 8, 8), 1, 8 * 8),
    (128, 256, 2, False, (16, 16, 16), (8, 8, 8), 0, 4 * 4),      # the stride-2 convolution of the residual unit ...
    (128, 256, 2, False, (16, 16, 16), (8, 8, 8), 0, 4 * 4),      # ... and of its shortcut: the same call
    (768, 128, 2, True, (8, 8, 8), (16, 16, 16), 0, 4 * 12),
]


def _t(base, c, dhw, bf=True, n=8):
    from multimodal_tta_amd import _lib
    return cg._fake_tensor(_lib, base, n, c, dhw, bf)


def _sets(ips=1):
    from multimodal_tta_amd._lib import ParamSets
    return ParamSets(ips, 1, 1 << 20, 0, 1 << 20, 0, 1 << 10, 0)


def _desc(cin, cout, stride, transposed, k=3, bf=True):
    from multimodal_tta_amd._lib import BF16, CONV_FWD, CONVT_FWD, F32, ConvDesc
    return ConvDesc(CONVT_FWD if transposed else CONV_FWD, k, stride, cin, cout, BF16 if bf else F32)


def _epi(desc, x, dy, x_nl=None, sets=None):
    from multimodal_tta_amd import _lib
    return int(_lib.load().mmtta_conv_wgrad_updates_in_epilogue(C.byref(desc), C.byref(x), C.byref(x_nl) if x_nl is not None else None,
                                                                 C.byref(dy), C.byref(sets) if sets is not None else None))


def _plan(desc, x, dy, sets=None):
    from multimodal_tta_amd import _lib
    out = (C.c_int32 * 4)()
    assert int(_lib.load().mmtta_conv_wgrad_plan_sets(C.byref(desc), C.byref(x), C.byref(dy), C.byref(sets) if sets is not None else None, out)) == 0
    return [int(v) for v in out]


def test_option_19_defaults_to_on_and_restores():
    from multimodal_tta_amd import ops
    assert cg.current_options((OPT,)) == {OPT: 1}
    with cg.pinned({OPT: 0}):
        assert cg.current_options((OPT,)) == {OPT: 0}
    with cg.pinned({OPT: 5}):
        assert cg.current_options((OPT,)) == {OPT: 1}, "a switch"
    assert ops.set_option(OPT, 1) == 1


def test_the_symbol_is_declared_exported_and_typed():
    from multimodal_tta_amd import _lib
    header = open(os.path.join(ROOT, "include", "mmtta.h")).read()
    assert "mmtta_conv_wgrad_updates_in_epilogue(" in header and "#define MMTTA_OPT_WGRAD_EPILOGUE_UPDATE 19" in header
    assert "mmtta_conv_wgrad_updates_in_epilogue" in _lib.exported_names()
    assert len(_lib.load().mmtta_conv_wgrad_updates_in_epilogue.argtypes) == 5


def test_the_headline_layers_at_24_volumes_in_flight():
    from multimodal_tta_amd._lib import NormOnLoad
    vals = cg.inflight_values(24)
    assert vals[WGRAD_WORKGROUPS] == 22
    with cg.pinned({**vals, OPT: 1}):
        for cin, cout, stride, tr, xe, ye, taken, per_slab in HEADLINE:
            d, x, dy = _desc(cin, cout, stride, tr), _t(X, cin, xe), _t(Y, cout, ye)
            what = f"{cin} -> {cout} stride {stride}{' transposed' if tr else ''}"
            assert _plan(d, x, dy, _sets())[:2] == [1, 0], what
            assert _epi(d, x, dy, sets=_sets()) == taken, what
            assert _epi(d, x, dy, NormOnLoad(scale=P, shift=P, relu=1), _sets()) == taken, f"{what}: under a norm-on-load"
            with cg.pinned({OPT: 0}):
                assert _epi(d, x, dy, sets=_sets()) == 0, f"{what}: option 19 = 0"
                assert _plan(d, x, dy, _sets())[:2] == [1, 0], f"{what}: the plan does not depend on the option"
            # two slabs per set: the reduction is no longer the identity
            with cg.pinned({WGRAD_WORKGROUPS: 2 * per_slab}):
                assert _plan(d, x, dy, _sets())[0] == 2, what
                assert _epi(d, x, dy, sets=_sets()) == 0, f"{what}: two slabs"


def test_the_query_declines_everything_else():
    from multimodal_tta_amd import _lib
    e = (8, 8, 8)
    with cg.pinned({WGRAD_WORKGROUPS: 1, OPT: 1}):
        ok = (_desc(64, 32, 1, False), _t(X, 64, e), _t(Y, 32, e))
        assert _epi(*ok, sets=_sets()) == 1 and _epi(*ok) == 1, "the eligible twin of the cases below (with and without sets)"
        assert _epi(_desc(32, 96, 1, False), _t(X, 32, e), _t(Y, 96, e), sets=_sets()) == 1, "three column blocks, one per workgroup"
        assert _epi(_desc(32, 64, 2, False), _t(X, 32, (16, 16, 16)), _t(Y, 64, e), sets=_sets()) == 0, "stride 2, a pair: not built"
        assert _epi(_desc(64, 32, 2, True), _t(X, 64, (4, 4, 4)), _t(Y, 32, e), sets=_sets()) == 0, "transposed: not built"
        assert _epi(_desc(40, 32, 1, False), _t(X, 40, e), _t(Y, 32, e), sets=_sets()) == 0, "Cg = 40"
        assert _epi(_desc(64, 40, 1, False), _t(X, 64, e), _t(Y, 40, e), sets=_sets()) == 0, "Cd = 40 does not fill its block"
        assert _epi(_desc(32, 32, 2, False), _t(X, 32, (16, 16, 16)), _t(Y, 32, e), sets=_sets()) == 0, "stride 2 with one column block"
        assert _epi(_desc(64, 64, 1, False), _t(X, 64, e), _t(Y, 64, e), sets=_sets()) == 0, "stride 1 with paired column blocks: not built"
        assert _epi(_desc(64, 32, 1, False, bf=False), _t(X, 64, e, bf=False), _t(Y, 32, e, bf=False), sets=_sets()) == 0, "fp32 precision"
        assert _epi(_desc(64, 32, 1, False), _t(X, 64, e, bf=False), _t(Y, 32, e, bf=False), sets=_sets()) == 0, "fp32-stored tensors"
        assert _epi(_desc(64, 32, 1, False), _t(X, 64, e), _t(Y, 32, e, bf=False), sets=_sets()) == 0, "fp32-stored dy"
        assert _epi(_desc(64, 32, 1, False, k=1), _t(X, 64, e), _t(Y, 32, e), sets=_sets()) == 0, "1x1x1"
        assert _epi(_desc(4, 32, 1, False), _t(X, 4, e), _t(Y, 32, e), sets=_sets()) == 0, "a thin layer"
        assert _epi(_desc(32, 3, 1, False), _t(X, 32, e), _t(Y, 3, e, bf=False), sets=_sets()) == 0, "a thin layer (the head)"
        leaky = _lib.norm_on_load(act=_lib.ACT_LEAKY_RELU, negative_slope=0.1)
        assert _epi(*ok, x_nl=leaky, sets=_sets()) == 0, "LeakyReLU on x: the instantiation without these kernels"
        with cg.pinned({11: 0}):
            assert _epi(*ok, sets=_sets()) == 0, "the fp32-operand kernel (option 11 = 0)"
        with cg.pinned({OPT: 0}):
            assert _epi(*ok, sets=_sets()) == 0, "option 19 = 0"
        assert _epi(_desc(64, 32, 1, False, k=5), _t(X, 64, e), _t(Y, 32, e)) < 0, "an invalid call is an error"
    with cg.pinned({WGRAD_WORKGROUPS: 128, OPT: 1}):
        assert _plan(ok[0], ok[1], ok[2], _sets())[0] == 2 and _epi(*ok, sets=_sets()) == 0, "two tiles, two slabs"


def _demangled_args(name, kernel):
    """The template arguments of `kernel` in an Itanium-mangled name, as a tuple of ints (Li<n>E / Lb<0|1>E)."""
    m = re.search(r"^_ZN5mmtta\d+" + kernel + r"I((?:L[ib]\d+E)+)E", name)      # (not the mmtta::leaky instantiation)
    return tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1))) if m else None


def test_the_new_kernels_add_no_scratch_beyond_the_rule():
    """The form that is built, for each optimizer kind, beside its twin wgrad_tr_kernel<4, 8, 1, true, true, false, 1>.  The
    twin already spills (36 registers, 148 bytes of scratch); the update form spills up to 10 registers more and stays
    because profiles/update_epilogue_ab.md shows a kernel-time gain for its three layers (the rule of
    profiles/raw_staging_ab.md).  It is held to the figures recorded there, and to the twin's two workgroups per CU."""
    from multimodal_tta_amd import _lib
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    table = kr.figures(_lib.LIB_PATH)
    upd = {}
    for name, fig in table.items():
        a = _demangled_args(name, "wgrad_tr_upd_kernel")       # (TZ, TY, SI, TD, NB, RG, RD, KIND)
        if a is not None:
            upd[a] = fig
    assert sorted(upd) == [(4, 8, 1, 0, 1, 0, 0, kind) for kind in (0, 1, 2)], sorted(upd)
    assert not any("wgrad_tr_upd_kernel" in name and "leaky" in name for name in table), "none in the LeakyReLU translation unit"
    twin = [fig for name, fig in table.items() if _demangled_args(name, "wgrad_tr_kernel") == (4, 8, 1, 1, 1, 0, 1)]
    assert len(twin) == 1 and (twin[0]["scratch"], twin[0]["vgpr_spill"]) == (148, 36), twin
    for key, fig in sorted(upd.items()):
        assert fig["lds"] == twin[0]["lds"] == 0, (key, fig)          # dynamic LDS only: the launch asks for the twin's bytes
        assert fig["vgpr"] + fig["agpr"] <= 256, (key, fig)
        assert fig["scratch"] <= 156 and fig["vgpr_spill"] <= 46, (key, fig)
