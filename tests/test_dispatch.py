"""Every dispatchable kernel instantiation of the convolution family is selected by at least one shape of the GPU
parity cases (tests/test_hip_conv.py::CASES / BF16_CASES) - asserted through the planner the launches themselves use
(``mmtta_conv_plan`` / ``mmtta_conv_wgrad_kernel`` are host-only, so this runs without a GPU too).

config ids: csrc/conv_igemm.hip::config_id (0-5 fp32 igemm, 6 direct, 7-12 bf16 igemm, 13 channel kernel, 14 the lean 4x8x8 tile
of the 32-output-channel bf16 layers: the default, id 7 = the 8x8x8 tile under MMTTA_OPT_IGEMM_LEAN = 0, parity case
test_lean_tile_matches_the_wide_tile; 15 class-fused);
weight-gradient ids: mmtta_conv_wgrad_kernel returns the planner's route, the enum csrc/conv_wgrad.hip::WRoute, whose values
are the ids (0 f32 s1, 1 f32 s2, 2 1x1, 3 small-channel, 6 tiny, 7 / 8 transposed-read bf16 s1 / s2: the default of bf16
precision, parity cases test_transposed_read_wgrad; 0 / 1 under option 11 = 0; ids 4 / 5 were round 1's staging-transposed
bf16 kernels, removed in round 3;
9 the 1x1x1 streaming kernel of bf16 precision, parity cases test_pointwise_conv_weight_gradient_on_transposed_reads;
10 the thin 27-tap layers of bf16 precision on transposed reads, parity cases test_thin_wgrad_on_transposed_reads).
VERDICT r1 P1: ids 2 and 9 (igemm <4,4,4,4,8,32>) used to be reachable only by the full-size bench."""
import ctypes as C

import torch

from test_hip_conv import BF16_CASES, CASES, THIN_TR_CASES, TR_CASES

# (case, (fwd, dgrad) config in fp32 mode, the same in bf16 mode, weight-gradient kernel (fp32 mode, bf16 mode))
DISPATCH = [
    ((32, 32, 3, 1, False, (1, 16, 16, 16)), (0, 0), (14, 14), (0, 7)),
    ((64, 64, 3, 1, False, (1, 8, 8, 8)), (1, 1), (8, 8), (0, 7)),
    ((128, 128, 3, 1, False, (1, 32, 32, 32)), (2, 2), (9, 9), (0, 7)),
    ((16, 32, 3, 2, False, (1, 8, 8, 8)), (3, 0), (10, 14), (1, 8)),
    ((32, 64, 3, 2, False, (1, 8, 8, 16)), (4, 0), (11, 14), (1, 8)),
    ((64, 128, 3, 2, False, (1, 5, 6, 7)), (5, 1), (12, 8), (1, 8)),
    ((128, 136, 3, 1, False, (2, 4, 6, 8)), (5, 5), (12, 12), (0, 7)),
    ((768, 128, 3, 2, True, (1, 8, 8, 8)), (2, 5), (9, 12), (1, 8)),
    ((256, 512, 1, 1, False, (1, 4, 4, 4)), (5, 5), (12, 12), (2, 9)),
    ((64, 3, 3, 2, True, (1, 3, 5, 70)), (6, 4), (6, 13), (3, 10)),
    ((4, 32, 3, 2, False, (1, 16, 16, 16)), (13, 6), (13, 6), (3, 10)),
    ((3, 3, 3, 1, False, (1, 8, 8, 8)), (6, 6), (6, 6), (6, 10)),
]


def _desc(t, dtype=None):
    from multimodal_tta_amd._lib import F32, Tensor
    n, d, h, w, c = t.shape
    sn, sd, sh, sw, _ = t.stride()
    return Tensor(t.data_ptr(), n, c, d, h, w, sn, 1, sd, sh, sw, F32 if dtype is None else dtype, 0)


def _cl(n, d, h, w, c):
    return torch.empty((n, d, h, w, (c + 3) // 4 * 4))[..., :c]


def test_every_kernel_instantiation_is_reached_by_a_parity_case():
    from multimodal_tta_amd import _lib
    from multimodal_tta_amd._lib import BF16, CONV_DGRAD, CONV_FWD, CONVT_DGRAD, CONVT_FWD, F32, ConvDesc, ConvPlan

    lib = _lib.load()
    # the launch-geometry knobs are process-wide and an adaptation plugin re-tunes them for its volumes in flight: the table
    # below holds for the documented defaults (4 volumes in flight), whatever ran before in this process
    from multimodal_tta_amd import ops
    ops.tune_for_volumes_in_flight(4)
    seen_cfg, seen_wg, splitk_wide = set(), set(), set()
    for case, want_f32, want_bf16, want_wg in DISPATCH:
        cin, cout, k, stride, transposed, (n, d, h, w) = case
        assert case in CASES, case
        x = _cl(n, d, h, w, cin)
        if transposed:
            y = _cl(n, 2 * d, 2 * h, 2 * w, cout)
        elif stride == 1:
            y = _cl(n, d, h, w, cout)
        else:
            y = _cl(n, (d + 1) // 2, (h + 1) // 2, (w + 1) // 2, cout)
        tx, ty = _desc(x), _desc(y)
        fo, do = (CONVT_FWD, CONVT_DGRAD) if transposed else (CONV_FWD, CONV_DGRAD)
        for dtype, want, wg in ((F32, want_f32, want_wg[0]), (BF16, want_bf16, want_wg[1])):
            if dtype == BF16 and (want != want_f32 or wg != want_wg[0]):
                assert case in BF16_CASES, f"{case}: bf16 instantiation without a bf16 parity case"
            got = []
            for op, a, b in ((fo, tx, ty), (do, ty, tx)):
                dsc, plan = ConvDesc(op, k, stride, cin, cout, dtype), ConvPlan()
                assert lib.mmtta_conv_plan(C.byref(dsc), C.byref(a), C.byref(b), C.byref(plan)) == 0
                got.append(int(plan.config))
                if plan.ksplit > 1:
                    splitk_wide.add(int(plan.config))
            assert tuple(got) == want, f"{case} dtype {dtype}: plan configs {got}, expected {want}"
            dsc = ConvDesc(fo, k, stride, cin, cout, dtype)
            kid = int(lib.mmtta_conv_wgrad_kernel(C.byref(dsc), C.byref(tx), C.byref(ty)))
            assert kid == wg, f"{case} dtype {dtype}: weight-gradient kernel {kid}, expected {wg}"
            seen_cfg.update(got)
            seen_wg.add(kid)
            if dtype == BF16 and 14 in got:                # the 8x8x8 tile (id 7) stays reachable: MMTTA_OPT_IGEMM_LEAN = 0
                prev = lib.mmtta_set_option(10, 0)
                try:
                    for op, a, b, g in ((fo, tx, ty, got[0]), (do, ty, tx, got[1])):
                        dsc0, plan0 = ConvDesc(op, k, stride, cin, cout, dtype), ConvPlan()
                        assert lib.mmtta_conv_plan(C.byref(dsc0), C.byref(a), C.byref(b), C.byref(plan0)) == 0
                        assert int(plan0.config) == (7 if g == 14 else g), f"{case}: option 10 = 0 plans {int(plan0.config)}"
                        seen_cfg.add(int(plan0.config))
                finally:
                    lib.mmtta_set_option(10, prev)
            if dtype == BF16 and wg == 10:
                assert case in THIN_TR_CASES, f"{case}: thin transposed-read instantiation without a parity case"
            if dtype == BF16 and wg in (7, 8):
                assert case in TR_CASES, f"{case}: transposed-read instantiation without a parity case"
                # the same layer with its module input bf16-stored (method.storage: bf16): the same kernel
                kid = int(lib.mmtta_conv_wgrad_kernel(C.byref(dsc), C.byref(_desc(x, BF16)), C.byref(ty)))
                assert kid == wg, f"{case} bf16-stored: weight-gradient kernel {kid}, expected {wg}"
                # MMTTA_OPT_WGRAD_VECTOR_STAGING = 0 (and every operand pair the 16-byte loader cannot take): the fp32-operand
                # kernels (ids 0 / 1)
                prev = lib.mmtta_set_option(11, 0)
                try:
                    kid0 = int(lib.mmtta_conv_wgrad_kernel(C.byref(dsc), C.byref(tx), C.byref(ty)))
                finally:
                    lib.mmtta_set_option(11, prev)
                assert kid0 == wg - 7, f"{case} option 0: weight-gradient kernel {kid0}, expected {wg - 7}"
                seen_wg.add(kid0)
    assert seen_cfg == set(range(15)), f"conv configs without a parity case: {sorted(set(range(15)) - seen_cfg)}"
    live_wg = set(range(11)) - {4, 5}            # ids 4 / 5 were the round-1 staging-transposed bf16 kernels (removed in round 3)
    assert seen_wg == live_wg, f"weight-gradient kernels without a parity case: {sorted(live_wg - seen_wg)}"
    assert {2, 9} <= splitk_wide, "the 32-channel-stage igemm also needs a split-K parity case"


def test_class_fused_kernel_is_planned_for_large_stride2_forms():
    """config 15 (igemm_cls8_kernel): the stride-2 transposed forms of a bf16 layer take the class-fused kernel once one
    workgroup per coarse 4x4x8 tile and 32 output channels makes >= MMTTA_OPT_CLASS_FUSED_MIN_WORKGROUPS (128) workgroups,
    and the per-class kernel below that; its parity cases force it on small shapes
    (tests/test_hip_conv.py::test_class_fused_stride2_forms_match_the_per_class_kernel)."""
    from multimodal_tta_amd import _lib
    from multimodal_tta_amd._lib import BF16, CONV_DGRAD, CONVT_FWD, ConvDesc, ConvPlan

    lib = _lib.load()
    for (cin, cout, transposed, coarse, want) in ((128, 32, True, (32, 32, 32), 15), (32, 64, False, (32, 32, 32), 15),
                                                  (128, 32, True, (8, 8, 8), 14), (768, 128, True, (8, 8, 8), 9)):
        d, h, w = coarse
        lo, hi = _cl(1, d, h, w, cin if transposed else cout), _cl(1, 2 * d, 2 * h, 2 * w, cout if transposed else cin)
        op = CONVT_FWD if transposed else CONV_DGRAD          # both read the coarse tensor and write the fine one
        dsc, plan = ConvDesc(op, 3, 2, cin, cout, BF16), ConvPlan()
        assert lib.mmtta_conv_plan(C.byref(dsc), C.byref(_desc(lo)), C.byref(_desc(hi)), C.byref(plan)) == 0
        assert int(plan.config) == want, (cin, cout, transposed, coarse, int(plan.config))
        if want == 15:
            assert plan.ksplit == 1 and plan.stats_rows == (d // 4) * (h // 4) * (w // 8)


def _t(base, c, dhw, dtype=0, n=1, row_pad=0, gap=0):
    """A channels-last descriptor at a synthetic address (the planner never reads tensor memory): voxel rows of c rounded up
    to 4 elements (8 for a bf16-stored tensor of more than 4 channels) plus `row_pad`, x-rows `gap` elements apart."""
    from multimodal_tta_amd._lib import Tensor
    d, h, w = dhw
    sw = ((c + 3) // 4 * 4 if (dtype == 0 or c <= 4) else (c + 7) // 8 * 8) + row_pad
    sh = w * sw + gap
    return Tensor(base, n, c, d, h, w, d * h * sh, 1, h * sh, sh, sw, dtype, 0)


def _route(lib, dsc, x, y, stats=None, add=None, norm=None, accumulate=0):
    from multimodal_tta_amd._lib import ConvEpilogue, NormOnLoadAct
    epi = ConvEpilogue(C.pointer(add), NormOnLoadAct()) if add is not None else None
    return int(lib.mmtta_conv_route(C.byref(dsc), C.byref(x), C.byref(norm) if norm is not None else None,
                                    C.byref(epi) if epi is not None else None, C.byref(y), accumulate, stats))


def _thin_kernel(lib, dsc, x, y, stats=None, accumulate=0):
    return int(lib.mmtta_conv_thin_kernel(C.byref(dsc), C.byref(x), None, None, C.byref(y), accumulate, stats))


def _config(lib, dsc, x, y):
    from multimodal_tta_amd._lib import ConvPlan
    plan = ConvPlan()
    assert lib.mmtta_conv_plan(C.byref(dsc), C.byref(x), C.byref(y), C.byref(plan)) == 0
    return int(plan.config)


def test_every_route_is_reached_and_run_time_operands_flip_only_the_two_pointwise_routes():
    """mmtta_conv_route names the kernel a run launches (csrc/conv_igemm.hip::CRoute, the function conv_run_body itself asks).
    Without run-time operands it is mmtta_conv_plan's config for every parity shape of DISPATCH; the two 1x1x1 routes that
    mmtta_conv_plan cannot see are expected from the gates of the commit before the planner existed (cb18d86):
      16  conv_run_body, csrc/conv_igemm.hip:1952 - pointwise_small_applicable (csrc/conv_direct.hip:1382-1389: k1 s1, no
          statistics, no add, no norm-on-load, <= 4 fp32 channels read from 16-byte-aligned rows, y.c % 4 == 0) and fp32 operands;
      17  conv_run_body, csrc/conv_igemm.hip:1957-1969 - k1 forward / input gradient with bf16 operands, K / 16 in
          {1, 2, 3, 4, 6, 8}, Np <= 64, no statistics, no norm-on-load, d * h * w >= 4096, x / y / add voxel-dense with 16-byte
          rows in one storage type."""
    from multimodal_tta_amd import _lib, ops
    from multimodal_tta_amd._lib import BF16, CONV_DGRAD, CONV_FWD, CONVT_DGRAD, CONVT_FWD, F32, ConvDesc, NormOnLoad

    lib = _lib.load()
    ops.tune_for_volumes_in_flight(4)
    X, Y, A, STATS = 1 << 30, 1 << 40, 1 << 41, 1 << 20
    seen, thin_seen = set(), set()
    for case, want_f32, want_bf16, _ in DISPATCH:
        cin, cout, k, stride, transposed, (n, d, h, w) = case
        fine = (2 * d, 2 * h, 2 * w) if transposed else ((d, h, w) if stride == 1 else ((d + 1) // 2, (h + 1) // 2, (w + 1) // 2))
        tx, ty = _t(X, cin, (d, h, w), n=n), _t(Y, cout, fine, n=n)
        fo, do = (CONVT_FWD, CONVT_DGRAD) if transposed else (CONV_FWD, CONV_DGRAD)
        for dtype, want in ((F32, want_f32), (BF16, want_bf16)):
            for lean in ((1, 0) if dtype == BF16 and 14 in want else (1,)):
                prev = lib.mmtta_set_option(10, lean)
                try:
                    for op, a, b, cfg in ((fo, tx, ty, want[0]), (do, ty, tx, want[1])):
                        dsc = ConvDesc(op, k, stride, cin, cout, dtype)
                        r = _route(lib, dsc, a, b)
                        assert r == _config(lib, dsc, a, b) == (7 if (cfg == 14 and not lean) else cfg), (case, dtype, op, r)
                        assert r == _route(lib, dsc, a, b, accumulate=1), "no gate reads `accumulate`"
                        seen.add(r)
                        # mmtta_conv_thin_kernel names a kernel of route 6 (ids 1 - 10) or 13 (11 - 13), and nothing elsewhere
                        kern = _thin_kernel(lib, dsc, a, b)
                        assert (1 <= kern <= 10) if r == 6 else (11 <= kern <= 13) if r == 13 else kern == 0, (case, dtype, op, r, kern)
                        thin_seen.add(kern)
                finally:
                    lib.mmtta_set_option(10, prev)
    # 15: test_class_fused_kernel_is_planned_for_large_stride2_forms
    dsc = ConvDesc(CONVT_FWD, 3, 2, 128, 32, BF16)
    lo, hi = _t(X, 128, (32, 32, 32)), _t(Y, 32, (64, 64, 64))
    assert _route(lib, dsc, lo, hi) == _config(lib, dsc, lo, hi) == 15
    seen.add(15)

    # 16: the input gradient of a 32 -> 3 1x1x1 head; x = dy has 3 channels, y = dx has 32
    for dtype in (F32, BF16):                      # K = 3 < 16: fp32 operands whatever desc.dtype says
        dsc = ConvDesc(CONV_DGRAD, 1, 1, 32, 3, dtype)
        dy, dx = _t(X, 3, (8, 8, 8)), _t(Y, 32, (8, 8, 8))
        assert _config(lib, dsc, dy, dx) == 0      # the fp32 igemm of the shape, tile <1,4,8,8,8,8>
        assert _route(lib, dsc, dy, dx) == 16
        assert _route(lib, dsc, dy, _t(Y, 32, (8, 8, 8), BF16)) == 16, "dx may be a bf16-stored gradient"
        assert _route(lib, dsc, dy, dx, stats=STATS) == 0
        assert _route(lib, dsc, dy, dx, add=_t(A, 32, (8, 8, 8))) == 0
        assert _route(lib, dsc, dy, dx, norm=NormOnLoad(mean=1 << 21, rstd=1 << 22)) == 0
        assert _route(lib, dsc, _t(X + 4, 3, (8, 8, 8)), dx) == 0, "dy off its 16-byte rows"
    seen.add(16)

    # 17: a bf16 64 -> 32 1x1x1 forward on voxel-dense tensors at 16^3, bf16- or fp32-stored
    dsc, e16, e8 = ConvDesc(CONV_FWD, 1, 1, 64, 32, BF16), (16, 16, 16), (8, 8, 8)
    for st in (BF16, F32):
        x, y = _t(X, 64, e16, st), _t(Y, 32, e16, st)
        assert _config(lib, dsc, x, y) == 14       # the lean bf16 igemm of the shape
        assert _route(lib, dsc, x, y) == 17
        assert _route(lib, dsc, x, y, add=_t(A, 32, e16, st)) == 17
        assert _route(lib, dsc, x, y, accumulate=1) == 17
        assert _route(lib, dsc, _t(X, 64, e8, st), _t(Y, 32, e8, st)) == 14, "d * h * w < 4096"
        assert _route(lib, dsc, x, y, stats=STATS) == 14
        assert _route(lib, dsc, x, y, norm=NormOnLoad(scale=1 << 21, shift=1 << 22)) == 14
        assert _route(lib, dsc, _t(X, 64, e16, st, row_pad=1), y) == 14, "ragged voxel row: no 16-byte items"
        assert _route(lib, dsc, x, _t(Y, 32, e16, st, gap=32)) == 14, "a gap between x-rows: not voxel-dense"
        assert _route(lib, dsc, x, y, add=_t(A, 32, e16, BF16 + F32 - st)) == 14, "add in the other storage type"
        assert _route(lib, dsc, x, _t(Y, 32, e16, BF16 + F32 - st)) == 14, "x and y in different storage types"
    assert _route(lib, ConvDesc(CONV_FWD, 1, 1, 64, 32, F32), _t(X, 64, e16), _t(Y, 32, e16)) == 0, "fp32 operands"
    seen.add(17)
    assert seen == set(range(18)), f"routes never asked for: {sorted(set(range(18)) - seen)}"
    assert 0 in thin_seen and any(1 <= k <= 10 for k in thin_seen) and any(k >= 11 for k in thin_seen), thin_seen
    # routes 16 and 17 are none of its kernels; argument errors come back as they do from mmtta_conv_route
    assert _thin_kernel(lib, ConvDesc(CONV_DGRAD, 1, 1, 32, 3, F32), _t(X, 3, (8, 8, 8)), _t(Y, 32, (8, 8, 8))) == 0
    assert _thin_kernel(lib, dsc, _t(X, 64, e16, BF16), _t(Y, 32, e16, BF16)) == 0
    assert _thin_kernel(lib, ConvDesc(CONV_FWD, 5, 1, 32, 32, F32), _t(X, 32, e8), _t(Y, 32, e8)) == -2
    assert _thin_kernel(lib, ConvDesc(CONV_FWD, 3, 1, 32, 32, F32), _t(X, 16, e8), _t(Y, 32, e8)) == -1
    # argument errors come back as negative status codes, as from mmtta_conv_wgrad_kernel
    assert _route(lib, ConvDesc(CONV_FWD, 5, 1, 32, 32, F32), _t(X, 32, e8), _t(Y, 32, e8)) == -2
    assert _route(lib, ConvDesc(CONV_FWD, 3, 1, 32, 32, F32), _t(X, 16, e8), _t(Y, 32, e8)) == -1


def test_streaming_pointwise_switch_is_read_from_the_environment():
    """MMTTA_POINTWISE_MFMA=0 (read once per process: a fresh child) sends route 17's calls to the implicit GEMM."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import ctypes as C\n"
            "from multimodal_tta_amd import _lib\n"
            "T = lambda base, c: _lib.Tensor(base, 1, c, 16, 16, 16, 4096 * c, 1, 256 * c, 16 * c, c, _lib.BF16, 0)\n"
            "d, x, y = _lib.ConvDesc(_lib.CONV_FWD, 1, 1, 64, 32, _lib.BF16), T(1 << 30, 64), T(1 << 40, 32)\n"
            "print(_lib.load().mmtta_conv_route(C.byref(d), C.byref(x), None, None, C.byref(y), 0, None))\n")
    env = dict(os.environ, MMTTA_POINTWISE_MFMA="0")          # (unset: 17, asserted in-process by the test above)
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, check=True)
    assert out.stdout.split()[-1] == "14", (out.stdout, out.stderr)
