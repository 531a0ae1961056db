"""BNM adaptation (``bnm_tta``, ``method=tta_bnm``): the host-side half, no GPU needed.

The symbols are declared, exported and typed; ``mmtta_nuclear_entropy_items`` refuses every bad argument with MMTTA_ERR_INVALID
(or _UNSUPPORTED) and a message naming it before anything reaches the device; the plugin is registered, its config composes
and every bad value raises a ValueError naming its key; the float64 restatement the GPU tests compare against
(``nuclear_reference.py``) has the gradient torch autograd gives its loss and the values worked out by hand; and the distance
of an fp32 run of that restatement from the float64 run - the figure the GPU tolerances are multiples of - is measured on the
GPU cases' inputs."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest

from nuclear_reference import boxes, nuclear, nuclear_torch

INVALID, UNSUPPORTED = -1, -2
FAKE = 4096          # 16-byte aligned addresses that are never dereferenced: the checks fail first
STEP = 1 << 28       # distance between the fake buffers: far more than any tensor below spans
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-4           # the GPU cases' smoothing: fp32's distance grows like 1 / sqrt(eps) on rank-deficient boxes


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from multimodal_tta_amd import _lib
    return _lib, _lib.load()


# ----------------------------------------------------------------------------- the inputs of the GPU cases, and fp32's distance
N = 2          # different volumes per case


@functools.lru_cache(maxsize=None)
def inputs(shape, R, seed):
    """Logits ~ N(0, 3^2) of N different volumes, fp32.  ``test_hip_nuclear.py`` draws its cases from here."""
    rng = np.random.default_rng(seed)
    l = rng.normal(0.0, 3.0, (N,) + tuple(shape) + (R,)).astype(np.float32)
    l.setflags(write=False)
    return l


def case_seed(shape, R):
    return 1000 * R + sum(shape)


def gpu_case_table():
    """(shape, block, softmax, R, dlogits bf16, entropy_weight, weight, ldc) of the GPU cases: every head and route - sigmoid
    R in {1, 3, 4} with fp32 and bf16 gradients, softmax R in {3, 4}, the generic route with R = 5 on both heads and with
    R = 3 in rows of 3 floats - against every block, with the shapes, the two entropy weights and the two weights cycling
    at co-prime periods; then the two shapes that need a block of their own, and R = 16."""
    heads = [(False, 1, False, None), (False, 3, True, None), (False, 4, False, None), (False, 4, True, None),
             (False, 3, False, None), (False, 1, True, None), (True, 3, False, None), (True, 4, False, None),
             (False, 5, False, None), (True, 5, False, None), (False, 3, False, 3), (True, 3, False, 3)]
    blocks = [(4, 4, 8), (2, 3, 5), (0, 0, 0), (1, 1, 1), (0, 4, 0)]
    shapes = [(5, 9, 33), (1, 5, 70), (3, 17, 4)]
    out = []
    i = 0
    for softmax, R, gbf, ldc in heads:
        for block in blocks:
            out.append((shapes[i % 3], block, softmax, R, gbf, (1.0, 0.0)[(i // 2) % 2], (1.0, 2.5)[(i // 3) % 2], ldc))
            i += 1
    for softmax, R, gbf, ldc in heads:
        # several workgroups per box; a one-voxel corner box (m < K on the softmax head)
        out.append(((16, 16, 32), (16, 16, 16), softmax, R, gbf, (1.0, 0.0)[i % 2], (1.0, 2.5)[(i // 2) % 2], ldc))
        out.append(((3, 3, 3), (2, 2, 2), softmax, R, gbf, (0.0, 1.0)[i % 2], (2.5, 1.0)[(i // 2) % 2], ldc))
        i += 1
    # the most classes the entry point takes: 137 sums per partial row, a 16 x 16 eigenproblem
    out.append(((3, 17, 4), (2, 3, 5), True, 16, False, 1.0, 1.0, None))
    out.append(((1, 5, 70), (0, 0, 0), True, 16, False, 0.0, 2.5, None))
    out.append(((5, 9, 33), (0, 0, 0), False, 16, False, 1.0, 2.5, None))
    return out


def case_id(case):
    shape, block, softmax, R, gbf, ew, w, ldc = case
    return "-".join(["x".join(map(str, shape)), "b" + "x".join(map(str, block)), "softmax" if softmax else "sigmoid", f"R{R}",
                     "bf16" if gbf else "fp32", f"ew{ew:g}", f"w{w:g}"] + ([f"ldc{ldc}"] if ldc else []))


def fp32_distance(l, block, weight, entropy_weight, softmax):
    """(gradient, H, N): max-norm of the gradient error over max |gradient|, relative error of H and of N, of the fp32 run of
    the restatement against its float64 run on one item."""
    r64 = nuclear(l, block, weight, entropy_weight, EPS, softmax)
    r32 = nuclear(l, block, weight, entropy_weight, EPS, softmax, dtype=np.float32)
    assert r32["dlogits"].dtype == np.float32
    g = np.abs(r32["dlogits"].astype(np.float64) - r64["dlogits"]).max() / np.abs(r64["dlogits"]).max()
    rel = lambda a, b: abs(a - b) / abs(b) if b != 0 else abs(a - b)
    return float(g), rel(r32["H"], r64["H"]), rel(r32["N"], r64["N"])


# The distances measured by test_fp32_arithmetic_of_the_restatement: the worst over the inputs of every GPU case.  The GPU
# tests' tolerances are 4 x FP32_GRADIENT for fp32 gradients (another summation order, the hardware exponential) and 1e-5
# relative for the sums (the figure of the project's DiceCE sums test).  The host test asserts that the constants bound what
# it measures and sit within a factor 1.25 of it.
FP32_GRADIENT = 1.0e-5
FP32_LOSS = 1.3e-7


def test_the_cases_cover_what_they_should():
    cases = gpu_case_table()
    assert {c[1] for c in cases} == {(4, 4, 8), (2, 3, 5), (0, 0, 0), (1, 1, 1), (0, 4, 0), (16, 16, 16), (2, 2, 2)}
    assert {c[0] for c in cases} == {(5, 9, 33), (1, 5, 70), (3, 17, 4), (16, 16, 32), (3, 3, 3)}
    assert ((5, 9, 33), (4, 4, 8)) in {(c[0], c[1]) for c in cases}          # ragged in every axis
    for softmax, Rs in ((False, {1, 3, 4, 5, 16}), (True, {3, 4, 5, 16})):
        mine = [c for c in cases if c[2] == softmax]
        assert {c[3] for c in mine} == Rs
        assert {c[5] for c in mine} == {0.0, 1.0} and {c[6] for c in mine} == {1.0, 2.5}
        assert {c[1] for c in mine if c[3] == 5} >= {(4, 4, 8), (0, 0, 0), (1, 1, 1), (2, 2, 2), (16, 16, 16)}
        assert {c[1] for c in mine if c[7] == 3} >= {(4, 4, 8), (0, 0, 0), (1, 1, 1)}
    assert {c[3] for c in cases if c[4]} == {1, 3, 4} and not any(c[4] for c in cases if c[2])


def test_fp32_arithmetic_of_the_restatement():
    """Measured on exactly the inputs of the GPU cases (every case of the table, both items): the fp32 run of the restatement
    against the float64 run.  Printed; the constants above must bound the figures, closely."""
    worst_g, worst_l = 0.0, 0.0
    for shape, block, softmax, R, _, ew, w, _ in gpu_case_table():
        l = inputs(shape, R, case_seed(shape, R))
        for n in range(N):
            g, h, nn = fp32_distance(l[n], block, w, ew, softmax)
            worst_g, worst_l = max(worst_g, g), max(worst_l, h, nn)
    print(f"fp32 restatement: gradient {worst_g:.3e} of its maximum, H / N {worst_l:.3e} relative")
    assert FP32_GRADIENT / 1.25 <= worst_g <= FP32_GRADIENT, worst_g
    assert FP32_LOSS / 1.25 <= worst_l <= FP32_LOSS, worst_l


# ----------------------------------------------------------------------------- the restatement against autograd, and by hand
@pytest.mark.parametrize("softmax", [False, True], ids=["sigmoid", "softmax"])
@pytest.mark.parametrize("block", [(4, 4, 8), (2, 3, 5), (0, 0, 0), (1, 1, 1)], ids=lambda b: "x".join(map(str, b)))
@pytest.mark.parametrize("entropy_weight", [0.0, 1.0])
def test_the_analytic_gradient_is_autograds(entropy_weight, block, softmax):
    import torch
    rng = np.random.default_rng(3)
    l = rng.normal(0.0, 3.0, (5, 9, 17, 3))
    for weight in (1.0, 2.5):
        ref = nuclear(l, block, weight, entropy_weight, EPS, softmax)
        lt = torch.tensor(l, dtype=torch.float64, requires_grad=True)
        L, H, Nn = nuclear_torch(lt, block, weight, entropy_weight, EPS, softmax)
        L.backward()
        g = lt.grad.numpy()
        L, H, Nn = L.item(), H.item(), Nn.item()
        assert abs(ref["H"] - H) <= 1e-12 * abs(H) and abs(ref["N"] - Nn) <= 1e-12 * abs(Nn)
        assert abs(ref["L"] - L) <= 1e-12 * abs(L)
        err = np.abs(ref["dlogits"] - g).max() / np.abs(g).max()
        assert err <= 1e-10, err
        assert 0.0 < Nn <= 1.0 + 1e-3


def test_boxes_start_at_multiples_and_border_boxes_are_smaller():
    bx = boxes((5, 9, 33), (4, 4, 8))
    assert len(bx) == 2 * 3 * 5
    assert bx[0] == (slice(0, 4), slice(0, 4), slice(0, 8)) and bx[-1] == (slice(4, 5), slice(8, 9), slice(32, 33))
    assert boxes((5, 9, 33), (0, 4, 64)) == [(slice(0, 5), slice(s, min(s + 4, 9)), slice(0, 33)) for s in (0, 4, 8)]
    assert sum((s[0].stop - s[0].start) * (s[1].stop - s[1].start) * (s[2].stop - s[2].start) for s in bx) == 5 * 9 * 33


def test_restatement_by_hand_on_two_voxels():
    """Two voxels, R = 1, one box: A = [[pa, 1 - pa], [pb, 1 - pb]], the eigenvalues of the 2 x 2 Gram matrix in closed form."""
    la, lb = 0.7, -1.3
    l = np.array([la, lb]).reshape(1, 1, 2, 1)
    pa, pb = 1 / (1 + math.exp(-la)), 1 / (1 + math.exp(-lb))
    a, o, d = pa * pa + pb * pb, pa * (1 - pa) + pb * (1 - pb), (1 - pa) ** 2 + (1 - pb) ** 2
    root = math.sqrt(((a - d) / 2) ** 2 + o * o)
    l1, l2 = (a + d) / 2 + root, (a + d) / 2 - root
    m, K = 2, 2
    nu = (math.sqrt(l1 + EPS * m) + math.sqrt(l2 + EPS * m)) / math.sqrt(m * min(m, K))
    hb = lambda p: -p * math.log(p) - (1 - p) * math.log(1 - p)
    r = nuclear(l, (0, 0, 0), 2.0, 1.0, EPS, False)
    assert abs(r["N"] - nu) < 1e-14 and abs(nu - 0.7295478695932511) < 1e-14
    assert abs(r["H"] - (hb(pa) + hb(pb)) / 2) < 1e-15 and abs(r["L"] - (r["H"] - 2.0 * nu)) < 1e-15
    # the same two voxels as two boxes of one voxel: m = 1, min(m, K) = 1, the one eigenvalue is p^2 + (1 - p)^2
    r = nuclear(l, (1, 1, 1), 1.0, 0.0, EPS, False)
    one = lambda p: math.sqrt(p * p + (1 - p) ** 2 + EPS) + math.sqrt(EPS)
    assert abs(r["N"] - (one(pa) + one(pb)) / 2) < 1e-14 and abs(r["L"] + r["N"]) < 1e-15


@pytest.mark.parametrize("softmax", [False, True], ids=["sigmoid", "softmax"])
def test_one_hot_balanced_rows_reach_one_and_a_constant_box_has_rank_one(softmax):
    R = 4
    eps = 1e-6
    # voxel i is (almost) one-hot in class i % R: balanced classes, nu -> 1 (up to the smoothing)
    l = np.full((4, 4, 8, R), -40.0)
    idx = np.arange(4 * 4 * 8).reshape(4, 4, 8)
    if softmax:
        np.put_along_axis(l, (idx % R)[..., None], 40.0, -1)
    else:
        l = np.where((idx % 2)[..., None] == 0, 40.0, -40.0) * np.ones(R)          # every region: half 1, half 0
    r = nuclear(l, (0, 0, 0), 1.0, 0.0, eps, softmax)
    K = R if softmax else 2
    assert abs(r["N"] - math.sqrt(1.0 / K + eps) * K / math.sqrt(K)) < 1e-9 and abs(r["N"] - 1.0) < 1e-5
    # every voxel the same row: rank 1, one singular value sqrt(m |p|^2), nu = (|p| + (K - 1) sqrt(eps)) / sqrt(K) - far from 1
    row = np.array([0.8, -1.7, 2.9, 0.3])
    l = np.broadcast_to(row, (4, 4, 8, R)).copy()
    r = nuclear(l, (0, 0, 0), 1.0, 0.0, eps, softmax)
    if softmax:
        p = np.exp(row) / np.exp(row).sum()
        want = (math.sqrt((p * p).sum() + eps) + (K - 1) * math.sqrt(eps)) / math.sqrt(K)
    else:
        p = 1 / (1 + np.exp(-row))
        want = np.mean([(math.sqrt(q * q + (1 - q) ** 2 + eps) + math.sqrt(eps)) / math.sqrt(2) for q in p])
    assert abs(r["N"] - want) < 1e-8, (r["N"], want)


# ----------------------------------------------------------------------------- the entry point
def test_the_nuclear_symbols_are_declared_exported_and_typed():
    _l, lib = _lib()
    header = open(os.path.join(ROOT, "include", "mmtta.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+mmtta_nuclear_entropy_items\s*\(", code) and re.search(r"\bint64_t\s+mmtta_nuclear_scratch\s*\(", code)
    assert {"mmtta_nuclear_entropy_items", "mmtta_nuclear_scratch"} <= set(_l.exported_names())
    assert ctypes.CDLL(_l.LIB_PATH).mmtta_nuclear_entropy_items is not None          # AttributeError: not exported
    assert len(lib.mmtta_nuclear_entropy_items.argtypes) == 14 and lib.mmtta_nuclear_entropy_items.restype is ctypes.c_int
    assert len(lib.mmtta_nuclear_scratch.argtypes) == 5 and lib.mmtta_nuclear_scratch.restype is ctypes.c_int64
    assert lib.mmtta_abi_version() == 2


def _tensor(_l, slot=0, n=2, c=3, d=4, h=5, w=6, ptr=True, dtype=None, ldc=4, flags=None):
    return _l.Tensor((FAKE + slot * STEP) if ptr is True else ptr, n, c, d, h, w, d * h * w * ldc, 1, h * w * ldc, w * ldc, ldc,
                     _l.F32 if dtype is None else dtype, _l.TENSOR_OWNS_PAD if flags is None else flags)


def _call(lib, _l, l=None, dl=None, softmax=0, block=(0, 0, 0), entropy_weight=1.0, weight=1.0, eps=1e-4, **ptrs):
    l = _tensor(_l, 0) if l is None else l
    dl = _tensor(_l, 2) if dl is None else dl
    ref = lambda t, name: None if ptrs.get(name) else ctypes.byref(t)
    slot = lambda name, k: None if ptrs.get(name) else FAKE + k * STEP
    return lib.mmtta_nuclear_entropy_items(ref(l, "no_l"), softmax, block[0], block[1], block[2], entropy_weight, weight, eps,
                                           ref(dl, "no_dl"), slot("no_scratch", 5), slot("no_loss", 6), slot("no_entropy", 7),
                                           slot("no_nuclear", 8), None)


def _err(lib):
    return lib.mmtta_last_error()


def test_nuclear_scratch_counts_partial_rows_values_and_coefficients():
    _l, lib = _lib()
    t = _tensor(_l, 0, n=3, c=3, d=5, h=9, w=33)
    scratch = lambda softmax, *b: lib.mmtta_nuclear_scratch(ctypes.byref(t), softmax, *b)
    # sigmoid head, one box of 1485 voxels: 2 chunks of 1024 voxels x (3 R + 1) sums, R values, 1 entropy sum, 2 R floats
    assert scratch(0, 0, 0, 0) == 3 * (2 * 10 + 3 + 1 + 3)
    assert scratch(0, 5, 9, 33) == scratch(0, 0, 0, 0) == scratch(0, 64, 64, 64)
    # 2 x 3 x 5 boxes of one chunk each; softmax head: R (R + 1) / 2 + 1 sums, one value, R * R floats (9 -> 5 doubles per 30 boxes: 135)
    assert scratch(0, 4, 4, 8) == 3 * (30 * 10 + 90 + 30 + 90)
    assert scratch(1, 4, 4, 8) == 3 * (30 * 7 + 30 + 30 + 135)
    assert lib.mmtta_nuclear_scratch(None, 0, 0, 0, 0) == -1
    assert scratch(0, -1, 0, 0) == -1 and scratch(0, 0, 0, -4) == -1
    wide = _tensor(_l, 0, c=17, ldc=20)
    assert lib.mmtta_nuclear_scratch(ctypes.byref(wide), 0, 0, 0, 0) == -1


def test_nuclear_entropy_rejects_null_pointers_without_a_gpu():
    _l, lib = _lib()
    for kw, word in (({"no_l": True}, b"logits"), ({"l": _tensor(_l, 0, ptr=None)}, b"logits"),
                     ({"no_dl": True}, b"dlogits"), ({"dl": _tensor(_l, 2, ptr=None)}, b"dlogits"),
                     ({"no_scratch": True}, b"scratch"), ({"no_loss": True}, b"loss"), ({"no_entropy": True}, b"entropy"),
                     ({"no_nuclear": True}, b"`nuclear`")):
        assert _call(lib, _l, **kw) == INVALID, kw
        assert b"null" in _err(lib) and word in _err(lib), (kw, _err(lib))


def test_nuclear_entropy_rejects_bad_scalars_without_a_gpu():
    _l, lib = _lib()
    for block in ((-1, 0, 0), (0, -2, 0), (4, 4, -8)):
        assert _call(lib, _l, block=block) == INVALID
        assert b"block" in _err(lib)
    for weight in (0.0, -1.0, 16.5, float("nan"), float("inf"), float("-inf")):
        assert _call(lib, _l, weight=weight) == INVALID
        assert b" weight" in _err(lib) and b"entropy_weight" not in _err(lib)
    for ew in (-0.5, 16.5, float("nan"), float("inf"), float("-inf")):
        assert _call(lib, _l, entropy_weight=ew) == INVALID
        assert b"entropy_weight" in _err(lib)
    for eps in (0.0, 1e-7, 0.2, -1e-4, float("nan"), float("inf")):
        assert _call(lib, _l, eps=eps) == INVALID
        assert b"eps" in _err(lib)
    # the ends of the ranges pass these checks (the aliasing check comes later)
    for kw in (dict(weight=16.0), dict(entropy_weight=0.0), dict(entropy_weight=16.0), dict(eps=1e-6), dict(eps=0.1)):
        assert _call(lib, _l, dl=_tensor(_l, 0), **kw) == INVALID and b"aliased" in _err(lib), kw


def test_nuclear_entropy_rejects_mismatched_and_aliased_tensors_without_a_gpu():
    _l, lib = _lib()
    for bad in (dict(n=3), dict(c=2), dict(d=8), dict(h=2), dict(w=8)):
        assert _call(lib, _l, dl=_tensor(_l, 2, **bad)) == INVALID
        assert b"shape mismatch" in _err(lib) and b"dlogits" in _err(lib)
    assert _call(lib, _l, dl=_tensor(_l, 2, ldc=8)) == INVALID
    assert b"row width" in _err(lib)
    # aliased: equal, and overlapping without being equal
    for kw in ({"dl": _tensor(_l, 0)}, {"dl": _tensor(_l, 0, ptr=FAKE + 16 * 7)}):
        assert _call(lib, _l, **kw) == INVALID, kw
        assert b"aliased" in _err(lib) and b"logits" in _err(lib)


def test_nuclear_entropy_refuses_what_it_has_no_kernel_for_without_a_gpu():
    _l, lib = _lib()
    wide = dict(c=17, ldc=20)
    assert _call(lib, _l, l=_tensor(_l, 0, **wide), dl=_tensor(_l, 2, **wide)) == UNSUPPORTED
    assert b"regions" in _err(lib)
    assert _call(lib, _l, l=_tensor(_l, 0, dtype=_l.BF16)) == UNSUPPORTED
    assert b"fp32" in _err(lib)
    # bf16 gradients: the sigmoid head on the fast route alone
    assert _call(lib, _l, dl=_tensor(_l, 2, dtype=_l.BF16), softmax=1) == UNSUPPORTED
    assert b"bf16" in _err(lib)
    five = dict(c=5, ldc=8)
    assert _call(lib, _l, l=_tensor(_l, 0, **five), dl=_tensor(_l, 2, dtype=_l.BF16, **five)) == UNSUPPORTED
    assert b"bf16" in _err(lib)
    # not channels-last: a channel stride other than 1
    t = _tensor(_l, 0)
    t.sc = 2
    assert _call(lib, _l, l=t) == UNSUPPORTED
    assert b"channels-last" in _err(lib)
    big = dict(n=1, d=1024, h=1024, w=512)          # 2^29 voxels x 4 floats = 2^31 elements in one item
    far = lambda slot: _tensor(_l, ptr=FAKE + slot * (1 << 40), **big)
    assert _call(lib, _l, l=far(0), dl=far(1)) == UNSUPPORTED
    assert b"2^31" in _err(lib) and b"item" in _err(lib)
    many = dict(n=65536, d=1, h=1, w=1)
    assert _call(lib, _l, l=_tensor(_l, 0, **many), dl=_tensor(_l, 2, **many)) == UNSUPPORTED
    assert b"items" in _err(lib)
    # boxes of one voxel over 60000 items of 4096 voxels: 60000 x 4096 x (10 + 3 + 1 + 3) doubles
    lots = dict(n=60000, d=16, h=16, w=16)
    spread = lambda slot: _tensor(_l, ptr=FAKE + slot * (1 << 40), **lots)
    assert _call(lib, _l, l=spread(0), dl=spread(1), block=(1, 1, 1)) == UNSUPPORTED
    assert b"scratch" in _err(lib)


def test_ops_nuclear_entropy_items_checks_its_arguments_before_the_library():
    import torch
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.ops import MmttaError
    z = torch.zeros(1, 2, 2, 2, 3)
    one, scr = torch.zeros(1), torch.zeros(64, dtype=torch.float64)          # (the scratch is checked last, on the device)
    for block in ([0, 0], [0, 0, -1], [1.0, 1, 1], [True, 1, 1], "444", None):
        with pytest.raises(MmttaError, match="block"):
            ops.nuclear_entropy_items(z, z.clone(), scr, one, one, one, block=block, weight=1.0)
        with pytest.raises(MmttaError, match="block"):
            ops.nuclear_scratch(z, block)
    with pytest.raises(MmttaError, match="nuclear must"):
        ops.nuclear_entropy_items(z, z.clone(), scr, one, one, torch.zeros(1, dtype=torch.float64), block=[0, 0, 0], weight=1.0)
    with pytest.raises(MmttaError, match="entropy must"):
        ops.nuclear_entropy_items(z, z.clone(), scr, one, torch.zeros(0), one, block=[0, 0, 0], weight=1.0)


# ----------------------------------------------------------------------------- plugin and config
def _cfg(*extra):
    from multimodal_tta_amd.config import compose
    return compose(overrides=["task=brats", "model=unet", "method=tta_bnm", *extra])


def test_bnm_tta_is_registered_and_its_config_composes():
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin, list_plugins
    from multimodal_tta_amd.tta import EntropyMinimizationTTA
    assert "bnm_tta" in list_plugins()
    assert compose(overrides=["method=tta_bnm"])["method"]["name"] == "bnm_tta"
    cfg = _cfg()
    assert cfg["method"]["name"] == "bnm_tta" and cfg["method"]["kind"] == "tta"
    assert dict(cfg["method"]["bnm"]) == {"weight": 1.0, "entropy_weight": 1.0, "block": [0, 0, 0], "eps": 1e-4}
    plug = get_plugin("bnm_tta")(cfg)
    assert isinstance(plug, EntropyMinimizationTTA) and type(plug).__name__ == "NuclearNormTTA"
    assert (plug.weight, plug.entropy_weight, plug.block, plug.eps) == (1.0, 1.0, [0, 0, 0], 1e-4)
    assert plug.fused_update is True and plug.views == 1
    assert [r[0] for r in plug.records] == ["losses", "entropy", "nuclear"]
    plug = get_plugin("bnm_tta")(_cfg("method.bnm.weight=16", "method.bnm.entropy_weight=0", "method.bnm.block=[16,16,16]",
                                      "method.bnm.eps=0.1"))
    assert (plug.weight, plug.entropy_weight, plug.block, plug.eps) == (16.0, 0.0, [16, 16, 16], 0.1)
    # the block is optional: the defaults are the yaml's
    cfg = _cfg()
    del cfg["method"]["bnm"]
    plug = get_plugin("bnm_tta")(cfg)
    assert (plug.weight, plug.entropy_weight, plug.block, plug.eps) == (1.0, 1.0, [0, 0, 0], 1e-4)


def test_weight_zero_constructs_and_records_the_entropy_as_the_loss():
    from multimodal_tta_amd.registry import get_plugin
    plug = get_plugin("bnm_tta")(_cfg("method.bnm.weight=0"))
    assert plug.weight == 0.0
    rec = {key: buf for key, buf, _ in plug.records}
    assert rec["losses"] == rec["entropy"] == "ent_loss" and rec["nuclear"] != "ent_loss"
    for ew in (0.0, 0.5, 2):
        cfg = _cfg("method.bnm.weight=0")
        cfg["method"]["bnm"]["entropy_weight"] = ew
        with pytest.raises(ValueError, match="method.bnm.entropy_weight "):
            get_plugin("bnm_tta")(cfg)


def test_tta_bnm_carries_every_key_of_tta_entmin():
    from multimodal_tta_amd.config import compose
    ent = compose(overrides=["task=brats", "model=unet", "method=tta_entmin"])["method"]
    bnm_m = _cfg()["method"]
    assert set(bnm_m) == set(ent) | {"bnm"}
    for k in ent:
        if k != "name":
            assert bnm_m[k] == ent[k], k


@pytest.mark.parametrize("key,value", [
    ("weight", -1.0), ("weight", 16.5), ("weight", float("nan")), ("weight", float("inf")), ("weight", True), ("weight", "1"),
    ("entropy_weight", -0.1), ("entropy_weight", 16.5), ("entropy_weight", float("nan")), ("entropy_weight", float("inf")),
    ("entropy_weight", False), ("entropy_weight", "1"),
    ("block", [0, 0]), ("block", [0, 0, 0, 0]), ("block", [4, -1, 4]), ("block", [4.0, 4, 4]), ("block", [True, 4, 4]),
    ("block", "16"), ("block", 16), ("block", ["4", "4", "4"]),
    ("eps", 0.0), ("eps", 1e-7), ("eps", 0.2), ("eps", float("nan")), ("eps", True), ("eps", "1e-4")])
def test_bnm_plugin_rejects_bad_hyper_parameters(key, value):
    from multimodal_tta_amd.registry import get_plugin
    cfg = _cfg()
    cfg["method"]["bnm"][key] = value
    with pytest.raises(ValueError, match=f"method.bnm.{key} "):
        get_plugin("bnm_tta")(cfg)
