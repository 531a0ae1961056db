"""Case table, float64 references and derived bounds of the kernels of csrc/pointwise.hip, one case per dispatch class.

Used by tests/test_pointwise_classes_host.py (no GPU: routes, conditions, coverage) and tests/test_hip_pointwise_classes.py
(the launches).  Nothing here touches the GPU.

Operands.  Every operand is a float64 numpy array [N, D, H, W, C] whose values are exactly representable in the storage
type the kernel reads (fp32 or bf16), so the reference and the kernel see the same numbers.  A `Lay` says where the view
sits in its buffer (row stride, channel offset, W window / step); the same Lay builds the host-only descriptor of the
route query and the device tensor.

Bounds (u = 2^-24; DESIGN.md, "Pointwise parity per dispatch class"):
  sums          |err| <= L * u * sum|term|,  L = trips per lane + lane partials (nvl) + 2 (the product and its conversion)
  finalize      the sum bounds pushed through the finalize formula, plus one fp32 rounding of the stored result
  elementwise   |err_i| <= r * u * (sum of |terms| of the reference expression at i); bf16-stored results add 2^-8 |ref_i|
The r of every op is in R below with its count.  Elements of a ReLU / LeakyReLU backward with |z_ref| < Z_NEAR are left out
of the elementwise comparison and their |dout|, |dout * xhat| are added to the two sum bounds.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from multimodal_tta_amd import _lib, ops

U = 2.0 ** -24
BF_ULP = 2.0 ** -8
Z_NEAR = 1e-4
NEAR_CAP = 1e-3          # share of a case's elements that may sit on the activation's kink
EPS = float(np.float32(1e-5))
SLOPE = float(np.float32(0.2))
MOMENTUM = 0.125

# fp32 roundings on the kernel's path, per element (an fma counts as one; a contraction only removes roundings)
R = {
    # sc = rs*g (1), mu*sc (1), b - . (1), fma(x, sc, sh) (1); LeakyReLU's k*v (1)
    "combine1": 5,
    # two sources: the above on each source's own terms, and the add (1)
    "combine2": 6,
    # y - mu (1), * rs (1), g*dz (1), - m1 (1), xhat*m2 (1), - (1), rs * (1); LeakyReLU's dz*k (1)
    "apply": 8,
    # the apply path; m1 / m2 carry the sum bound of their own (added separately)
    "small": 8,
    # fma per input (COUNT), the prefill of accumulate is exact: r = COUNT
    "lincomb": None,
    # 1 - lam (1) per axis, then three nested lerps of mul, mul, add (3 each), weights' own rounding (1)
    "upsample_fwd": 11,
    # w = wz*wy*wx (2) and its factors (1), one fma per gathered output (<= 125), the add of accumulate (1)
    "upsample_bwd": None,
}


# ----------------------------------------------------------------------------- values
def rbf(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.bfloat16).double().numpy()


def rf32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def stored(a, bf):
    return rbf(a) if bf else rf32(a)


def away_from_zero(rng, shape, offset=0.0):
    """randn pushed out of (-0.5, 0.5): one dropped voxel always moves a sum by >= 0.5."""
    x = rng.standard_normal(shape)
    return x + 0.5 * np.sign(x) + offset


# ----------------------------------------------------------------------------- layouts
@dataclass(frozen=True)
class Lay:
    ldc: int = 0        # row stride in elements (0: C, a tight row)
    c_off: int = 0      # first channel of the view inside the row
    w_buf: int = 0      # W extent of the buffer (0: the view's)
    w_off: int = 0
    w_step: int = 1
    own: bool = False   # the view owns the pad lanes of its rows (ops.new_cl)

    def geometry(self, shape):
        n, c, d, h, w = shape
        ldc = self.ldc or c
        wb = self.w_buf or w
        assert self.c_off + c <= ldc and self.w_off + (w - 1) * self.w_step < wb
        return ldc, wb

    def index(self, shape):
        n, c, d, h, w = shape
        return (slice(None), slice(None), slice(None), slice(self.w_off, self.w_off + (w - 1) * self.w_step + 1, self.w_step),
                slice(self.c_off, self.c_off + c))


TIGHT = Lay()


def pad4(c):
    return Lay(ldc=(c + 3) // 4 * 4, own=True)


def pad8(c):
    return Lay(ldc=(c + 7) // 8 * 8, own=True)


def host_desc(shape, lay: Lay, bf: bool, slot: int):
    """Descriptor with a made-up, 4 KiB aligned base address: the route query reads addresses for alignment only."""
    n, c, d, h, w = shape
    ldc, wb = lay.geometry(shape)
    es = 2 if bf else 4
    base = ((slot + 1) << 28) + (lay.w_off * ldc + lay.c_off) * es
    sh = wb * ldc
    return _lib.Tensor(base, n, c, d, h, w, d * h * sh, 1, h * sh, sh, ldc * lay.w_step, _lib.BF16 if bf else _lib.F32,
                       _lib.TENSOR_OWNS_PAD if lay.own else 0)


def owned_mask(shape, lay: Lay):
    """Boolean mask over the buffer [N, D, H, Wbuf, ldc]: the elements a kernel writing this view may change."""
    n, c, d, h, w = shape
    ldc, wb = lay.geometry(shape)
    m = np.zeros((n, d, h, wb, ldc), dtype=bool)
    idx = lay.index(shape)
    m[idx] = True
    if lay.own:
        m[idx[:4] + (slice(lay.c_off + c, ldc),)] = True
    return m


# ----------------------------------------------------------------------------- cases
@dataclass
class Case:
    name: str
    op: str                       # stats | bwd_reduce | stats_chain | bwd_chain | combine | apply | small | lincomb | up_fwd | up_bwd
    shape: Tuple[int, int, int, int, int]          # N, C, D, H, W (upsample: the small tensor)
    want: Dict[str, object]       # route fields the case exists for
    st: Tuple[int, ...] = ()      # bf16 flags, per op (see operands())
    lays: Dict[str, Lay] = field(default_factory=dict)
    act: str = "none"             # none | relu | leaky
    kw: Dict[str, object] = field(default_factory=dict)
    seed: int = 0

    def lay(self, who):
        return self.lays.get(who, self.lays.get("*", TIGHT))


ACT_CODE = {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "leaky": _lib.ACT_LEAKY_RELU}


def act_slope(act):
    return {"none": 1.0, "relu": 0.0, "leaky": SLOPE}[act]


def operand_names(case: Case):
    return {"stats": ["x"], "stats_chain": ["x"], "bwd_reduce": ["dout", "y"], "bwd_chain": ["dout", "y"],
            "apply": ["dout", "y", "dy"], "small": ["dout", "y", "dy"],
            "combine": ["a", "b", "out"] if case.kw.get("two") else ["a", "out"],
            "lincomb": [f"in{k}" for k in range(case.kw.get("count", 0))] + ["out"],
            "up_fwd": ["x", "y"], "up_bwd": ["dy", "dx"]}[case.op]


def operand_shape(case: Case, who):
    n, c, d, h, w = case.shape
    big = (case.op == "up_fwd" and who == "y") or (case.op == "up_bwd" and who == "dy")
    return (n, c, 2 * d, 2 * h, 2 * w) if big else case.shape


def operand_bf(case: Case, who):
    st = case.st
    if case.op in ("stats", "stats_chain"):
        return bool(st[0])
    if case.op in ("bwd_reduce", "bwd_chain"):
        return bool(st[0] if who == "y" else st[1])            # st = (y, dout)
    if case.op in ("apply", "small"):
        return bool(st[1] if who == "y" else st[0])            # st = (dout / dy, y)
    if case.op == "lincomb":
        return bool(st[1] if who == "out" else st[0])          # st = (inputs, out)
    return bool(st[0])                                         # combine, upsample: one storage


ROUTE_OP = {"stats": "channel_stats", "stats_chain": "channel_stats", "bwd_reduce": "norm_bwd_reduce",
            "bwd_chain": "norm_bwd_reduce", "apply": "norm_bwd_apply", "small": "norm_bwd_small", "combine": "combine",
            "lincomb": "lincomb", "up_fwd": "upsample_fwd", "up_bwd": "upsample_bwd"}
# made-up coefficient addresses (16-byte aligned, as torch allocations are)
FAKE = 0x7000000


def _fake_nl(case: Case):
    if case.op in ("stats", "stats_chain", "lincomb", "up_fwd", "up_bwd"):
        return None, None
    mk = lambda: _lib.norm_on_load(act=ACT_CODE[case.act], negative_slope=SLOPE)
    t = mk()
    t.mean, t.rstd, t.gamma, t.beta = FAKE, FAKE + 0x10000, FAKE + 0x20000, FAKE + 0x30000
    t2 = None
    if case.op == "combine" and case.kw.get("two"):
        t2 = _lib.norm_on_load(act=ACT_CODE[case.kw.get("act_b", "none")], negative_slope=SLOPE)
    return t, t2


def host_route(case: Case):
    """The route of the case from made-up addresses (no GPU)."""
    names = operand_names(case)
    descs = [host_desc(operand_shape(case, who), case.lay(who), operand_bf(case, who), i) for i, who in enumerate(names)]
    t, t2 = _fake_nl(case)
    return ops.pointwise_route(ROUTE_OP[case.op], descs, t, t2, FAKE + 0x40000, FAKE + 0x50000)


def check_route(case: Case, route):
    bad = {k: (route[k], v) for k, v in case.want.items() if route[k] != v}
    assert not bad, f"{case.name}: the case no longer reaches its class, (got, wanted) = {bad}\n  route {route}"


def klass(route):
    """The template instantiation a route names (mmtta.h: the comments of MMTTA_PW_*)."""
    f = route["family"]
    keep = {"reduce": ("mode", "vec", "bf16_a", "bf16_b"), "reduce_stream": ("mode", "it", "bf16_a", "bf16_b"),
            "elementwise": ("mode", "vec", "bf16_a", "bf16_b", "bf16_o"), "combine8": ("bf16_a", "has_b", "it"),
            "norm_bwd_apply8": ("bf16_b", "it", "bf16_a"), "norm_bwd_small": ("bf16_b", "bf16_a"),
            "lincomb": ("vec", "count", "bf16_a", "bf16_o"), "upsample_fwd": ("vec", "bf16_a"), "upsample_bwd": ("vec", "bf16_a")}[f]
    return (f,) + tuple(route[k] for k in keep)


def sum_chain(route):
    """L of the sum bound: the longest chain of fp32 additions a partial sum goes through, + 2."""
    if route["family"] == "norm_bwd_small":
        return route["trips"] + 2          # the 64 lane partials are added in fp64
    return route["trips"] + route["nvl"] + 2


def _cases():
    out = []
    add = out.append
    S = "reduce_stream"
    # ---- streamed reduction, both modes.  (name, shape, lay of every operand, route fields)
    stream_geoms = [
        ("it1_c32", (1, 32, 8, 8, 8), None, dict(it=1, rows_per_block=1)),
        ("it2_c64", (1, 64, 8, 8, 8), None, dict(it=2, rows_per_block=1)),
        ("it4_c128", (1, 128, 8, 8, 8), None, dict(it=4, rows_per_block=1)),
        ("rpb4_c4", (5, 4, 33, 32, 31), None, dict(it=1, rows_per_block=4, rows_per_n=1023)),
        ("rpb2_c4", (2, 4, 16, 25, 41), None, dict(it=1, rows_per_block=2, rows_per_n=513)),
        ("c1024", (1, 1024, 4, 4, 5), None, dict(it=4, nvl=1, cpl=256, rows_per_n=3)),
        ("c3_pad", (2, 3, 5, 6, 7), "pad", dict(it=1, cpl=1)),
        ("c33_pad", (1, 33, 5, 6, 7), "pad", dict(cpl=16)),
        ("row_of_1", (2, 8, 1, 1, 1), None, dict(rows_per_n=1, it=1)),
        ("row_of_31", (1, 8, 1, 1, 31), None, dict(rows_per_n=1, it=1)),
        ("short_last_row", (1, 16, 3, 5, 7), None, dict(rows_per_n=4)),      # 105 voxels: 32, 32, 32, 9
        ("n3", (3, 12, 4, 5, 6), None, dict(rows_per_n=4)),
    ]
    storages1 = [(0, 0), (1, 0), (1, 1)]
    acts = ["none", "relu", "leaky"]
    k = 0
    for name, shape, lay, want in stream_geoms:
        for mode in (0, 1):
            for st in ([(0,), (1,)] if mode == 0 else storages1):
                # every geometry in fp32; bf16 storages on the geometries that change the instantiation or the tail
                if any(st) and name not in ("it1_c32", "it2_c64", "it4_c128", "c3_pad", "short_last_row", "c1024", "row_of_31"):
                    continue
                bf_x = bool(st[0])
                lays = {}
                if lay == "pad":
                    lays = {"x": pad8(shape[1]) if bf_x and shape[1] > 4 else pad4(shape[1])}
                    lays["y"] = lays["x"]
                    if mode == 1:
                        bf_d = bool(st[1])
                        lays["dout"] = pad8(shape[1]) if bf_d and shape[1] > 4 else pad4(shape[1])
                act = "none" if mode == 0 else acts[k % 3]
                k += 1
                kw = {"per_item": name == "n3", "affine": name != "row_of_1"} if mode == 1 else {}
                add(Case(f"{'stats' if mode == 0 else 'bwd'}_{name}_{''.join('fb'[s] for s in st)}_{act}",
                         "stats" if mode == 0 else "bwd_reduce", shape,
                         dict(family=S, mode=mode, vec=4, bf16_a=st[0], bf16_b=st[1] if mode else 0, cb_passes=1,
                              leaky=int(act == "leaky"), **want), st, lays, act, kw, seed=100 + k))
    # the thin pair: an fp32 activation next to a bf16 gradient (C <= 4), at every IT (cpl 1: IT follows the row length)
    for name, shape, it in (("it1", (1, 4, 6, 5, 7), 1), ("it2", (1, 3, 66, 64, 64), 2), ("it4", (1, 4, 96, 96, 96), 4)):
        lays = {"*": pad4(shape[1])} if shape[1] % 4 else {}
        add(Case(f"bwd_thin_{name}_fb_relu", "bwd_reduce", shape, dict(family=S, mode=1, it=it, bf16_a=0, bf16_b=1, cpl=1, nvl=256),
                 (0, 1), lays, "relu", {"affine": True}, seed=150 + it))
    # ---- channel_reduce_kernel: what the streamed form does not take
    old_geoms = [
        ("wslice", (2, 8, 3, 4, 5), Lay(w_buf=9, w_off=2), dict(vec=4, cb_passes=1)),
        ("wstride", (1, 4, 3, 4, 5), Lay(w_buf=11, w_step=2), dict(vec=4, cb_passes=1)),
        ("tight3", (2, 3, 4, 5, 7), TIGHT, dict(vec=1, cb_passes=1)),
        ("c1028", (1, 1028, 2, 3, 5), TIGHT, dict(vec=4, cb_passes=2, cpl=256)),
        ("c259", (1, 259, 2, 3, 5), TIGHT, dict(vec=1, cb_passes=2, cpl=256)),
    ]
    for name, shape, lay, want in old_geoms:
        for mode in (0, 1):
            sts = [(0,), (1,)] if mode == 0 else [(0, 0), (1, 0), (1, 1)] + ([(0, 1)] if shape[1] <= 4 else [])
            for st in sts:
                if any(st) and name in ("c1028", "c259"):
                    continue
                if name == "wslice" and mode == 1 and st == (0, 1):
                    continue
                act = "none" if mode == 0 else acts[k % 3]
                k += 1
                add(Case(f"{'stats' if mode == 0 else 'bwd'}_old_{name}_{''.join('fb'[s] for s in st)}_{act}",
                         "stats" if mode == 0 else "bwd_reduce", shape,
                         dict(family="reduce", mode=mode, bf16_a=st[0], bf16_b=st[1] if mode else 0, leaky=int(act == "leaky"), **want),
                         st, {"*": lay}, act, {"affine": True, "per_item": name == "tight3"} if mode else {}, seed=200 + k))
    # ---- reduce -> finalize, judged against float64 statistics of the input
    fin = [
        ("instance", (2, 8, 4, 5, 6), dict(kind="INSTANCE")),
        ("instance_scale_shift", (2, 8, 4, 5, 6), dict(kind="INSTANCE", scale_shift=True, affine=True)),
        ("instance_rows_gt_64", (1, 4, 13, 13, 13), dict(kind="INSTANCE")),                 # 2197 voxels: 69 rows
        ("batch_train_ema", (3, 8, 4, 5, 6), dict(kind="BATCH", training=True, running=True, scale_shift=True, affine=True)),
        ("batch_eval", (2, 8, 4, 5, 6), dict(kind="BATCH", training=False, running=True, scale_shift=True, affine=True)),
        ("group_1", (2, 8, 4, 5, 6), dict(kind="GROUP", groups=1)),
        ("group_4", (2, 8, 4, 5, 6), dict(kind="GROUP", groups=4, scale_shift=True, affine=True)),
        ("group_c", (2, 8, 4, 5, 6), dict(kind="GROUP", groups=8)),
        # |mean| / std = 30 (the values have std 1.43): S and Q carry the mean, Q / cnt - mu^2 cancels it
        ("offset_instance", (2, 32, 8, 8, 8), dict(kind="INSTANCE", offset=43.0)),
        ("offset_batch", (2, 32, 8, 8, 8), dict(kind="BATCH", training=True, running=True, offset=43.0)),
        ("offset_group", (2, 32, 8, 8, 8), dict(kind="GROUP", groups=4, offset=43.0)),
    ]
    for i, (name, shape, kw) in enumerate(fin):
        add(Case(f"stats_chain_{name}", "stats_chain", shape, dict(family=S, mode=0), (0,), {}, "none", kw, seed=300 + i))
    bfin = [
        ("instance", (2, 8, 4, 5, 6), dict(kind="INSTANCE", affine=True)),
        ("instance_dgamma", (2, 8, 4, 5, 6), dict(kind="INSTANCE", affine=True, dgamma=True)),
        ("instance_rows_gt_64", (1, 4, 13, 13, 13), dict(kind="INSTANCE", affine=True)),
        ("batch_train", (3, 8, 4, 5, 6), dict(kind="BATCH", training=True, affine=True, dgamma=True)),
        ("batch_eval", (2, 8, 4, 5, 6), dict(kind="BATCH", training=False, affine=True, dgamma=True)),
        ("group_1", (2, 8, 4, 5, 6), dict(kind="GROUP", groups=1, affine=True)),
        ("group_4_dgamma", (2, 8, 4, 5, 6), dict(kind="GROUP", groups=4, affine=True, dgamma=True)),
        ("group_c_accumulate", (2, 8, 4, 5, 6), dict(kind="GROUP", groups=8, affine=True, dgamma=True, accumulate=True)),
    ]
    for i, (name, shape, kw) in enumerate(bfin):
        act = acts[i % 3]
        add(Case(f"bwd_chain_{name}_{act}", "bwd_chain", shape, dict(family=S, mode=1, leaky=int(act == "leaky")), (0, 0), {}, act, kw,
                 seed=400 + i))
    # ---- combine
    for bf in (0, 1):
        for two in (0, 1):
            for it, shape in ((2, (2, 16, 5, 6, 7)), (4, (1, 2048, 16, 16, 16))):
                act = acts[(bf + two + it) % 3]
                add(Case(f"combine8_it{it}_{'fb'[bf]}_{'two' if two else 'one'}_{act}", "combine", shape,
                         dict(family="combine8", it=it, has_b=two, bf16_a=bf, leaky=int(act == "leaky")), (bf,), {}, act,
                         {"two": two, "act_b": "none", "per_item": it == 2 and two == 1}, seed=500 + 4 * bf + 2 * two + it))
    ew0 = [
        ("v4_c12", (2, 12, 3, 5, 7), "tight", 4), ("v4_c6_pad", (1, 6, 3, 5, 7), "pad", 4), ("v1_cslice", (2, 5, 3, 4, 5), "cslice", 1),
    ]
    for bf in (0, 1):
        for i, (name, shape, lay, vec) in enumerate(ew0):
            c = shape[1]
            lays = {"tight": {}, "pad": {"*": pad8(c) if bf else pad4(c)}, "cslice": {"*": Lay(ldc=12, c_off=3)}}[lay]
            act = acts[(i + bf) % 3]
            two = (i + bf) % 2
            add(Case(f"combine_ew_{name}_{'fb'[bf]}_{act}", "combine", shape,
                     dict(family="elementwise", mode=0, vec=vec, bf16_a=bf, leaky=int(act == "leaky") or int(bool(two) and act == "none")),
                     (bf,), lays, act, {"two": two, "act_b": "leaky" if act == "none" else "relu", "per_item": name == "v4_c12"},
                     seed=520 + 3 * bf + i))
    # ---- norm backward apply
    for st in ((0, 0), (0, 1), (1, 1)):
        for it, shape in ((2, (2, 16, 5, 6, 7)), (4, (1, 2048, 16, 16, 16))):
            act = acts[(st[0] + st[1] + it // 2) % 3]
            add(Case(f"apply8_it{it}_{'fb'[st[0]]}{'fb'[st[1]]}_{act}", "apply", shape,
                     dict(family="norm_bwd_apply8", it=it, bf16_a=st[0], bf16_b=st[1], leaky=int(act == "leaky")), st, {}, act,
                     {"per_item": it == 2}, seed=600 + 10 * st[0] + 5 * st[1] + it))
    for st in ((0, 0), (0, 1), (1, 1), (1, 0)):
        for vec in (4, 1):
            c = 3 if st == (1, 0) else (12 if vec == 4 else 5)
            shape = (2, c, 3, 5, 7)
            if vec == 4:
                lays = {"dout": pad4(c), "dy": pad4(c), "y": pad4(c)} if c == 3 else {}
            else:
                lays = {"*": TIGHT} if c == 3 else {"*": Lay(ldc=12, c_off=3)}
            act = acts[(st[0] + 2 * st[1] + vec) % 3]
            add(Case(f"apply_ew_v{vec}_{'fb'[st[0]]}{'fb'[st[1]]}_{act}", "apply", shape,
                     dict(family="elementwise", mode=1, vec=vec, bf16_a=st[0], bf16_b=st[1], bf16_o=st[0], leaky=int(act == "leaky")),
                     st, lays, act, {"per_item": vec == 1}, seed=640 + 10 * st[0] + 5 * st[1] + vec))
    # ---- the one-launch backward
    small = [((0, 0), (2, 32, 1, 1, 1), {}), ((0, 1), (1, 32, 1, 1, 3), {}), ((1, 1), (1, 32, 16, 16, 16), {}),
             ((0, 0), (2, 512, 2, 3, 5), {"per_item": True}), ((1, 1), (2, 64, 3, 5, 7), {"in_place": True}),
             ((0, 1), (1, 32, 4, 8, 5), {"in_place": True})]
    for i, (st, shape, kw) in enumerate(small):
        act = acts[i % 3]
        add(Case(f"small_{'fb'[st[0]]}{'fb'[st[1]]}_c{shape[1]}_v{shape[2] * shape[3] * shape[4]}_{act}", "small", shape,
                 dict(family="norm_bwd_small", bf16_a=st[0], bf16_b=st[1], leaky=int(act == "leaky")), st, {}, act, kw, seed=700 + i))
    # ---- lincomb: every COUNT in both VEC forms; the four storage pairs and accumulate rotate over them
    pairs = [(0, 0), (1, 1), (0, 1), (1, 0)]
    for vec in (4, 1):
        for count in range(1, 9):
            for j, st in enumerate(pairs):
                acc = (count + j) % 2
                sl = j == (count % 4)             # the output is a channel slice of a wider tensor
                c = 8 if vec == 4 else 5
                lays = {}
                if vec == 1:
                    lays = {"*": Lay(ldc=7, c_off=1)} if not sl else {"out": Lay(ldc=11, c_off=3)}
                elif sl:
                    lays = {"out": Lay(ldc=24, c_off=8)}
                add(Case(f"lincomb_v{vec}_n{count}_{'fb'[st[0]]}{'fb'[st[1]]}{'_acc' if acc else ''}{'_slice' if sl else ''}", "lincomb",
                         (2, c, 3, 4, 5), dict(family="lincomb", vec=vec, count=count, bf16_a=st[0], bf16_o=st[1]), st, lays, "none",
                         {"count": count, "accumulate": bool(acc)}, seed=800 + 40 * (vec == 1) + 4 * count + j))
    # ---- trilinear x2 and its adjoint
    ups = [("v4", (2, 8, 3, 4, 5), {}, 4), ("v4_extent1", (1, 4, 1, 5, 3), {}, 4), ("v4_pad6", (1, 6, 3, 3, 3), "pad", 4),
           ("v1_tight3", (2, 3, 3, 5, 1), {}, 1), ("v1_sliced_src", (1, 5, 2, 3, 4), "slice", 1)]
    for op in ("up_fwd", "up_bwd"):
        src, dst = ("x", "y") if op == "up_fwd" else ("dy", "dx")
        for bf in (0, 1):
            for i, (name, shape, lay, vec) in enumerate(ups):
                c = shape[1]
                lays = lay if isinstance(lay, dict) else (
                    {"*": pad8(c) if bf else pad4(c)} if lay == "pad" else {src: Lay(ldc=9, c_off=2, w_buf=2 * shape[4] + 3, w_off=1)})
                acc = op == "up_bwd" and (i + bf) % 2 == 1
                add(Case(f"{op}_{name}_{'fb'[bf]}{'_acc' if acc else ''}", op, shape,
                         dict(family="upsample_fwd" if op == "up_fwd" else "upsample_bwd", vec=vec, bf16_a=bf, second_trip=0), (bf,),
                         lays, "none", {"accumulate": acc}, seed=900 + 20 * (op == "up_bwd") + 5 * bf + i))
    # ---- the second trip of the grid-stride loops: the only large cases (scalar path, 3 channels in tight rows)
    big = (1, 3, 89, 89, 89)          # 2 114 907 work items on 8192 x 256 threads
    add(Case("second_trip_combine", "combine", big, dict(family="elementwise", mode=0, vec=1, second_trip=1, grid_x=8192), (0,), {}, "relu",
             {"two": 1, "act_b": "none"}, seed=990))
    add(Case("second_trip_apply", "apply", big, dict(family="elementwise", mode=1, vec=1, second_trip=1, grid_x=8192), (0, 0), {}, "relu",
             {}, seed=991))
    add(Case("second_trip_lincomb", "lincomb", big, dict(family="lincomb", vec=1, count=2, second_trip=1, grid_x=8192), (0, 0), {}, "none",
             {"count": 2, "accumulate": False}, seed=992))
    add(Case("second_trip_up_fwd", "up_fwd", (1, 3, 56, 56, 56), dict(family="upsample_fwd", vec=1, second_trip=1, grid_x=16384), (0,),
             {}, "none", {}, seed=993))
    add(Case("second_trip_up_bwd", "up_bwd", (1, 3, 112, 112, 112), dict(family="upsample_bwd", vec=1, second_trip=1, grid_x=16384),
             (1,), {}, "none", {"accumulate": False}, seed=994))
    names = [c.name for c in out]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def cases_of(*ops_):
    return [c for c in CASES if c.op in ops_]


# ----------------------------------------------------------------------------- operands of a case
def coefficients(case: Case, rng, x=None):
    """mean / rstd [N, C] (fp32 values: float64 statistics of `x` where given), gamma / beta ([C], or [N, C] per item)."""
    n, c = case.shape[:2]
    if x is not None:
        mean = rf32(x.mean((1, 2, 3)))
        rstd = rf32(1.0 / np.sqrt(x.var((1, 2, 3)) + EPS))
    else:
        mean = rf32(0.3 * rng.standard_normal((n, c)))
        rstd = rf32(0.6 + rng.random((n, c)))
    gamma = beta = None
    if case.kw.get("affine", True):
        shape = (n, c) if case.kw.get("per_item") else (c,)
        gamma = rf32(1.0 + 0.4 * rng.standard_normal(shape))
        beta = rf32(0.3 * rng.standard_normal(shape))
    return mean, rstd, gamma, beta


def _bcast(v, n, c, fill):
    """[C] or [N, C] or None -> [N, 1, 1, 1, C]"""
    if v is None:
        return np.full((n, 1, 1, 1, c), fill)
    return np.broadcast_to(v.reshape((-1, c)), (n, c)).reshape(n, 1, 1, 1, c)


def nl_terms(x, mean, rstd, gamma, beta):
    """x * sc + sh with sc = rstd * gamma, sh = beta - mean * sc, and the sum of the absolute values of its terms."""
    n, c = x.shape[0], x.shape[-1]
    sc = _bcast(rstd, n, c, 1.0) * _bcast(gamma, n, c, 1.0)
    ms = _bcast(mean, n, c, 0.0) * sc
    b = _bcast(beta, n, c, 0.0)
    return x * sc + b - ms, np.abs(x * sc) + np.abs(b) + np.abs(ms)


def activate(v, act):
    return v if act == "none" else np.where(v > 0, v, act_slope(act) * v)


def bwd_terms(dout, y, mean, rstd, gamma, beta, act):
    """dz, xhat and the mask of elements whose activation derivative the kernel's fp32 z may decide the other way."""
    n, c = y.shape[0], y.shape[-1]
    xhat = (y - _bcast(mean, n, c, 0.0)) * _bcast(rstd, n, c, 1.0)
    z = _bcast(gamma, n, c, 1.0) * xhat + _bcast(beta, n, c, 0.0)
    if act == "none":
        return dout.copy(), xhat, np.zeros(y.shape, dtype=bool)
    return dout * np.where(z > 0, 1.0, act_slope(act)), xhat, np.abs(z) < Z_NEAR


def make(case: Case):
    """Operands (float64, exactly representable in their storage), the float64 reference and the derived bounds."""
    rng = np.random.default_rng(case.seed)
    n, c, d, h, w = case.shape
    vs = (n, d, h, w, c)
    o = {}
    if case.op in ("stats", "stats_chain"):
        o["x"] = stored(away_from_zero(rng, vs, case.kw.get("offset", 0.0)), case.st[0])
        if case.op == "stats_chain":
            if case.kw.get("affine"):
                o["gamma"], o["beta"] = rf32(1.0 + 0.4 * rng.standard_normal(c)), rf32(0.3 * rng.standard_normal(c))
            if case.kw.get("running"):
                o["rm0"], o["rv0"] = rf32(0.3 * rng.standard_normal(c)), rf32(0.5 + rng.random(c))
    elif case.op in ("bwd_reduce", "bwd_chain", "apply", "small"):
        ybf, dbf = operand_bf(case, "y"), operand_bf(case, "dout")
        o["y"] = stored(rng.standard_normal(vs) * 1.3 + 0.2, ybf)
        o["dout"] = stored(away_from_zero(rng, vs), dbf)
        o["mean"], o["rstd"], o["gamma"], o["beta"] = coefficients(case, rng, o["y"] if case.op in ("small", "bwd_chain") else None)
        if case.op == "apply":
            o["m1"] = rf32(0.2 * rng.standard_normal((n, c)))
            o["m2"] = rf32(0.2 * rng.standard_normal((n, c)))
        if case.op == "bwd_chain" and case.kw.get("accumulate"):
            o["dgamma0"] = rf32(rng.standard_normal(c))
            o["dbeta0"] = rf32(rng.standard_normal(c))
    elif case.op == "combine":
        bf = case.st[0]
        o["a"] = stored(rng.standard_normal(vs) * 1.3, bf)
        o["ca"] = coefficients(case, rng)
        if case.kw.get("two"):
            o["b"] = stored(rng.standard_normal(vs), bf)
            o["cb"] = coefficients(case, rng)
    elif case.op == "lincomb":
        for k in range(case.kw["count"]):
            o[f"in{k}"] = stored(rng.standard_normal(vs), case.st[0])
        o["w"] = rf32(rng.standard_normal(case.kw["count"]) + 0.1 * np.arange(1, case.kw["count"] + 1))
        if case.kw.get("accumulate"):
            o["out0"] = stored(rng.standard_normal(vs), case.st[1])
    elif case.op == "up_fwd":
        o["x"] = stored(rng.standard_normal(vs), case.st[0])
    elif case.op == "up_bwd":
        o["dy"] = stored(rng.standard_normal((n, 2 * d, 2 * h, 2 * w, c), dtype=np.float32), case.st[0])
        if case.kw.get("accumulate"):
            o["dx0"] = stored(rng.standard_normal(vs), case.st[0])
    return o


# ----------------------------------------------------------------------------- references and bounds
def row_sums(v, route):
    """[N, D, H, W, C] -> [N, rows, C]: the sums over the voxels of each partial row the route reports."""
    n, c = v.shape[0], v.shape[-1]
    flat = v.reshape(n, -1, c)
    return np.add.reduceat(flat, np.arange(0, flat.shape[1], route["vox_per_row"]), axis=1)


def ref_sums(case: Case, o, route):
    """{name: (ref [N, rows, C], bound [N, rows, C])} of the two sums per partial row, from the operands (float64).  The sums
    and bounds of an (item, channel) are their sums over the rows (the rows are added in fp64)."""
    L = sum_chain(route) * U
    rs = lambda v: row_sums(v, route)
    if case.op in ("stats", "stats_chain"):
        x = o["x"]
        return {"s0": (rs(x), L * rs(np.abs(x))), "s1": (rs(x * x), L * rs(x * x))}
    dz, xhat, near = bwd_terms(o["dout"], o["y"], o["mean"], o["rstd"], o["gamma"], o["beta"], case.act)
    flip = np.abs(o["dout"]) * near
    return {"s0": (rs(dz), L * rs(np.abs(dz)) + rs(flip)), "s1": (rs(dz * xhat), L * rs(np.abs(dz * xhat)) + rs(flip * np.abs(xhat))),
            "near": near}


def near_share(case: Case, o):
    if case.act == "none" or case.op not in ("bwd_reduce", "bwd_chain", "apply", "small"):
        return 0.0
    return float(bwd_terms(o["dout"], o["y"], o["mean"], o["rstd"], o["gamma"], o["beta"], case.act)[2].mean())


def pool(v, case: Case):
    """Per (item, channel) sums -> the sums of the statistics group each (item, channel) belongs to, and its count factor."""
    kind = case.kw["kind"]
    n, c = v.shape
    if kind == "INSTANCE":
        return v, 1
    if kind == "BATCH":
        return np.broadcast_to(v.sum(0, keepdims=True), (n, c)), n
    g = case.kw["groups"]
    return np.repeat(v.reshape(n, g, c // g).sum(2), c // g, axis=1), c // g


def ref_stats_chain(case: Case, o, route):
    """{name: (ref, bound)} of what channel_stats -> norm_stats_finalize writes, from float64 statistics of x."""
    n, c, d, h, w = case.shape
    sums = ref_sums(case, o, route)
    S, f = pool(sums["s0"][0].sum(1), case)
    dS, _ = pool(sums["s0"][1].sum(1), case)
    Q, _ = pool(sums["s1"][0].sum(1), case)
    dQ, _ = pool(sums["s1"][1].sum(1), case)
    cnt = d * h * w * f
    out = {}
    gamma, beta = o.get("gamma"), o.get("beta")
    g = np.ones(c) if gamma is None else gamma
    b = np.zeros(c) if beta is None else beta
    if case.kw["kind"] == "BATCH" and not case.kw.get("training", True):
        mean = np.broadcast_to(o["rm0"], (n, c))
        rstd = 1.0 / np.sqrt(np.broadcast_to(o["rv0"], (n, c)) + EPS)
        dmean, drstd = np.zeros((n, c)), U * rstd
    else:
        mu = S / cnt
        var = np.maximum(Q / cnt - mu * mu, 0.0)
        dmu = dS / cnt
        dvar = dQ / cnt + 2 * np.abs(mu) * dmu + dmu * dmu
        mean, dmean = mu, dmu + U * np.abs(mu)
        rstd = 1.0 / np.sqrt(var + EPS)
        drstd = 1.0 / np.sqrt(np.maximum(var - dvar, 0.0) + EPS) - rstd + U * rstd          # exact, not the first-order rstd^3 / 2
        out["_rstd_rel"] = (drstd / rstd).max()
        if case.kw.get("running"):
            unb = var * cnt / (cnt - 1.0)
            rm = (1 - MOMENTUM) * o["rm0"] + MOMENTUM * mu[0]
            rv = (1 - MOMENTUM) * o["rv0"] + MOMENTUM * unb[0]
            out["running_mean"] = (rm, MOMENTUM * dmu[0] + U * np.abs(rm))
            out["running_var"] = (rv, MOMENTUM * dvar[0] * cnt / (cnt - 1.0) + U * np.abs(rv))
    out["mean"], out["rstd"] = (mean, dmean), (rstd, drstd)
    if case.kw.get("scale_shift"):
        sc = rstd * g
        dsc = np.abs(g) * drstd + U * np.abs(sc)
        sh = b - mean * sc
        out["scale"] = (sc, dsc)
        out["shift"] = (sh, np.abs(mean) * dsc + np.abs(sc) * dmean + 2 * U * (np.abs(b) + np.abs(mean * sc)))
    return out


def ref_bwd_chain(case: Case, o, route):
    n, c, d, h, w = case.shape
    sums = ref_sums(case, o, route)
    g = np.ones(c) if o["gamma"] is None else o["gamma"]
    sums = {k: (v[0].sum(1), v[1].sum(1)) for k, v in sums.items() if k != "near"}
    A, f = pool(sums["s0"][0] * g, case)
    dA, _ = pool(sums["s0"][1] * np.abs(g), case)
    B, _ = pool(sums["s1"][0] * g, case)
    dB, _ = pool(sums["s1"][1] * np.abs(g), case)
    cnt = d * h * w * f
    out = {}
    if case.kw["kind"] == "BATCH" and not case.kw.get("training", True):
        out["m1"] = out["m2"] = (np.zeros((n, c)), np.zeros((n, c)))
    else:
        out["m1"] = (A / cnt, dA / cnt + U * np.abs(A / cnt))
        out["m2"] = (B / cnt, dB / cnt + U * np.abs(B / cnt))
    if case.kw.get("dgamma"):
        for name, key, prev in (("dgamma", "s1", "dgamma0"), ("dbeta", "s0", "dbeta0")):
            v, dv = sums[key][0].sum(0), sums[key][1].sum(0)
            if case.kw.get("accumulate"):
                out[name] = (o[prev] + v, dv + U * np.abs(v) + U * np.abs(o[prev] + v))
            else:
                out[name] = (v, dv + U * np.abs(v))
    return out


def store_bound(ref, bound, bf):
    return bound + (BF_ULP * np.abs(ref) if bf else 0.0)


def ref_combine(case: Case, o):
    va, ta = nl_terms(o["a"], *o["ca"])
    leaky = case.act == "leaky" or (case.kw.get("two") and case.kw.get("act_b") == "leaky")
    ref = activate(va, case.act)
    terms = ta
    if case.kw.get("two"):
        vb, tb = nl_terms(o["b"], *o["cb"])
        ref = ref + activate(vb, case.kw["act_b"])
        terms = terms + tb
    r = R["combine2"] if case.kw.get("two") else R["combine1"]
    return ref, store_bound(ref, (r - (0 if leaky else 1)) * U * terms, case.st[0])


def ref_apply(case: Case, o, m1=None, m2=None, dm=None):
    """dy, its bound and the elements left out.  `m1` / `m2`: the coefficients the kernel read ([N, C]); `dm`: their bounds."""
    n, c = case.shape[:2]
    dz, xhat, near = bwd_terms(o["dout"], o["y"], o["mean"], o["rstd"], o["gamma"], o["beta"], case.act)
    m1 = o["m1"] if m1 is None else m1
    m2 = o["m2"] if m2 is None else m2
    rs, g = _bcast(o["rstd"], n, c, 1.0), _bcast(o["gamma"], n, c, 1.0)
    M1, M2 = _bcast(m1, n, c, 0.0), _bcast(m2, n, c, 0.0)
    ref = rs * (g * dz - M1 - xhat * M2)
    terms = np.abs(rs) * (np.abs(g * dz) + np.abs(M1) + np.abs(xhat * M2))
    bound = (R["apply"] - (0 if case.act == "leaky" else 1)) * U * terms
    if dm is not None:
        bound = bound + np.abs(rs) * (_bcast(dm[0], n, c, 0.0) + np.abs(xhat) * _bcast(dm[1], n, c, 0.0))
    return ref, store_bound(ref, bound, operand_bf(case, "dy")), near


def ref_small(case: Case, o, route):
    n, c, d, h, w = case.shape
    sums = {k: (v[0].sum(1), v[1].sum(1)) for k, v in ref_sums(case, o, route).items() if k != "near"}
    g = _bcast(o["gamma"], n, c, 1.0).reshape(n, c)
    cnt = d * h * w
    m1, m2 = g * sums["s0"][0] / cnt, g * sums["s1"][0] / cnt
    dm = (np.abs(g) * sums["s0"][1] / cnt + U * np.abs(m1), np.abs(g) * sums["s1"][1] / cnt + U * np.abs(m2))
    return ref_apply(case, o, m1, m2, dm)


def ref_lincomb(case: Case, o):
    k = case.kw["count"]
    ref = sum(o["w"][i] * o[f"in{i}"] for i in range(k))
    terms = sum(np.abs(o["w"][i] * o[f"in{i}"]) for i in range(k))
    if case.kw.get("accumulate"):
        ref, terms = ref + o["out0"], terms + np.abs(o["out0"])
    return ref, store_bound(ref, k * U * terms, case.st[1])


def axis_matrix(n_in, n_out):
    """[n_out, n_in] weights of the align_corners=True linear resample along one axis, in float64."""
    a = np.zeros((n_out, n_in))
    for o_ in range(n_out):
        src = o_ * (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        i0 = min(int(src), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        lam = src - i0
        a[o_, i0] += 1.0 - lam
        a[o_, i1] += lam
    return a


def _apply3(v, mats, transpose=False):
    for axis, m in zip((1, 2, 3), mats):
        m = m.T if transpose else m
        v = np.moveaxis(np.tensordot(m, v, axes=([1], [axis])), 0, axis)
    return v


def ref_upsample(case: Case, o):
    """The coordinates are the exact ones; the kernel's fp32 lam = scale * dst - i0 is off by <= 3 u * extent per axis, which
    moves a weight by as much (the interpolant is continuous in lam, across a change of i0 too)."""
    n, c, d, h, w = case.shape
    mats = [axis_matrix(d, 2 * d), axis_matrix(h, 2 * h), axis_matrix(w, 2 * w)]
    supp = [(m > 0).astype(np.float64) for m in mats]
    dlam = 3 * U * (d + h + w)
    if case.op == "up_fwd":
        ref = _apply3(o["x"], mats)
        bound = R["upsample_fwd"] * U * _apply3(np.abs(o["x"]), mats) + dlam * _apply3(np.abs(o["x"]), supp)
        return ref, store_bound(ref, bound, case.st[0])
    ref = _apply3(o["dy"], mats, True)
    terms = _apply3(np.abs(o["dy"]), mats, True)
    bound = (125 + 3) * U * terms + dlam * _apply3(np.abs(o["dy"]), supp, True)
    if case.kw.get("accumulate"):
        ref = ref + o["dx0"]
        bound = bound + U * (terms + np.abs(o["dx0"]))
    return ref, store_bound(ref, bound, case.st[0])


# ----------------------------------------------------------------------------- the reachable classes, written out
def _p(*axes):
    return set(itertools.product(*axes))


FB = (0, 1)
# instantiation classes (klass()): family, then the template arguments in the order of mmtta.h's MMTTA_PW_* comments
REACHABLE = (
    # channel_reduce_kernel<MODE, VEC, XBF, DBF>: mode 0 has no dout; the fp32-x / bf16-dout pair needs C <= 4, which the
    # vec-4 form takes only for a view the streamed form refuses (a W-strided C = 4 here)
    _p(["reduce"], [0], [4, 1], FB, [0]) | _p(["reduce"], [1], [4, 1], FB, FB)
    # channel_reduce_stream_kernel<MODE, IT, XBF, DBF>
    | _p(["reduce_stream"], [0], [1, 2, 4], FB, [0]) | _p(["reduce_stream"], [1], [1, 2, 4], FB, FB)
    # elementwise_kernel<0, VEC, B, B, B> (one storage) and <1, VEC, ABF, BBF, OBF = ABF>
    | {("elementwise", 0, v, b, b, b) for v in (4, 1) for b in FB} | {("elementwise", 1, v, a, b, a) for v in (4, 1) for a in FB for b in FB}
    | _p(["combine8"], FB, FB, [2, 4])
    # norm_bwd_apply8_kernel<YBF, IT, DBF> and norm_bwd_small_kernel<YBF, DBF>: a bf16 gradient only next to a bf16 activation
    # with C >= 8 (the thin pair has C <= 4, below an octet)
    | {("norm_bwd_apply8", y, it, d_) for it in (2, 4) for (d_, y) in ((0, 0), (0, 1), (1, 1))}
    | {("norm_bwd_small", y, d_) for (d_, y) in ((0, 0), (0, 1), (1, 1))}
    | _p(["lincomb"], [4, 1], range(1, 9), FB, FB)
    | _p(["upsample_fwd"], [4, 1], FB) | _p(["upsample_bwd"], [4, 1], FB)
)
# Instantiations that exist and that no operand reaches:
#   norm_bwd_apply8_kernel<false, IT, true> and norm_bwd_small_kernel<false, true> are never instantiated (no dispatch line);
#   channel_reduce_kernel<0, VEC, XBF, true> / channel_reduce_stream_kernel<0, IT, XBF, true>: mode 0 reads no dout, the
#   launchers name DBF = false only;
#   copy_strided_kernel is not a route of this query (a layout copy, covered by tests/test_hip_pointwise.py).
REACHABLE_ROWS_PER_BLOCK = {1, 2, 4}          # 3 is reachable too (1536 .. 2047 rows in the launch): the same loop as 2 and 4
REACHABLE_CB = {("reduce", 1), ("reduce", 2), ("reduce_stream", 1)}
REACHABLE_SECOND_TRIP = _p(["elementwise"], [0, 1], FB) | _p(["lincomb", "upsample_fwd", "upsample_bwd"], [0], FB)
LEAKY_FAMILIES = {"reduce", "reduce_stream", "elementwise", "combine8", "norm_bwd_apply8", "norm_bwd_small"}
