"""PETAL adaptation (``petal_tta``, ``method=tta_petal``): the host-side half, no GPU needed.

The config composes and the plugin reads and validates its keys; the table builder gives k_t = floor(delta n_t) per tensor
with the alignment padding in no row; a NumPy restatement of the restore rule of DESIGN.md section 7 (``rank_restore``,
which tests/test_hip_petal.py holds the kernels to) agrees with a plain sort on hand-made cases; the new entry points refuse
bad arguments before anything reaches the device."""
import ctypes
import math

import numpy as np
import pytest

INVALID, UNSUPPORTED = -1, -2
FAKE = 4096          # a 16-byte aligned address that is never dereferenced: the checks fail first


# ----------------------------------------------------------------------------- the rule, restated
def keys_of(g):
    """The magnitude keys of fp32 values: their bits without the sign, as unsigned integers."""
    return np.ascontiguousarray(g, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def rank_restore(g, rows):
    """g: fp32 [n]; rows: (start, length, rank).  -> (gamma uint32 [rows], mask bool [n]): per row the rank-th smallest key
    (0-based, ``np.partition``) and the elements with a key strictly below it; elements of no row are never in the mask."""
    k = keys_of(g)
    gamma = np.zeros(len(rows), dtype=np.uint32)
    mask = np.zeros(k.shape[0], dtype=bool)
    for r, (start, length, rank) in enumerate(rows):
        seg = k[start:start + length]
        gamma[r] = np.partition(seg, rank)[rank]
        mask[start:start + length] = seg < gamma[r]
    return gamma, mask


def sorted_restore(g, rows):
    """The same by a plain sort of |g| as Python floats (no NaNs): the hand-made cases' reference."""
    gamma, mask = [], np.zeros(len(g), dtype=bool)
    for start, length, rank in rows:
        mags = [abs(float(v)) for v in g[start:start + length]]
        thr = sorted(mags)[rank]
        gamma.append(thr)
        for i, m in enumerate(mags):
            mask[start + i] = m < thr
    return gamma, mask


@pytest.mark.parametrize("g,rows", [
    ([3.0, -1.0, 2.0, 0.5], [(0, 4, 0)]),                                   # rank 0: nothing lies below the minimum
    ([3.0, -1.0, 2.0, 0.5], [(0, 4, 3)]),                                   # the maximum: the three others
    ([3.0, -1.0, 2.0, 0.5, 9.0, 9.0, 9.0, 9.0, -7.0, 6.0], [(0, 3, 1), (8, 2, 1)]),       # two rows, a gap between them
    ([1.0, -1.0, 1.0, 0.25, 1.0, -0.125, 5.0, 1.0], [(0, 8, 3)]),           # ties at gamma (1.0 five times): they stay
    ([0.0, -0.0, 0.0, -0.0, 1e-40, -1e-42, 2.0], [(0, 7, 2)]),              # +0 == -0; gamma is a zero: nothing restored
    ([0.0, -0.0, 0.0, -0.0, 1e-40, -1e-42, 2.0], [(0, 7, 5)]),              # denormals order by magnitude
    ([0.0] * 6, [(0, 6, 4)]),                                               # an all-zero gradient restores nothing
    ([float("inf"), -3.0, float("-inf"), 2.0], [(0, 4, 2)]),
])
def test_rank_restore_agrees_with_a_plain_sort(g, rows):
    g = np.array(g, dtype=np.float32)
    gamma, mask = rank_restore(g, rows)
    want_gamma, want_mask = sorted_restore(g, rows)
    assert [float(np.array([v], dtype=np.uint32).view(np.float32)[0]) for v in gamma] == [float(np.float32(v)) for v in want_gamma]
    assert mask.tolist() == want_mask.tolist()
    for r, (start, length, rank) in enumerate(rows):
        seg = keys_of(g)[start:start + length]
        ties = int((seg == gamma[r]).sum())
        assert int(mask[start:start + length].sum()) <= rank and (ties > 1 or int(mask[start:start + length].sum()) == rank)
    covered = np.zeros(len(g), dtype=bool)
    for start, length, _ in rows:
        covered[start:start + length] = True
    assert not mask[~covered].any()


def test_keys_order_the_special_values():
    g = np.array([np.nan, np.inf, -np.inf, 3.0, -0.0, 0.0, 1e-45, -np.nan], dtype=np.float32)
    k = keys_of(g)
    assert k[4] == k[5] == 0 and k[6] == 1 and k[1] == k[2] == 0x7F800000 and k[0] > k[1] and k[7] > k[1] and k[3] < k[1]
    # a NaN is the largest key: it is never restored while the rank lies below it
    _, mask = rank_restore(g, [(0, 8, 5)])
    assert not mask[0] and not mask[7] and mask[[3, 4, 5, 6]].all()


# ----------------------------------------------------------------------------- config and plugin
def test_petal_is_a_registered_plugin():
    import multimodal_tta_amd  # noqa: F401
    from multimodal_tta_amd.cotta import MeanTeacherTTA
    from multimodal_tta_amd.registry import get_plugin, list_plugins
    assert {"petal_tta", "cotta_tta", "eata_tta"} <= set(list_plugins())
    assert issubclass(get_plugin("petal_tta"), MeanTeacherTTA) and get_plugin("petal_tta") is not MeanTeacherTTA
    assert get_plugin("cotta_tta") is MeanTeacherTTA


def test_tta_petal_config_composes_and_the_plugin_reads_it():
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin
    cfg = compose(overrides=["task=brats", "dataset=brats", "model=unet", "method=tta_petal"])
    assert cfg["method"]["name"] == "petal_tta" and cfg["method"]["kind"] == "tta"
    c = cfg["method"]["petal"]
    assert list(c["mirror_axes"]) == ["h", "w"] and c["alpha"] == 0.999 and c["quantile"] == 0.03
    assert "restore_p" not in c and "seed" not in c and "cotta" not in cfg["method"]
    plug = get_plugin("petal_tta")(cfg)
    assert plug.mirror_axes == ["h", "w"] and plug.views == 4 and plug.view_axes == [0, 2, 1, 3]
    assert plug.alpha == 0.999 and plug.quantile == 0.03 and plug.fused_update is False
    assert ("restored", "cotta_restored") in [(k, b) for k, b, _ in plug.records]
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_petal", "method.petal.mirror_axes=[w]",
                             "method.petal.alpha=0.5", "method.petal.quantile=0", "method.episodic=false"])
    cfg["method"]["cotta"] = {"mirror_axes": ["d", "h", "w"], "alpha": 0.25}          # not this plugin's block
    plug = get_plugin("petal_tta")(cfg)
    assert plug.views == 2 and plug.alpha == 0.5 and plug.quantile == 0.0 and plug.episodic is False


def test_tta_petal_is_tta_cotta_with_its_own_block():
    from multimodal_tta_amd.config import compose
    cot = compose(overrides=["task=brats", "model=unet", "method=tta_cotta"])["method"]
    pet = compose(overrides=["task=brats", "model=unet", "method=tta_petal"])["method"]
    assert set(pet) == (set(cot) - {"cotta"}) | {"petal"}
    for k in cot:
        if k not in ("name", "cotta"):
            assert pet[k] == cot[k], k
    assert set(pet["petal"]) == (set(cot["cotta"]) - {"restore_p", "seed"}) | {"quantile"}
    for k in pet["petal"]:
        if k != "quantile":
            assert pet["petal"][k] == cot["cotta"][k], k


def _cfg(**petal):
    from multimodal_tta_amd.config import compose
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_petal"])
    for k, v in petal.items():
        cfg["method"]["petal"][k] = v
    return cfg


@pytest.mark.parametrize("key,bad", [("quantile", -0.01), ("quantile", 1), ("quantile", 1.0), ("quantile", True), ("quantile", "3%"),
                                     ("quantile", float("nan")), ("alpha", 1.5), ("alpha", True), ("mirror_axes", ["x"])])
def test_petal_plugin_rejects_bad_keys(key, bad):
    from multimodal_tta_amd.registry import get_plugin
    with pytest.raises(ValueError, match=f"method.petal.{key}"):
        get_plugin("petal_tta")(_cfg(**{key: bad}))


def test_petal_plugin_accepts_the_ends_of_the_range_and_rejects_moddrop():
    from multimodal_tta_amd.registry import get_plugin
    for kw in ({"quantile": 0}, {"quantile": 0.0}, {"quantile": 0.999}, {"alpha": 0.0}, {"alpha": 1.0}):
        get_plugin("petal_tta")(_cfg(**kw))
    cfg = _cfg()
    cfg["method"]["moddrop"] = {"enabled": True, "p": 0.5, "seed": 0}
    with pytest.raises(NotImplementedError, match="method.moddrop.enabled"):
        get_plugin("petal_tta")(cfg)


# ----------------------------------------------------------------------------- the table
class _Ref:
    def __init__(self, offset, numel, trainable=True):
        self.offset, self.numel, self.trainable = offset, numel, trainable


def test_rank_rows_give_floor_of_delta_n_and_leave_the_padding_out():
    from multimodal_tta_amd.petal import rank_rows
    # an arena layout: offsets are multiples of 4, numels are anything; a frozen tensor behind the trainable ones
    refs = [_Ref(0, 3456), _Ref(3456, 7), _Ref(3464, 1), _Ref(3468, 100), _Ref(3568, 33), _Ref(3604, 3538944), _Ref(3542548, 64, False)]
    for delta in (0.03, 0.2, 0.0, 0.999):
        rows = rank_rows(list(reversed(refs)), delta)
        assert [r[:2] for r in rows] == [(r.offset, r.numel) for r in refs if r.trainable]
        for start, length, rank in rows:
            assert rank == math.floor(delta * length) and 0 <= rank < length and start % 4 == 0
        covered = np.zeros(3542548, dtype=bool)
        for start, length, _ in rows:
            assert not covered[start:start + length].any()
            covered[start:start + length] = True
        for pad in (3463, 3465, 3466, 3467, 3601, 3602, 3603):
            assert not covered[pad]
    assert [r[2] for r in rank_rows(refs, 0.03)] == [103, 0, 0, 3, 0, 106168]          # delta n < 1: nothing to restore
    assert [r[2] for r in rank_rows(refs, 0.2)] == [691, 1, 0, 20, 6, 707788]


# ----------------------------------------------------------------------------- the entry points, without a GPU
def _lib():
    import __graft_entry__ as ge
    ge.build()
    from multimodal_tta_amd import _lib
    return _lib, _lib.load()


def host_table(lib, rows, cum=None):
    """The host copy of the segment table: [count][3] then the running chunk counts; kept alive by the caller."""
    flat, run = [], [0]
    for start, length, rank in rows:
        flat += [start, length, rank]
        run.append(run[-1] + max(0, lib.mmtta_magnitude_select_chunks(length)))
    return np.array(flat + (run if cum is None else cum), dtype=np.int64)


def test_the_library_exports_the_petal_entry_points():
    _l, lib = _lib()
    for name in ("mmtta_magnitude_select_class", "mmtta_magnitude_select_chunks", "mmtta_magnitude_select_scratch_bytes",
                 "mmtta_magnitude_select_sets", "mmtta_petal_update_partials", "mmtta_petal_update_sets"):
        assert hasattr(ctypes.CDLL(_l.LIB_PATH), name) and name in _l.exported_names()
    assert lib.mmtta_abi_version() == 2


def test_the_class_query_names_one_boundary():
    _l, lib = _lib()
    assert lib.mmtta_magnitude_select_class(0) == -1 and lib.mmtta_magnitude_select_class(1) == 0
    assert lib.mmtta_magnitude_select_class(1 << 30) == 1
    classes = [lib.mmtta_magnitude_select_class(n) for n in range(1, 1 << 16)]
    assert classes == sorted(classes) and classes[-1] == 1          # one workgroup up to the boundary, chunked behind it
    b = classes.index(1) + 1
    assert lib.mmtta_magnitude_select_chunks(b - 1) == 0 and lib.mmtta_magnitude_select_chunks(b) >= 1
    assert lib.mmtta_magnitude_select_scratch_bytes(0, 1) == -1 and lib.mmtta_magnitude_select_scratch_bytes(1, 0) == -1
    assert lib.mmtta_magnitude_select_scratch_bytes(3, 2) == 2 * lib.mmtta_magnitude_select_scratch_bytes(3, 1) > 0


GOOD = [(0, 1000, 30), (1000, 7, 0), (1008, 40000, 1200)]
BAD_ROWS = [
    ([(0, 1000, 30), (1000, 7, 0), (1004, 40000, 1200)], b"starts at"),          # overlaps the row before it
    ([(1008, 40000, 1200), (0, 1000, 30)], b"starts at"),                         # out of order
    ([(0, 1000, 30), (1002, 7, 0)], b"starts at"),                                # no multiple of 4
    ([(0, 0, 0)], b"length"),
    ([(0, 1000, 1000)], b"rank"),
    ([(0, 1000, -1)], b"rank"),
    ([(0, 1000, 30), (1000, 7, 0), (1008, 50000, 1200)], b"ends at"),             # behind the set (n = 41008 below)
]


def test_magnitude_select_rejects_bad_arguments_without_a_gpu():
    _l, lib = _lib()
    good = host_table(lib, GOOD)

    def call(g=FAKE, table=FAKE, host=good, count=3, sets=2, stride=41008, gamma=FAKE, scratch=FAKE):
        hp = None if host is None else host.ctypes.data
        return lib.mmtta_magnitude_select_sets(g, table, hp, count, sets, stride, gamma, scratch, None)

    for k in ("g", "table", "host", "gamma", "scratch"):
        assert call(**{k: None}) == INVALID and b"null argument" in lib.mmtta_last_error()
    assert call(sets=0) == INVALID and b"sets" in lib.mmtta_last_error()
    assert call(stride=41010) == INVALID and b"stride" in lib.mmtta_last_error()
    assert call(stride=41004) == INVALID and b"ends at" in lib.mmtta_last_error()          # below the end of the last row
    assert call(count=0) == INVALID and b"count" in lib.mmtta_last_error()
    for rows, msg in BAD_ROWS:
        t = host_table(lib, rows)
        assert call(host=t, count=len(rows)) == INVALID and msg in lib.mmtta_last_error(), rows
    assert call(host=host_table(lib, GOOD, cum=[0, 0, 0, 0])) == INVALID and b"chunk counts" in lib.mmtta_last_error()
    assert call(host=host_table(lib, GOOD, cum=[1, 1, 1, 4])) == INVALID and b"chunk counts" in lib.mmtta_last_error()
    assert call(count=(1 << 20) + 1) == UNSUPPORTED and b"rows" in lib.mmtta_last_error()
    assert call(sets=65536) == UNSUPPORTED and b"sets" in lib.mmtta_last_error()
    huge = host_table(lib, [(0, 1 << 31, 5)])
    assert call(host=huge, count=1, stride=1 << 32) == UNSUPPORTED and b"2^31" in lib.mmtta_last_error()
    assert call(g=FAKE + 4) == UNSUPPORTED and b"aligned" in lib.mmtta_last_error()


def test_petal_update_rejects_bad_arguments_without_a_gpu():
    _l, lib = _lib()
    good = host_table(lib, GOOD)

    def call(w=FAKE, teacher=FAKE, source=FAKE, g=FAKE, gamma=FAKE, table=FAKE, host=good, count=3, n=41008, sets=2, ws=41008,
             ts=41008, gs=41012, alpha=0.9, partial=FAKE, restored=FAKE):
        hp = None if host is None else host.ctypes.data
        return lib.mmtta_petal_update_sets(w, teacher, source, g, gamma, table, hp, count, n, sets, ws, ts, gs, alpha, partial,
                                           restored, None)

    for k in ("w", "teacher", "source", "g", "gamma", "table", "host", "partial", "restored"):
        assert call(**{k: None}) == INVALID and b"null argument" in lib.mmtta_last_error()
    for a in (-0.5, 1.001, float("nan")):
        assert call(alpha=a) == INVALID and b"alpha" in lib.mmtta_last_error()
    assert call(sets=0) == INVALID and b"sets" in lib.mmtta_last_error()
    assert call(n=-1) == INVALID
    for kw in ({"ws": 41010}, {"ts": 41004}, {"gs": 41010}, {"gs": 41004}, {"ws": 41004, "sets": 1}):
        assert call(**kw) == INVALID and b"strides" in lib.mmtta_last_error(), kw
    assert call(n=41004, ws=41004, ts=41004, gs=41004) == INVALID and b"ends at" in lib.mmtta_last_error()
    for rows, msg in BAD_ROWS:
        t = host_table(lib, rows)
        assert call(host=t, count=len(rows)) == INVALID and msg in lib.mmtta_last_error(), rows
    assert call(host=host_table(lib, GOOD, cum=[0, 0, 0, 7])) == INVALID and b"chunk counts" in lib.mmtta_last_error()
    assert call(count=(1 << 20) + 1) == UNSUPPORTED and call(sets=65536) == UNSUPPORTED
    assert call(w=FAKE + 4) == UNSUPPORTED and b"aligned" in lib.mmtta_last_error()
    assert lib.mmtta_petal_update_partials(-1, 1) == -1 and lib.mmtta_petal_update_partials(8, 0) == -1
    assert lib.mmtta_petal_update_partials(1003, 3) == 3          # one workgroup per set
    assert lib.mmtta_petal_update_partials(1 << 20, 2) > 2
