"""Host side of MMTTA_OPT_HEAD_LOSS_PAIR (option 17): the eligibility query of the head convolution with the entropy
objective in its epilogue, the refusals of its entry point, the symbols and the option.  Nothing here launches a kernel: the
query is host-only, and the entry point refuses an ineligible call before it touches the device (the descriptors carry
made-up, suitably aligned addresses)."""
import ctypes as C
import os

import pytest

OPT = 17
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -2
BASE = 0x7F0000000000      # 16-byte aligned; never dereferenced


def _lib_():
    import __graft_entry__ as ge
    ge.build()
    from multimodal_tta_amd import _lib
    return _lib, _lib.load()


def _cl(_lib, n, c, d, h, w, ldc=4, dtype=None, owns_pad=True, ptr=BASE):
    """A channels-last descriptor of dense rows of `ldc` lanes."""
    sw, sh, sd, sn = ldc, w * ldc, h * w * ldc, d * h * w * ldc
    return _lib.Tensor(ptr, n, c, d, h, w, sn, 1, sd, sh, sw, _lib.F32 if dtype is None else dtype,
                       _lib.TENSOR_OWNS_PAD if (owns_pad and ldc != c) else 0)


def _ask(_lib, lib, desc, x, y, dz, softmax=0, per_item=1, x_norm=None, add=None, add_norm=None):
    epi = None
    if add is not None:
        epi = _lib.ConvEpilogue(C.pointer(add), add_norm if add_norm is not None else _lib.norm_on_load())
    ref = lambda v: C.byref(v) if v is not None else None
    q = lib.mmtta_conv_head_loss_eligible(C.byref(desc), C.byref(x), ref(x_norm), ref(epi), C.byref(y), ref(dz), softmax, per_item)
    # the entry point must agree with the query: an ineligible call is refused by status before anything is launched
    if q == 0:
        st = lib.mmtta_conv_head_loss_run_sets(C.byref(desc), C.byref(x), ref(x_norm), BASE, None, ref(epi), C.byref(y), ref(dz),
                                               softmax, per_item, BASE, BASE, None, None)
        assert st == ERR_UNSUPPORTED, f"ineligible call: status {st}, {lib.mmtta_last_error()!r}"
        assert b"mmtta_conv_head_loss_eligible" in lib.mmtta_last_error()
    return q


@pytest.fixture()
def default_option():
    _lib, lib = _lib_()
    prev = lib.mmtta_set_option(OPT, 3)
    prev13 = lib.mmtta_set_option(13, 2)
    yield _lib, lib
    lib.mmtta_set_option(13, prev13)
    lib.mmtta_set_option(OPT, prev)


def test_symbols_are_declared_exported_and_typed():
    _lib, lib = _lib_()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mmtta.h")).read()
    for name in ("mmtta_conv_head_loss_eligible", "mmtta_conv_head_loss_partials", "mmtta_conv_head_loss_run_sets"):
        assert name + "(" in header
        assert name in _lib.exported_names()
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(_lib._SIGNATURES[name][1])
    assert "#define MMTTA_OPT_HEAD_LOSS_PAIR 17" in header
    assert lib.mmtta_abi_version() == 2


def test_option_17_round_trips():
    _lib, lib = _lib_()
    first = lib.mmtta_set_option(OPT, 0)
    try:
        assert first in (0, 1, 2, 3)
        assert lib.mmtta_set_option(OPT, 1) == 0
        assert lib.mmtta_set_option(OPT, 2) == 1
        assert lib.mmtta_set_option(OPT, 3) == 2
        assert lib.mmtta_set_option(OPT, 7) == 3          # two bits: 7 is stored as 3
        assert lib.mmtta_set_option(OPT, 0) == 3
    finally:
        lib.mmtta_set_option(OPT, first)
    assert lib.mmtta_set_option(OPT, first) == first


@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("gbf", [False, True], ids=["fp32-grad", "bf16-grad"])
def test_the_bf16_sigmoid_head_is_eligible(default_option, R, gbf):
    _lib, lib = default_option
    desc = _lib.ConvDesc(_lib.CONV_FWD, 3, 1, R, R, _lib.BF16)
    x, y, add = (_cl(_lib, 2, R, 8, 16, 64) for _ in range(3))
    dz = _cl(_lib, 2, R, 8, 16, 64, dtype=_lib.BF16 if gbf else _lib.F32)
    assert _ask(_lib, lib, desc, x, y, dz) == 1
    assert _ask(_lib, lib, desc, x, y, dz, add=add) == 1
    assert lib.mmtta_conv_head_loss_partials(C.byref(desc), C.byref(x), C.byref(y)) == 2 * 2 * 2 * 1      # 4 x 8 x 64 tiles
    # a batch of one is its own objective either way; a batch of two is not one objective
    one = [_cl(_lib, 1, R, 8, 16, 64) for _ in range(3)]
    assert _ask(_lib, lib, desc, *one, per_item=0) == 1
    assert _ask(_lib, lib, desc, x, y, dz, per_item=0) == 0
    # the switch: bit 0 clear says no, in the same process
    prev = lib.mmtta_set_option(OPT, 2)
    try:
        assert _ask(_lib, lib, desc, x, y, dz) == 0
    finally:
        lib.mmtta_set_option(OPT, prev)


def test_refusals(default_option):
    _lib, lib = default_option
    t = lambda c=3, **k: _cl(_lib, 2, c, 8, 16, 64, **k)
    bf = _lib.ConvDesc(_lib.CONV_FWD, 3, 1, 3, 3, _lib.BF16)
    assert _ask(_lib, lib, bf, t(), t(), t()) == 1
    # softmax head
    assert _ask(_lib, lib, bf, t(), t(), t(), softmax=1) == 0
    # R = 5: not a direct (<= 4 produced channels) convolution at all
    d5 = _lib.ConvDesc(_lib.CONV_FWD, 3, 1, 5, 5, _lib.BF16)
    assert _ask(_lib, lib, d5, t(5, ldc=8), t(5, ldc=8), t(5, ldc=8)) == 0
    # fp32 precision: the vector-ALU row kernel, not the matrix tiles; likewise bf16 precision with option 13 = 0
    f32 = _lib.ConvDesc(_lib.CONV_FWD, 3, 1, 3, 3, _lib.F32)
    assert _ask(_lib, lib, f32, t(), t(), t()) == 0
    prev = lib.mmtta_set_option(13, 0)
    try:
        assert _ask(_lib, lib, bf, t(), t(), t()) == 0
    finally:
        lib.mmtta_set_option(13, prev)
    # dlogits without its pad lane (a slice of someone else's rows), or in rows that are not dense
    assert _ask(_lib, lib, bf, t(), t(), t(owns_pad=False)) == 0
    assert _ask(_lib, lib, bf, t(), t(), t(ldc=8)) == 0
    assert _ask(_lib, lib, bf, t(), t(), None) == 0
    # logits the vector loss kernel would not take either (rows of 8 lanes): the two launches stay
    assert _ask(_lib, lib, bf, t(), t(ldc=8), t()) == 0
    # bf16-stored thin tensors (the input-gradient form of the kernel), the input-gradient op, a stride-2 head
    assert _ask(_lib, lib, bf, t(dtype=_lib.BF16), t(), t()) == 0
    assert _ask(_lib, lib, _lib.ConvDesc(_lib.CONV_DGRAD, 3, 1, 3, 3, _lib.BF16), t(), t(), t()) == 0
    # a LeakyReLU on the fused add: that instantiation has no twin
    leaky = _lib.norm_on_load(None, None, None, None, True, None, None, False, _lib.ACT_LEAKY_RELU, 0.1)
    assert _ask(_lib, lib, bf, t(), t(), t(), add=t(), add_norm=leaky) == 0
    # more workgroups per item than an item has partial slots: 2049 tiles of 4 x 8 x 64
    big = lambda **k: _cl(_lib, 1, 3, 4 * 2049, 8, 64, **k)
    assert _ask(_lib, lib, bf, big(), big(), big()) == 0
    # shape mismatches are the convolution's own errors (negative status), not a quiet "no"
    assert lib.mmtta_conv_head_loss_eligible(C.byref(bf), C.byref(t()), None, None, C.byref(_cl(_lib, 2, 3, 8, 16, 32)),
                                             C.byref(t()), 0, 1) == ERR_INVALID
    assert _ask(_lib, lib, bf, t(), t(), _cl(_lib, 2, 3, 8, 16, 32)) == 0
