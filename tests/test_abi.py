"""The C ABI library loads on a box without a GPU and exports every symbol include/mmtta.h declares;
the ctypes table of the Python binding covers exactly that set."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    text = open(os.path.join(ROOT, "include", "mmtta.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mmtta_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as ge
    ge.build()
    from multimodal_tta_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = declared_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/mmtta.h but not exported by libmmtta.so"
    assert lib.mmtta_abi_version() == 2


def test_binding_table_matches_header():
    from multimodal_tta_amd import _lib
    assert sorted(_lib.exported_names()) == declared_functions()
    _lib.load()


def test_argument_validation_without_a_gpu():
    """Entry points reject bad arguments before touching the device."""
    from multimodal_tta_amd import _lib
    lib = _lib.load()
    d = _lib.ConvDesc(0, 5, 1, 4, 4, 0)     # ksize 5: unsupported
    assert lib.mmtta_conv_packed_bytes(ctypes.byref(d)) == -1
    assert b"ksize" in lib.mmtta_last_error()
    d = _lib.ConvDesc(0, 3, 1, 4, 32, 0)
    assert lib.mmtta_conv_packed_bytes(ctypes.byref(d)) == 27 * 32 * 32 * 4
    assert lib.mmtta_copy_strided(None, None, None) == -1


def test_conv_queries_share_the_operands_of_conv_route():
    """The host-only queries about a run take what mmtta_conv_route takes, and return its error codes for a bad descriptor."""
    from multimodal_tta_amd import _lib
    lib = _lib.load()
    bad = _lib.ConvDesc(0, 5, 1, 4, 4, 0)       # ksize 5: unsupported
    t = _lib.Tensor(1 << 30, 1, 4, 4, 4, 8, 512, 1, 128, 32, 4, _lib.F32, 0)
    for name in ("mmtta_conv_stages_raw", "mmtta_conv_cls8_pipelined", "mmtta_conv_thin_lean", "mmtta_conv_thin_kernel"):
        assert name in declared_functions()
        fn = getattr(lib, name)
        assert fn.argtypes == lib.mmtta_conv_route.argtypes and fn.restype == lib.mmtta_conv_route.restype, name
        assert fn(ctypes.byref(bad), ctypes.byref(t), None, None, ctypes.byref(t), 0, None) == -2, name
    ok = _lib.ConvDesc(0, 3, 1, 4, 4, 0)        # 4 -> 4, 3x3x3 stride 1, fp32: the row kernel of route 6
    assert lib.mmtta_conv_route(ctypes.byref(ok), ctypes.byref(t), None, None, ctypes.byref(t), 0, None) == 6
    assert lib.mmtta_conv_thin_kernel(ctypes.byref(ok), ctypes.byref(t), None, None, ctypes.byref(t), 0, None) == 3


# mmtta_set_option: what each key stores for the raw values -1, 0, 1, 2, 3, 7 (None: refused with MMTTA_ERR_INVALID, the
# option keeps its value).  Written out from the header's description of every key, not computed.
OPTION_PROBES = (-1, 0, 1, 2, 3, 7)
_AS_IS, _FLAG = (-1, 0, 1, 2, 3, 7), (1, 0, 1, 1, 1, 1)
_AT_LEAST_1, _BITS01 = (None, None, 1, 2, 3, 7), (3, 0, 1, 2, 3, 3)
OPTION_STORES = {
    1: _AS_IS,                                                    # PROFILE_MAIN_KERNEL_ONLY
    2: _AT_LEAST_1, 3: _AT_LEAST_1, 4: _AT_LEAST_1, 5: _AT_LEAST_1,      # SPLITK_BELOW, SPLITK_TARGET, WGRAD_WORKGROUPS, WGRAD_THIN_SLABS
    6: _FLAG, 9: _FLAG, 10: _FLAG, 11: _FLAG,                     # IGEMM_PIPELINE, EPILOGUE_VEC16, IGEMM_LEAN, WGRAD_VECTOR_STAGING
    12: (0, 0, 1, 2, 3, 7),                                       # CLASS_FUSED_MIN_WORKGROUPS: not below 0
    13: (0, 0, 1, 2, 3, 3),                                       # THIN_MFMA: 0 .. 3
    14: _FLAG, 15: _FLAG,                                         # IGEMM_FRAGMENT_REUSE, LAME_TILED
    16: _BITS01, 17: _BITS01, 18: _BITS01,                        # RAW_STAGING, HEAD_LOSS_PAIR, THIN_LEAN: two bits
    19: _FLAG, 20: _FLAG,                                         # WGRAD_EPILOGUE_UPDATE, CLS8_PIPELINE
    21: (1, 0, 1, 0, 1, 1),                                       # CLS8_LEAN_EPILOGUE: bit 0
}


def test_set_option_returns_the_previous_value_and_stores_the_normalised_one():
    from multimodal_tta_amd import ops
    header = open(os.path.join(ROOT, "include", "mmtta.h")).read()
    assert sorted(int(k) for k in re.findall(r"#define MMTTA_OPT_[A-Z0-9_]+ (\d+)", header)) == sorted(OPTION_STORES)
    invalid = -1                                                  # MMTTA_ERR_INVALID
    saved = {key: ops.set_option(key, 1) for key in OPTION_STORES}      # (1 is a value every key takes, and stores as 1)
    try:
        for key, stores in OPTION_STORES.items():
            for raw, want in zip(OPTION_PROBES, stores):
                assert ops.set_option(key, raw) == (invalid if want is None else 1), f"key {key}, value {raw}: the previous value is 1"
                assert ops.set_option(key, 1) == (1 if want is None else want), f"key {key}, value {raw}: stored"
        for key in (7, 8, 22):
            assert ops.set_option(key, 1) == invalid and ops.set_option(key, 0) == invalid, f"key {key} does not exist"
    finally:
        for key, val in saved.items():
            ops.set_option(key, val)
    assert {key: ops.set_option(key, val) for key, val in saved.items()} == saved, "every option is what it was"
