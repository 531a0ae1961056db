"""Per-volume norm parameter sets (mmtta_norm_sets, ``method.norm_sets``): the host-side half, no GPU needed.

The two ``_sets`` entry points check their descriptor before anything reaches the device, and the method configs carry
the switch (off by default)."""
import ctypes

import pytest


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from multimodal_tta_amd import _lib
    return _lib, _lib.load()


def _finalize(lib, _l, n, sets):
    return lib.mmtta_norm_stats_finalize_sets(1, 1, None, 1, n, 8, 64, 1e-5, 1, None, None, 0.1, None, None, None, None,
                                              None, None, None, None, None, ctypes.byref(sets) if sets is not None else None,
                                              None)


def _bwd_finalize(lib, _l, n, sets):
    return lib.mmtta_norm_bwd_finalize_sets(1, 1, None, 1, n, 8, 64, None, 1, None, None, None, None, 0, None,
                                            ctypes.byref(sets) if sets is not None else None, None)


@pytest.mark.parametrize("call", [_finalize, _bwd_finalize])
def test_norm_sets_entry_points_reject_bad_descriptors_without_a_gpu(call):
    _l, lib = _lib()
    # items_per_set must divide the batch
    assert call(lib, _l, 3, _l.NormSets(2, 0, 16, 16)) == -1
    assert b"items_per_set" in lib.mmtta_last_error()
    assert call(lib, _l, 4, _l.NormSets(0, 0, 16, 16)) == -1
    assert b"items_per_set" in lib.mmtta_last_error()
    # strides keep 16-byte alignment (multiples of 4 fp32 elements)
    assert call(lib, _l, 4, _l.NormSets(1, 0, 6, 16)) == -1
    assert b"16-byte" in lib.mmtta_last_error()
    assert call(lib, _l, 4, _l.NormSets(1, 0, 16, 18)) == -1
    assert b"16-byte" in lib.mmtta_last_error()
    assert call(lib, _l, 4, _l.NormSets(1, 0, -4, 16)) == -1
    # the descriptor is required
    assert call(lib, _l, 4, None) == -1
    assert b"null norm-sets descriptor" in lib.mmtta_last_error()


def test_norm_sets_finalize_checks_its_own_outputs_without_a_gpu():
    _l, lib = _lib()
    fake = ctypes.c_void_p(16)          # never dereferenced: the checks fail first
    st = lib.mmtta_norm_stats_finalize_sets(1, 1, None, 1, 2, 8, 64, 1e-5, 1, None, None, 0.1, None, None, None, None,
                                            None, None, fake, None, None, ctypes.byref(_l.NormSets(1, 0, 16, 16)), None)
    assert st == -1 and b"gamma_items" in lib.mmtta_last_error()
    st = lib.mmtta_norm_bwd_finalize_sets(1, 1, None, 1, 2, 8, 64, None, 1, None, None, None, fake, 0, None,
                                          ctypes.byref(_l.NormSets(1, 0, 16, 16)), None)
    assert st == -1 and b"dbeta needs dgamma" in lib.mmtta_last_error()


def test_norm_on_load_carries_the_per_item_flag():
    from multimodal_tta_amd import _lib
    assert _lib.norm_on_load().per_item == 0
    assert _lib.norm_on_load(per_item=True).per_item == 1
    assert ctypes.sizeof(_lib.NormOnLoad) == 56 and _lib.NormOnLoad.per_item.offset == 36
    assert ctypes.sizeof(_lib.NormSets) == 24


@pytest.mark.parametrize("method", ["tta_entmin", "tta_moddrop"])
def test_norm_sets_key_parses_from_the_method_configs(method):
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin

    cfg = compose(overrides=["task=brats", "model=unet", f"method={method}"])
    assert cfg["method"]["norm_sets"] is False
    assert get_plugin("entmin_tta")(cfg).norm_sets is False
    cfg = compose(overrides=["task=brats", "model=unet", f"method={method}", "method.norm_sets=true"])
    assert get_plugin("entmin_tta")(cfg).norm_sets is True


def test_norm_sets_entry_points_reject_overlapping_sets_without_a_gpu():
    """Several sets whose written vectors would overlap (stride below C) are refused: their first items would race on the
    same running statistics / affine gradients."""
    _l, lib = _lib()
    fake = ctypes.c_void_p(16)          # never dereferenced: the checks fail first
    st = lib.mmtta_norm_stats_finalize_sets(1, 1, None, 1, 4, 8, 64, 1e-5, 1, fake, fake, 0.1, None, None, None, None,
                                            None, None, None, None, None, ctypes.byref(_l.NormSets(1, 0, 16, 4)), None)
    assert st == -1 and b"running statistics of the sets would overlap" in lib.mmtta_last_error()
    st = lib.mmtta_norm_bwd_finalize_sets(1, 1, None, 1, 4, 8, 64, None, 1, None, None, fake, fake, 0, None,
                                          ctypes.byref(_l.NormSets(1, 0, 0, 16)), None)
    assert st == -1 and b"affine gradients of the sets would overlap" in lib.mmtta_last_error()
    # one set spanning the batch overlaps nothing: the stride checks do not apply (the call then fails later, on its null
    # partials, still before any launch)
    st = lib.mmtta_norm_bwd_finalize_sets(1, 1, None, 1, 4, 8, 64, None, 1, None, None, fake, fake, 0, None,
                                          ctypes.byref(_l.NormSets(4, 0, 0, 0)), None)
    assert st == -1 and b"overlap" not in lib.mmtta_last_error()
