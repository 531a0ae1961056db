"""EATA adaptation (``eata_tta``, ``method=tta_eata``): the host-side half, no GPU needed.

The config composes and the plugin reads its keys; the new entry points (weighted entropy, pseudo-label loss, Fisher
accumulation / scaling, penalty pass) refuse every bad argument with MMTTA_ERR_INVALID and a message before anything reaches
the device; the Fisher state round-trips through the mapping of parameter names."""
import ctypes

import pytest

INVALID = -1
FAKE = 4096          # a 16-byte aligned address that is never dereferenced: the checks fail first


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from multimodal_tta_amd import _lib
    return _lib, _lib.load()


def test_tta_eata_config_composes_and_the_plugin_reads_it():
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin

    cfg = compose(overrides=["task=brats", "dataset=brats", "model=unet", "method=tta_eata"])
    assert cfg["method"]["name"] == "eata_tta" and cfg["method"]["kind"] == "tta"
    e = cfg["method"]["eata"]
    assert e["e_margin"] == 0.4 and e["fisher_alpha"] == 2000.0 and e["fisher"]["volumes"] == 8 and e["fisher"]["path"] is None
    plug = get_plugin("eata_tta")(cfg)
    assert plug.e_margin == 0.4 and plug.fisher_alpha == 2000.0 and plug.fisher_volumes == 8 and plug.fisher_path is None
    assert plug.fused_update is False and plug.needs_fisher
    assert abs(plug.margin(3) - 0.4 * 0.6931471805599453) < 1e-12          # sigmoid head: K = 2
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_eata", "method.eata.e_margin=0.25",
                             "method.eata.fisher_alpha=0", "method.eata.fisher.volumes=3", "method.eata.fisher.path=f.pt"])
    plug = get_plugin("eata_tta")(cfg)
    assert plug.e_margin == 0.25 and plug.fisher_alpha == 0.0 and plug.fisher_volumes == 3 and plug.fisher_path == "f.pt"
    assert not plug.needs_fisher                                            # lambda = 0: no estimate is asked for
    plug.softmax = True
    assert abs(plug.margin(4) - 0.25 * 1.3862943611198906) < 1e-12         # softmax head: K = R
    assert [k for k, _, _ in plug.records] == ["losses", "kept", "penalty"]


def test_tta_eata_carries_every_key_of_tta_entmin():
    from multimodal_tta_amd.config import compose
    ent = compose(overrides=["task=brats", "model=unet", "method=tta_entmin"])["method"]
    eata = compose(overrides=["task=brats", "model=unet", "method=tta_eata"])["method"]
    assert set(eata) == set(ent) | {"eata"}
    for k in ent:
        if k != "name":
            assert eata[k] == ent[k], k


@pytest.mark.parametrize("key,value", [("e_margin", 0.0), ("e_margin", -1.0), ("e_margin", float("nan")),
                                       ("e_margin", float("inf")), ("fisher_alpha", -0.1), ("fisher_alpha", float("inf")),
                                       ("fisher_alpha", float("nan")), ("fisher_alpha", True)])
def test_eata_plugin_rejects_bad_hyper_parameters(key, value):
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_eata"])
    cfg["method"]["eata"][key] = value
    with pytest.raises(ValueError, match=f"method.eata.{key}"):
        get_plugin("eata_tta")(cfg)


@pytest.mark.parametrize("value", [0, -3, 2.5, True])
def test_eata_plugin_rejects_a_bad_fisher_volume_count(value):
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin
    cfg = compose(overrides=["task=brats", "model=unet", "method=tta_eata"])
    cfg["method"]["eata"]["fisher"]["volumes"] = value
    with pytest.raises(ValueError, match="method.eata.fisher.volumes"):
        get_plugin("eata_tta")(cfg)


def test_eata_is_a_registered_plugin():
    import multimodal_tta_amd  # noqa: F401
    from multimodal_tta_amd.registry import list_plugins
    assert "eata_tta" in list_plugins()
    assert {"entmin_tta", "sar_tta", "cotta_tta"} <= set(list_plugins())


def _tensor(_l, n=2, c=3, d=4, h=4, w=4, ptr=FAKE):
    ldc = 4
    return _l.Tensor(ptr, n, c, d, h, w, d * h * w * ldc, 1, h * w * ldc, w * ldc, ldc, _l.F32, _l.TENSOR_OWNS_PAD)


def _weighted(lib, _l, z=None, g=None, margin=0.3, keep_out=FAKE, partial=FAKE, loss=FAKE, kept=FAKE):
    z = _tensor(_l) if z is None else z
    g = _tensor(_l) if g is None else g
    return lib.mmtta_entropy_weighted_items(ctypes.byref(z), 0, margin, keep_out, ctypes.byref(g), partial, loss, kept, None)


def test_weighted_entropy_rejects_bad_arguments_without_a_gpu():
    _l, lib = _lib()
    for m in (float("nan"), float("inf"), float("-inf"), 0.0, -0.5):
        assert _weighted(lib, _l, margin=m) == INVALID
        assert b"margin" in lib.mmtta_last_error()
    assert _weighted(lib, _l, keep_out=None) == INVALID
    assert b"null mask output" in lib.mmtta_last_error()
    for kw in ({"partial": None}, {"loss": None}, {"kept": None}, {"z": _tensor(_l, ptr=None)}, {"g": _tensor(_l, ptr=None)}):
        assert _weighted(lib, _l, **kw) == INVALID
        assert b"null argument" in lib.mmtta_last_error()
    for bad in (_tensor(_l, n=3), _tensor(_l, c=2), _tensor(_l, d=5), _tensor(_l, h=3), _tensor(_l, w=2)):
        assert _weighted(lib, _l, g=bad) == INVALID
        assert b"shape mismatch" in lib.mmtta_last_error()
    assert lib.mmtta_entropy_weighted_partials(None) == -1
    z = _tensor(_l, n=3, d=4, h=4, w=4)
    assert lib.mmtta_entropy_weighted_partials(ctypes.byref(z)) == 2 * 3 * 1
    assert lib.mmtta_entropy_weighted_partials(ctypes.byref(z)) == lib.mmtta_entropy_filtered_partials(ctypes.byref(z))


def _pseudo(lib, _l, z=None, g=None, partial=FAKE, loss=FAKE):
    z = _tensor(_l) if z is None else z
    g = _tensor(_l) if g is None else g
    return lib.mmtta_pseudo_label_loss_items(ctypes.byref(z), 0, ctypes.byref(g), partial, loss, None)


def test_pseudo_label_loss_rejects_bad_arguments_without_a_gpu():
    _l, lib = _lib()
    for kw in ({"partial": None}, {"loss": None}, {"z": _tensor(_l, ptr=None)}, {"g": _tensor(_l, ptr=None)}):
        assert _pseudo(lib, _l, **kw) == INVALID
        assert b"null argument" in lib.mmtta_last_error()
    assert lib.mmtta_pseudo_label_loss_items(None, 0, None, FAKE, FAKE, None) == INVALID
    for bad in (_tensor(_l, n=3), _tensor(_l, c=2), _tensor(_l, d=5), _tensor(_l, h=3), _tensor(_l, w=2)):
        assert _pseudo(lib, _l, g=bad) == INVALID
        assert b"shape mismatch" in lib.mmtta_last_error()
    assert _pseudo(lib, _l, z=_tensor(_l, n=0), g=_tensor(_l, n=0)) == INVALID
    assert b"empty batch" in lib.mmtta_last_error()
    assert lib.mmtta_pseudo_label_partials(None) == -1
    assert lib.mmtta_pseudo_label_partials(ctypes.byref(_tensor(_l, n=3))) == 3


def test_fisher_accumulate_and_scale_reject_bad_arguments_without_a_gpu():
    _l, lib = _lib()

    def acc(f=FAKE, g=FAKE, n=64, sets=2, stride=128):
        return lib.mmtta_fisher_accumulate_sets(f, g, n, sets, stride, None)

    for kw in ({"f": None}, {"g": None}):
        assert acc(**kw) == INVALID
        assert b"null argument" in lib.mmtta_last_error()
    assert acc(n=-1) == INVALID
    assert b"n = -1" in lib.mmtta_last_error()
    for s in (0, -2):
        assert acc(sets=s) == INVALID
        assert b"sets" in lib.mmtta_last_error()
    for kw in ({"stride": 130}, {"stride": 60}, {"stride": -4}):
        assert acc(**kw) == INVALID
        assert b"set_stride" in lib.mmtta_last_error()
    assert lib.mmtta_fisher_scale(None, 64, 2.0, None) == INVALID
    assert b"null argument" in lib.mmtta_last_error()
    assert lib.mmtta_fisher_scale(FAKE, -4, 2.0, None) == INVALID
    for c in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.mmtta_fisher_scale(FAKE, 64, c, None) == INVALID
        assert b"count" in lib.mmtta_last_error()


def _penalty(lib, w=FAKE, g=FAKE, f=FAKE, src=FAKE, n=64, sets=2, replicas=3, stride=128, lam=1.0, partial=FAKE, penalty=FAKE):
    return lib.mmtta_fisher_penalty_sets(w, g, f, src, n, sets, replicas, stride, lam, partial, penalty, None)


def test_fisher_penalty_rejects_bad_arguments_without_a_gpu():
    _l, lib = _lib()
    for lam in (float("nan"), float("inf"), -1e-3, 3e38):
        assert _penalty(lib, lam=lam) == INVALID
        assert b"lambda" in lib.mmtta_last_error()
    for kw in ({"w": None}, {"g": None}, {"f": None}, {"src": None}, {"partial": None}, {"penalty": None}):
        assert _penalty(lib, **kw) == INVALID
        assert b"null argument" in lib.mmtta_last_error()
    for kw in ({"n": 6}, {"stride": 130}, {"n": -4}):
        assert _penalty(lib, **kw) == INVALID
        assert b"multiples of 4" in lib.mmtta_last_error()
    for kw in ({"n": 256}, {"sets": 4}, {"sets": 0}):
        assert _penalty(lib, **kw) == INVALID
        assert b"do not fit" in lib.mmtta_last_error()
    assert lib.mmtta_fisher_penalty_partials(64, 2) == 2
    assert lib.mmtta_fisher_penalty_partials(-4, 1) == -1
    assert lib.mmtta_fisher_penalty_partials(64, 0) == -1


def _refs():
    import torch
    from multimodal_tta_amd.engine import GROUP_FROZEN, GROUP_NO_DECAY, ParamRef
    shapes = {"a.weight": (2, 3, 1, 1, 1), "a.bias": (2,), "n.weight": (5,), "frozen.weight": (3,)}
    refs, off = [], 0
    for name, shape in shapes.items():
        r = ParamRef(name, torch.nn.Parameter(torch.zeros(shape)))
        r.offset = off
        off += (r.numel + 3) // 4 * 4
        r.group = GROUP_FROZEN if name.startswith("frozen") else GROUP_NO_DECAY
        refs.append(r)
    return refs, 8 + 4 + 8          # the trainable span ends where the frozen parameter starts


def test_fisher_state_round_trips_through_the_parameter_names():
    import io

    import torch
    from multimodal_tta_amd.eata import fisher_from_state, fisher_to_state
    from multimodal_tta_amd.ops import MmttaError
    refs, n_train = _refs()
    span = torch.zeros(n_train)
    for r in refs[:3]:
        span[r.offset:r.offset + r.numel] = torch.rand(r.numel) + 0.5
    state = fisher_to_state(span, refs, 5)
    assert state["volumes"] == 5 and set(state["fisher"]) == {"a.weight", "a.bias", "n.weight"}
    assert state["fisher"]["a.weight"].shape == (2, 3, 1, 1, 1)
    buf = io.BytesIO()
    torch.save(state, buf)          # the file form: loaded with weights_only=True
    buf.seek(0)
    loaded = torch.load(buf, map_location="cpu", weights_only=True)
    assert torch.equal(fisher_from_state(loaded, refs, n_train, "cpu"), span)
    missing = {"volumes": 5, "fisher": {k: v for k, v in state["fisher"].items() if k != "a.bias"}}
    with pytest.raises(MmttaError, match="a.bias"):
        fisher_from_state(missing, refs, n_train, "cpu")
    shaped = {"volumes": 5, "fisher": dict(state["fisher"], **{"n.weight": torch.zeros(4)})}
    with pytest.raises(MmttaError, match="n.weight"):
        fisher_from_state(shaped, refs, n_train, "cpu")
    with pytest.raises(MmttaError):
        fisher_from_state({"fisher": state["fisher"]}, refs, n_train, "cpu")
