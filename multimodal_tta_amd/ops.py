"""Thin, typed Python wrappers over the C ABI (one function per entry point of include/mmtta.h).

Activations are channels-last views: torch tensors of logical shape [N, D, H, W, C] with unit
stride along C (possibly a channel slice of a wider buffer, which is how ``torch.cat`` of the
reference - src/models/unet_multimodal_midfusion.py:135, monai SkipConnection - disappears:
producers write straight into their slice).  Everything runs on torch's current CUDA stream, so
the calls can be captured into a graph.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import (BF16, CONV_DGRAD, CONV_FWD, CONVT_DGRAD, CONVT_FWD, F32, NORM_BATCH, NORM_GROUP, NORM_INSTANCE,
                   ConvDesc, ConvEpilogue, ConvPlan, MmttaError, ParamSets, check, desc_cl, desc_ncdhw, ptr, stream_ptr)

NORM_KINDS = {"INSTANCE": NORM_INSTANCE, "BATCH": NORM_BATCH, "GROUP": NORM_GROUP}
PRECISIONS = {"fp32": F32, "f32": F32, "bf16": BF16}


def _require_cuda() -> None:
    if not torch.cuda.is_available():
        raise MmttaError("the adaptation path needs an MI355X (gfx950) device; no CPU fallback exists")


# ----------------------------------------------------------------------------- workspace
class _WorkspaceSelectors(type):
    """`Workspace.slot / lane / frozen` select the scratch buffer of the launches that follow; they are per THREAD (a second
    Python thread driving its own lane does not disturb another thread's selection), with the old class-attribute syntax."""
    _tls = threading.local()

    def _get(cls, name, default):
        return getattr(_WorkspaceSelectors._tls, name, default)

    slot = property(lambda cls: cls._get("slot", 0), lambda cls, v: setattr(_WorkspaceSelectors._tls, "slot", int(v)))
    lane = property(lambda cls: cls._get("lane", 0), lambda cls, v: setattr(_WorkspaceSelectors._tls, "lane", int(v)))
    frozen = property(lambda cls: cls._get("frozen", False), lambda cls, v: setattr(_WorkspaceSelectors._tls, "frozen", bool(v)))


class Workspace(metaclass=_WorkspaceSelectors):
    """One grow-only scratch buffer per device, shared by split-K convs and weight gradients
    (stream ordered).  It must reach its final size before a graph capture starts.

    A buffer that has to grow is REPLACED, never freed: hipGraphs captured for an earlier (smaller) input shape have
    the old address baked into their kernel nodes and stay replayable (the adaptation plugin keeps one graph per input
    shape); handing the old block back to the caching allocator would let those replays scribble over whatever tensor
    received it next."""

    _buffers: Dict[Tuple[int, int, int], torch.Tensor] = {}
    _retired: list = []     # superseded buffers, kept alive for the graphs that reference them
    captured: set = set()   # (device index, lane) pairs on which a hipGraph has been captured (the plugin records them)
    min_bytes = 1 << 20     # first allocation of a slot (tests lower it to provoke growth with small shapes)
    # frozen / slot / lane: thread-local selectors (metaclass above).  slot 0: main launch sequence, 1..: the side streams of
    # the weight gradients (engine.ConvLayer.wgrad); lane: runtimes that run concurrently on different streams keep separate scratch

    @classmethod
    def get(cls, nbytes: int, device: torch.device) -> torch.Tensor:
        """The scratch buffer of the current slot: kernels of the two streams run concurrently and must not share
        scratch."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        key = (idx, cls.slot, cls.lane)
        buf = cls._buffers.get(key)
        if buf is None or buf.numel() < nbytes:
            if cls.frozen:
                raise MmttaError("workspace would have to grow during graph capture; run one eager warm-up step first")
            if buf is not None and (idx, cls.lane) in cls.captured:
                cls._retired.append(buf)        # a captured graph may replay with the old address: keep the block alive
            # grow geometrically: a run over volumes of many sizes retires O(log) buffers, not one per new size; a buffer no
            # graph can reference is simply dropped (the allocator reuses it)
            grown = 0 if buf is None else buf.numel() + buf.numel() // 2
            buf = torch.empty(max(nbytes, grown, cls.min_bytes), dtype=torch.uint8, device=device)
            cls._buffers[key] = buf
        return buf


# ----------------------------------------------------------------------------- streams / hardware queues
_HELPER_STREAMS: Dict[int, "torch.cuda.Stream"] = {}


def helper_stream(device) -> "torch.cuda.Stream":
    """One reusable non-default stream per device (graph capture from the default stream)."""
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    if idx not in _HELPER_STREAMS:
        _HELPER_STREAMS[idx] = torch.cuda.Stream(device=idx)
    return _HELPER_STREAMS[idx]


_QUEUE_WARNED = False


def hw_queue_status() -> dict:
    """How many hardware queues the HIP runtime of this process multiplexes its streams over, as far as the package can
    know: GPU_MAX_HW_QUEUES is read when HIP starts, so a host that initialised the GPU BEFORE importing this package runs
    with whatever the environment held then (the runtime's default is 4)."""
    import multimodal_tta_amd as pkg
    raw = pkg.HW_QUEUES_AT_HIP_START
    try:
        queues = int(raw) if raw is not None else 4
    except ValueError:
        queues = 4
    return {"queues": queues, "hip_started_before_import": bool(pkg.HIP_STARTED_BEFORE_IMPORT), "env_at_hip_start": raw}


def lanes_effective(count: int) -> int:
    """Lanes that can be expected to run on their own hardware queue: with the runtime's default of 4 queues the lanes beyond
    the second have been measured sharing a queue with an earlier stream (profiles/r02_hw_queues.txt)."""
    q = hw_queue_status()["queues"]
    return int(count) if q >= 8 else min(int(count), 2)


def lane_streams(count: int, device) -> list:
    """`count` streams for volumes adapted concurrently on one GPU, each bound to its OWN hardware queue.

    The HIP runtime gives a stream its hardware queue at the stream's first command and has GPU_MAX_HW_QUEUES of them
    (8: set by the package at import, read at HIP start-up); once they are used up, later streams share the queue of an
    existing one, and two lanes on one queue serialise (measured, 4 lanes: 36 vs 53 volumes/s for the same code,
    depending only on which streams had been touched first).  So the lanes' streams are created AND given their first
    command here, before any other stream of the process does work."""
    global _QUEUE_WARNED
    st = hw_queue_status()
    if int(count) > 2 and st["queues"] < 8 and not _QUEUE_WARNED:
        _QUEUE_WARNED = True
        import warnings
        warnings.warn(
            f"{count} lanes requested but the HIP runtime of this process started with GPU_MAX_HW_QUEUES="
            f"{st['env_at_hip_start'] or 'unset (4 queues)'}"
            + (" (the GPU was initialised before multimodal_tta_amd was imported, so the package could not set it)"
               if st["hip_started_before_import"] else "")
            + ": lanes beyond the second share a hardware queue and serialise - measured 42 instead of 50 volumes/s for four "
              "lanes (profiles/r02_hw_queues.txt).  Export GPU_MAX_HW_QUEUES=8 before the first CUDA call, or use "
              "method.group (volumes batched into one launch sequence) with method.lanes <= 2.", RuntimeWarning)
    device = torch.device(device)
    streams = [torch.cuda.Stream(device=device) for _ in range(int(count))]
    for s in streams:
        with torch.cuda.stream(s):
            torch.zeros(1, device=device)
    torch.cuda.synchronize(device)
    return streams


# ----------------------------------------------------------------------------- library options
_OPTION_EPOCH = 0


def set_option(key: int, value: int) -> int:
    """``mmtta_set_option`` + invalidation of every cached launch plan: the launch-geometry knobs (split-K thresholds,
    weight-gradient slab counts) change workspace sizes and the number of statistics rows a convolution writes, so a
    plan made under the old value must not size buffers for a launch made under the new one.  Set options BEFORE the
    first adaptation step of a plugin: graphs already captured keep the geometry they were captured with."""
    global _OPTION_EPOCH
    prev = int(_lib.load().mmtta_set_option(int(key), int(value)))
    _OPTION_EPOCH += 1
    return prev


# launch-geometry knobs (include/mmtta.h: per batch item) measured best for 4 volumes in flight on one GPU; the optimum
# scales inversely with the volumes in flight (lanes x group): one volume alone wants 384 / 512 / 512 / 1024 (round 1), sixteen
# want 24 / 32 / 32 / 64 (profiles/r03_tuning_sweep.txt) - the launches of all volumes together should fill the chip about once
TUNE_AT_4 = {2: 96, 3: 128, 4: 128, 5: 256, 12: 128}      # SPLITK_BELOW, SPLITK_TARGET, WGRAD_WORKGROUPS, WGRAD_THIN_SLABS, CLASS_FUSED_MIN_WORKGROUPS
if os.environ.get("MMTTA_SPLITK_AT4"):                    # measurement switch: "below,target" at 4 volumes in flight
    TUNE_AT_4[2], TUNE_AT_4[3] = (int(v) for v in os.environ["MMTTA_SPLITK_AT4"].split(","))
_TUNED_FOR: Optional[int] = None


def tune_for_volumes_in_flight(volumes: int) -> Dict[int, int]:
    """Set the four launch-geometry knobs for `volumes` volumes in flight on this GPU (method.lanes x method.group).  Process
    wide, like the knobs themselves; call before the first adaptation step (cached plans are dropped, captured graphs keep the
    geometry they were captured with).  MMTTA_NO_AUTOTUNE=1 leaves the knobs alone (sweeps set them by hand)."""
    global _TUNED_FOR
    volumes = max(1, int(volumes))
    vals = {k: max(1, (v * 4 + volumes - 1) // volumes) for k, v in TUNE_AT_4.items()}
    if os.environ.get("MMTTA_NO_AUTOTUNE", "0") == "1" or _TUNED_FOR == volumes:
        return vals
    for k, v in vals.items():
        set_option(k, v)
    _TUNED_FOR = volumes
    return vals


ACT_NONE, ACT_RELU, ACT_LEAKY_RELU = _lib.ACT_NONE, _lib.ACT_RELU, _lib.ACT_LEAKY_RELU


# ----------------------------------------------------------------------------- norm on load
@dataclass
class NL:
    """Pending normalisation(+activation) of a raw conv output; consumers apply it when they read.  The activation is
    `act` (ACT_NONE / ACT_RELU / ACT_LEAKY_RELU with `negative_slope`) or, when `act` is None, ReLU if `relu`."""
    mean: torch.Tensor
    rstd: torch.Tensor
    gamma: Optional[torch.Tensor] = None
    beta: Optional[torch.Tensor] = None
    relu: bool = True
    scale: Optional[torch.Tensor] = None     # precombined rstd*gamma and beta - mean*rstd*gamma (fast consumer path)
    shift: Optional[torch.Tensor] = None
    per_item: bool = False                   # gamma / beta are [N*C], one copy per batch item (norm_stats_finalize_sets)
    act: Optional[int] = None                # ACT_* code; None: ACT_RELU if relu else ACT_NONE
    negative_slope: float = 0.0              # ACT_LEAKY_RELU: v > 0 ? v : negative_slope * v

    def struct(self) -> _lib.NormOnLoad:
        return _lib.norm_on_load(self.mean, self.rstd, self.gamma, self.beta, self.relu, self.scale, self.shift,
                                 self.per_item, self.act, self.negative_slope)


def _nl_ref(nl: Optional[NL]):
    if nl is None:
        return None, None
    s = nl.struct()
    return s, C.byref(s)


# ----------------------------------------------------------------------------- layout
def row_pad(c: int, dtype: torch.dtype = torch.float32) -> int:
    """Padded channel count of a voxel row: 16-byte rows for fp32 (4 channels), and for bf16 rows of more than 4 channels
    (8 channels: the implicit GEMM stages 8 channels per 16-byte load); a bf16 row of <= 4 channels is 8 bytes."""
    if dtype == torch.bfloat16 and c > 4:
        return (c + 7) // 8 * 8
    return (c + 3) // 4 * 4


def new_cl(n: int, d: int, h: int, w: int, c: int, device, ldc: Optional[int] = None, zero: bool = False,
           dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Allocate a channels-last buffer [n,d,h,w,ldc] and return the [.., :c] view."""
    ldc = c if ldc is None else ldc
    buf = (torch.zeros if zero else torch.empty)((n, d, h, w, ldc), dtype=dtype, device=device)
    if ldc == c:
        return buf
    view = buf[..., :c]
    view._mmtta_owns_pad = True     # this view owns the pad lanes of its rows (any further slice does not)
    return view


def to_cl(x: torch.Tensor, out: Optional[torch.Tensor] = None, ldc: Optional[int] = None) -> torch.Tensor:
    """NCDHW -> channels-last (reference tensor contract: src/datasets/brats.py:343-347)."""
    _require_cuda()
    n, c, d, h, w = x.shape
    if out is None:
        out = new_cl(n, d, h, w, c, x.device, ldc if ldc is not None else (c + 3) // 4 * 4, zero=True)
    src = desc_ncdhw(x)
    dst = desc_cl(out)
    check(_lib.load().mmtta_copy_strided(C.byref(src), C.byref(dst), stream_ptr()), "copy_strided")
    return out


def from_cl(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """channels-last -> contiguous NCDHW (what reference src/evaluation/seg_eval.py:300 expects back)."""
    n, d, h, w, c = x.shape
    if out is None:
        out = torch.empty((n, c, d, h, w), dtype=torch.float32, device=x.device)
    src = desc_cl(x)
    # describe `out` with the logical (n,c,d,h,w) of src
    dst = desc_ncdhw(out)
    check(_lib.load().mmtta_copy_strided(C.byref(src), C.byref(dst), stream_ptr()), "copy_strided")
    return out


# ----------------------------------------------------------------------------- profiling hook
IGEMM_KERNELS = ["igemm_f32_kernel<1,4,8,8,8,8>", "igemm_f32_kernel<2,4,4,8,8,16>", "igemm_f32_kernel<4,4,4,4,8,32>",
                 "igemm_f32_kernel<1,1,4,4,8,8>", "igemm_f32_kernel<2,2,4,4,8,8>", "igemm_f32_kernel<4,4,4,4,8,8>",
                 "direct_conv_kernel",
                 "igemm_kernel<1,4,8,8,8,16,bf16>", "igemm_kernel<2,4,4,8,8,32,bf16>", "igemm_kernel<4,4,4,4,8,32,bf16>",
                 "igemm_kernel<1,1,4,4,8,16,bf16>", "igemm_kernel<2,2,4,4,8,16,bf16>", "igemm_kernel<4,4,4,4,8,16,bf16>",
                 "direct_chan_kernel", "igemm_kernel<1,2,4,8,8,16,bf16>", "igemm_cls8_kernel<16,bf16>"]


WGRAD_KERNELS = ["wgrad_f32_kernel<4,4,8,7>", "wgrad_f32_kernel<2,2,8,7>", "wgrad_f32_kernel<4,4,8,1>", "wgrad_small_kernel",
                 "wgrad_bf16_kernel<4,4,1>", "wgrad_bf16_kernel<2,4,2>", "wgrad_tiny_kernel",
                 "wgrad_tr_kernel<4,8,1>", "wgrad_tr_kernel<2,4,2>", "wgrad_tr1_kernel", "wgrad_thin_tr_kernel"]


class KernelProfiler:
    """Brackets every conv launch with events on the launch stream and books its algorithmic FLOPs
    (bench.py roofline: FLOPs per launch / measured duration).  Off unless installed in ops.PROFILER."""

    def __init__(self, reps: int = 1, what_if: Sequence[str] = ()):
        self.records = []   # (kernel name, launches, flops, start event, end event)
        self.what_if = tuple(what_if)       # "no_norm_on_load", "no_stats": see ConvOp._run
        # reps > 1: every profiled call is issued `reps` more times back to back between the two events, so the
        # queue stays ahead of the GPU and the host's launch latency does not leak into the measured duration
        # (outputs of accumulating calls are then wrong: use only in a throw-away pass)
        self.reps = max(1, int(reps))

    def begin(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def end(self, name: str, launches: int, flops: float, e0, detail: str = "", nbytes: float = 0.0) -> None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.records.append((name, launches, flops, e0, e1, detail, nbytes))

    def by_layer(self):
        """Per (kernel, layer shape) totals: scripts/layer_times.py prints them."""
        torch.cuda.synchronize()
        out = {}
        for name, launches, flops, e0, e1, detail, nbytes in self.records:
            d = out.setdefault((name, detail), {"launches": 0, "flops": 0.0, "ms": 0.0, "bytes": 0.0})
            d["launches"] += launches
            d["flops"] += flops
            d["bytes"] += nbytes
            d["ms"] += e0.elapsed_time(e1)
        return out

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, launches, flops, e0, e1, _detail, nbytes in self.records:
            d = out.setdefault(name, {"launches": 0, "flops": 0.0, "ms": 0.0, "calls": 0, "bytes": 0.0})
            d["launches"] += launches
            d["flops"] += flops
            d["bytes"] += nbytes
            d["ms"] += e0.elapsed_time(e1)
            d["calls"] += 1
        return out


PROFILER: Optional[KernelProfiler] = None


# ----------------------------------------------------------------------------- convolution
class ConvOp:
    """One Conv3d / ConvTranspose3d module's kernels: forward, input gradient, weight gradient.

    Holds the two packed weight images (forward and input-gradient orientation), refreshed by
    ``pack`` after every optimizer step.
    """

    def __init__(self, cin: int, cout: int, ksize: int, stride: int, transposed: bool, device, dtype: int = F32,
                 n_sets: int = 1):
        """``n_sets`` > 1: the op holds that many packed weight images back to back - one per parameter set of a group of
        volumes (x the members of a set family, e.g. the M modality encoders); which batch item reads which image is said by
        ``set_param_sets`` (mmtta_param_sets)."""
        _require_cuda()
        self.cin, self.cout, self.k, self.stride, self.transposed = cin, cout, ksize, stride, transposed
        self.device = torch.device(device)
        fwd_op, dg_op = (CONVT_FWD, CONVT_DGRAD) if transposed else (CONV_FWD, CONV_DGRAD)
        self.d_fwd = ConvDesc(fwd_op, ksize, stride, cin, cout, dtype)
        self.d_dgrad = ConvDesc(dg_op, ksize, stride, cin, cout, dtype)
        lib = _lib.load()
        nb_f = lib.mmtta_conv_packed_bytes(C.byref(self.d_fwd))
        nb_d = lib.mmtta_conv_packed_bytes(C.byref(self.d_dgrad))
        if nb_f < 0 or nb_d < 0:
            check(-2, "conv_packed_bytes")
        self.n_sets = max(1, int(n_sets))
        self.nb_fwd, self.nb_dgrad = int(nb_f), int(nb_d)        # bytes of ONE image (multiples of 16)
        # zero-filled once: the pack kernels write only the entries a weight owns (padding and, for the gather-GEMM
        # up-convolution image, the slots no tap maps to stay zero)
        self.packed_fwd = torch.zeros(nb_f * self.n_sets, dtype=torch.uint8, device=self.device)
        self.packed_dgrad = torch.zeros(nb_d * self.n_sets, dtype=torch.uint8, device=self.device)
        self._plans: Dict[Tuple, ConvPlan] = {}
        self.need_dgrad = True
        # per-item parameter sets (None: one set for the whole batch).  `sets_ctl.use_sets` (the owning runtime) switches
        # them on for the launches of a volume group and off for the plain batched forward of the nn.Module facade
        self.sets_grouped: Optional[Tuple[ParamSets, ParamSets]] = None      # (forward image, input-gradient image)
        self.sets_plain: Optional[Tuple[ParamSets, ParamSets]] = None        # a family of modules inside ONE weight set
        self.sets_ctl = None
        self.shared_sets = False
        self._sets_views: Dict[Tuple, ParamSets] = {}      # sets_grouped with items_per_set x views (filled by _sets)

    def set_param_sets(self, items_per_set: int, inner: int, weight_outer: int, weight_inner: int, bias_outer: int,
                       bias_inner: int, ctl, shared: bool = False) -> None:
        """Batch item n uses set q = n // items_per_set, stored (q // inner) outer + (q % inner) inner strides behind set 0;
        the packed images of the op are laid out [outer][inner].  ``shared``: the outer sets are all alike (a frozen layer:
        every volume of a group reads the images and bias of set 0, outer strides 0)."""
        if self.n_sets % inner:
            raise MmttaError(f"{self.n_sets} packed images cannot hold families of {inner} sets")
        mk = lambda nb, outer: ParamSets(int(items_per_set), int(inner), nb * int(inner) * outer, nb, int(weight_outer) * outer,
                                         int(weight_inner), int(bias_outer) * outer, int(bias_inner))
        o = 0 if shared else 1
        self.sets_grouped = (mk(self.nb_fwd, o), mk(self.nb_dgrad, o))
        self._sets_views = {}
        self.shared_sets = bool(shared)
        if shared and self.n_sets > inner:
            # only the images of set 0's members are packed and read: the others are not kept
            self.packed_fwd = torch.zeros(self.nb_fwd * int(inner), dtype=torch.uint8, device=self.device)
            self.packed_dgrad = torch.zeros(self.nb_dgrad * int(inner), dtype=torch.uint8, device=self.device)
        # without a volume group (the nn.Module facade: one weight set for the whole batch) a family of modules - the M
        # modality encoders as the batch items of one launch - still selects its member's weights: outer strides 0
        self.sets_plain = (mk(self.nb_fwd, 0), mk(self.nb_dgrad, 0)) if inner > 1 else None
        self.sets_ctl = ctl

    def _sets(self, desc) -> Optional[ParamSets]:
        grouped = self.sets_ctl is not None and getattr(self.sets_ctl, "use_sets", False)
        pair = self.sets_grouped if grouped else self.sets_plain
        if pair is None:
            return None
        dgrad = int(desc.op) in (CONV_DGRAD, CONVT_DGRAD)
        sets = pair[1] if dgrad else pair[0]
        views = int(getattr(self.sets_ctl, "views", 1))
        if views == 1:
            return sets
        # every set brings `views` consecutive batch items (engine.Runtime.views: the views of a volume - or, in a family of
        # modules, of one member's input) that share it; its weight gradient sums over them
        key = (grouped, dgrad, views)
        scaled = self._sets_views.get(key)
        if scaled is None:
            scaled = ParamSets.from_buffer_copy(sets)
            scaled.items_per_set = int(sets.items_per_set) * views
            self._sets_views[key] = scaled
        return scaled

    def packed_image(self, dgrad: bool, index: int) -> torch.Tensor:
        """The packed image of parameter set ``index`` (a view)."""
        nb, buf = (self.nb_dgrad, self.packed_dgrad) if dgrad else (self.nb_fwd, self.packed_fwd)
        return buf[index * nb:(index + 1) * nb]

    def weight_shape(self) -> Tuple[int, ...]:
        k = self.k
        return (self.cin, self.cout, k, k, k) if self.transposed else (self.cout, self.cin, k, k, k)

    def pack(self, weight: torch.Tensor, index: int = 0) -> None:
        """Refresh the packed images of parameter set ``index`` from its master weight."""
        if tuple(weight.shape) != self.weight_shape() or weight.dtype != torch.float32 or not weight.is_contiguous():
            raise MmttaError(f"weight must be contiguous fp32 {self.weight_shape()}, got {tuple(weight.shape)}")
        lib = _lib.load()
        s = stream_ptr()
        check(lib.mmtta_conv_pack_weights(C.byref(self.d_fwd), ptr(weight), ptr(self.packed_image(False, index)), s), "pack fwd")
        if self.need_dgrad:
            check(lib.mmtta_conv_pack_weights(C.byref(self.d_dgrad), ptr(weight), ptr(self.packed_image(True, index)), s),
                  "pack dgrad")

    def out_shape(self, x: torch.Tensor) -> Tuple[int, int, int, int, int]:
        n, d, h, w, _ = x.shape
        if self.transposed:
            return (n, d * 2, h * 2, w * 2, self.cout)
        if self.stride == 1:
            return (n, d, h, w, self.cout)
        return (n, (d + 1) // 2, (h + 1) // 2, (w + 1) // 2, self.cout)

    def plan(self, desc: ConvDesc, x: torch.Tensor, y: torch.Tensor) -> ConvPlan:
        # the planned geometry (tile form, statistics rows) also depends on storage type, strides and pointer alignment
        # (class-fused / lean / row-loader gates): all of it is part of the key
        key = (desc.op, tuple(x.shape), tuple(y.shape), x.dtype, y.dtype, x.stride(), y.stride(), x.data_ptr() % 16,
               y.data_ptr() % 16, _OPTION_EPOCH)
        p = self._plans.get(key)
        if p is None:
            p = ConvPlan()
            dx, dy = desc_cl(x), desc_cl(y)
            check(_lib.load().mmtta_conv_plan(C.byref(desc), C.byref(dx), C.byref(dy), C.byref(p)), "conv_plan")
            self._plans[key] = p
        return p

    def stats_rows(self, x: torch.Tensor, y: torch.Tensor) -> int:
        return int(self.plan(self.d_fwd, x, y).stats_rows)

    def _run(self, desc, packed, x, x_nl, bias, y, accumulate, stats, add, add_nl):
        p = self.plan(desc, x, y)
        ws = Workspace.get(int(p.workspace_bytes), x.device) if p.workspace_bytes > 0 else None
        dx, dy = desc_cl(x), desc_cl(y)
        nls, nlr = _nl_ref(x_nl)
        epi = None
        keep = None
        if add is not None:
            keep = desc_cl(add)
            epi = ConvEpilogue(C.pointer(keep), add_nl.struct() if add_nl is not None else _lib.norm_on_load())
        sets = self._sets(desc)
        def launch(nlr=nlr, stats=stats):
            check(
                _lib.load().mmtta_conv_run_sets(
                    C.byref(desc), C.byref(dx), nlr, ptr(packed), ptr(bias), C.byref(epi) if epi is not None else None,
                    C.byref(dy), 1 if accumulate else 0, ptr(stats), ptr(ws), int(p.workspace_bytes),
                    C.byref(sets) if sets is not None else None, stream_ptr()),
                "conv_run")

        launch()
        if PROFILER is not None:
            # what-if timings (scripts/layer_times.py --what-if): the TIMED repeats alone drop the norm-on-load of the input
            # or the statistics rows of the output; the real launch above already produced the step's values
            kw = {}
            if "no_norm_on_load" in PROFILER.what_if:
                kw["nlr"] = None
            if "no_stats" in PROFILER.what_if:
                kw["stats"] = None
            e0 = PROFILER.begin()
            for _ in range(PROFILER.reps):
                launch(**kw)
            PROFILER.end(self._kernel_name(p.config, desc, x, y), PROFILER.reps,
                         self.flops(x, y, desc) * PROFILER.reps, e0, self._detail(desc.op, x),
                         self.io_bytes(x, y, packed) * PROFILER.reps)

    def _kernel_name(self, config: int, desc, x: torch.Tensor, y: torch.Tensor) -> str:
        """Profiler label of the kernel a conv_run call dispatches to (mirrors csrc: the thin layers have matrix-core
        variants in bf16 mode; 'bf16' in the label selects the bf16 MFMA peak in bench.py)."""
        name = IGEMM_KERNELS[config]
        if int(desc.dtype) == BF16:
            if config == 13 and (self.cin_of(desc) >= 2 or self.cout_of(desc) > 32):
                return "chan_mfma_kernel<bf16>"
            if config == 6 and int(desc.op) == CONVT_FWD and self.k == 3 and self.stride == 2 and self.cin in (32, 64):
                return "upconv8_kernel<bf16>"
        return name

    def cin_of(self, desc) -> int:
        """Channels the op READS (dgrad ops run the layer backwards)."""
        return self.cout if int(desc.op) in (CONV_DGRAD, CONVT_DGRAD) else self.cin

    def cout_of(self, desc) -> int:
        return self.cin if int(desc.op) in (CONV_DGRAD, CONVT_DGRAD) else self.cout

    def _detail(self, op: int, x: torch.Tensor) -> str:
        kind = {CONV_FWD: "fwd", CONV_DGRAD: "dgrad", CONVT_FWD: "fwdT", CONVT_DGRAD: "dgradT", -1: "wgrad"}[op]
        return (f"{kind} {'convT' if self.transposed else 'conv'} {self.cin}->{self.cout} k{self.k}s{self.stride} "
                f"read {x.shape[1]}x{x.shape[2]}x{x.shape[3]}")

    def flops(self, x: torch.Tensor, y: torch.Tensor, desc=None) -> float:
        """Algorithmic FLOPs (2 x MACs) of one forward / input-gradient / weight-gradient of this module for
        the tensor pair (read, produced): MACs = coarse-grid voxels x Cin x Cout x taps."""
        coarse = min(x.shape[1] * x.shape[2] * x.shape[3], y.shape[1] * y.shape[2] * y.shape[3]) * x.shape[0]
        return 2.0 * coarse * self.cin * self.cout * self.k ** 3

    @staticmethod
    def io_bytes(a: torch.Tensor, b: torch.Tensor, w: torch.Tensor) -> float:
        """Algorithmic bytes of one call (SURVEY.md section 8d convention): each activation tensor of the call once
        (logical channels, storage element size) plus the weight image / weight gradient once."""
        return float(a.numel() * a.element_size() + b.numel() * b.element_size() + w.numel() * w.element_size())

    def forward(self, x: torch.Tensor, x_nl: Optional[NL], bias: Optional[torch.Tensor], y: torch.Tensor,
                stats: Optional[torch.Tensor] = None, add: Optional[torch.Tensor] = None,
                add_nl: Optional[NL] = None, accumulate: bool = False) -> None:
        self._run(self.d_fwd, self.packed_fwd, x, x_nl, bias, y, accumulate, stats, add, add_nl)

    # ---- the head convolution with the entropy objective as its tail (MMTTA_OPT_HEAD_LOSS_PAIR bit 0)
    def _head_loss_args(self, x, x_nl, y, dlogits, add, add_nl):
        dx, dy, dg = desc_cl(x), desc_cl(y), desc_cl(dlogits)
        nls, nlr = _nl_ref(x_nl)
        epi = keep = None
        if add is not None:
            keep = desc_cl(add)
            epi = ConvEpilogue(C.pointer(keep), add_nl.struct() if add_nl is not None else _lib.norm_on_load())
        return dx, dy, dg, nls, nlr, keep, epi

    def head_loss_eligible(self, x: torch.Tensor, x_nl: Optional[NL], y: torch.Tensor, dlogits: torch.Tensor,
                           add: Optional[torch.Tensor] = None, add_nl: Optional[NL] = None, softmax: bool = False,
                           per_item: bool = True) -> bool:
        """Whether ``forward_head_loss`` takes this call (mmtta_conv_head_loss_eligible; host only, launches nothing)."""
        dx, dy, dg, nls, nlr, keep, epi = self._head_loss_args(x, x_nl, y, dlogits, add, add_nl)
        r = int(_lib.load().mmtta_conv_head_loss_eligible(C.byref(self.d_fwd), C.byref(dx), nlr,
                                                          C.byref(epi) if epi is not None else None, C.byref(dy), C.byref(dg),
                                                          1 if softmax else 0, 1 if per_item else 0))
        if r < 0:
            check(r, "conv_head_loss_eligible")
        return r == 1

    def head_loss_partials(self, x: torch.Tensor, y: torch.Tensor) -> int:
        dx, dy = desc_cl(x), desc_cl(y)
        n = int(_lib.load().mmtta_conv_head_loss_partials(C.byref(self.d_fwd), C.byref(dx), C.byref(dy)))
        if n < 0:
            check(-2, "conv_head_loss_partials")
        return n

    def forward_head_loss(self, x: torch.Tensor, x_nl: Optional[NL], bias: Optional[torch.Tensor], y: torch.Tensor,
                          dlogits: torch.Tensor, partial: torch.Tensor, loss: torch.Tensor, add: Optional[torch.Tensor] = None,
                          add_nl: Optional[NL] = None, softmax: bool = False, per_item: bool = True) -> None:
        """``forward`` followed by ``entropy_loss_items(y, dlogits, ...)`` without the logits: ``y`` is described, not
        written; ``dlogits`` bit for bit and ``loss`` [N] as the two calls give them (mmtta_conv_head_loss_run_sets).  Refused
        (MmttaError) for a call ``head_loss_eligible`` says no to."""
        if loss.numel() < (y.shape[0] if per_item else 1):
            raise MmttaError("forward_head_loss: one loss slot per batch item")
        if partial.dtype != torch.float64 or partial.numel() < self.head_loss_partials(x, y):
            raise MmttaError("forward_head_loss: `partial` holds head_loss_partials(x, y) doubles")
        dx, dy, dg, nls, nlr, keep, epi = self._head_loss_args(x, x_nl, y, dlogits, add, add_nl)
        sets = self._sets(self.d_fwd)

        def launch():
            check(_lib.load().mmtta_conv_head_loss_run_sets(
                C.byref(self.d_fwd), C.byref(dx), nlr, ptr(self.packed_fwd), ptr(bias), C.byref(epi) if epi is not None else None,
                C.byref(dy), C.byref(dg), 1 if softmax else 0, 1 if per_item else 0, ptr(partial), ptr(loss),
                C.byref(sets) if sets is not None else None, stream_ptr()), "conv_head_loss_run")

        launch()
        if PROFILER is not None:
            e0 = PROFILER.begin()
            for _ in range(PROFILER.reps):
                launch()
            # what the launch moves: x (and the fused add) in, the gradient out - no logits
            nbytes = self.io_bytes(x, dlogits, self.packed_fwd) + (add.numel() * add.element_size() if add is not None else 0.0)
            PROFILER.end("conv3_mfma4_loss_kernel<bf16>", PROFILER.reps, self.flops(x, y, self.d_fwd) * PROFILER.reps, e0,
                         self._detail(CONV_FWD, x), nbytes * PROFILER.reps)

    def dgrad(self, dy: torch.Tensor, dx: torch.Tensor, accumulate: bool = False, add: Optional[torch.Tensor] = None) -> None:
        """dx (+)= conv^T(dy) [+ add]: ``add`` is a second gradient term of the same tensor (the identity branch of a
        ResidualUnit) summed in the epilogue instead of by a separate pass over dx."""
        self._run(self.d_dgrad, self.packed_dgrad, dy, None, None, dx, accumulate, None, add, None)

    def _wgrad_args(self, x: torch.Tensor, dy: torch.Tensor, workspace: bool = True):
        """What every weight-gradient call shares: the library, the references (desc, x, dy, sets-or-None; each keeps its
        structure alive), the sets, and - unless the call launches nothing - the workspace and its size in bytes."""
        lib = _lib.load()
        sets = self._sets(self.d_fwd)
        refs = (C.byref(self.d_fwd), C.byref(desc_cl(x)), C.byref(desc_cl(dy)), C.byref(sets) if sets is not None else None)
        if not workspace:
            return lib, refs, sets, None, 0
        need = int(lib.mmtta_conv_wgrad_workspace_bytes_sets(*refs))
        if need < 0:
            check(-1, "conv_wgrad_workspace_bytes")
        return lib, refs, sets, Workspace.get(need, x.device), need

    def wgrad(self, x: torch.Tensor, x_nl: Optional[NL], dy: torch.Tensor, dw: torch.Tensor,
              db: Optional[torch.Tensor], accumulate: bool = False) -> None:
        lib, (d, tx, tdy, sref), sets, ws, need = self._wgrad_args(x, dy)
        nls, nlr = _nl_ref(x_nl)
        def launch():
            check(lib.mmtta_conv_wgrad_sets(d, tx, nlr, tdy, ptr(dw), ptr(db), 1 if accumulate else 0, ptr(ws), need, sref,
                                            stream_ptr()), "conv_wgrad")

        launch()
        if PROFILER is not None:
            e0 = PROFILER.begin()
            for _ in range(PROFILER.reps):
                launch()
            kid = lib.mmtta_conv_wgrad_kernel(d, tx, tdy)
            nsets = x.shape[0] // int(sets.items_per_set) if sets is not None else 1
            PROFILER.end(WGRAD_KERNELS[kid], PROFILER.reps, self.flops(x, dy) * PROFILER.reps, e0, self._detail(-1, x),
                         (self.io_bytes(x, dy, dw) + (nsets - 1) * dw.numel() * 4.0) * PROFILER.reps)


    def wgrad_plan(self, x: torch.Tensor, dy: torch.Tensor) -> dict:
        """The weight gradient's reduction plan for this problem (mmtta_conv_wgrad_plan_sets): partial slabs per set, chunks
        of the pre-reduce stage (0: none) and the padded channel counts of a slab.  Launches nothing."""
        lib, refs, _, _, _ = self._wgrad_args(x, dy, workspace=False)
        out = (C.c_int32 * 4)()
        check(lib.mmtta_conv_wgrad_plan_sets(*refs, out), "conv_wgrad_plan")
        return {"nsl": int(out[0]), "pre_chunks": int(out[1]), "CGp": int(out[2]), "CDp": int(out[3])}

    def plain_bf16_images(self) -> bool:
        """Both images are bare 27-tap bf16 images (what the fused weight update writes): bf16 operands, K >= 16 each way."""
        if self.k != 3 or int(self.d_fwd.dtype) != BF16 or min(self.cin, self.cout) < 16:
            return False
        img = 27 * ((self.cin + 31) // 32 * 32) * ((self.cout + 31) // 32 * 32) * 2
        return self.nb_fwd == img and self.nb_dgrad == img

    def update_target(self, spec: "OptimSpec", w_p, w_m, w_v, b_p, b_m, b_v, b_grad, w_decay: bool, b_decay: bool,
                      step: torch.Tensor) -> _lib.UpdateTarget:
        """mmtta_update_target of this op's parameter set 0 (tensors: the first element of set 0's slices)."""
        t = _lib.UpdateTarget()
        t.optim = spec.struct()
        t.w_p, t.w_m, t.w_v = ptr(w_p), ptr(w_m), ptr(w_v)
        t.b_p, t.b_m, t.b_v, t.b_grad = ptr(b_p), ptr(b_m), ptr(b_v), ptr(b_grad)
        t.image[0] = ptr(self.packed_image(False, 0))
        t.image[1] = ptr(self.packed_image(True, 0)) if self.need_dgrad else None
        pair = self.sets_grouped
        for i in range(2):
            t.image_outer[i] = int(pair[i].packed_outer) if pair is not None else 0
            t.image_inner[i] = int(pair[i].packed_inner) if pair is not None else 0
        t.step = ptr(step)
        t.w_decay, t.b_decay = int(bool(w_decay)), int(bool(b_decay))
        return t

    def wgrad_update(self, x: torch.Tensor, x_nl: Optional[NL], dy: torch.Tensor, target: _lib.UpdateTarget) -> None:
        """Weight gradient + optimizer step + repack of both images (mmtta_conv_wgrad_update_sets): the layer's parameters,
        moments and images of every set in the batch are updated in place; the step counter is read, not advanced."""
        lib, (d, tx, tdy, sref), _, ws, need = self._wgrad_args(x, dy)
        nls, nlr = _nl_ref(x_nl)
        check(lib.mmtta_conv_wgrad_update_sets(d, tx, nlr, tdy, C.byref(target), ptr(ws), need, sref, stream_ptr()),
              "conv_wgrad_update")


def fused_update_enabled() -> bool:
    """The fused weight update is on (MMTTA_FUSED_UPDATE=0 in the environment switches it off)."""
    return bool(_lib.load().mmtta_fused_update_enabled())


class BatchedPacker:
    """Every packed weight image of a model refreshed by ONE kernel launch (the table is built once: parameter
    and image addresses are stable while the arena lives)."""

    def __init__(self, items, device):
        """items: list of (ConvDesc, master weight tensor, packed image tensor)."""
        lib = _lib.load()
        n = len(items)
        arr = (_lib.PackItem * n)()
        for i, (desc, w, packed) in enumerate(items):
            arr[i].desc = desc
            arr[i].w_master = ptr(w)
            arr[i].packed = ptr(packed)
        nbytes = int(lib.mmtta_conv_pack_table_bytes(n))
        host = (C.c_uint8 * nbytes)()
        total = C.c_int64(0)
        check(lib.mmtta_conv_pack_table_build(arr, n, host, C.byref(total)), "conv_pack_table_build")
        self.table = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(device)
        self.count, self.total = n, int(total.value)
        self._keep = [t for it in items for t in it[1:]]
        self.items = list(items)

    def run(self) -> None:
        check(_lib.load().mmtta_conv_pack_batched(ptr(self.table), self.count, self.total, stream_ptr()),
              "conv_pack_batched")


# ----------------------------------------------------------------------------- normalisation
def reduce_rows_per_n(x: torch.Tensor) -> int:
    t = desc_cl(x)
    return int(_lib.load().mmtta_reduce_rows_per_n(C.byref(t)))


def channel_stats(x: torch.Tensor, part: torch.Tensor) -> None:
    t = desc_cl(x)
    check(_lib.load().mmtta_channel_stats(C.byref(t), ptr(part), stream_ptr()), "channel_stats")


def norm_stats_finalize(kind: int, groups: int, part: Optional[torch.Tensor], rows_per_n: int, n: int, c: int,
                        count: int, eps: float, training: bool, running_mean, running_var, momentum: float,
                        mean: torch.Tensor, rstd: torch.Tensor, scratch: torch.Tensor, gamma=None, beta=None,
                        scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None) -> None:
    check(_lib.load().mmtta_norm_stats_finalize(kind, groups, ptr(part), rows_per_n, n, c, count, eps,
                                                1 if training else 0, ptr(running_mean), ptr(running_var),
                                                momentum, ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(scale),
                                                ptr(shift), ptr(scratch), stream_ptr()),
          "norm_stats_finalize")


def norm_sets(items_per_set: int, affine_stride: int, stats_stride: int = 0) -> _lib.NormSets:
    """mmtta_norm_sets: batch item n uses norm set n // items_per_set; set q's gamma / beta (and their gradients) sit
    q * affine_stride, its running statistics q * stats_stride elements behind set 0's."""
    return _lib.NormSets(int(items_per_set), 0, int(affine_stride), int(stats_stride))


def norm_stats_finalize_sets(kind: int, groups: int, part: Optional[torch.Tensor], rows_per_n: int, n: int, c: int,
                             count: int, eps: float, training: bool, running_mean, running_var, momentum: float,
                             mean: torch.Tensor, rstd: torch.Tensor, scratch: torch.Tensor, sets: _lib.NormSets,
                             gamma=None, beta=None, scale: Optional[torch.Tensor] = None,
                             shift: Optional[torch.Tensor] = None, gamma_items: Optional[torch.Tensor] = None,
                             beta_items: Optional[torch.Tensor] = None) -> None:
    """norm_stats_finalize per norm set (``sets``: norm_sets); gamma / beta / running statistics are set 0's."""
    check(_lib.load().mmtta_norm_stats_finalize_sets(kind, groups, ptr(part), rows_per_n, n, c, count, eps,
                                                     1 if training else 0, ptr(running_mean), ptr(running_var),
                                                     momentum, ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(scale),
                                                     ptr(shift), ptr(gamma_items), ptr(beta_items), ptr(scratch),
                                                     C.byref(sets), stream_ptr()),
          "norm_stats_finalize_sets")


def combine(a: torch.Tensor, a_nl: Optional[NL], b: Optional[torch.Tensor], b_nl: Optional[NL], out: torch.Tensor) -> None:
    ta, to = desc_cl(a), desc_cl(out)
    tb = desc_cl(b) if b is not None else None
    sa, ra = _nl_ref(a_nl)
    sb, rb = _nl_ref(b_nl)
    check(_lib.load().mmtta_combine(C.byref(ta), ra, C.byref(tb) if tb is not None else None, rb, C.byref(to),
                                    stream_ptr()), "combine")


def norm_bwd_reduce(dout: torch.Tensor, y: torch.Tensor, nl: NL, part: torch.Tensor) -> None:
    td, ty = desc_cl(dout), desc_cl(y)
    s, r = _nl_ref(nl)
    check(_lib.load().mmtta_norm_bwd_reduce(C.byref(td), C.byref(ty), r, ptr(part), stream_ptr()), "norm_bwd_reduce")


def norm_bwd_finalize(kind: int, groups: int, part: torch.Tensor, rows_per_n: int, n: int, c: int, count: int,
                      gamma, training: bool, m1: torch.Tensor, m2: torch.Tensor, dgamma, dbeta, accumulate: bool,
                      scratch: torch.Tensor) -> None:
    check(_lib.load().mmtta_norm_bwd_finalize(kind, groups, ptr(part), rows_per_n, n, c, count, ptr(gamma),
                                              1 if training else 0, ptr(m1), ptr(m2), ptr(dgamma), ptr(dbeta),
                                              1 if accumulate else 0, ptr(scratch), stream_ptr()),
          "norm_bwd_finalize")


def norm_bwd_finalize_sets(kind: int, groups: int, part: torch.Tensor, rows_per_n: int, n: int, c: int, count: int,
                           gamma, training: bool, m1: torch.Tensor, m2: torch.Tensor, dgamma, dbeta, accumulate: bool,
                           scratch: torch.Tensor, sets: _lib.NormSets) -> None:
    """norm_bwd_finalize per norm set: gamma / dgamma / dbeta are set 0's, set q's sit q * sets.affine_stride behind."""
    check(_lib.load().mmtta_norm_bwd_finalize_sets(kind, groups, ptr(part), rows_per_n, n, c, count, ptr(gamma),
                                                   1 if training else 0, ptr(m1), ptr(m2), ptr(dgamma), ptr(dbeta),
                                                   1 if accumulate else 0, ptr(scratch), C.byref(sets), stream_ptr()),
          "norm_bwd_finalize_sets")


def norm_bwd_apply(dout: torch.Tensor, y: torch.Tensor, nl: NL, m1: torch.Tensor, m2: torch.Tensor,
                   dy: torch.Tensor) -> None:
    td, ty, to = desc_cl(dout), desc_cl(y), desc_cl(dy)
    s, r = _nl_ref(nl)
    check(_lib.load().mmtta_norm_bwd_apply(C.byref(td), C.byref(ty), r, ptr(m1), ptr(m2), C.byref(to), stream_ptr()),
          "norm_bwd_apply")


def small_norm_backward_max() -> int:
    """Largest voxel count per batch item that takes the one-launch norm backward (A/B aid: MMTTA_NORM_SMALL=<voxels>, 0 =
    three passes at every level)."""
    return int(os.environ.get("MMTTA_NORM_SMALL", "512"))


def norm_bwd_small_ok(dout: torch.Tensor, y: torch.Tensor, nl: NL, dy: torch.Tensor) -> bool:
    """True when mmtta_norm_bwd_small (instance-norm backward of a small tensor in one launch) takes these tensors."""
    td, ty, to = desc_cl(dout), desc_cl(y), desc_cl(dy)
    s, r = _nl_ref(nl)
    return bool(_lib.load().mmtta_norm_bwd_small_ok(C.byref(td), C.byref(ty), r, C.byref(to)))


def norm_bwd_small(dout: torch.Tensor, y: torch.Tensor, nl: NL, count: int, dy: torch.Tensor) -> None:
    td, ty, to = desc_cl(dout), desc_cl(y), desc_cl(dy)
    s, r = _nl_ref(nl)
    check(_lib.load().mmtta_norm_bwd_small(C.byref(td), C.byref(ty), r, int(count), C.byref(to), stream_ptr()),
          "norm_bwd_small")


# ----------------------------------------------------------------------------- resample / glue
def upsample2x_fwd(x: torch.Tensor, y: torch.Tensor) -> None:
    tx, ty = desc_cl(x), desc_cl(y)
    check(_lib.load().mmtta_upsample2x_fwd(C.byref(tx), C.byref(ty), stream_ptr()), "upsample2x_fwd")


def upsample2x_bwd(dy: torch.Tensor, dx: torch.Tensor, accumulate: bool = False) -> None:
    ty, tx = desc_cl(dy), desc_cl(dx)
    check(_lib.load().mmtta_upsample2x_bwd(C.byref(ty), C.byref(tx), 1 if accumulate else 0, stream_ptr()),
          "upsample2x_bwd")


def lincomb(inputs: Sequence[torch.Tensor], weights: Sequence[float], out: torch.Tensor, accumulate: bool = False) -> None:
    k = len(inputs)
    descs = [desc_cl(t) for t in inputs]
    arr = (C.POINTER(_lib.Tensor) * k)(*[C.pointer(d) for d in descs])
    w = (C.c_float * k)(*[float(x) for x in weights])
    to = desc_cl(out)
    check(_lib.load().mmtta_lincomb(k, arr, w, C.byref(to), 1 if accumulate else 0, stream_ptr()), "lincomb")


def pointwise_route(op: str, operands: Sequence, nl=None, nl2=None, m1=None, m2=None) -> Dict[str, object]:
    """Which kernel of csrc/pointwise.hip the entry point `op` (one of _lib.PW_OPS) launches for these operands, and its launch
    geometry: mmtta_pointwise_route_t as a dict, `family` by name.  Host-only - nothing is launched.  `operands` in the
    order of include/mmtta.h: tensors (channels-last views) or ready _lib.Tensor descriptors; `nl` / `nl2` NL objects or
    _lib.NormOnLoad structs; `m1` / `m2` tensors or addresses (norm_bwd_apply: read for their alignment)."""
    descs = [t if isinstance(t, _lib.Tensor) else desc_cl(t) for t in operands]
    arr = (C.POINTER(_lib.Tensor) * len(descs))(*[C.pointer(d) for d in descs])
    structs = [None if t is None else (t.struct() if isinstance(t, NL) else t) for t in (nl, nl2)]
    refs = [None if s is None else C.byref(s) for s in structs]
    addr = [a if a is None or isinstance(a, int) else ptr(a) for a in (m1, m2)]
    out = _lib.PointwiseRoute()
    check(_lib.load().mmtta_pointwise_route(_lib.PW_OPS.index(op), arr, len(descs), refs[0], refs[1], addr[0], addr[1],
                                            C.byref(out)), f"pointwise_route({op})")
    route = {name: int(getattr(out, name)) for name, _ in _lib.PointwiseRoute._fields_}
    route["family"] = _lib.PW_FAMILIES[route["family"]]
    return route


# ----------------------------------------------------------------------------- loss / optimizer / metric
def entropy_partials(logits: torch.Tensor) -> int:
    t = desc_cl(logits)
    return int(_lib.load().mmtta_entropy_partials(C.byref(t)))


def entropy_loss(logits: torch.Tensor, dlogits: torch.Tensor, partial: torch.Tensor, loss: torch.Tensor,
                 softmax: bool = False) -> None:
    tz, tg = desc_cl(logits), desc_cl(dlogits)
    check(_lib.load().mmtta_entropy_loss(C.byref(tz), 1 if softmax else 0, C.byref(tg), ptr(partial), ptr(loss),
                                         stream_ptr()), "entropy_loss")


def entropy_partials_items(logits: torch.Tensor) -> int:
    t = desc_cl(logits)
    return int(_lib.load().mmtta_entropy_partials_items(C.byref(t)))


def entropy_loss_items(logits: torch.Tensor, dlogits: torch.Tensor, partial: torch.Tensor, loss: torch.Tensor,
                       softmax: bool = False) -> None:
    """The objective of every batch item on its own (N independent volumes in one launch): loss [N]."""
    if loss.numel() < logits.shape[0]:
        raise MmttaError("entropy_loss_items: one loss slot per batch item")
    tz, tg = desc_cl(logits), desc_cl(dlogits)
    check(_lib.load().mmtta_entropy_loss_items(C.byref(tz), 1 if softmax else 0, C.byref(tg), ptr(partial), ptr(loss),
                                               stream_ptr()), "entropy_loss_items")


def entropy_filtered_partials(logits: torch.Tensor) -> int:
    t = desc_cl(logits)
    return int(_lib.load().mmtta_entropy_filtered_partials(C.byref(t)))


def entropy_filtered_items(logits: torch.Tensor, dlogits: torch.Tensor, margin: float, keep_in: Optional[torch.Tensor],
                           keep_out: torch.Tensor, partial: torch.Tensor, loss: torch.Tensor, kept: torch.Tensor,
                           softmax: bool = False) -> None:
    """SAR's reliable-entropy objective of every batch item on its own: elements with H < margin (and keep_in) enter the
    loss.  keep_in / keep_out: uint8, one byte per element (N*D*H*W*R, or N*D*H*W for softmax heads); loss fp32 [N], kept
    int64 [N]; dlogits = keep * dH/dz / kept."""
    n, d, h, w, r = logits.shape
    elems = n * d * h * w * (1 if softmax else r)
    for name, t in (("keep_in", keep_in), ("keep_out", keep_out)):
        if t is not None and (t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() < elems):
            raise MmttaError(f"entropy_filtered_items: {name} must be contiguous uint8 of at least {elems} elements")
    if loss.numel() < n or kept.numel() < n or kept.dtype != torch.int64:
        raise MmttaError("entropy_filtered_items: one loss slot and one int64 count per batch item")
    if partial.dtype != torch.float64 or partial.numel() < entropy_filtered_partials(logits):
        raise MmttaError("entropy_filtered_items: partial must be fp64 of entropy_filtered_partials(logits) elements")
    tz, tg = desc_cl(logits), desc_cl(dlogits)
    check(_lib.load().mmtta_entropy_filtered_items(C.byref(tz), 1 if softmax else 0, float(margin), ptr(keep_in), ptr(keep_out),
                                                   C.byref(tg), ptr(partial), ptr(loss), ptr(kept), stream_ptr()),
          "entropy_filtered_items")


def _view_axes(view_axes: Sequence[int]):
    """The host array of view codes the MEMO entry points read at launch (bit 0 = W, 1 = H, 2 = D mirrored; bit 4 = H and W
    transposed before the mirrors, H == W only: a quarter turn in the (H, W) plane is code 18, 3 or 17 for k = 1, 2, 3)."""
    return (C.c_int32 * len(view_axes))(*[int(a) for a in view_axes])


def mirror_views(x: torch.Tensor, y: torch.Tensor, view_axes: Sequence[int]) -> None:
    """y[g * V + v] = x[g] under the code view_axes[v] (transposed in (H, W) where bit 4 is set, then mirrored along the axes
    of bits 0-2): channels-last [G,D,H,W,C] -> [G*V,D,H,W,C], whole voxel rows (pad lanes included), fp32 or bf16, bit-exact."""
    tx, ty = desc_cl(x), desc_cl(y)
    check(_lib.load().mmtta_mirror_views(C.byref(tx), C.byref(ty), len(view_axes), _view_axes(view_axes), stream_ptr()),
          "mirror_views")


def intensity_range_partials(x: torch.Tensor) -> int:
    t = desc_cl(x)
    return int(_lib.load().mmtta_intensity_range_partials(C.byref(t)))


def intensity_range(x: torch.Tensor, partial: torch.Tensor, out: torch.Tensor) -> None:
    """out [G, C, 2] fp32 = (min, max) of every channel of every volume of the staged input x [G,D,H,W,C] (fp32 or bf16
    4-channel voxel rows; the pad lanes do not enter)."""
    g, c = int(x.shape[0]), int(x.shape[4])
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < g * c * 2:
        raise MmttaError(f"intensity_range: out must be contiguous fp32 of at least {g * c * 2} elements")
    if partial.dtype != torch.float32 or partial.numel() < intensity_range_partials(x):
        raise MmttaError("intensity_range: partial must be fp32 of intensity_range_partials(x) elements")
    tx = desc_cl(x)
    check(_lib.load().mmtta_intensity_range(C.byref(tx), ptr(partial), ptr(out), stream_ptr()), "intensity_range")


def augment_views(x: torch.Tensor, y: torch.Tensor, view_axes: Sequence[int], table_host: torch.Tensor, table: torch.Tensor,
                  value_range: torch.Tensor, seed: int, ordinals: torch.Tensor) -> None:
    """y[g * V + v] = x[g] under the code view_axes[v] (as ``mirror_views``) and put through view v's intensity transform
    (``intensity.py``): ``table`` device fp32 [G, V, C, 4] with the rows (g, a, b, sigma), ``table_host`` its host copy (the
    entry point checks view 0's rows on it), ``value_range`` what ``intensity_range`` wrote for x, ``ordinals`` device int32
    [>= G].  An all-identity table gives ``mirror_views``' bits."""
    g, c, v = int(x.shape[0]), int(x.shape[4]), len(view_axes)
    n = g * v * c * 4
    for name, t, cuda in (("table", table, True), ("table_host", table_host, False)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n or t.is_cuda != cuda:
            raise MmttaError(f"augment_views: {name} must be contiguous fp32 [{g}, {v}, {c}, 4] on the "
                             f"{'device' if cuda else 'host'}, got {tuple(t.shape)} {t.dtype} {t.device}")
    if value_range.dtype != torch.float32 or not value_range.is_contiguous() or value_range.numel() < g * c * 2 or not value_range.is_cuda:
        raise MmttaError(f"augment_views: value_range must be contiguous device fp32 of at least {g * c * 2} elements")
    if ordinals.dtype != torch.int32 or ordinals.numel() < g or not ordinals.is_cuda:
        raise MmttaError("augment_views: ordinals must be device int32 [>= volumes]")
    tx, ty = desc_cl(x), desc_cl(y)
    check(_lib.load().mmtta_augment_views(C.byref(tx), C.byref(ty), v, _view_axes(view_axes), ptr(table_host), ptr(table),
                                          ptr(value_range), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(ordinals), stream_ptr()),
          "augment_views")


def memo_partials(logits: torch.Tensor, views: int) -> int:
    t = desc_cl(logits)
    return int(_lib.load().mmtta_memo_partials(C.byref(t), int(views)))


def memo_loss_items(logits: torch.Tensor, dlogits: torch.Tensor, view_axes: Sequence[int], partial: torch.Tensor,
                    loss: torch.Tensor, softmax: bool = False) -> None:
    """MEMO's marginal entropy of every volume on its own: logits / dlogits [G*V,D,H,W,R] (item g*V+v = view v of volume g,
    each in its own mirrored / turned frame), loss fp32 [G]."""
    views = len(view_axes)
    need = memo_partials(logits, views)          # -1 for a bad view count: the entry point below says which
    if loss.numel() < logits.shape[0] // max(views, 1):
        raise MmttaError("memo_loss_items: one loss slot per volume")
    if partial.dtype != torch.float64 or partial.numel() < need:
        raise MmttaError("memo_loss_items: partial must be fp64 of memo_partials(logits, views) elements")
    tz, tg = desc_cl(logits), desc_cl(dlogits)
    check(_lib.load().mmtta_memo_loss_items(C.byref(tz), 1 if softmax else 0, views, _view_axes(view_axes), C.byref(tg),
                                            ptr(partial), ptr(loss), stream_ptr()), "memo_loss_items")


def memo_ensemble(logits: torch.Tensor, out: torch.Tensor, view_axes: Sequence[int], softmax: bool = False) -> None:
    """out [G,D,H,W,R] = logit (sigmoid head) or log (softmax head) of the mean over the views of the predicted
    probabilities, in the volume's own frame."""
    tz, to = desc_cl(logits), desc_cl(out)
    check(_lib.load().mmtta_memo_ensemble(C.byref(tz), 1 if softmax else 0, len(view_axes), _view_axes(view_axes), C.byref(to),
                                          stream_ptr()), "memo_ensemble")


def _affine_matrices(what: str, host: torch.Tensor, dev: torch.Tensor, volumes: int, count: int) -> None:
    n = volumes * count * 12
    for name, t, cuda in (("the device matrices", dev, True), ("their host copy", host, False)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n or t.is_cuda != cuda:
            raise MmttaError(f"{what}: {name} must be contiguous fp32 [{volumes}, {count}, 12] on the "
                             f"{'device' if cuda else 'host'}, got {tuple(t.shape)} {t.dtype} {t.device}")


def affine_views(x: torch.Tensor, y: torch.Tensor, first: int, matrices_host: torch.Tensor, matrices: torch.Tensor) -> None:
    """y[g * V + first + j] = the trilinear resample of x[g] under matrix (g, j) (``affine.py``: a view voxel -> the frame
    coordinate it samples; corners outside contribute 0): channels-last [G,D,H,W,C] -> [G*V,D,H,W,C], fp32 or bf16 rows, pad
    lanes 0.  ``matrices`` device fp32 [G, count, 12], ``matrices_host`` its host copy; V = first + count.  The items below
    ``first`` are not touched."""
    g, v = int(x.shape[0]), int(y.shape[0]) // max(int(x.shape[0]), 1)
    count = v - int(first)
    _affine_matrices("affine_views", matrices_host, matrices, g, max(count, 0))
    tx, ty = desc_cl(x), desc_cl(y)
    check(_lib.load().mmtta_affine_views(C.byref(tx), C.byref(ty), v, int(first), count, ptr(matrices_host), ptr(matrices),
                                         stream_ptr()), "affine_views")


def affine_ensemble(logits: torch.Tensor, out: torch.Tensor, view_axes: Sequence[int], first: int, inv_host: torch.Tensor,
                    inv: torch.Tensor, softmax: bool = False) -> None:
    """``memo_ensemble`` over ``first`` coded views (``view_axes[:first]``) followed by affine views (code 0): out [G,D,H,W,R]
    = logit (sigmoid head) or log (softmax head) of the coverage-weighted mean of the predicted probabilities in the volume's
    frame; an affine view's probabilities come back through the trilinear gather under ``inv`` (device fp32 [G, count, 12]:
    a frame voxel -> the view coordinate that shows it; ``inv_host`` its host copy)."""
    v = len(view_axes)
    count = v - int(first)
    _affine_matrices("affine_ensemble", inv_host, inv, int(out.shape[0]), max(count, 0))
    tz, to = desc_cl(logits), desc_cl(out)
    check(_lib.load().mmtta_affine_ensemble(C.byref(tz), 1 if softmax else 0, v, _view_axes(view_axes), int(first), count,
                                            ptr(inv_host), ptr(inv), C.byref(to), stream_ptr()), "affine_ensemble")


def consistency_partials(logits: torch.Tensor) -> int:
    t = desc_cl(logits)
    return int(_lib.load().mmtta_consistency_partials(C.byref(t)))


def consistency_loss_items(logits: torch.Tensor, target: torch.Tensor, dlogits: torch.Tensor, partial: torch.Tensor,
                           loss: torch.Tensor, softmax: bool = False) -> None:
    """CoTTA's consistency loss of every batch item on its own: the student's logits against the teacher's target (logit of
    its mean probability, softmax head: log of it - ``memo_ensemble``'s output), all [N,D,H,W,R]; loss fp32 [N]; dlogits =
    (sigmoid(z) - sigmoid(t)) / count, softmax head (softmax(z) - exp(t)) / count."""
    if loss.numel() < logits.shape[0]:
        raise MmttaError("consistency_loss_items: one loss slot per batch item")
    if partial.dtype != torch.float64 or partial.numel() < consistency_partials(logits):
        raise MmttaError("consistency_loss_items: partial must be fp64 of consistency_partials(logits) elements")
    tz, tt, tg = desc_cl(logits), desc_cl(target), desc_cl(dlogits)
    check(_lib.load().mmtta_consistency_loss_items(C.byref(tz), C.byref(tt), 1 if softmax else 0, C.byref(tg), ptr(partial),
                                                   ptr(loss), stream_ptr()), "consistency_loss_items")


def cotta_update_partials(n: int, sets: int) -> int:
    return int(_lib.load().mmtta_cotta_update_partials(int(n), int(sets)))


def cotta_update_sets(w: torch.Tensor, teacher: torch.Tensor, source: torch.Tensor, n: int, sets: int, alpha: float,
                      restore_p: float, seed: int, step: torch.Tensor, ordinals: torch.Tensor, partial: torch.Tensor,
                      restored: torch.Tensor) -> None:
    """CoTTA's pass after the student's optimizer step over the first ``sets`` rows of ``w`` / ``teacher`` ([rows, >= n]
    fp32) and the shared ``source`` ([>= n]): teacher = alpha teacher + (1 - alpha) w, then w[i] = source[i] where the
    Philox4x32-10 draw of (seed; i >> 2, step, ordinal) is below ``restore_p``.  ``step``: the device int32 step counter;
    ``ordinals``: device int32 [>= sets]; ``restored``: int64 [>= sets], the restored elements per row."""
    for name, t in (("w", w), ("teacher", teacher)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.shape[0] < sets or t.shape[1] < n:
            raise MmttaError(f"cotta_update_sets: {name} must be contiguous fp32 [>= {sets}, >= {n}], got {tuple(t.shape)}")
    if source.dtype != torch.float32 or not source.is_contiguous() or source.numel() < n:
        raise MmttaError(f"cotta_update_sets: source must be contiguous fp32 of at least {n} elements")
    if step.dtype != torch.int32 or ordinals.dtype != torch.int32 or ordinals.numel() < sets:
        raise MmttaError("cotta_update_sets: step must be a device int32 scalar, ordinals device int32 [>= sets]")
    if restored.dtype != torch.int64 or restored.numel() < sets:
        raise MmttaError("cotta_update_sets: one int64 count per set")
    if partial.dtype != torch.int64 or partial.numel() < cotta_update_partials(n, sets):
        raise MmttaError("cotta_update_sets: partial must be int64 of cotta_update_partials(n, sets) elements")
    check(_lib.load().mmtta_cotta_update_sets(ptr(w), ptr(teacher), ptr(source), int(n), int(sets), int(w.shape[1]),
                                              int(teacher.shape[1]), float(alpha), float(restore_p),
                                              int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(step), ptr(ordinals), ptr(partial),
                                              ptr(restored), stream_ptr()), "cotta_update_sets")


def magnitude_select_class(length: int) -> int:
    """Which kernel of magnitude_select_sets serves a row of ``length`` elements: 0 one workgroup, 1 chunked."""
    return int(_lib.load().mmtta_magnitude_select_class(int(length)))


@dataclass
class RankTable:
    """The segment table of magnitude_select_sets / petal_update_sets: ``rows`` (start, length, rank), its device array
    ([count][3] then the [count + 1] running chunk counts) and the host copy the argument checks read."""
    rows: List[Tuple[int, int, int]]
    device: torch.Tensor
    host: torch.Tensor

    @property
    def count(self) -> int:
        return len(self.rows)


def rank_segments_table(rows: Sequence[Tuple[int, int, int]], device) -> RankTable:
    lib = _lib.load()
    flat, cum = [], [0]
    for start, length, rank in rows:
        flat += [int(start), int(length), int(rank)]
        cum.append(cum[-1] + max(0, int(lib.mmtta_magnitude_select_chunks(int(length)))))
    host = torch.tensor(flat + cum, dtype=torch.int64)
    return RankTable([tuple(int(v) for v in r) for r in rows], host.to(device), host)


def magnitude_select_scratch(table: RankTable, sets: int) -> int:
    """int32 elements of magnitude_select_sets' scratch."""
    nbytes = int(_lib.load().mmtta_magnitude_select_scratch_bytes(int(table.count), int(sets)))
    if nbytes < 0:
        check(-1, "magnitude_select_scratch_bytes")
    return nbytes // 4


def magnitude_select_sets(g: torch.Tensor, table: RankTable, sets: int, gamma: torch.Tensor, scratch: torch.Tensor) -> None:
    """gamma[s, r] (int32 [>= sets, count]: the uint32 bits) = the rank-th smallest magnitude key (bits & 0x7fffffff) of row
    r of ``table`` in row s of ``g`` (fp32 [>= sets, width])."""
    if g.dtype != torch.float32 or not g.is_contiguous() or g.dim() != 2 or g.shape[0] < sets:
        raise MmttaError(f"magnitude_select_sets: g must be contiguous fp32 [>= {sets}, width], got {tuple(g.shape)}")
    if gamma.dtype != torch.int32 or not gamma.is_contiguous() or gamma.dim() != 2 or gamma.shape[0] < sets or gamma.shape[1] != table.count:
        raise MmttaError(f"magnitude_select_sets: gamma must be contiguous int32 [>= {sets}, {table.count}]")
    if scratch.dtype != torch.int32 or scratch.numel() < magnitude_select_scratch(table, sets):
        raise MmttaError("magnitude_select_sets: scratch must be int32 of magnitude_select_scratch(table, sets) elements")
    check(_lib.load().mmtta_magnitude_select_sets(ptr(g), ptr(table.device), ptr(table.host), table.count, int(sets),
                                                  int(g.shape[1]), ptr(gamma), ptr(scratch), stream_ptr()), "magnitude_select_sets")


def petal_update_partials(n: int, sets: int) -> int:
    return int(_lib.load().mmtta_petal_update_partials(int(n), int(sets)))


def petal_update_sets(w: torch.Tensor, teacher: torch.Tensor, source: torch.Tensor, g: torch.Tensor, gamma: torch.Tensor,
                      table: RankTable, n: int, sets: int, alpha: float, partial: torch.Tensor, restored: torch.Tensor) -> None:
    """PETAL's pass after the student's optimizer step over the first ``sets`` rows of ``w`` / ``teacher`` / ``g`` ([rows, >= n]
    fp32) and the shared ``source``: teacher = alpha teacher + (1 - alpha) w (cotta_update_sets' arithmetic), then w[i] =
    source[i] where i lies in row r of ``table`` and the magnitude key of g[i] is below gamma[s, r].  ``restored``: int64
    [>= sets], the restored elements per row."""
    for name, t in (("w", w), ("teacher", teacher), ("g", g)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.shape[0] < sets or t.shape[1] < n:
            raise MmttaError(f"petal_update_sets: {name} must be contiguous fp32 [>= {sets}, >= {n}], got {tuple(t.shape)}")
    if source.dtype != torch.float32 or not source.is_contiguous() or source.numel() < n:
        raise MmttaError(f"petal_update_sets: source must be contiguous fp32 of at least {n} elements")
    if gamma.dtype != torch.int32 or not gamma.is_contiguous() or gamma.dim() != 2 or gamma.shape[0] < sets or gamma.shape[1] != table.count:
        raise MmttaError(f"petal_update_sets: gamma must be contiguous int32 [>= {sets}, {table.count}]")
    if restored.dtype != torch.int64 or restored.numel() < sets:
        raise MmttaError("petal_update_sets: one int64 count per set")
    if partial.dtype != torch.int64 or partial.numel() < petal_update_partials(n, sets):
        raise MmttaError("petal_update_sets: partial must be int64 of petal_update_partials(n, sets) elements")
    check(_lib.load().mmtta_petal_update_sets(ptr(w), ptr(teacher), ptr(source), ptr(g), ptr(gamma), ptr(table.device),
                                              ptr(table.host), table.count, int(n), int(sets), int(w.shape[1]),
                                              int(teacher.shape[1]), int(g.shape[1]), float(alpha), ptr(partial), ptr(restored),
                                              stream_ptr()), "petal_update_sets")


def entropy_weighted_partials(logits: torch.Tensor) -> int:
    t = desc_cl(logits)
    return int(_lib.load().mmtta_entropy_weighted_partials(C.byref(t)))


def entropy_weighted_items(logits: torch.Tensor, dlogits: torch.Tensor, margin: float, keep_out: torch.Tensor,
                           partial: torch.Tensor, loss: torch.Tensor, kept: torch.Tensor, softmax: bool = False) -> None:
    """EATA's weighted reliable entropy of every batch item on its own: elements with H < margin enter the loss with the
    weight c = exp(margin - H) (no gradient through c).  keep_out: uint8, one byte per element (N*D*H*W*R, or N*D*H*W for
    softmax heads) - the mask of ``entropy_filtered_items`` bit for bit; loss fp32 [N] = sum c H / kept, kept int64 [N];
    dlogits = keep * c * dH/dz / kept."""
    n, d, h, w, r = logits.shape
    elems = n * d * h * w * (1 if softmax else r)
    if keep_out.dtype != torch.uint8 or not keep_out.is_contiguous() or keep_out.numel() < elems:
        raise MmttaError(f"entropy_weighted_items: keep_out must be contiguous uint8 of at least {elems} elements")
    if loss.numel() < n or kept.numel() < n or kept.dtype != torch.int64:
        raise MmttaError("entropy_weighted_items: one loss slot and one int64 count per batch item")
    if partial.dtype != torch.float64 or partial.numel() < entropy_weighted_partials(logits):
        raise MmttaError("entropy_weighted_items: partial must be fp64 of entropy_weighted_partials(logits) elements")
    tz, tg = desc_cl(logits), desc_cl(dlogits)
    check(_lib.load().mmtta_entropy_weighted_items(C.byref(tz), 1 if softmax else 0, float(margin), ptr(keep_out), C.byref(tg),
                                                   ptr(partial), ptr(loss), ptr(kept), stream_ptr()), "entropy_weighted_items")


def pseudo_label_partials(logits: torch.Tensor) -> int:
    t = desc_cl(logits)
    return int(_lib.load().mmtta_pseudo_label_partials(C.byref(t)))


def pseudo_label_loss_items(logits: torch.Tensor, dlogits: torch.Tensor, partial: torch.Tensor, loss: torch.Tensor,
                            softmax: bool = False) -> None:
    """The loss of EATA's Fisher estimate for every batch item on its own: cross entropy against the model's own hard
    prediction (sigmoid head: y = 1[z >= 0], softmax head: the first arg max); loss fp32 [N], dlogits = (p - y) / count."""
    if loss.numel() < logits.shape[0]:
        raise MmttaError("pseudo_label_loss_items: one loss slot per batch item")
    if partial.dtype != torch.float64 or partial.numel() < pseudo_label_partials(logits):
        raise MmttaError("pseudo_label_loss_items: partial must be fp64 of pseudo_label_partials(logits) elements")
    tz, tg = desc_cl(logits), desc_cl(dlogits)
    check(_lib.load().mmtta_pseudo_label_loss_items(C.byref(tz), 1 if softmax else 0, C.byref(tg), ptr(partial), ptr(loss),
                                                    stream_ptr()), "pseudo_label_loss_items")


def fisher_accumulate_sets(fisher: torch.Tensor, grads: torch.Tensor, n: int, sets: int) -> None:
    """fisher[:n] += grads[s, :n] ** 2 for s = 0 .. sets-1 in that order (fp32, torch's ``F + g * g``).  ``grads``:
    contiguous fp32 [>= sets, >= n] with a row length that is a multiple of 4."""
    if fisher.dtype != torch.float32 or not fisher.is_contiguous() or fisher.numel() < n:
        raise MmttaError(f"fisher_accumulate_sets: fisher must be contiguous fp32 of at least {n} elements")
    if grads.dtype != torch.float32 or not grads.is_contiguous() or grads.dim() != 2 or grads.shape[0] < sets or grads.shape[1] < n:
        raise MmttaError(f"fisher_accumulate_sets: grads must be contiguous fp32 [>= {sets}, >= {n}], got {tuple(grads.shape)}")
    check(_lib.load().mmtta_fisher_accumulate_sets(ptr(fisher), ptr(grads), int(n), int(sets), int(grads.shape[1]), stream_ptr()),
          "fisher_accumulate_sets")


def fisher_scale(fisher: torch.Tensor, n: int, count: int) -> None:
    """fisher[:n] /= float(count): the end of a Fisher estimate over ``count`` volumes."""
    if fisher.dtype != torch.float32 or not fisher.is_contiguous() or fisher.numel() < n:
        raise MmttaError(f"fisher_scale: fisher must be contiguous fp32 of at least {n} elements")
    check(_lib.load().mmtta_fisher_scale(ptr(fisher), int(n), float(count), stream_ptr()), "fisher_scale")


def fisher_penalty_partials(n: int, sets: int) -> int:
    return int(_lib.load().mmtta_fisher_penalty_partials(int(n), int(sets)))


def fisher_penalty_sets(w: torch.Tensor, g: torch.Tensor, fisher: torch.Tensor, source: torch.Tensor, n: int, sets: int,
                        lam: float, partial: torch.Tensor, penalty: torch.Tensor) -> None:
    """EATA's regulariser over the first ``sets`` replicas of the arena ([replicas, total]; the first ``n`` elements of a
    replica train): g += 2 lam F (w - source), penalty[s] = lam sum F (w - source)^2, with ``fisher`` and ``source`` ([>= n])
    shared by the replicas."""
    for t in (w, g):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.shape != w.shape:
            raise MmttaError("fisher_penalty_sets: w and g must be contiguous fp32 [replicas, total] of equal shape")
    for name, t in (("fisher", fisher), ("source", source)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < n:
            raise MmttaError(f"fisher_penalty_sets: {name} must be contiguous fp32 of at least {n} elements")
    if penalty.dtype != torch.float32 or penalty.numel() < sets:
        raise MmttaError("fisher_penalty_sets: one fp32 penalty slot per set")
    if partial.dtype != torch.float64 or partial.numel() < fisher_penalty_partials(n, sets):
        raise MmttaError("fisher_penalty_sets: partial must be fp64 of fisher_penalty_partials(n, sets) elements")
    check(_lib.load().mmtta_fisher_penalty_sets(ptr(w), ptr(g), ptr(fisher), ptr(source), int(n), int(sets), int(w.shape[0]),
                                                int(w.shape[1]), float(lam), ptr(partial), ptr(penalty), stream_ptr()),
          "fisher_penalty_sets")


def _patch_grid(grid: Sequence[int]):
    """The host array (gd, gh, gw) the DeYO entry points read at launch."""
    if len(grid) != 3:
        raise MmttaError(f"patch grid {list(grid)!r}: expected three patch counts (gd, gh, gw)")
    return (C.c_int32 * 3)(*[int(g) for g in grid])


def patch_table(perms: Sequence[Sequence[int]]) -> torch.Tensor:
    """The host table int32 [N, 2, P] of ``patch_shuffle`` / ``deyo_loss_items`` from one permutation of range(P) per batch
    item: row 0 the permutation (slot j of the shuffled volume holds patch perm[j]), row 1 its inverse.  Raises unless every
    permutation is a bijection of [0, P) - what is uploaded is checked here, the kernels only clamp."""
    n = len(perms)
    p = len(perms[0]) if n else 0
    table = torch.empty((n, 2, max(p, 1)), dtype=torch.int32)
    for i, perm in enumerate(perms):
        row = [int(v) for v in perm]
        if len(row) != p or p < 1 or sorted(row) != list(range(p)):
            raise MmttaError(f"patch_table: item {i}: {row!r} is no permutation of range({p})")
        table[i, 0] = torch.tensor(row, dtype=torch.int32)
        table[i, 1, torch.tensor(row, dtype=torch.int64)] = torch.arange(p, dtype=torch.int32)
    return table


def _check_patch_table(what: str, table: torch.Tensor, n: int, grid: Sequence[int]) -> None:
    need = n * 2 * max(int(grid[0]) * int(grid[1]) * int(grid[2]), 0)
    if table.dtype != torch.int32 or not table.is_contiguous() or not table.is_cuda or table.numel() < need:
        raise MmttaError(f"{what}: table must be contiguous device int32 of at least {need} elements ([{n}, 2, P])")


def patch_shuffle(x: torch.Tensor, y: torch.Tensor, grid: Sequence[int], table: torch.Tensor) -> None:
    """y[n, slot j (+) o] = x[n, patch perm_n[j] (+) o]: the patches of a (gd, gh, gw) grid of every batch item permuted by
    row 0 of the item's ``table`` entry (device int32 [N, 2, P], the upload of ``patch_table``).  Channels-last [N,D,H,W,C]
    of one shape, whole voxel rows (pad lanes included), fp32 or bf16, bit-exact; not in place."""
    garr = _patch_grid(grid)
    _check_patch_table("patch_shuffle", table, int(x.shape[0]), grid)
    tx, ty = desc_cl(x), desc_cl(y)
    check(_lib.load().mmtta_patch_shuffle(C.byref(tx), C.byref(ty), garr, ptr(table), stream_ptr()), "patch_shuffle")


def deyo_partials(logits: torch.Tensor) -> int:
    t = desc_cl(logits)
    return int(_lib.load().mmtta_deyo_partials(C.byref(t)))


def deyo_loss_items(logits: torch.Tensor, logits_shuffled: torch.Tensor, dlogits: torch.Tensor, grid: Sequence[int],
                    table: torch.Tensor, margin: float, margin0: float, plpd_threshold: float, keep_out: torch.Tensor,
                    partial: torch.Tensor, loss: torch.Tensor, kept: torch.Tensor, kept_entropy: torch.Tensor,
                    softmax: bool = False) -> None:
    """DeYO's objective of every batch item on its own: elements with H < margin (``kept_entropy`` of them) whose pseudo-label
    probability drops by more than ``plpd_threshold`` from ``logits`` to ``logits_shuffled`` read through the patch
    permutation (``kept`` of them) enter the loss with the weight a = exp(margin0 - H) + exp(PLPD) (no gradient through a).
    keep_out: uint8, one byte per element (N*D*H*W*R, or N*D*H*W for softmax heads); loss fp32 [N] = sum a H / kept; kept,
    kept_entropy int64 [N]; dlogits = keep * a * dH/dz / kept; ``table`` as for ``patch_shuffle``."""
    n, d, h, w, r = logits.shape
    elems = n * d * h * w * (1 if softmax else r)
    garr = _patch_grid(grid)
    _check_patch_table("deyo_loss_items", table, n, grid)
    if keep_out.dtype != torch.uint8 or not keep_out.is_contiguous() or keep_out.numel() < elems:
        raise MmttaError(f"deyo_loss_items: keep_out must be contiguous uint8 of at least {elems} elements")
    if loss.numel() < n or kept.numel() < n or kept.dtype != torch.int64 or kept_entropy.numel() < n or \
            kept_entropy.dtype != torch.int64:
        raise MmttaError("deyo_loss_items: one loss slot and two int64 counts per batch item")
    if partial.dtype != torch.float64 or partial.numel() < deyo_partials(logits):
        raise MmttaError("deyo_loss_items: partial must be fp64 of deyo_partials(logits) elements")
    tz, ts, tg = desc_cl(logits), desc_cl(logits_shuffled), desc_cl(dlogits)
    check(_lib.load().mmtta_deyo_loss_items(C.byref(tz), C.byref(ts), garr, ptr(table), 1 if softmax else 0, float(margin),
                                            float(margin0), float(plpd_threshold), ptr(keep_out), C.byref(tg), ptr(partial),
                                            ptr(loss), ptr(kept), ptr(kept_entropy), stream_ptr()), "deyo_loss_items")


def lame_refine(logits0: torch.Tensor, x: Optional[torch.Tensor], out: torch.Tensor, work: torch.Tensor, flipped: torch.Tensor, *,
                connectivity: int, weight: float, sigma: float, iterations: int, present: Optional[Sequence[bool]] = None,
                softmax: bool = False) -> None:
    """LAME's output refinement (include/mmtta.h, mmtta_lame_refine): ``iterations`` Jacobi iterations of
    l <- logits0 + weight * sum_j w_ij y(l_j) over the ``connectivity`` spatial neighbours, y = tanh(l / 2) (or the softmax
    row), w_ij = exp(-|x_i - x_j|^2 / (2 sigma^2)) / connectivity on the channels of the staged input ``x`` that ``present``
    marks (default: all; ``sigma`` 0: w_ij = 1 / connectivity and ``x`` may be None).  The result lands in ``out``; ``work``
    is the second ping-pong buffer; ``flipped`` int64 [N] counts the elements whose hard prediction changed.  Channels-last
    fp32 [N,D,H,W,R] logits of one shape and row width, three distinct buffers."""
    n = int(logits0.shape[0])
    if flipped.dtype != torch.int64 or not flipped.is_cuda or not flipped.is_contiguous() or flipped.numel() < n:
        raise MmttaError(f"lame_refine: flipped must be contiguous device int64 of at least {n} elements (one per batch item)")
    mask = 0xFFFFFFFF
    if present is not None:
        if x is not None and len(present) != int(x.shape[-1]):
            raise MmttaError(f"lame_refine: present has {len(present)} entries for the {int(x.shape[-1])} channels of x")
        if len(present) > 32:
            raise MmttaError("lame_refine: at most 32 channels in the mask")
        mask = sum(1 << c for c, p in enumerate(present) if p)
    if float(sigma) > 0.0 and x is None:
        raise MmttaError("lame_refine: sigma > 0 needs the staged input x")
    t0, tw, to = desc_cl(logits0), desc_cl(work), desc_cl(out)
    tx = desc_cl(x) if (x is not None and float(sigma) > 0.0) else None
    check(_lib.load().mmtta_lame_refine(C.byref(t0), None if tx is None else C.byref(tx), mask, 1 if softmax else 0,
                                        int(connectivity), float(weight), float(sigma), int(iterations), C.byref(tw),
                                        C.byref(to), ptr(flipped), stream_ptr()), "lame_refine")


def guard_counts(reference: torch.Tensor, adapted: torch.Tensor, threshold: float, counts: torch.Tensor) -> None:
    """The guard's counts (include/mmtta.h, mmtta_guard_counts): ``counts`` int64 [N,R,3] = (s, a, i) = the voxels of the
    ``reference`` mask, of the ``adapted`` mask and of both, per item and region, under the evaluator's rule
    sigmoid(z) >= ``threshold``.  Channels-last fp32 [N,D,H,W,R] logits of one shape and row width; zeroed by the call."""
    n, r = int(reference.shape[0]), int(reference.shape[-1])
    if counts.dtype != torch.int64 or not counts.is_cuda or not counts.is_contiguous() or counts.numel() < n * r * 3:
        raise MmttaError(f"guard_counts: counts must be contiguous device int64 of at least {n * r * 3} elements ([N,R,3])")
    tr, ta = desc_cl(reference), desc_cl(adapted)
    check(_lib.load().mmtta_guard_counts(C.byref(tr), C.byref(ta), float(threshold), ptr(counts), stream_ptr()), "guard_counts")


def guard_select(counts: torch.Tensor, rule: Any, reference: torch.Tensor, logits: torch.Tensor, fallback: torch.Tensor) -> None:
    """The guard's decision and fall-back (include/mmtta.h, mmtta_guard_select): the integer rule ``rule`` (a
    ``guard.GuardRule`` or an ``_lib.GuardRule``) on ``counts`` int64 [N,R,3] -> ``fallback`` int32 [N,R], and the
    ``reference`` logits copied over ``logits`` in place where it fails (the whole item, or the failing channels under the
    region scope); a passing item's logits are not touched.  Nothing is read on the host."""
    n, r = int(reference.shape[0]), int(reference.shape[-1])
    if counts.dtype != torch.int64 or not counts.is_cuda or not counts.is_contiguous() or counts.numel() < n * r * 3:
        raise MmttaError(f"guard_select: counts must be contiguous device int64 of at least {n * r * 3} elements ([N,R,3])")
    if fallback.dtype != torch.int32 or not fallback.is_cuda or not fallback.is_contiguous() or fallback.numel() < n * r:
        raise MmttaError(f"guard_select: fallback must be contiguous device int32 of at least {n * r} elements ([N,R])")
    rs = rule if isinstance(rule, _lib.GuardRule) else rule.struct()
    tr, tl = desc_cl(reference), desc_cl(logits)
    check(_lib.load().mmtta_guard_select(ptr(counts), C.byref(rs), C.byref(tr), C.byref(tl), ptr(fallback), stream_ptr()),
          "guard_select")


CRF_FORMS = ("potts", "quadratic")


def crf_partials(logits: torch.Tensor) -> int:
    """fp64 elements of the block-partial scratch ``crf_entropy_items`` needs for ``logits``."""
    t = desc_cl(logits)
    return int(_lib.load().mmtta_crf_partials(C.byref(t)))


def crf_entropy_items(logits: torch.Tensor, x: Optional[torch.Tensor], dlogits: torch.Tensor, partial: torch.Tensor,
                      loss: torch.Tensor, entropy: torch.Tensor, pairwise: torch.Tensor, *, connectivity: int, weight: float,
                      sigma: float, form: str = "potts", present: Optional[Sequence[bool]] = None, softmax: bool = False) -> None:
    """CRF-regularised entropy (include/mmtta.h, mmtta_crf_entropy_items): per batch item L = H + weight * P with H the mean
    entropy and P = 1 / (2 n E) sum_i sum_{j in N(i)} a_ij phi(p_i, p_j) over the ``connectivity`` spatial neighbours, phi the
    ``potts`` or ``quadratic`` form, a_ij = exp(-|x_i - x_j|^2 / (2 sigma^2)) on the channels of the staged input ``x`` that
    ``present`` marks (default: all; ``sigma`` 0: a_ij = 1 and ``x`` may be None).  ``dlogits`` receives dL/dlogits; ``loss``,
    ``entropy`` and ``pairwise`` (fp32, one slot per batch item) L, H and P; ``partial`` is fp64 scratch of
    ``crf_partials(logits)`` elements."""
    n = int(logits.shape[0])
    if form not in CRF_FORMS:
        raise MmttaError(f"crf_entropy_items: form must be one of {CRF_FORMS}, got {form!r}")
    for name, t in (("loss", loss), ("entropy", entropy), ("pairwise", pairwise)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < n:
            raise MmttaError(f"crf_entropy_items: {name} must be contiguous fp32 of at least {n} elements (one per batch item)")
    mask = 0xFFFFFFFF
    if present is not None:
        if x is not None and len(present) != int(x.shape[-1]):
            raise MmttaError(f"crf_entropy_items: present has {len(present)} entries for the {int(x.shape[-1])} channels of x")
        if len(present) > 32:
            raise MmttaError("crf_entropy_items: at most 32 channels in the mask")
        mask = sum(1 << c for c, p in enumerate(present) if p)
    if float(sigma) > 0.0 and x is None:
        raise MmttaError("crf_entropy_items: sigma > 0 needs the staged input x")
    if partial.dtype != torch.float64 or not partial.is_contiguous() or partial.numel() < crf_partials(logits):
        raise MmttaError("crf_entropy_items: partial must be contiguous fp64 of crf_partials(logits) elements")
    tz, tg = desc_cl(logits), desc_cl(dlogits)
    tx = desc_cl(x) if (x is not None and float(sigma) > 0.0) else None
    check(_lib.load().mmtta_crf_entropy_items(C.byref(tz), None if tx is None else C.byref(tx), mask, 1 if softmax else 0,
                                              int(connectivity), CRF_FORMS.index(form), float(weight), float(sigma),
                                              C.byref(tg), ptr(partial), ptr(loss), ptr(entropy), ptr(pairwise), stream_ptr()),
          "crf_entropy_items")


def _nuclear_block(block: Sequence[int], what: str) -> Tuple[int, int, int]:
    ok = isinstance(block, (list, tuple)) and len(block) == 3 and all(
        isinstance(b, int) and not isinstance(b, bool) and b >= 0 for b in block)
    if not ok:
        raise MmttaError(f"{what}: block must be three integers >= 0 (0: the whole extent), got {block!r}")
    return int(block[0]), int(block[1]), int(block[2])


def nuclear_scratch(logits: torch.Tensor, block: Sequence[int], softmax: bool = False) -> int:
    """fp64 elements of the scratch ``nuclear_entropy_items`` needs for ``logits`` cut into boxes of ``block`` voxels."""
    bd, bh, bw = _nuclear_block(block, "nuclear_scratch")
    t = desc_cl(logits)
    n = int(_lib.load().mmtta_nuclear_scratch(C.byref(t), 1 if softmax else 0, bd, bh, bw))
    if n < 0:
        raise MmttaError(f"nuclear_scratch: no scratch size for logits {tuple(logits.shape)} and block {list(block)}")
    return n


def nuclear_entropy_items(logits: torch.Tensor, dlogits: torch.Tensor, scratch: torch.Tensor, loss: torch.Tensor,
                          entropy: torch.Tensor, nuclear: torch.Tensor, *, block: Sequence[int], weight: float,
                          entropy_weight: float = 1.0, eps: float = 1e-4, softmax: bool = False) -> None:
    """Entropy minus a regional nuclear norm (include/mmtta.h, mmtta_nuclear_entropy_items): per batch item
    L = entropy_weight * H - weight * N with H the mean entropy and N the mean over the boxes of ``block`` = [bd, bh, bw] voxels
    (0: the whole extent) of the smoothed, normalised nuclear norm of the box's prediction matrix - per region the rows
    (p, 1 - p) on the sigmoid head, the rows softmax(l) on the softmax head.  ``dlogits`` receives dL/dlogits; ``loss``,
    ``entropy`` and ``nuclear`` (fp32, one slot per batch item) L, H and N; ``scratch`` is fp64 of
    ``nuclear_scratch(logits, block, softmax)`` elements."""
    n = int(logits.shape[0])
    bd, bh, bw = _nuclear_block(block, "nuclear_entropy_items")
    for name, t in (("loss", loss), ("entropy", entropy), ("nuclear", nuclear)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < n:
            raise MmttaError(f"nuclear_entropy_items: {name} must be contiguous fp32 of at least {n} elements (one per batch item)")
    if scratch.dtype != torch.float64 or not scratch.is_contiguous() or scratch.numel() < nuclear_scratch(logits, block, softmax):
        raise MmttaError("nuclear_entropy_items: scratch must be contiguous fp64 of nuclear_scratch(logits, block, softmax) elements")
    tz, tg = desc_cl(logits), desc_cl(dlogits)
    check(_lib.load().mmtta_nuclear_entropy_items(C.byref(tz), 1 if softmax else 0, bd, bh, bw, float(entropy_weight),
                                                  float(weight), float(eps), C.byref(tg), ptr(scratch), ptr(loss), ptr(entropy),
                                                  ptr(nuclear), stream_ptr()), "nuclear_entropy_items")


def _keep_mask(present: Optional[Sequence[bool]], channels: int) -> int:
    if present is None:
        return (1 << channels) - 1
    if len(present) != channels:
        raise MmttaError(f"input_norm: the modality mask has {len(present)} entries for {channels} input channels")
    return sum(1 << c for c, p in enumerate(present) if p)


def _input_norm_tables(what: str, n: int, c: int, **tables: Optional[torch.Tensor]) -> None:
    for name, (t, width) in tables.items():
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda or t.numel() < n * c * width:
            raise MmttaError(f"{what}: {name} must be contiguous device fp32 of at least {n * c * width} elements "
                             f"([{n}, {c}, {width}])")


def _input_branches(what: str, branches: Sequence[Tuple[torch.Tensor, torch.Tensor, int, int, int]], c: int):
    """The mmtta_input_norm_branch array of ``branches`` and the descriptors it points to (kept alive by the caller)."""
    descs = [desc_cl(dy) for dy, *_ in branches]
    arr = (_lib.InputNormBranch * max(len(branches), 1))()
    for r, (dy, weight, set_stride, k, stride) in enumerate(branches):
        if weight.dtype != torch.float32 or not weight.is_contiguous() or weight.numel() != int(dy.shape[-1]) * c * int(k) ** 3:
            raise MmttaError(f"{what}: weight of branch {r} must be contiguous fp32 [{int(dy.shape[-1])}, {c}, {k}, {k}, {k}]")
        arr[r] = _lib.InputNormBranch(C.pointer(descs[r]), ptr(weight), int(set_stride), int(k), int(stride))
    return arr, descs


def input_norm_apply(x: torch.Tensor, y: torch.Tensor, theta: torch.Tensor, value_range: torch.Tensor,
                     present: Optional[Sequence[bool]] = None, gamma: bool = False) -> None:
    """The input normaliser's map (include/mmtta.h, mmtta_input_norm_apply): y = exp(s) u + b per volume and channel, from
    the raw fp32 staged volume ``x`` into ``y`` (fp32 or bf16 rows), with ``theta`` [N, C, 4] = (s, b, g, 0), ``value_range``
    what ``intensity_range`` wrote for x; the channels ``present`` marks absent, and rows of theta that are zero, pass through."""
    n, c = int(x.shape[0]), int(x.shape[-1])
    _input_norm_tables("input_norm_apply", n, c, theta=(theta, 4), value_range=(value_range, 2))
    tx, ty = desc_cl(x), desc_cl(y)
    check(_lib.load().mmtta_input_norm_apply(C.byref(tx), C.byref(ty), ptr(theta), ptr(value_range), _keep_mask(present, c),
                                             1 if gamma else 0, stream_ptr()), "input_norm_apply")


def input_norm_grad_partials(x: torch.Tensor) -> int:
    """fp64 elements of the scratch ``input_norm_grad`` needs for the staged volume ``x``."""
    t = desc_cl(x)
    n = int(_lib.load().mmtta_input_norm_grad_partials(C.byref(t)))
    if n < 0:
        raise MmttaError(f"input_norm_grad_partials: no scratch size for x {tuple(x.shape)}")
    return n


def input_norm_grad(x: torch.Tensor, branches: Sequence[Tuple[torch.Tensor, torch.Tensor, int, int, int]], theta: torch.Tensor,
                    value_range: torch.Tensor, partial: torch.Tensor, grad: torch.Tensor, *,
                    present: Optional[Sequence[bool]] = None, gamma: bool = False, exp_avg: Optional[torch.Tensor] = None,
                    exp_avg_sq: Optional[torch.Tensor] = None, step: Optional[torch.Tensor] = None, lr: float = 0.0,
                    bounds: Sequence[float] = (0.0, 0.0, 0.0)) -> None:
    """The reduced input gradient of the first level (include/mmtta.h, mmtta_input_norm_grad): ``grad`` [N, C, 4] =
    (dL/ds, dL/db, dL/dg, 0) from the raw volume ``x`` and the ``branches`` that read it - (dy, weight, set_stride, k, stride)
    each: the output gradient the backward left (channels-last, fp32 or bf16, maybe a channel slice), the fp32 weights
    [c0, C, 3, 3, 3] of set 0 and the elements between the sets of consecutive items.  With ``lr`` > 0 the same call takes
    Adam's step on ``theta`` (state ``exp_avg`` / ``exp_avg_sq`` [N, C, 4], device int32 ``step`` [N]) and clamps it to
    +- ``bounds`` = (log_scale, shift, log_gamma)."""
    n, c = int(x.shape[0]), int(x.shape[-1])
    _input_norm_tables("input_norm_grad", n, c, theta=(theta, 4), value_range=(value_range, 2), grad=(grad, 4),
                       exp_avg=(exp_avg, 4), exp_avg_sq=(exp_avg_sq, 4))
    if partial.dtype != torch.float64 or not partial.is_contiguous() or partial.numel() < input_norm_grad_partials(x):
        raise MmttaError("input_norm_grad: partial must be contiguous fp64 of input_norm_grad_partials(x) elements")
    if step is not None and (step.dtype != torch.int32 or not step.is_contiguous() or step.numel() < n):
        raise MmttaError(f"input_norm_grad: step must be contiguous device int32 of at least {n} elements")
    arr, descs = _input_branches("input_norm_grad", branches, c)
    tx = desc_cl(x)
    check(_lib.load().mmtta_input_norm_grad(C.byref(tx), arr, len(branches), ptr(theta), ptr(value_range),
                                            _keep_mask(present, c), 1 if gamma else 0, ptr(partial), ptr(grad), ptr(exp_avg),
                                            ptr(exp_avg_sq), ptr(step), float(lr), float(bounds[0]), float(bounds[1]),
                                            float(bounds[2]), stream_ptr()), "input_norm_grad")


BIAS_ANCHORS = {"min": 0, "zero": 1}      # MMTTA_BIAS_ANCHOR_*
BIAS_ROW = 20                             # coefficients of a theta / grad row of the bias field, whatever the order


def _bias_field_args(what: str, x: torch.Tensor, tables: Sequence[torch.Tensor], order: int, anchor: str) -> int:
    if anchor not in BIAS_ANCHORS:
        raise MmttaError(f"{what}: anchor = {anchor!r} (min | zero)")
    if isinstance(order, bool) or not isinstance(order, int):
        raise MmttaError(f"{what}: order = {order!r} (an int)")
    if len(tables) != 3:
        raise MmttaError(f"{what}: tables must be the three Legendre tables (D, H, W), got {len(tables)}")
    for t, extent, axis in zip(tables, x.shape[1:4], "DHW"):
        if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda or t.numel() != 4 * int(extent):
            raise MmttaError(f"{what}: the table of axis {axis} must be contiguous device fp32 [4, {int(extent)}]")
    return BIAS_ANCHORS[anchor]


def bias_field_apply(x: torch.Tensor, y: torch.Tensor, theta: torch.Tensor, value_range: torch.Tensor,
                     tables: Sequence[torch.Tensor], order: int, anchor: str = "min",
                     present: Optional[Sequence[bool]] = None) -> None:
    """The bias field's map (include/mmtta.h, mmtta_bias_field_apply): y = (x - a) exp(F) + a per volume and channel, from the
    raw fp32 staged volume ``x`` into ``y`` (fp32 or bf16 rows), with ``theta`` [N, C, 20] the coefficients of F in the
    Legendre basis of total degree ``order``, ``tables`` the three [4, extent] tables of ``biasfield.legendre_tables`` and
    ``value_range`` what ``intensity_range`` wrote for x (``anchor`` "min": a = the channel's minimum; "zero": a = 0).  The
    channels ``present`` marks absent, and channels whose coefficients are all zero, pass through."""
    n, c = int(x.shape[0]), int(x.shape[-1])
    _input_norm_tables("bias_field_apply", n, c, theta=(theta, BIAS_ROW), value_range=(value_range, 2))
    code = _bias_field_args("bias_field_apply", x, tables, order, anchor)
    tx, ty = desc_cl(x), desc_cl(y)
    check(_lib.load().mmtta_bias_field_apply(C.byref(tx), C.byref(ty), ptr(theta), ptr(value_range), ptr(tables[0]), ptr(tables[1]),
                                             ptr(tables[2]), order, code, _keep_mask(present, c), stream_ptr()), "bias_field_apply")


def bias_field_grad_partials(x: torch.Tensor, order: int) -> int:
    """fp64 elements of the scratch ``bias_field_grad`` needs for the staged volume ``x`` at ``order``."""
    t = desc_cl(x)
    n = int(_lib.load().mmtta_bias_field_grad_partials(C.byref(t), int(order)))
    if n < 0:
        raise MmttaError(f"bias_field_grad_partials: no scratch size for x {tuple(x.shape)} at order {order}")
    return n


def bias_field_grad(x: torch.Tensor, branches: Sequence[Tuple[torch.Tensor, torch.Tensor, int, int, int]], theta: torch.Tensor,
                    value_range: torch.Tensor, tables: Sequence[torch.Tensor], order: int, partial: torch.Tensor,
                    grad: torch.Tensor, *, anchor: str = "min", present: Optional[Sequence[bool]] = None,
                    exp_avg: Optional[torch.Tensor] = None, exp_avg_sq: Optional[torch.Tensor] = None,
                    step: Optional[torch.Tensor] = None, lr: float = 0.0, bounds: Sequence[float] = (0.0, 0.0),
                    l2: float = 0.0) -> None:
    """The reduced input gradient of the first level against the field's basis (include/mmtta.h, mmtta_bias_field_grad):
    ``grad`` [N, C, 20] = dL/dtheta_ck + 2 ``l2`` theta_ck (k >= 1), the terms past the order's 0; ``x``, ``branches`` and the
    optimizer state as ``input_norm_grad`` takes them (rows of 20), ``tables`` / ``order`` / ``anchor`` as ``bias_field_apply``.
    With ``lr`` > 0 the same call takes Adam's step on ``theta`` and clamps the constant coefficient to +- ``bounds[0]`` and
    every other one to +- ``bounds[1]``."""
    n, c = int(x.shape[0]), int(x.shape[-1])
    _input_norm_tables("bias_field_grad", n, c, theta=(theta, BIAS_ROW), value_range=(value_range, 2), grad=(grad, BIAS_ROW),
                       exp_avg=(exp_avg, BIAS_ROW), exp_avg_sq=(exp_avg_sq, BIAS_ROW))
    code = _bias_field_args("bias_field_grad", x, tables, order, anchor)
    if partial.dtype != torch.float64 or not partial.is_contiguous() or partial.numel() < bias_field_grad_partials(x, order):
        raise MmttaError("bias_field_grad: partial must be contiguous fp64 of bias_field_grad_partials(x, order) elements")
    if step is not None and (step.dtype != torch.int32 or not step.is_contiguous() or step.numel() < n):
        raise MmttaError(f"bias_field_grad: step must be contiguous device int32 of at least {n} elements")
    arr, descs = _input_branches("bias_field_grad", branches, c)
    tx = desc_cl(x)
    check(_lib.load().mmtta_bias_field_grad(C.byref(tx), arr, len(branches), ptr(theta), ptr(value_range), ptr(tables[0]),
                                            ptr(tables[1]), ptr(tables[2]), order, code, _keep_mask(present, c), ptr(partial),
                                            ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), ptr(step), float(lr), float(bounds[0]),
                                            float(bounds[1]), float(l2), stream_ptr()), "bias_field_grad")


def modality_views(x: torch.Tensor, y: torch.Tensor, keep_masks: Sequence[int]) -> None:
    """y[g * V + v] = x[g] with channel c kept iff bit c of keep_masks[v] is set: channels-last [G,D,H,W,C] -> [G*V,D,H,W,C],
    fp32 or bf16.  Kept values keep their bits; a dropped channel and the pad lanes ``y`` owns are stored as +0."""
    masks = [int(m) for m in keep_masks]
    if any(not (0 <= m < 1 << 32) for m in masks):
        raise MmttaError(f"modality_views: keep_masks = {masks!r} (32-bit channel masks)")
    tx, ty = desc_cl(x), desc_cl(y)
    check(_lib.load().mmtta_modality_views(C.byref(tx), C.byref(ty), len(masks), (C.c_uint32 * max(len(masks), 1))(*masks),
                                           stream_ptr()), "modality_views")


def modcons_partials(logits: torch.Tensor, views: int) -> int:
    t = desc_cl(logits)
    return int(_lib.load().mmtta_modcons_partials(C.byref(t), int(views)))


def modcons_loss_items(logits: torch.Tensor, dlogits: torch.Tensor, views: int, partial: torch.Tensor, loss: torch.Tensor,
                       entropy: torch.Tensor, consistency: torch.Tensor, view_kl: torch.Tensor, disagree: torch.Tensor,
                       weight: float = 1.0, entropy_weight: float = 1.0, detach: bool = True, softmax: bool = False) -> None:
    """The modality-consistency objective of every volume on its own: logits / dlogits [G*V,D,H,W,R] (item g*V+v = view v of
    volume g, view 0 the full one); loss = entropy_weight * entropy + weight * consistency, all three fp32 [G]; view_kl fp32
    [G, V-1] (the mean KL of view 0's prediction to view v's); disagree int64 [G, V-1] (elements whose hard label differs)."""
    views = int(views)
    need = modcons_partials(logits, views)          # -1 for a bad view count: the entry point below says which
    g = int(logits.shape[0]) // max(views, 1)
    for name, t in (("loss", loss), ("entropy", entropy), ("consistency", consistency)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < g:
            raise MmttaError(f"modcons_loss_items: {name} must be contiguous fp32 with one slot per volume")
    if view_kl.dtype != torch.float32 or not view_kl.is_contiguous() or view_kl.numel() < g * (views - 1):
        raise MmttaError("modcons_loss_items: view_kl must be contiguous fp32 [volumes, views - 1]")
    if disagree.dtype != torch.int64 or not disagree.is_contiguous() or disagree.numel() < g * (views - 1):
        raise MmttaError("modcons_loss_items: disagree must be contiguous int64 [volumes, views - 1]")
    if partial.dtype != torch.float64 or partial.numel() < need:
        raise MmttaError("modcons_loss_items: partial must be fp64 of modcons_partials(logits, views) elements")
    tz, tg = desc_cl(logits), desc_cl(dlogits)
    check(_lib.load().mmtta_modcons_loss_items(C.byref(tz), 1 if softmax else 0, views, float(weight), float(entropy_weight),
                                               1 if detach else 0, C.byref(tg), ptr(partial), ptr(loss), ptr(entropy),
                                               ptr(consistency), ptr(view_kl), ptr(disagree), stream_ptr()), "modcons_loss_items")


def _window_grid(what: str, grid, origins: torch.Tensor, tables: Optional[torch.Tensor], roi: Sequence[int]) -> "_lib.WindowGrid":
    """The mmtta_window_grid of ``grid`` (``window.WindowGrid``: extents, starts per axis) after the checks that need the device
    buffers: int32 ``origins`` of at least W_n x 3 elements and fp32 ``tables`` of at least sum(count x roi) elements."""
    counts = [len(s) for s in grid.starts]
    windows = counts[0] * counts[1] * counts[2]
    if origins.dtype != torch.int32 or not origins.is_contiguous() or not origins.is_cuda or origins.numel() < windows * 3:
        raise MmttaError(f"{what}: origins must be contiguous device int32 of at least {windows * 3} elements ([{windows}, 3])")
    need = sum(c * int(r) for c, r in zip(counts, roi))
    if tables is not None and (tables.dtype != torch.float32 or not tables.is_contiguous() or not tables.is_cuda
                               or tables.numel() < need):
        raise MmttaError(f"{what}: tables must be contiguous device fp32 of at least {need} elements")
    return _lib.WindowGrid((C.c_int32 * 3)(*[int(e) for e in grid.extents]), (C.c_int32 * 3)(*counts))


def window_views(x: torch.Tensor, y: torch.Tensor, grid, origins: torch.Tensor, pad_value: float = 0.0) -> None:
    """y[g * W_n + w] = x[g] cropped at window w's origin (include/mmtta.h, mmtta_window_views): channels-last [G,D,H,W,C] ->
    [G*W_n,rd,rh,rw,C], fp32 or bf16.  Kept values keep their bits; outside the volume the channels take ``pad_value`` and the
    pad lanes ``y`` owns +0.  ``grid``: the ``window.WindowGrid`` of x's extents; ``origins``: its device copy, int32 [W_n, 3]."""
    wg = _window_grid("window_views", grid, origins, None, y.shape[1:4])
    flat = [int(o) for origin in grid.origins for o in origin]
    tx, ty = desc_cl(x), desc_cl(y)
    check(_lib.load().mmtta_window_views(C.byref(tx), C.byref(ty), C.byref(wg), (C.c_int32 * max(len(flat), 1))(*flat),
                                         ptr(origins), float(pad_value), stream_ptr()), "window_views")


def window_partials(logits: torch.Tensor) -> int:
    t = desc_cl(logits)
    return int(_lib.load().mmtta_window_partials(C.byref(t)))


def window_entropy_items(logits: torch.Tensor, dlogits: torch.Tensor, grid, origins: torch.Tensor, tables: torch.Tensor,
                         partial: torch.Tensor, loss: torch.Tensor, softmax: bool = False) -> None:
    """The sliding-window entropy of every volume on its own (include/mmtta.h, mmtta_window_entropy_items): logits / dlogits
    [G*W_n,rd,rh,rw,R] (item g*W_n+w = window w of volume g); loss fp32 [G] = the entropy of the windows' voxels under the
    weights of ``tables``, over the voxels of the unpadded volume."""
    wg = _window_grid("window_entropy_items", grid, origins, tables, logits.shape[1:4])
    windows = len(grid.origins)
    if loss.dtype != torch.float32 or not loss.is_contiguous() or loss.numel() < int(logits.shape[0]) // max(windows, 1):
        raise MmttaError("window_entropy_items: loss must be contiguous fp32 with one slot per volume")
    if partial.dtype != torch.float64 or partial.numel() < window_partials(logits):
        raise MmttaError("window_entropy_items: partial must be fp64 of window_partials(logits) elements")
    tz, tg = desc_cl(logits), desc_cl(dlogits)
    check(_lib.load().mmtta_window_entropy_items(C.byref(tz), 1 if softmax else 0, C.byref(wg), ptr(tables), C.byref(tg),
                                                 ptr(partial), ptr(loss), stream_ptr()), "window_entropy_items")


def window_blend(logits: torch.Tensor, out: torch.Tensor, grid, origins: torch.Tensor, tables: torch.Tensor) -> None:
    """out[g](v) = sum over the windows w that cover voxel v of a_w(v) * logits[g*W_n+w](v - o_w), fp32, fma in ascending window
    order (include/mmtta.h, mmtta_window_blend): [G*W_n,rd,rh,rw,R] -> [G,D,H,W,R] at the volume's extents."""
    wg = _window_grid("window_blend", grid, origins, tables, logits.shape[1:4])
    tz, to = desc_cl(logits), desc_cl(out)
    check(_lib.load().mmtta_window_blend(C.byref(tz), C.byref(to), C.byref(wg), ptr(origins), ptr(tables), stream_ptr()),
          "window_blend")


def sam_ascent_partials(n: int, sets: int) -> int:
    return int(_lib.load().mmtta_sam_ascent_partials(int(n), int(sets)))


def sam_ascent_sets(p: torch.Tensor, g: torch.Tensor, saved: torch.Tensor, partial: torch.Tensor, n: int, sets: int,
                    rho: float) -> None:
    """SAM's ascent over the first ``sets`` replicas of the arena ([replicas, total]; the first ``n`` elements of a replica
    train): saved[r, :n] = p[r, :n], p += rho * g / (||g|| + 1e-12), the norm per replica.  ``saved``: [>= sets, >= n]."""
    for t in (p, g):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.shape != p.shape:
            raise MmttaError("sam_ascent_sets: p and g must be contiguous fp32 [replicas, total] of equal shape")
    if saved.dtype != torch.float32 or not saved.is_contiguous() or saved.dim() != 2 or saved.shape[0] < sets \
            or saved.shape[1] < n:
        raise MmttaError(f"sam_ascent_sets: saved must be contiguous fp32 [>= {sets}, >= {n}], got {tuple(saved.shape)}")
    if partial.dtype != torch.float64 or partial.numel() < sam_ascent_partials(n, sets):
        raise MmttaError("sam_ascent_sets: partial must be fp64 of sam_ascent_partials(n, sets) elements")
    check(_lib.load().mmtta_sam_ascent_sets(ptr(p), ptr(g), ptr(saved), int(saved.shape[1]), ptr(partial), int(n), int(sets),
                                            int(p.shape[0]), int(p.shape[1]), float(rho), stream_ptr()), "sam_ascent_sets")


def adam_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, n_decay: int, lr: float,
              beta1: float, beta2: float, eps: float, weight_decay: float, step: torch.Tensor) -> None:
    n = p.numel()
    for t in (p, g, m, v):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise MmttaError("adam: p, g, m, v must be contiguous fp32 of equal length")
    if step.dtype != torch.int32:
        raise MmttaError("adam: step must be a device int32 scalar")
    check(_lib.load().mmtta_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), n, int(n_decay), lr, beta1, beta2, eps,
                                      weight_decay, ptr(step), stream_ptr()), "adam_step")


OPTIMIZERS = {"adam": _lib.OPTIM_ADAM, "adamw": _lib.OPTIM_ADAMW, "sgd": _lib.OPTIM_SGD}


@dataclass
class OptimSpec:
    """Hyper-parameters of the fused arena optimizer, read the way the reference's factory reads them (reference
    src/core/experiment_manager.py:199-237: `training.optimizer` names the class, `training.optimizers.<name>` holds
    its keyword arguments, `training.learning_rate / weight_decay / momentum` are the fall-backs)."""
    name: str = "adam"
    lr: float = 1e-3
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    weight_decay: float = 0.0
    momentum: float = 0.0
    dampening: float = 0.0
    nesterov: bool = False

    def struct(self) -> _lib.OptimDesc:
        return _lib.OptimDesc(OPTIMIZERS[self.name], self.lr, self.beta1, self.beta2, self.eps, self.weight_decay,
                              self.momentum, self.dampening, 1 if self.nesterov else 0)


def optim_step(spec: OptimSpec, p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: Optional[torch.Tensor],
               n_decay: int, step: torch.Tensor) -> None:
    """One step of torch.optim.{Adam, AdamW, SGD} over the flat arena ([0, n_decay) decays)."""
    n = p.numel()
    for t in (p, g, m) + ((v,) if v is not None else ()):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise MmttaError("optimizer: p, g, m, v must be contiguous fp32 of equal length")
    if step.dtype != torch.int32:
        raise MmttaError("optimizer: step must be a device int32 scalar")
    d = spec.struct()
    check(_lib.load().mmtta_optim_step(C.byref(d), ptr(p), ptr(g), ptr(m), ptr(v), n, int(n_decay), ptr(step),
                                       stream_ptr()), "optim_step")


def optim_step_sets(spec: OptimSpec, p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: Optional[torch.Tensor], n: int,
                    n_decay: int, sets: int, step: torch.Tensor) -> None:
    """One optimizer step over the first ``sets`` replicas of the arena ([replica][total], the first ``n`` elements of a
    replica train, its first ``n_decay`` decay) in one launch; one shared step counter."""
    for t in (p, g, m) + ((v,) if v is not None else ()):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.shape != p.shape:
            raise MmttaError("optimizer: p, g, m, v must be contiguous fp32 [replicas, total] of equal shape")
    if not (1 <= sets <= p.shape[0] and 0 <= n_decay <= n <= p.shape[1]):
        raise MmttaError(f"optimizer: {sets} sets of {n} ({n_decay} decaying) elements do not fit {tuple(p.shape)}")
    if step.dtype != torch.int32:
        raise MmttaError("optimizer: step must be a device int32 scalar")
    d = spec.struct()
    check(_lib.load().mmtta_optim_step_sets(C.byref(d), ptr(p), ptr(g), ptr(m), ptr(v), int(n), int(n_decay), int(sets),
                                            int(p.shape[1]), ptr(step), stream_ptr()), "optim_step_sets")


def optim_segments_table(segments: Sequence[Tuple[int, int, bool]], device) -> Tuple[torch.Tensor, int]:
    """Device table of mmtta_optim_step_segments: [count][3] (start, length, decay) then the [count] running starts."""
    rows, starts, run = [], [], 0
    for a, n, dec in segments:
        if a % 4 or n % 4 or n <= 0:
            raise MmttaError(f"optimizer segment ({a}, {n}) is not a positive run of whole 16-byte groups")
        rows += [int(a), int(n), 1 if dec else 0]
        starts.append(run)
        run += int(n)
    return torch.tensor(rows + starts, dtype=torch.int64).to(device), run


def optim_step_segments(spec: OptimSpec, p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: Optional[torch.Tensor],
                        table: torch.Tensor, count: int, total: int, sets: int, step: torch.Tensor) -> None:
    """optim_step_sets over the segments of ``table`` (optim_segments_table) of the first ``sets`` replicas, then the step
    counter advances once."""
    for t in (p, g, m) + ((v,) if v is not None else ()):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.shape != p.shape:
            raise MmttaError("optimizer: p, g, m, v must be contiguous fp32 [replicas, total] of equal shape")
    if not 1 <= sets <= p.shape[0]:
        raise MmttaError(f"optimizer: {sets} sets do not fit {tuple(p.shape)}")
    d = spec.struct()
    check(_lib.load().mmtta_optim_step_segments(C.byref(d), ptr(p), ptr(g), ptr(m), ptr(v), ptr(table), int(count), int(total),
                                                int(sets), int(p.shape[1]), ptr(step), stream_ptr()), "optim_step_segments")


def _desc_any(t: torch.Tensor, channels_last: bool):
    return desc_cl(t) if channels_last else desc_ncdhw(t)


def mask_dice_counts(logits: torch.Tensor, label_ncdhw: torch.Tensor, threshold: float, counts: torch.Tensor,
                     mask: Optional[torch.Tensor] = None, logits_channels_last: bool = True) -> None:
    tz = _desc_any(logits, logits_channels_last)
    tl = desc_ncdhw(label_ncdhw)
    check(_lib.load().mmtta_mask_dice_counts(C.byref(tz), C.byref(tl), float(threshold), ptr(counts), ptr(mask),
                                             stream_ptr()), "mask_dice_counts")


_DCE_SCRATCH: Dict[Tuple, torch.Tensor] = {}     # block partials of dice_ce_sums, per (device, size)


def dice_ce_sums(logits: torch.Tensor, label_ncdhw: torch.Tensor, weight: Optional[torch.Tensor], squared_pred: bool,
                 out: torch.Tensor, logits_channels_last: bool = True, softmax: bool = False) -> None:
    tz = _desc_any(logits, logits_channels_last)
    tl = desc_ncdhw(label_ncdhw)
    lib = _lib.load()
    nbytes = int(lib.mmtta_dice_ce_scratch_bytes(C.byref(tz)))
    if nbytes < 0:
        check(-2, "dice_ce_scratch_bytes")
    key = (logits.device.index, nbytes, int(torch.cuda.current_stream().cuda_stream))   # per stream: lanes run concurrently
    scratch = _DCE_SCRATCH.get(key)
    if scratch is None:
        scratch = _DCE_SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=logits.device)
    check(lib.mmtta_dice_ce_sums(C.byref(tz), C.byref(tl), ptr(weight), 1 if squared_pred else 0, 1 if softmax else 0, ptr(out),
                                 ptr(scratch), stream_ptr()), "dice_ce_sums")


def dice_ce_grad(logits: torch.Tensor, label_ncdhw: torch.Tensor, weight: Optional[torch.Tensor], squared_pred: bool,
                 jaccard: bool, include_background: bool, lambda_dice: float, lambda_ce: float, sums: torch.Tensor,
                 dlogits: torch.Tensor, logits_channels_last: bool = True, smooth_nr: float = 1e-5,
                 smooth_dr: float = 1e-5, softmax: bool = False) -> None:
    """d DiceCE / d logits from the device-resident sums of ``dice_ce_sums`` (same layouts as there)."""
    tz = _desc_any(logits, logits_channels_last)
    tg = _desc_any(dlogits, logits_channels_last)
    tl = desc_ncdhw(label_ncdhw)
    check(_lib.load().mmtta_dice_ce_grad(C.byref(tz), C.byref(tl), ptr(weight), 1 if squared_pred else 0, 1 if softmax else 0,
                                         1 if jaccard else 0, 1 if include_background else 0, float(lambda_dice),
                                         float(lambda_ce), float(smooth_nr), float(smooth_dr), ptr(sums), C.byref(tg),
                                         stream_ptr()), "dice_ce_grad")


CALIBRATION_SCOPES = {"volume": 0, "union": 1}


def calibration_bins(logits: torch.Tensor, label_ncdhw: torch.Tensor, bins: int, out: torch.Tensor, softmax: bool = False,
                     scope: str = "volume", logits_channels_last: bool = False) -> None:
    """Reliability histogram + Brier / NLL sums of every (volume, region) -> ``out`` fp64 [N, Rout, 3*bins + 2] on the
    device (include/mmtta.h: mmtta_calibration_bins), queued on the current stream.  Scratch, where the library asks for
    any, is the lane's ``Workspace``."""
    if scope not in CALIBRATION_SCOPES:
        raise MmttaError(f"calibration_bins: scope {scope!r} (one of {sorted(CALIBRATION_SCOPES)})")
    tz = _desc_any(logits, logits_channels_last)
    tl = desc_ncdhw(label_ncdhw)
    rout = 1 if softmax else int(tz.c)
    if out.dtype != torch.float64 or not out.is_contiguous() or not out.is_cuda or out.numel() != tz.n * rout * (3 * int(bins) + 2):
        raise MmttaError(f"calibration_bins: `out` must be a dense CUDA float64 [{tz.n}, {rout}, {3 * int(bins) + 2}] tensor, got "
                         f"{out.dtype} {tuple(out.shape)}")
    lib = _lib.load()
    nbytes = int(lib.mmtta_calibration_scratch_bytes(C.byref(tz), int(bins)))
    if nbytes < 0:
        check(-1, "calibration_scratch_bytes")
    scratch = Workspace.get(nbytes, logits.device) if nbytes > 0 else None
    check(lib.mmtta_calibration_bins(C.byref(tz), C.byref(tl), 1 if softmax else 0, int(bins), CALIBRATION_SCOPES[scope],
                                     ptr(out), ptr(scratch), stream_ptr()), "calibration_bins")


_SURF_SCRATCH: Dict[Tuple, torch.Tensor] = {}    # working set of surface_distances, per (device, size)


def surface_distances(pred_mask: torch.Tensor, label_ncdhw: torch.Tensor, spacing: Sequence[float],
                      percentile: float = 95.0, asd_symmetric: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """pred_mask uint8 [B,R,D,H,W] (dense; from ``mask_dice_counts``) + labels -> (hd, asd) fp32 [B,R] on the device,
    as MONAI returns them (reference src/evaluation/seg_eval.py:327-341); the evaluator applies the fix-ups."""
    if pred_mask.dtype != torch.uint8 or not pred_mask.is_contiguous() or pred_mask.shape != label_ncdhw.shape:
        raise MmttaError(f"surface_distances: mask must be dense uint8 of the label's shape, got {pred_mask.dtype} "
                         f"{tuple(pred_mask.shape)} vs {tuple(label_ncdhw.shape)}")
    B, R, D, H, W = (int(v) for v in pred_mask.shape)
    lib = _lib.load()
    nbytes = int(lib.mmtta_surface_scratch_bytes(B * R, D, H, W))
    if nbytes < 0:
        raise MmttaError(f"surface_distances: extent {(D, H, W)} unsupported (at most 1024 per axis)")
    key = (pred_mask.device.index, nbytes, int(torch.cuda.current_stream().cuda_stream))  # per stream: lanes run concurrently
    scratch = _SURF_SCRATCH.get(key)
    if scratch is None:
        for k in [k for k in _SURF_SCRATCH if k[2] == key[2]]:      # a new shape on this stream replaces its old working set
            del _SURF_SCRATCH[k]
        scratch = _SURF_SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=pred_mask.device)
    hd = torch.empty((B, R), dtype=torch.float32, device=pred_mask.device)
    asd = torch.empty((B, R), dtype=torch.float32, device=pred_mask.device)
    sp = (C.c_double * 3)(*[float(v) for v in spacing])
    tl = desc_ncdhw(label_ncdhw)
    check(lib.mmtta_surface_distances(ptr(pred_mask), C.byref(tl), sp, float(percentile), 1 if asd_symmetric else 0,
                                      ptr(hd), ptr(asd), ptr(scratch), stream_ptr()), "surface_distances")
    return hd, asd


_CC_SCRATCH: Dict[Tuple, torch.Tensor] = {}      # working set of components_filter, per (device, size, stream)
COMPONENT_CONNECTIVITIES = (6, 18, 26)
COMPONENTS_MAX_REGIONS = 64


def _per_region(value, R: int, what: str) -> List[int]:
    vals = [value] * R if isinstance(value, (bool, int)) else list(value)
    if len(vals) != R:
        raise MmttaError(f"components_filter: {what} has {len(vals)} entries for {R} regions")
    return [int(v) for v in vals]


def components_filter(mask: torch.Tensor, label_ncdhw: Optional[torch.Tensor] = None, connectivity: int = 26, min_voxels=0,
                      keep_largest=False, out: Optional[torch.Tensor] = None, want_counts: bool = True, want_stats: bool = True,
                      want_labels: bool = False) -> Dict[str, Optional[torch.Tensor]]:
    """Connected components of every (volume, region) of ``mask`` (uint8 [B,R,D,H,W], dense; from ``mask_dice_counts``),
    then the size filter and the keep-largest filter (include/mmtta.h: mmtta_components_filter), queued on the current
    stream.  ``min_voxels`` / ``keep_largest``: one value, or one per region.  ``out``: where the filtered mask goes
    (default: a new tensor; pass ``mask`` itself to filter in place).  Returns the device tensors: ``mask`` uint8,
    ``counts`` int64 [B,R,3] (inter, psum, gsum of the filtered mask; needs a label), ``stats`` int64 [B,R,3]
    (components, kept, removed voxels), ``labels`` int32 [B,R,D,H,W] of the raw mask (1 + smallest voxel index)."""
    if mask.dtype != torch.uint8 or mask.dim() != 5 or not mask.is_contiguous() or not mask.is_cuda:
        raise MmttaError(f"components_filter: mask must be a dense CUDA uint8 [B,R,D,H,W] tensor, got {mask.dtype} {tuple(mask.shape)}")
    B, R, D, H, W = (int(v) for v in mask.shape)
    if min(B, R, D, H, W) < 1:
        raise MmttaError(f"components_filter: empty mask {tuple(mask.shape)}")
    if R > COMPONENTS_MAX_REGIONS:
        raise MmttaError(f"components_filter: {R} regions, at most {COMPONENTS_MAX_REGIONS}")
    if connectivity not in COMPONENT_CONNECTIVITIES:
        raise MmttaError(f"components_filter: connectivity {connectivity!r} (one of {list(COMPONENT_CONNECTIVITIES)})")
    if out is None:
        out = torch.empty_like(mask)
    elif out.dtype != torch.uint8 or out.shape != mask.shape or not out.is_contiguous() or out.device != mask.device:
        raise MmttaError(f"components_filter: `out` must be dense uint8 of the mask's shape, got {out.dtype} {tuple(out.shape)}")
    if label_ncdhw is not None and (tuple(label_ncdhw.shape) != tuple(mask.shape) or label_ncdhw.device != mask.device or
                                    label_ncdhw.dtype != torch.float32):
        raise MmttaError(f"components_filter: label must be float32 of the mask's shape on the mask's device, got "
                         f"{label_ncdhw.dtype} {tuple(label_ncdhw.shape)} on {label_ncdhw.device} vs {tuple(mask.shape)} on "
                         f"{mask.device}")
    mv = _per_region(min_voxels, R, "min_voxels")
    if any(v < 0 for v in mv):
        raise MmttaError(f"components_filter: min_voxels must not be negative, got {mv}")
    kl = _per_region(keep_largest, R, "keep_largest")
    lib = _lib.load()
    nbytes = int(lib.mmtta_components_scratch_bytes(B * R, D, H, W))
    if nbytes < 0:
        raise MmttaError(f"components_filter: extent {(B * R, D, H, W)} unsupported (D*H*W <= 2**31 - 2, B*R <= 65535, "
                         f"B*R*D*H*W below 2**32: split the batch)")
    key = (mask.device.index, nbytes, int(torch.cuda.current_stream().cuda_stream))      # per stream: lanes run concurrently
    scratch = _CC_SCRATCH.get(key)
    if scratch is None:
        for k in [k for k in _CC_SCRATCH if k[2] == key[2]]:       # a new shape on this stream replaces its old working set
            del _CC_SCRATCH[k]
        scratch = _CC_SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=mask.device)
    dev = mask.device
    counts = torch.empty((B, R, 3), dtype=torch.int64, device=dev) if (want_counts and label_ncdhw is not None) else None
    stats = torch.empty((B, R, 3), dtype=torch.int64, device=dev) if want_stats else None
    labels = torch.empty((B, R, D, H, W), dtype=torch.int32, device=dev) if want_labels else None
    tl = desc_ncdhw(label_ncdhw) if label_ncdhw is not None else None
    check(lib.mmtta_components_filter(ptr(mask), ptr(out), C.byref(tl) if tl is not None else None, B, R, D, H, W,
                                      int(connectivity), (C.c_int64 * R)(*mv), (C.c_int32 * R)(*kl), ptr(counts), ptr(stats),
                                      ptr(labels), ptr(scratch), stream_ptr()), "components_filter")
    return {"mask": out, "counts": counts, "stats": stats, "labels": labels}


_FN_SCRATCH: Dict[Tuple, torch.Tensor] = {}      # working set of fill_nest, per (device, size, stream)
FILL_NEST_MODES = ("clip", "grow")
FILL_NEST_COLUMNS = ("holes", "filled_holes", "filled_voxels", "nested_voxels")


def fill_nest(mask: torch.Tensor, label_ncdhw: Optional[torch.Tensor] = None, fill_holes=False, fill_connectivity: int = 6,
              max_hole_voxels=0, nesting: Sequence[int] = (), nesting_mode: str = "clip",
              want_counts: bool = True) -> Dict[str, Optional[torch.Tensor]]:
    """Hole filling, then region nesting, IN PLACE on every (volume, region) of ``mask`` (uint8 [B,R,D,H,W], dense; from
    ``mask_dice_counts`` or ``components_filter``), queued on the current stream (include/mmtta.h: mmtta_mask_fill_nest).
    A hole is a component of the background at ``fill_connectivity`` that touches no face of the volume; region r fills
    its holes where ``fill_holes[r]`` is set and the hole has at most ``max_hole_voxels[r]`` voxels (0: no cap); both take
    one value, or one per region.  ``nesting``: region indices, innermost first (empty, or at least two distinct ones);
    ``clip`` cuts every region of the chain to the ones further out, ``grow`` extends it by the ones further in.  Returns
    the device tensors ``mask`` (the argument, 0 / 1), ``counts`` int64 [B,R,3] (inter, psum, gsum of the final mask; needs a
    label) and ``stats`` int64 [B,R,4] (``FILL_NEST_COLUMNS``)."""
    if mask.dtype != torch.uint8 or mask.dim() != 5 or not mask.is_contiguous() or not mask.is_cuda:
        raise MmttaError(f"fill_nest: mask must be a dense CUDA uint8 [B,R,D,H,W] tensor, got {mask.dtype} {tuple(mask.shape)}")
    B, R, D, H, W = (int(v) for v in mask.shape)
    if min(B, R, D, H, W) < 1:
        raise MmttaError(f"fill_nest: empty mask {tuple(mask.shape)}")
    if R > COMPONENTS_MAX_REGIONS:
        raise MmttaError(f"fill_nest: {R} regions, at most {COMPONENTS_MAX_REGIONS}")
    if isinstance(fill_connectivity, bool) or fill_connectivity not in COMPONENT_CONNECTIVITIES:
        raise MmttaError(f"fill_nest: fill_connectivity {fill_connectivity!r} (one of {list(COMPONENT_CONNECTIVITIES)})")
    if nesting_mode not in FILL_NEST_MODES:
        raise MmttaError(f"fill_nest: nesting_mode {nesting_mode!r} (one of {list(FILL_NEST_MODES)})")
    if label_ncdhw is not None and (tuple(label_ncdhw.shape) != tuple(mask.shape) or label_ncdhw.device != mask.device or
                                    label_ncdhw.dtype != torch.float32):
        raise MmttaError(f"fill_nest: label must be float32 of the mask's shape on the mask's device, got "
                         f"{label_ncdhw.dtype} {tuple(label_ncdhw.shape)} on {label_ncdhw.device} vs {tuple(mask.shape)} on "
                         f"{mask.device}")
    per = []
    for value, what in ((fill_holes, "fill_holes"), (max_hole_voxels, "max_hole_voxels")):
        vals = [value] * R if isinstance(value, (bool, int)) else list(value)
        if len(vals) != R:
            raise MmttaError(f"fill_nest: {what} has {len(vals)} entries for {R} regions")
        per.append([int(v) for v in vals])
    fh, cap = per
    if any(v < 0 for v in cap):
        raise MmttaError(f"fill_nest: max_hole_voxels must not be negative, got {cap}")
    chain = [int(c) for c in nesting]
    if len(chain) == 1 or len(set(chain)) != len(chain) or any(not 0 <= c < R for c in chain):
        raise MmttaError(f"fill_nest: nesting {chain} must be empty or at least two distinct region indices in 0 ... {R - 1}")
    lib = _lib.load()
    nbytes = int(lib.mmtta_mask_fill_nest_scratch_bytes(B * R, D, H, W))
    if nbytes < 0:
        raise MmttaError(f"fill_nest: extent {(B * R, D, H, W)} unsupported (D*H*W <= 2**31 - 2, B*R <= 65535, "
                         f"B*R*D*H*W below 2**32: split the batch)")
    key = (mask.device.index, nbytes, int(torch.cuda.current_stream().cuda_stream))      # per stream: lanes run concurrently
    scratch = _FN_SCRATCH.get(key)
    if scratch is None:
        for k in [k for k in _FN_SCRATCH if k[2] == key[2]]:       # a new shape on this stream replaces its old working set
            del _FN_SCRATCH[k]
        scratch = _FN_SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=mask.device)
    counts = torch.empty((B, R, 3), dtype=torch.int64, device=mask.device) if (want_counts and label_ncdhw is not None) else None
    stats = torch.empty((B, R, 4), dtype=torch.int64, device=mask.device)
    tl = desc_ncdhw(label_ncdhw) if label_ncdhw is not None else None
    check(lib.mmtta_mask_fill_nest(ptr(mask), C.byref(tl) if tl is not None else None, B, R, D, H, W, int(fill_connectivity),
                                   (C.c_int32 * R)(*fh), (C.c_int64 * R)(*cap), (C.c_int32 * max(1, len(chain)))(*chain),
                                   len(chain), FILL_NEST_MODES.index(nesting_mode), ptr(counts), ptr(stats), ptr(scratch),
                                   stream_ptr()), "fill_nest")
    return {"mask": mask, "counts": counts, "stats": stats}


_LW_SCRATCH: Dict[Tuple, torch.Tensor] = {}      # working set of lesionwise_scores, per (device, size, stream)
LESIONWISE_MAX_DILATION = 8
LESIONWISE_COLUMNS = ("lesions", "lesions_kept", "lesions_found", "pred_components", "matched_components", "dice_q", "fp_voxels")
LESIONWISE_Q_ONE = 1 << 30                       # a lesion's Dice is summed in units of 2^-30


def lesionwise_scores(mask: torch.Tensor, label_ncdhw: torch.Tensor, iterations: int = 3, dilation_connectivity: int = 18,
                      min_lesion_voxels=0, want_labels: bool = False) -> Dict[str, Optional[torch.Tensor]]:
    """Lesion-wise scores of every (volume, region) of ``mask`` (uint8 [B,R,D,H,W], dense; from ``mask_dice_counts`` or
    ``components_filter``) against ``label_ncdhw`` (include/mmtta.h: mmtta_lesionwise_scores), queued on the current stream.
    The ground truth is dilated ``iterations`` times with the ``dilation_connectivity`` neighbourhood; the 26-connected
    components of that are the lesions, those of the mask the predicted components.  ``min_lesion_voxels``: one value, or
    one per region.  Returns the device tensors ``stats`` int64 [B,R,7] (``LESIONWISE_COLUMNS``; ``dice_q`` in units of
    2^-30) and ``labels`` int32 [B,R,D,H,W] (the lesion of every ground-truth voxel, 1 + smallest voxel index of the dilated
    component; with ``want_labels``)."""
    if mask.dtype != torch.uint8 or mask.dim() != 5 or not mask.is_contiguous() or not mask.is_cuda:
        raise MmttaError(f"lesionwise_scores: mask must be a dense CUDA uint8 [B,R,D,H,W] tensor, got {mask.dtype} {tuple(mask.shape)}")
    B, R, D, H, W = (int(v) for v in mask.shape)
    if min(B, R, D, H, W) < 1:
        raise MmttaError(f"lesionwise_scores: empty mask {tuple(mask.shape)}")
    if R > COMPONENTS_MAX_REGIONS:
        raise MmttaError(f"lesionwise_scores: {R} regions, at most {COMPONENTS_MAX_REGIONS}")
    if isinstance(iterations, bool) or not isinstance(iterations, int) or not 0 <= iterations <= LESIONWISE_MAX_DILATION:
        raise MmttaError(f"lesionwise_scores: iterations {iterations!r} (an integer in 0 ... {LESIONWISE_MAX_DILATION})")
    if dilation_connectivity not in COMPONENT_CONNECTIVITIES:
        raise MmttaError(f"lesionwise_scores: dilation_connectivity {dilation_connectivity!r} (one of {list(COMPONENT_CONNECTIVITIES)})")
    if (not torch.is_tensor(label_ncdhw) or tuple(label_ncdhw.shape) != tuple(mask.shape) or label_ncdhw.device != mask.device or
            label_ncdhw.dtype != torch.float32):
        raise MmttaError(f"lesionwise_scores: label must be float32 of the mask's shape {tuple(mask.shape)} on the mask's device")
    vals = [min_lesion_voxels] * R if isinstance(min_lesion_voxels, (bool, int)) else list(min_lesion_voxels)
    if len(vals) != R:
        raise MmttaError(f"lesionwise_scores: min_lesion_voxels has {len(vals)} entries for {R} regions")
    mv = [int(v) for v in vals]
    if any(v < 0 for v in mv):
        raise MmttaError(f"lesionwise_scores: min_lesion_voxels must not be negative, got {mv}")
    lib = _lib.load()
    nbytes = int(lib.mmtta_lesionwise_scratch_bytes(B * R, D, H, W))
    if nbytes < 0:
        raise MmttaError(f"lesionwise_scores: extent {(B * R, D, H, W)} unsupported (D*H*W <= 2**31 - 2, B*R <= 65535, "
                         f"B*R*D*H*W below 2**32: split the batch)")
    key = (mask.device.index, nbytes, int(torch.cuda.current_stream().cuda_stream))      # per stream: lanes run concurrently
    scratch = _LW_SCRATCH.get(key)
    if scratch is None:
        for k in [k for k in _LW_SCRATCH if k[2] == key[2]]:       # a new shape on this stream replaces its old working set
            del _LW_SCRATCH[k]
        scratch = _LW_SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=mask.device)
    stats = torch.empty((B, R, 7), dtype=torch.int64, device=mask.device)
    labels = torch.empty((B, R, D, H, W), dtype=torch.int32, device=mask.device) if want_labels else None
    tl = desc_ncdhw(label_ncdhw)
    check(lib.mmtta_lesionwise_scores(ptr(mask), C.byref(tl), B, R, D, H, W, int(iterations), int(dilation_connectivity),
                                      (C.c_int64 * R)(*mv), ptr(stats), ptr(labels), ptr(scratch), stream_ptr()),
          "lesionwise_scores")
    return {"stats": stats, "labels": labels}


_LW_HD_SCRATCH: Dict[Tuple, torch.Tensor] = {}   # working set of lesionwise_hd95 beside the one of lesionwise_scores, likewise
LESIONWISE_HD_COLUMNS = ("hd_q", "lesions_scored", "overflow")
LESIONWISE_HD_Q_ONE = 1 << 20                    # a lesion's HD is summed in units of 2^-20
LESIONWISE_HD_MAX_EXTENT = 1024


def lesionwise_hd95(mask: torch.Tensor, label_ncdhw: torch.Tensor, iterations: int = 3, dilation_connectivity: int = 18,
                    min_lesion_voxels=0, spacing: Sequence[float] = (1.0, 1.0, 1.0), percentile: float = 95.0,
                    want_lesion_hd: bool = False, want_labels: bool = False) -> Dict[str, Optional[torch.Tensor]]:
    """Lesion-wise scores AND lesion-wise HD of every (volume, region) of ``mask`` against ``label_ncdhw``: ``lesionwise_scores``
    followed, on the same scratch and the current stream, by include/mmtta.h: mmtta_lesionwise_hd95.  Every kept lesion with a
    match gets the ``percentile`` Hausdorff distance between the surface of its own voxels and the surface of the predicted
    components matched to it, in the units of ``spacing`` (D, H, W order).  Returns the device tensors ``stats`` int64 [B,R,7]
    (identical to ``lesionwise_scores``' own), ``hd_stats`` int64 [B,R,3] (``LESIONWISE_HD_COLUMNS``; ``hd_q`` in units of
    2^-20; ``overflow`` > 0: the region's surface lists did not fit and none of its lesions is scored), ``lesion_hd`` float32
    [B,R,D,H,W] (NaN, and a lesion's HD at index lesion label - 1; with ``want_lesion_hd``) and ``labels`` (with
    ``want_labels``)."""
    try:
        sp = [float(v) for v in spacing]
    except (TypeError, ValueError):
        sp = []
    if len(sp) != 3 or not all(math.isfinite(v) and v > 0.0 for v in sp):
        raise MmttaError(f"lesionwise_hd95: spacing must be three positive finite numbers (D, H, W), got {spacing!r}")
    if isinstance(percentile, bool) or not isinstance(percentile, (int, float)) or not 0.0 <= float(percentile) <= 100.0:
        raise MmttaError(f"lesionwise_hd95: percentile {percentile!r} (a number in [0, 100])")
    if torch.is_tensor(mask) and mask.dim() == 5 and max(int(v) for v in mask.shape[2:]) > LESIONWISE_HD_MAX_EXTENT:
        raise MmttaError(f"lesionwise_hd95: extent {tuple(mask.shape[2:])} unsupported (at most {LESIONWISE_HD_MAX_EXTENT} per axis)")
    res = lesionwise_scores(mask, label_ncdhw, iterations, dilation_connectivity, min_lesion_voxels, want_labels=want_labels)
    B, R, D, H, W = (int(v) for v in mask.shape)
    vals = [min_lesion_voxels] * R if isinstance(min_lesion_voxels, (bool, int)) else list(min_lesion_voxels)
    mv = [int(v) for v in vals]
    lib = _lib.load()
    stream = int(torch.cuda.current_stream().cuda_stream)
    lw_scratch = _LW_SCRATCH[(mask.device.index, int(lib.mmtta_lesionwise_scratch_bytes(B * R, D, H, W)), stream)]
    nbytes = int(lib.mmtta_lesionwise_hd95_scratch_bytes(B * R, D, H, W))
    if nbytes < 0:
        raise MmttaError(f"lesionwise_hd95: extent {(B * R, D, H, W)} unsupported")
    key = (mask.device.index, nbytes, stream)
    scratch = _LW_HD_SCRATCH.get(key)
    if scratch is None:
        for k in [k for k in _LW_HD_SCRATCH if k[2] == key[2]]:
            del _LW_HD_SCRATCH[k]
        scratch = _LW_HD_SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=mask.device)
    hd_stats = torch.empty((B, R, 3), dtype=torch.int64, device=mask.device)
    lesion_hd = torch.empty((B, R, D, H, W), dtype=torch.float32, device=mask.device) if want_lesion_hd else None
    tl = desc_ncdhw(label_ncdhw)
    check(lib.mmtta_lesionwise_hd95(ptr(mask), C.byref(tl), B, R, D, H, W, (C.c_double * 3)(*sp), float(percentile),
                                    (C.c_int64 * R)(*mv), ptr(lw_scratch), ptr(hd_stats), ptr(lesion_hd), ptr(scratch),
                                    stream_ptr()), "lesionwise_hd95")
    return {"stats": res["stats"], "hd_stats": hd_stats, "lesion_hd": lesion_hd, "labels": res["labels"]}


_SD_SCRATCH: Dict[Tuple, torch.Tensor] = {}      # working set of surface_dice, per (device, size, stream)
SURFACE_DICE_COLUMNS = ("hits_pred", "edge_pred", "hits_gt", "edge_gt")
SURFACE_DICE_MAX_TOLERANCES = 4
SURFACE_DICE_MAX_RADIUS = 8                      # search window per axis, in voxels


def surface_dice_radius(spacing: Sequence[float], tolerance: float) -> Tuple[int, int, int]:
    """The search window of the NSD kernels for ``tolerance`` (the largest of a call) at ``spacing`` (D, H, W): per axis the
    largest k >= 0 with float32(sqrt((k s)^2)) <= float32(tolerance), found by the loop the library runs.  A radius above
    ``SURFACE_DICE_MAX_RADIUS`` is reported as ``SURFACE_DICE_MAX_RADIUS + 1``."""
    tau = C.c_float(float(tolerance)).value          # rounded to float32, as the kernel holds it
    out = []
    for s in spacing:
        k = 0
        while k <= SURFACE_DICE_MAX_RADIUS:
            f = float(k + 1) * float(s)
            if not C.c_float(math.sqrt(f * f)).value <= tau:
                break
            k += 1
        out.append(k)
    return out[0], out[1], out[2]


def _nsd_arguments(who: str, spacing, tolerances) -> Tuple[List[float], List[float]]:
    try:
        sp = [float(v) for v in spacing]
    except (TypeError, ValueError):
        sp = []
    if len(sp) != 3 or not all(math.isfinite(v) and v > 0.0 for v in sp):
        raise MmttaError(f"{who}: spacing must be three positive finite numbers (D, H, W), got {spacing!r}")
    try:
        tol = [float(v) for v in tolerances]
        ok = not isinstance(tolerances, (str, bytes)) and all(not isinstance(v, (bool, str, bytes)) for v in tolerances)
    except (TypeError, ValueError):
        tol, ok = [], False
    if not ok or not 1 <= len(tol) <= SURFACE_DICE_MAX_TOLERANCES or not all(math.isfinite(v) and v >= 0.0 for v in tol):
        raise MmttaError(f"{who}: tolerances must be 1 ... {SURFACE_DICE_MAX_TOLERANCES} finite numbers >= 0, got {tolerances!r}")
    rad = surface_dice_radius(sp, max(tol))
    if max(rad) > SURFACE_DICE_MAX_RADIUS:
        raise MmttaError(f"{who}: tolerances {tol} need a search window of more than {SURFACE_DICE_MAX_RADIUS} voxels at spacing "
                         f"{sp}; surface_distances (HD95 / ASD) is the tool for large distances")
    return sp, tol


def surface_dice(pred_mask: torch.Tensor, label_ncdhw: torch.Tensor, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                 tolerances: Sequence[float] = (1.0,)) -> torch.Tensor:
    """The counts behind the normalised surface Dice of every (volume, region) of ``pred_mask`` (uint8 [B,R,D,H,W], dense)
    against ``label_ncdhw`` at each of ``tolerances`` (1 ... 4, in the units of ``spacing``, D, H, W order), queued on the
    current stream (include/mmtta.h: mmtta_surface_dice).  Returns int64 [B,R,T,4] on the device (``SURFACE_DICE_COLUMNS``):
    NSD = (hits_pred + hits_gt) / (edge_pred + edge_gt)."""
    sp, tol = _nsd_arguments("surface_dice", spacing, tolerances)
    if (not torch.is_tensor(pred_mask) or pred_mask.dtype != torch.uint8 or pred_mask.dim() != 5 or not pred_mask.is_contiguous()
            or not pred_mask.is_cuda):
        raise MmttaError("surface_dice: mask must be a dense CUDA uint8 [B,R,D,H,W] tensor")
    if (not torch.is_tensor(label_ncdhw) or tuple(label_ncdhw.shape) != tuple(pred_mask.shape) or label_ncdhw.device != pred_mask.device
            or label_ncdhw.dtype != torch.float32):
        raise MmttaError(f"surface_dice: label must be float32 of the mask's shape {tuple(pred_mask.shape)} on the mask's device")
    B, R, D, H, W = (int(v) for v in pred_mask.shape)
    if min(B, R, D, H, W) < 1:
        raise MmttaError(f"surface_dice: empty mask {tuple(pred_mask.shape)}")
    lib = _lib.load()
    nbytes = int(lib.mmtta_surface_dice_scratch_bytes(B * R, D, H, W))
    if nbytes < 0:
        raise MmttaError(f"surface_dice: extent {(B * R, D, H, W)} unsupported (at most 1024 per axis, B*R <= 65535)")
    key = (pred_mask.device.index, nbytes, int(torch.cuda.current_stream().cuda_stream))     # per stream: lanes run concurrently
    scratch = _SD_SCRATCH.get(key)
    if scratch is None:
        for k in [k for k in _SD_SCRATCH if k[2] == key[2]]:       # a new shape on this stream replaces its old working set
            del _SD_SCRATCH[k]
        scratch = _SD_SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=pred_mask.device)
    T = len(tol)
    counts = torch.empty((B, R, T, 4), dtype=torch.int64, device=pred_mask.device)
    tl = desc_ncdhw(label_ncdhw)
    check(lib.mmtta_surface_dice(ptr(pred_mask), C.byref(tl), (C.c_double * 3)(*sp), (C.c_double * T)(*tol), T, ptr(counts),
                                 ptr(scratch), stream_ptr()), "surface_dice")
    return counts


_LW_NSD_SCRATCH: Dict[Tuple, torch.Tensor] = {}  # working set of lesionwise_nsd beside the one of lesionwise_scores, likewise
LESIONWISE_NSD_Q_ONE = 1 << 30                   # a lesion's NSD is summed in units of 2^-30


def lesionwise_nsd_list_slots() -> int:
    """Distinct lesions a thread of the P -> A direction of ``mmtta_lesionwise_nsd`` keeps in registers; an edge voxel with more
    of them in its window is handled by the launch for marked voxels."""
    return int(_lib.load().mmtta_lesionwise_nsd_list_slots())


def lesionwise_nsd_after_scores(mask: torch.Tensor, min_lesion_voxels, spacing: Sequence[float], tolerances: Sequence[float],
                                want_lesion_nsd: bool = False) -> Dict[str, Optional[torch.Tensor]]:
    """The lesion-wise NSD pass alone (include/mmtta.h: mmtta_lesionwise_nsd), on the current stream, behind a
    ``lesionwise_scores`` (or ``lesionwise_hd95``) call with the same mask and ``min_lesion_voxels`` on this stream, whose
    scratch it reads.  Returns ``nsd_stats`` int64 [B,R,T] (sum over the scored lesions of their NSD in units of 2^-30) and
    ``lesion_nsd`` float32 [B,R,T,D,H,W] (NaN, and a lesion's NSD at index lesion label - 1; with ``want_lesion_nsd``)."""
    sp, tol = _nsd_arguments("lesionwise_nsd", spacing, tolerances)
    if (not torch.is_tensor(mask) or mask.dtype != torch.uint8 or mask.dim() != 5 or not mask.is_contiguous() or not mask.is_cuda):
        raise MmttaError("lesionwise_nsd: mask must be a dense CUDA uint8 [B,R,D,H,W] tensor, got "
                         f"{getattr(mask, 'dtype', type(mask))} {tuple(getattr(mask, 'shape', ()))}")
    B, R, D, H, W = (int(v) for v in mask.shape)
    if min(B, R, D, H, W) < 1:
        raise MmttaError(f"lesionwise_nsd: empty mask {tuple(mask.shape)}")
    if R > COMPONENTS_MAX_REGIONS:
        raise MmttaError(f"lesionwise_nsd: {R} regions, at most {COMPONENTS_MAX_REGIONS}")
    vals = [min_lesion_voxels] * R if isinstance(min_lesion_voxels, (bool, int)) else list(min_lesion_voxels)
    if len(vals) != R:
        raise MmttaError(f"lesionwise_nsd: min_lesion_voxels has {len(vals)} entries for {R} regions")
    mv = [int(v) for v in vals]
    if any(v < 0 for v in mv):
        raise MmttaError(f"lesionwise_nsd: min_lesion_voxels must not be negative, got {mv}")
    lib = _lib.load()
    stream = int(torch.cuda.current_stream().cuda_stream)
    lw_scratch = _LW_SCRATCH.get((mask.device.index, int(lib.mmtta_lesionwise_scratch_bytes(B * R, D, H, W)), stream))
    if lw_scratch is None:
        raise MmttaError("lesionwise_nsd: no lesionwise_scores call of this shape on this stream to read from")
    nbytes = int(lib.mmtta_lesionwise_nsd_scratch_bytes(B * R, D, H, W))
    if nbytes < 0:
        raise MmttaError(f"lesionwise_nsd: extent {(B * R, D, H, W)} unsupported")
    key = (mask.device.index, nbytes, stream)
    scratch = _LW_NSD_SCRATCH.get(key)
    if scratch is None:
        for k in [k for k in _LW_NSD_SCRATCH if k[2] == key[2]]:
            del _LW_NSD_SCRATCH[k]
        scratch = _LW_NSD_SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=mask.device)
    T = len(tol)
    nsd_stats = torch.empty((B, R, T), dtype=torch.int64, device=mask.device)
    lesion_nsd = torch.empty((B, R, T, D, H, W), dtype=torch.float32, device=mask.device) if want_lesion_nsd else None
    check(lib.mmtta_lesionwise_nsd(ptr(mask), B, R, D, H, W, (C.c_double * 3)(*sp), (C.c_double * T)(*tol), T,
                                   (C.c_int64 * R)(*mv), ptr(lw_scratch), ptr(nsd_stats), ptr(lesion_nsd), ptr(scratch),
                                   stream_ptr()), "lesionwise_nsd")
    return {"nsd_stats": nsd_stats, "lesion_nsd": lesion_nsd}


def lesionwise_nsd(mask: torch.Tensor, label_ncdhw: torch.Tensor, iterations: int = 3, dilation_connectivity: int = 18,
                   min_lesion_voxels=0, spacing: Sequence[float] = (1.0, 1.0, 1.0), tolerances: Sequence[float] = (0.5, 1.0),
                   want_lesion_nsd: bool = False, want_labels: bool = False) -> Dict[str, Optional[torch.Tensor]]:
    """Lesion-wise scores AND lesion-wise NSD of every (volume, region) of ``mask`` against ``label_ncdhw``:
    ``lesionwise_scores`` followed, on the same scratch and the current stream, by ``lesionwise_nsd_after_scores``.  Returns
    the device tensors ``stats`` int64 [B,R,7] (identical to ``lesionwise_scores``' own), ``nsd_stats``, ``lesion_nsd`` and
    ``labels`` (with ``want_labels``)."""
    _nsd_arguments("lesionwise_nsd", spacing, tolerances)      # refused before anything is queued
    res = lesionwise_scores(mask, label_ncdhw, iterations, dilation_connectivity, min_lesion_voxels, want_labels=want_labels)
    nsd = lesionwise_nsd_after_scores(mask, min_lesion_voxels, spacing, tolerances, want_lesion_nsd)
    return {"stats": res["stats"], "nsd_stats": nsd["nsd_stats"], "lesion_nsd": nsd["lesion_nsd"], "labels": res["labels"]}
