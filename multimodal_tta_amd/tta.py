"""``entmin_tta``: per-test-volume entropy-minimisation adaptation, registered in the reference's
free PLUGINS slot (reference src/registry.py:66,94-96; selected through the existing ``method``
config group, reference configs/config.yaml:7).

The reference ships no adaptation code; the semantics are this repo's (SURVEY.md
Appendix C, executable form: oracle/tta.py).  The step skeleton is the reference's supervised step
(src/core/trainers/seg_trainer.py:105-145): forward -> loss -> backward -> optimizer.step, with
the entropy objective as the loss, Adam built with the reference's decay / no-decay split
(src/core/experiment_manager.py:199-237, configs/training/default.yaml:30-56), then the
reference's evaluation tail (src/evaluation/seg_eval.py:300-308).

MI355X shape of the loop: the whole step (weight repack, forward, fused loss+gradient, backward,
fused Adam over the flat arena) is ONE captured hipGraph replayed ``steps`` times; nothing
returns to the host inside a volume except the final per-region counts (one small copy).
"""
from __future__ import annotations

import math
import warnings
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .config import as_cfg, get_config, method_block
from .engine import HeadLossTail
from .guard import parse_guard
from .models.base import DEFAULT_NO_DECAY_KEYS, HipSegModel
from .ops import MmttaError
from .registry import register_plugin


def select_params(model: torch.nn.Module, spec) -> List[str]:
    """Names of the parameters that adapt: 'all' | 'norm_affine' | substring or list of substrings."""
    names = [n for n, _ in model.named_parameters()]
    if spec is None or spec == "all":
        return names
    if spec == "norm_affine":
        return [n for n in names if ".adn.N." in n]
    pats = [spec] if isinstance(spec, str) else list(spec)
    return [n for n in names if any(s in n for s in pats)]


def modality_mask(num_modalities: int, missing: Sequence[int], p_drop: float,
                  gen: Optional[torch.Generator]) -> List[bool]:
    """present[m] for one step: permanently missing channels plus a seeded Bernoulli(p) drop of each
    present one; at least one modality always survives."""
    miss = set(int(i) for i in missing)
    present = [m not in miss for m in range(num_modalities)]
    if p_drop > 0.0 and gen is not None:
        u = torch.rand(num_modalities, generator=gen)
        dropped = [present[m] and bool(u[m] < p_drop) for m in range(num_modalities)]
        if all(dropped[m] or not present[m] for m in range(num_modalities)):
            first = next(m for m in range(num_modalities) if present[m])
            dropped[first] = False
        present = [present[m] and not dropped[m] for m in range(num_modalities)]
    return present


def drop_modality(x: torch.Tensor, present: Sequence[bool]) -> torch.Tensor:
    """Zero the absent channels (0 is the background value of the data: reference src/datasets/brats.py:7)."""
    if all(present):
        return x
    keep = torch.tensor([1.0 if p else 0.0 for p in present], dtype=x.dtype, device=x.device)
    return x * keep.view(1, -1, 1, 1, 1)


@register_plugin("entmin_tta")
class EntropyMinimizationTTA:
    """Construct with the ROOT config (like the reference's evaluation strategies,
    src/core/experiment_manager.py:369-370), then ``setup(model, device)`` once and
    ``adapt_volume(x)`` per test volume."""
    # the wide 27-tap layers update inside their weight-gradient launch (engine.Runtime.enable_fused_update); a subclass whose
    # step needs the whole gradient before any weight moves (SAR: the global gradient norm) switches it off
    fused_update = True
    # batch items a volume brings into the adaptation launches (memo_tta: its mirrored views); told to the model at every
    # setup, so a model that another plugin set up with views is built for this plugin's figure again
    views = 1

    def __init__(self, config: Any = None):
        cfg = as_cfg(config)
        self.cfg = cfg
        m = method_block(cfg)
        self.steps = int(get_config(m, "steps", 10))
        self.episodic = bool(get_config(m, "episodic", True))
        self.params_spec = get_config(m, "params", "all")
        self.precision = str(get_config(m, "precision", "fp32")).lower()
        self.storage = str(get_config(m, "storage", "bf16")).lower()      # activation storage of bf16 precision
        self.grad_storage = str(get_config(m, "grad_storage", "bf16")).lower()      # activation-gradient storage, likewise
        self.missing = [int(i) for i in (get_config(m, "missing_modalities", []) or [])]
        md = get_config(m, "moddrop", {}) or {}
        self.moddrop_p = float(get_config(md, "p", 0.0)) if bool(get_config(md, "enabled", False)) else 0.0
        self.moddrop_seed = int(get_config(md, "seed", 0))
        self.use_graph = bool(get_config(m, "use_graph", True))
        # volumes adapted side by side as the batch items of ONE launch sequence, each with its own replica of the weights
        # and optimizer state (mmtta_param_sets): a volume alone fills a quarter of the chip or less at the lower levels
        self.group = max(1, int(get_config(m, "group", 1)))
        self.lanes = max(1, int(get_config(m, "lanes", 1)))      # the evaluator's lanes: volumes in flight = lanes x group
        # norm layers with parameters (BatchNorm, GroupNorm, affine InstanceNorm) per volume of a group: own affines, own Adam
        # state, own running statistics (mmtta_norm_sets).  Off: such models fall back to group 1
        self.norm_sets = bool(get_config(m, "norm_sets", False))
        # launch geometry (split-K, weight-gradient slabs) is chosen for this many volumes in flight; `auto` = lanes x group.
        # Two runs agree BIT FOR BIT when they use the same figure (the geometry fixes the summation order), whatever their
        # lanes / group are - which is how the grouped arrangement is checked against one volume at a time
        tv = get_config(m, "tune_volumes", "auto")
        self.tune_volumes = None if tv in (None, "auto") else max(1, int(tv))
        self.side_streams = int(get_config(m, "side_streams", 0))   # 0: weight gradients stay on the main stream
        tr = get_config(cfg, "training", {}) or {}
        # the reference's factory (src/core/experiment_manager.py:199-237): `training.optimizer` names the class
        # (default "sgd" there, "adam" in the shipped configs/training/default.yaml:11), `training.optimizers.<name>` holds
        # its arguments, `training.{learning_rate,weight_decay,momentum}` are the fall-backs
        opt_name = str(get_config(tr, "optimizer", "sgd")).lower()
        if opt_name not in ops.OPTIMIZERS:
            raise ValueError(f"Unsupported optimizer: {opt_name}")
        oc = get_config(tr, f"optimizers.{opt_name}", {}) or {}
        if bool(get_config(oc, "amsgrad", False)):
            raise NotImplementedError("amsgrad")
        if bool(get_config(oc, "maximize", False)):
            raise NotImplementedError("maximize")
        betas = get_config(oc, "betas", [0.9, 0.999])
        self.optim = ops.OptimSpec(
            name=opt_name,
            lr=float(get_config(oc, "lr", get_config(tr, "learning_rate", 1e-3))),
            beta1=float(betas[0]), beta2=float(betas[1]),
            eps=float(get_config(oc, "eps", 1e-8)),
            # the reference's parameter groups always carry a weight decay (`optimizers.<name>.weight_decay`, else
            # `training.weight_decay`, else 0), so torch's own AdamW default of 1e-2 never applies
            weight_decay=float(get_config(oc, "weight_decay", get_config(tr, "weight_decay", 0.0))),
            momentum=float(get_config(oc, "momentum", get_config(tr, "momentum", 0.0))) if opt_name == "sgd" else 0.0,
            dampening=float(get_config(oc, "dampening", 0.0)) if opt_name == "sgd" else 0.0,
            nesterov=bool(get_config(oc, "nesterov", False)) if opt_name == "sgd" else False)
        if self.optim.nesterov and (self.optim.momentum <= 0.0 or self.optim.dampening != 0.0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")      # torch.optim.SGD's message
        rules = get_config(tr, "param_groups", {}) or {}
        self.no_decay_keys = list(get_config(rules, "no_decay_keys", []))
        self.treat_1d = bool(get_config(rules, "treat_1d_as_no_decay", True))
        crit = get_config(tr, "criterion", {}) or {}
        self.softmax = bool(get_config(crit, "softmax", False))
        if self.precision not in ops.PRECISIONS:
            raise ValueError(f"method.precision={self.precision}: expected one of {sorted(ops.PRECISIONS)}")
        # the do-no-harm guard (guard.py): off unless ``method.guard.enable``; then every volume is checked against what this
        # plugin returns for it at ``steps = 0``
        self.guard = parse_guard(cfg)
        self.model: Optional[HipSegModel] = None
        self.rt = None
        self._graphs: Dict[Tuple, torch.cuda.CUDAGraph] = {}
        self._gen: Optional[torch.Generator] = None
        self.lane = 0      # plugins that adapt different volumes concurrently (own stream each) take distinct lanes
        # the per-volume number of the methods that draw random numbers per volume (cotta_tta's restore, the intensity views
        # of memo_tta and cotta_tta): see ``_setup_ordinals`` / ``_take_ordinals``
        self._ordinals: Optional[torch.Tensor] = None        # device int32 [replicas]
        self._ordinals_host: List[int] = []                  # the same numbers for the host-side draws, one per volume
        self._served = 0

    # ------------------------------------------------------------------ setup
    def setup(self, model: HipSegModel, device) -> "EntropyMinimizationTTA":
        if not isinstance(model, HipSegModel):
            raise TypeError("entmin_tta drives the HIP-backed models of this package (registered as 'unet', "
                            "'unet_multimodal_deepfusion', 'unet_multimodal_midfusion')")
        device = torch.device(device)
        self.model = model
        ops.tune_for_volumes_in_flight(self.tune_volumes or self.lanes * self.group)      # launch geometry for that many volumes
        names = select_params(model, self.params_spec)
        model.set_precision(self.precision, self.storage, self.grad_storage)
        model.set_group(self.group)
        model.set_views(self.views)
        model.set_norm_sets(self.norm_sets)
        model.configure_training(set(names), self.no_decay_keys, self.treat_1d)
        model.to(device)
        try:
            self.rt = model.runtime(device)
        except NotImplementedError as exc:
            if self.group == 1:
                raise
            # norm layers with parameters (BatchNorm / affine norms) are per-model, not per-volume: such a model adapts one
            # volume per launch sequence; the lanes still keep several volumes in flight
            warnings.warn(f"method.group = {self.group} -> 1: {exc}")
            self.group = 1
            model.set_group(1)
            self.rt = model.runtime(device)
        if self.norm_sets and int(self.rt.group) < self.group:
            # (the deep-fusion network with such norms runs its modality encoders one after another, without volume groups)
            warnings.warn(f"method.group = {self.group} -> {int(self.rt.group)}: {type(self.rt).__name__} has no per-volume "
                          "parameter sets for this model (a family of modality encoders in one launch needs parameter-free "
                          "per-item norms, INSTANCE); method.norm_sets does not apply to it")
        self.group = int(self.rt.group)          # what the runtime supports (a runtime without per-volume sets reports 1)
        self.rt.overlap_wgrad = self.side_streams > 0
        self.rt.n_side = max(1, self.side_streams)
        self.rt.arena.snapshot_source()
        self.rt.snapshot_buffers()
        # the wide 27-tap layers step their optimizer and repack their images inside their weight-gradient launch
        self.rt.enable_fused_update(self.optim if self.fused_update else None)
        self._graphs.clear()
        if self.tune_volumes is None and self.views > 1:
            # `auto`: launch geometry for the items of the widest launches - lanes x group x views, with the group the runtime
            # settled on (models that fall back to group 1 are tuned for group 1)
            ops.tune_for_volumes_in_flight(self.lanes * self.group * self.views)
        return self

    # ------------------------------------------------------------------ per-volume ordinals
    def _setup_ordinals(self) -> None:
        """Called from the ``setup`` of a method that draws per volume: one device slot per replica, and the count of volumes
        served starts at ``lane * 2^24`` (the lanes of an evaluator draw apart)."""
        ar = self.rt.arena
        self._ordinals = torch.zeros(ar.replicas, dtype=torch.int32, device=ar.device)
        self._ordinals_host = []
        self._served = int(self.lane) << 24

    def _take_ordinals(self, B: int, ordinals: Optional[Sequence[int]]) -> List[int]:
        """The ordinals of the ``B`` volumes of one ``adapt_volume`` call, on the host and in ``self._ordinals[:B]``: the
        caller's, or by default the volumes served so far.  The ordinal, never the replica slot, enters a draw - which is
        what keeps a group of volumes equal to the same volumes served one at a time."""
        self._check_volumes(B)          # (one ordinal per replica)
        if ordinals is None:
            ordinals = [self._served + b for b in range(B)]
            self._served += B
        ordinals = [int(o) for o in ordinals]
        if len(ordinals) != B or any(not (0 <= o < 1 << 32) for o in ordinals):
            raise ValueError(f"ordinals = {ordinals!r}: expected {B} numbers (one per volume) with 0 <= ordinal < 2^32")
        self._ordinals[:B].copy_(torch.from_numpy(np.array(ordinals, dtype=np.uint32).view(np.int32)))
        self._ordinals_host = ordinals
        return ordinals

    # ------------------------------------------------------------------ one step
    def _step_launches(self, x: torch.Tensor, present: Optional[Sequence[bool]], *views: torch.Tensor) -> None:
        """The launches of one step (what the graph captures): the method's ``_update`` between the runtime's switches."""
        rt = self.rt
        ops.Workspace.lane = self.lane
        rt.training = True
        rt.use_sets = rt.group > 1          # the batch items of volume g read / write parameter replica g
        loop_views = rt.views
        try:
            self._update(x, present, *views)
        finally:
            rt.use_sets = False
            rt.views = loop_views

    def _forward(self, x: torch.Tensor, present: Optional[Sequence[bool]]) -> torch.Tensor:
        return self.rt.forward_cl(x) if present is None else self.rt.forward_cl(x, present=present)

    def _dlogits(self, logits: torch.Tensor) -> torch.Tensor:
        """The step's gradient buffer for ``logits`` (the categorical objectives write fp32 only)."""
        n, d, h, w, r = logits.shape
        gdt = self.rt.thin_grad_dtype() if (not self.softmax and r <= 4) else torch.float32
        return self.rt.pool.cl("dlogits", n, d, h, w, r, ldc=(r + 3) // 4 * 4, dtype=gdt)

    def _update(self, x: torch.Tensor, present: Optional[Sequence[bool]]) -> None:
        """The method's own launch sequence: pack, forward, objective, backward, optimizer.  It leaves every per-step record
        (``records``) in its pool buffer, one slot per replica.  A method with another objective keeps three parts: the
        buffers it owns, its loss call, and ``_backward_and_step``."""
        self.rt.pack_all(fused_current=True)
        logits, dlogits = self._entropy_objective(x, present)
        self._backward_and_step(dlogits, int(logits.shape[0]), fused=True)

    def _entropy_objective(self, x: torch.Tensor, present: Optional[Sequence[bool]]) -> Tuple[torch.Tensor, torch.Tensor]:
        """Tent's objective on ``x``: the forward and the mean entropy of its logits, per volume of a group -> (logits,
        dlogits), the loss in ``ent_loss``."""
        rt = self.rt
        loss = rt.pool.flat("ent_loss", rt.group)
        # the objective may ride in the epilogue of the network's last convolution, which then stores no logits (nothing
        # else reads a step's logits): every volume its own objective, as below - or the batch of one
        per_item = rt.group > 1
        tail = None
        if getattr(rt, "supports_head_tail", False) and not self.softmax and (per_item or int(x.shape[0]) == 1):
            tail = HeadLossTail(self._dlogits, loss, per_item)
        kw = {} if present is None else {"present": present}
        logits = rt.forward_cl(x, **kw) if tail is None else rt.forward_cl(x, tail=tail, **kw)
        if tail is not None and tail.done:
            dlogits = tail.dlogits
        elif rt.group > 1:
            dlogits = self._dlogits(logits)
            # every volume of the group is its own objective (own mean, own gradient scale): loss [group]
            partial = rt.pool.flat("ent_partial", ops.entropy_partials_items(logits), dtype=torch.float64)
            ops.entropy_loss_items(logits, dlogits, partial, loss, softmax=self.softmax)
        else:
            dlogits = self._dlogits(logits)
            partial = rt.pool.flat("ent_partial", ops.entropy_partials(logits), dtype=torch.float64)
            ops.entropy_loss(logits, dlogits, partial, loss, softmax=self.softmax)
        return logits, dlogits

    def _backward_and_step(self, dlogits: torch.Tensor, volumes: int, fused: bool = False, between=None, after=None,
                           always_backward: bool = False) -> None:
        """The tail of every step: the backward of ``dlogits`` and the optimizer over ``volumes`` replicas - nothing at all
        where no parameter trains, unless ``always_backward`` (a method that reads the input gradients: the backward runs,
        the optimizer does not).  ``fused``: the step packed with ``fused_current`` and lets the backward update
        ``rt.fused_layers`` in place.  ``between()`` runs after the backward (the gradients are in the arena, no weight has
        moved), ``after()`` after the optimizer."""
        rt = self.rt
        train = rt.arena.n_train > 0
        if not (train or always_backward):
            return
        fused = fused and train and bool(rt.fused_layers)
        rt.fused_active = fused         # only this backward updates the fused layers in place
        try:
            rt.run_backward(dlogits)
        finally:
            rt.fused_active = False
        if between is not None:
            between()
        if train:
            if fused:
                self.optimizer_step(volumes, fused=True)
            else:
                self.optimizer_step(volumes)
            if after is not None:
                after()

    def optimizer_step(self, volumes: int = 1, fused: bool = False) -> None:
        """The arena optimizer: ONE launch over [decay | no-decay] of every replica in use (+ the device step counter).
        ``fused``: the backward before it was the fused update of ``rt.fused_layers``; only the leftover segments remain."""
        ar = self.rt.arena
        if fused:
            # the fused layers were updated by their weight-gradient launches: the segments of everything else
            table, count, total = self.rt.leftover
            ops.optim_step_segments(self.optim, ar.params_all, ar.grads_all, ar.exp_avg_all, ar.exp_avg_sq_all, table, count,
                                    total, min(volumes, ar.replicas), ar.step)
            return
        if ar.replicas > 1:
            ops.optim_step_sets(self.optim, ar.params_all, ar.grads_all, ar.exp_avg_all, ar.exp_avg_sq_all, ar.n_train, ar.n_decay,
                                min(volumes, ar.replicas), ar.step)
            return
        ops.optim_step(self.optim, ar.params[:ar.n_train], ar.grads[:ar.n_train], ar.exp_avg[:ar.n_train],
                       ar.exp_avg_sq[:ar.n_train], ar.n_decay, ar.step)

    def _step(self, x_cl: torch.Tensor, present: Optional[Sequence[bool]], *views: torch.Tensor) -> None:
        if not self.use_graph:
            self._step_launches(x_cl, present, *views)
            return
        key = (tuple(x_cl.shape), x_cl.data_ptr(), None if present is None else tuple(present))
        g = self._graphs.get(key)
        if g is None:
            # eager warm-up (allocates every buffer, sizes the workspace), then capture.  Both run on the CALLER's stream
            # when that is not the default stream: a lane keeps its one stream (= its hardware queue, ops.lane_streams)
            # for everything, no helper streams are created per capture
            cur = torch.cuda.current_stream(x_cl.device)
            on_default = cur == torch.cuda.default_stream(x_cl.device)
            work = ops.helper_stream(x_cl.device) if on_default else cur
            if on_default:
                work.wait_stream(cur)
            with torch.cuda.stream(work):
                self._step_launches(x_cl, present, *views)
            if on_default:
                cur.wait_stream(work)
            torch.cuda.synchronize()
            try:
                ops.Workspace.frozen = True
                ops.Workspace.captured.add((x_cl.device.index if x_cl.device.index is not None else torch.cuda.current_device(),
                                            self.lane))
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=work):
                    self._step_launches(x_cl, present, *views)
            except Exception as exc:  # capture is an optimisation: the eager launches are the same kernels
                warnings.warn(f"hipGraph capture failed ({exc}); running the step eagerly")
                self.use_graph = False
                g = None
            finally:
                ops.Workspace.frozen = False
            self._graphs[key] = g
            return  # the warm-up already performed this step
        self.rt.refresh_frozen()          # frozen layers' images are not repacked inside the step (engine.Runtime.pack_all)
        g.replay()

    # ------------------------------------------------------------------ per volume
    # what is read after every step: (result key, pool buffer with one slot per replica, dtype).  The loop keeps the history
    # and returns it under the result key, [steps] - or [steps, B] for B > 1 volumes of a group
    records: Tuple[Tuple[str, str, torch.dtype], ...] = (("losses", "ent_loss", torch.float32),)

    def _records(self) -> Tuple[Tuple, ...]:
        """``records`` as one call reads them (after ``setup``: channels and views are known).  A method adds its wide
        entries here, (result key, pool buffer, dtype, row shape): the buffer holds one row of that shape per replica, and
        the history comes back as a copy, [steps, B, *row shape] for any B."""
        return self.records

    def _check_volumes(self, n: int, who: str = "", why: str = "", exc=ValueError) -> None:
        """A call takes at most ``method.group`` volumes; ``who`` ("bnm_tta adapts ") and ``why`` (" (the reason)") are the
        method's own clauses of the message."""
        group = int(self.rt.group) if self.rt is not None else self.group
        if n > group:
            raise exc(f"method.group = {group}: {who}at most {group} volumes per call{why}, got {n}")

    def _refuse_moddrop(self, clause: str) -> None:
        """For the constructor of a method that stages something once per volume: modality dropout redraws it every step."""
        if bool(get_config(method_block(self.cfg, "moddrop"), "enabled", False)):
            raise NotImplementedError(f"method.moddrop.enabled: {clause}")

    def _refuse_running_stats(self, who: str, forward: str, owner: str = "the plain forward") -> None:
        """For the ``setup`` of a method with an extra train-mode ``forward``: it would move the running statistics."""
        if self.rt.buffers:
            norm = get_config(get_config(self.cfg, "model", {}) or {}, "norm", "BATCH")
            raise NotImplementedError(f"{who}: model.norm = {norm!r} keeps running statistics, which {forward} would move "
                                      f"(running_mean, running_var, num_batches_tracked belong to {owner}); use a model.norm "
                                      "without them (INSTANCE, GROUP)")

    def _reset(self) -> None:
        """The episodic reset at the start of a volume: weights, optimizer state and running statistics of the source."""
        self.rt.arena.restore_source()
        self.rt.restore_buffers()

    def _stage(self, x_cl: torch.Tensor) -> Tuple[torch.Tensor, Tuple[torch.Tensor, ...]]:
        """What ``_update`` is given every step: its input and any further tensors, from the staged volumes ``x_cl``.  A
        method whose step input is views sets ``rt.views`` here; the loop keeps it until ``_final_logits`` and resets it."""
        return x_cl, ()

    def _final_logits(self, x_cl: torch.Tensor, x_step: torch.Tensor, present: Optional[Sequence[bool]]) -> torch.Tensor:
        """The returned logits: the eval-mode forward of the staged volumes (the images are packed)."""
        return self._forward(x_cl, present)

    @staticmethod
    def _whole_rows(t: torch.Tensor) -> torch.Tensor:
        """A channels-last view with its pad lanes, where the view owns them: the rows as one run of memory."""
        if getattr(t, "_mmtta_owns_pad", False) and int(t.stride(3)) > int(t.shape[4]):
            return torch.as_strided(t, (*t.shape[:4], int(t.stride(3))), t.stride(), t.storage_offset())
        return t

    def _guard_reference(self, x_cl: torch.Tensor, x_step: torch.Tensor, present: Optional[Sequence[bool]]) -> torch.Tensor:
        """What this plugin returns at ``steps = 0``, after the reset and ``_stage`` and before the first step, copied out of
        the runtime's buffer into a pool buffer of the same row width (the final forward writes the runtime's again).  It
        leaves no trace: an eval-mode forward moves no running statistics, the images it packs are those the first step
        packs, and the runtime's switches are put back as ``_stage`` left them."""
        rt = self.rt
        training, views = rt.training, rt.views
        try:
            rt.training = False
            ops.Workspace.lane = self.lane
            rt.use_sets = rt.group > 1
            rt.pack_all(fused_current=True)
            z = self._final_logits(x_cl, x_step, present)
            n, d, h, w, r = z.shape
            ref = rt.pool.cl("guard_reference", n, d, h, w, r, ldc=max(int(z.stride(3)), r), zero=True)
            if getattr(z, "_mmtta_owns_pad", False):
                self._whole_rows(ref).copy_(self._whole_rows(z))          # one run of 16-byte rows
            else:
                ref.copy_(z)
        finally:
            rt.use_sets = False
            rt.views = views
            rt.training = training
        return ref

    def _guard_apply(self, reference: torch.Tensor, logits_cl: torch.Tensor, out: Dict[str, Any]) -> None:
        """Queue the counts and the select on the current stream, outside the captured step; nothing is read on the host.
        ``out`` gets ``guard_counts`` int64 [B,R,3], ``guard_fallback`` int32 [B,R] and ``guard_reference_cl``."""
        n, r = int(logits_cl.shape[0]), int(logits_cl.shape[-1])
        pool = self.rt.pool
        counts = pool.flat("guard_counts", n * r * 3, dtype=torch.int64, zero=True)
        fallback = pool.flat("guard_fallback", n * r, dtype=torch.int32, zero=True)
        ops.guard_counts(reference, logits_cl, self.guard.threshold, counts)
        ops.guard_select(counts, self.guard.rule, reference, logits_cl, fallback)
        out["guard_counts"] = counts.view(n, r, 3).clone()
        out["guard_fallback"] = fallback.view(n, r).clone()
        out["guard_reference_cl"] = reference

    @torch.no_grad()
    def adapt_volume(self, x: torch.Tensor, steps: Optional[int] = None) -> Dict[str, Any]:
        """x: [1,C,D,H,W] fp32 on the plugin's device - or, with ``method.group`` = G > 1, up to G volumes [B,C,D,H,W]
        that adapt independently (volume b on parameter replica b).  Returns the final logits (channels-last view
        [B,D,H,W,R]) and the per-step ``records``: the losses ([steps], or [steps, B] for a group).  With
        ``method.guard.enable`` the logits of a volume (or region) that fails the guard's rule are the reference's, and the
        result also holds ``guard_counts``, ``guard_fallback`` and ``guard_reference_cl`` (``guard.py``)."""
        if self.rt is None:
            raise MmttaError("call setup(model, device) first")
        rt = self.rt
        steps = self.steps if steps is None else int(steps)
        B = int(x.shape[0])
        # (without a group the batch items share the one weight set: any number of them - unless they are a volume's views)
        if rt.group > 1 or self.views > 1:
            self._check_volumes(B)
        if self.episodic:
            self._reset()
        C = x.shape[1]
        masked = bool(self.missing) or self.moddrop_p > 0.0
        gen = torch.Generator().manual_seed(self.moddrop_seed) if self.moddrop_p > 0.0 else None
        base_present = modality_mask(C, self.missing, 0.0, None)
        x = x.float()
        wants_present = masked and getattr(rt, "supports_present", False)
        # a runtime that applies the mask while its first level stages the input (models/unet.py) reads the volume as it is;
        # the others get the masked volume re-staged whenever the mask changes (mask, then mirror: views are staged from it)
        restage = masked and not getattr(rt, "input_mask_on_load", False)
        x_cl = rt.stage_input(drop_modality(x, base_present) if restage else x)
        grouped = rt.group > 1
        rows, width = max(steps, 1), B if grouped else 1
        recs = []          # (key, wide, the buffer [slots, *row], its history [rows, slots, *row])
        for key, buf, dt, *row in self._records():
            row, slots = tuple(row[0]) if row else (), rt.group if row else width
            numel = math.prod(row)
            recs.append((key, bool(row), rt.pool.flat(buf, rt.group * numel, dtype=dt, zero=True).view(rt.group, *row)[:slots],
                         rt.pool.flat(buf + "_hist", rows * slots * numel, dtype=dt).view(rows, slots, *row)))
        try:
            x_step, views = self._stage(x_cl)
            reference = None
            if self.guard.enable:
                reference = self._guard_reference(x_cl, x_step, base_present if wants_present else None)
            for t in range(steps):
                present = None
                if masked:
                    p = modality_mask(C, self.missing, self.moddrop_p, gen)
                    if self.moddrop_p > 0.0 and restage:
                        rt.stage_input(drop_modality(x, p))
                    present = p if wants_present else None
                self._step(x_step, present, *views)
                for _, _, buf, hist in recs:          # (outside the captured step)
                    hist[t].copy_(buf)
            if masked and self.moddrop_p > 0.0 and restage:
                rt.stage_input(drop_modality(x, base_present))
            rt.training = False
            ops.Workspace.lane = self.lane
            rt.use_sets = grouped
            rt.pack_all(fused_current=True)
            logits_cl = self._final_logits(x_cl, x_step, base_present if wants_present else None)
        finally:
            rt.use_sets = False
            rt.views = 1
        out = {"logits_cl": logits_cl}
        if reference is not None:
            self._guard_apply(reference, logits_cl, out)
        for key, wide, _, hist in recs:
            out[key] = hist[:steps, :B].clone() if wide else hist[:steps, 0] if width == 1 else hist[:steps]
        return out

    def logits(self, result: Dict[str, Any]) -> torch.Tensor:
        return ops.from_cl(result["logits_cl"])
