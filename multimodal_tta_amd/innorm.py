"""``innorm_tta``: entropy minimisation that adapts the network's INPUT (Karani et al., MedIA 2021, "Test-time adaptable neural
networks for robust medical image segmentation": the segmentation network is frozen and a shallow image normaliser adapts
per test volume).  The dominant shift between centres is an intensity shift per modality - scanner gain, SUV scaling, a
z-score over another mask -, the family the reference normalises by (a per-channel clip and a masked z-score) and augments
with (``RandScaleIntensity``, ``RandShiftIntensity``); MEMO and CoTTA draw it as random views, this plugin learns it.

Every volume of a group carries theta = (s_c, b_c, g_c) per modality, 0 at the start and reset with the weights:

    u  = x                                                     (innorm.gamma: false)
    u  = ((x - lo) / (hi - lo))^exp(g_c) (hi - lo) + lo        (innorm.gamma: true; lo, hi: the channel's range over the volume)
    x' = exp(s_c) u + b_c

One step: x' is written from the raw volume (``ops.input_norm_apply``); the parent's sequence - forward, entropy, backward,
the optimizer on whatever ``method.params`` selects - runs on x'; theta takes one Adam step on dL/dtheta and is clamped to
its box (``ops.input_norm_grad``: the first level's input gradient reduced to 3 numbers per modality, never stored as a
volume; between the backward and the optimizer, so both gradients are taken at the step's weights and the step's theta).
The returned logits are the eval forward of x' at the final theta.  With ``method.params: []`` the network is the source
model bit for bit and only theta adapts - Karani's setting.

Where this differs from the paper: the normaliser is 2 - 3 numbers per modality, not a small convolutional network; the
objective is Tent's entropy, not a denoising-autoencoder prior; the only prior on theta is the box.  It sits on top of Tent
alone (not on SAR / MEMO / CoTTA / EATA / DeYO / CRF / BNM), on the ``unet`` model (not the deep-fusion network, whose
family batch and re-staging path would be a second integration), and not together with modality dropout.

``lr: 0`` takes the parent's step untouched - nothing new is launched - and is ``entmin_tta`` bit for bit.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Sequence, Tuple

import torch

from . import ops
from .config import expect, get_config, is_number, method_block
from .models.unet import UNetRuntime
from .ops import MmttaError
from .registry import register_plugin
from .tta import EntropyMinimizationTTA

MAX_LOG_SCALE, MAX_SHIFT, MAX_LOG_GAMMA = 4.0, 16.0, 2.0
MAX_COUT, MAX_CIN = 64, 4


class InputMapTTA(EntropyMinimizationTTA):
    """What the plugins that adapt an input map share (``innorm_tta`` here, ``biasfield_tta`` in biasfield.py): a raw fp32 copy
    of the staged volumes, one step - the map, the parent's forward, loss and backward, the step on the map's theta from the
    first level's reduced input gradient, the optimizer - and the final logits through the map at the final theta.  A
    subclass sets ``plugin`` (its name in messages), ``prefix`` (of its pool buffers), ``row`` (floats of a theta / grad row),
    ``record`` (the result key of the per-step dL/dtheta) and ``lr``, and provides ``_apply`` and ``_input_step``."""
    plugin, prefix, row, record = "", "", 4, ""

    def __init__(self, config: Any = None):
        super().__init__(config)
        self._refuse_moddrop(f"{self.plugin} learns one theta per volume on a fixed set of modalities; modality dropout redraws "
                             "them every step")
        self.lr = 0.0
        self._raw: Optional[torch.Tensor] = None           # the raw fp32 staged volumes of the call
        self._x_in: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ setup
    def setup(self, model, device) -> "InputMapTTA":
        if self.lr > 0.0 and getattr(model, "runtime_cls", None) is not UNetRuntime:
            raise NotImplementedError(f"{self.plugin} drives the 'unet' model; {type(model).__name__} (the deep-fusion family: "
                                      "modality encoders in one launch, re-staged inputs) has no reduced input gradient")
        super().setup(model, device)
        if self.lr == 0.0:
            return self
        rt = self.rt
        layers = rt.input_layers()
        for layer in layers:
            op = layer.op
            if (op.transposed or op.k != 3 or op.stride != 2 or op.cout % 4 or op.cout > MAX_COUT or op.cin > MAX_CIN
                    or len(layer.members) != 1):
                what = f"{'convT' if op.transposed else 'conv'} {op.cin}->{op.cout} k{op.k}s{op.stride}"
                raise NotImplementedError(f"{self.plugin}: the model's first level reads its input through a {what}; the "
                                          f"reduced input gradient gathers k = 3, stride 2 convolutions of <= {MAX_CIN} "
                                          f"channels into a multiple of 4 up to {MAX_COUT}")
        # the gradient reads the arena's weights of the step: no first-level layer may update inside the backward
        if any(layer in rt.fused_layers for layer in layers):
            raise MmttaError(f"{self.plugin}: a first-level convolution is in the fused weight update; its weights would move "
                             "before the input gradient reads them")
        self._input_layers = layers
        return self

    # ------------------------------------------------------------------ theta
    def _tables(self) -> Dict[str, torch.Tensor]:
        rt, c, p, w = self.rt, self.rt.in_channels, self.prefix, self.row
        g = rt.group
        return {"theta": rt.pool.flat(f"{p}_theta", g * c * w, zero=True), "grad": rt.pool.flat(f"{p}_grad", g * c * w, zero=True),
                "exp_avg": rt.pool.flat(f"{p}_exp_avg", g * c * w, zero=True),
                "exp_avg_sq": rt.pool.flat(f"{p}_exp_avg_sq", g * c * w, zero=True),
                "step": rt.pool.flat(f"{p}_step", g, dtype=torch.int32, zero=True),
                "range": rt.pool.flat(f"{p}_range", g * c * 2, zero=True)}

    def _reset(self) -> None:
        super()._reset()
        if self.lr > 0.0:
            t = self._tables()
            t["theta"].zero_()
            t["step"].zero_()        # (step 0 starts from zero moments whatever the buffers hold)

    def _apply(self, raw: torch.Tensor, x: torch.Tensor, present: Optional[Sequence[bool]]) -> None:
        """x = the map of the raw volumes at the current theta."""
        raise NotImplementedError

    def _input_step(self, raw: torch.Tensor, present: Optional[Sequence[bool]]) -> None:
        """dL/dtheta from what the backward left, Adam's step on theta and the clamp."""
        raise NotImplementedError

    def _input_branches(self):
        """The convolutions that read the input, as ``ops.input_norm_grad`` takes them."""
        rt, ar = self.rt, self.rt.arena
        branches = []
        for dy, layer, k, stride in rt.input_branches():
            w = layer.weight
            shared = layer.frozen or not rt.use_sets or ar.replicas == 1      # (a frozen layer's replicas all hold the source)
            branches.append((dy, ar.replica_data(w, 0), 0 if shared else ar.total, k, stride))
        return branches

    def _stage(self, x_cl: torch.Tensor) -> Tuple[torch.Tensor, Tuple[torch.Tensor, ...]]:
        if self.lr == 0.0:
            return super()._stage(x_cl)
        rt, p = self.rt, self.prefix
        n, d, h, w, c = x_cl.shape
        self._check_volumes(n, f"{self.plugin} adapts ")          # (every volume has its own theta)
        # the raw volume stays in fp32: a value is rounded once, after the map
        raw = rt.pool.cl("x_raw", n, d, h, w, c, ldc=(c + 3) // 4 * 4, zero=True, dtype=torch.float32)
        ops.to_cl(self._x_in, out=raw)
        t = self._tables()
        partial = rt.pool.flat(f"{p}_range_partial", ops.intensity_range_partials(raw))
        ops.intensity_range(raw, partial, t["range"])
        self._raw = raw
        return x_cl, (raw,)

    # ------------------------------------------------------------------ one step
    def _update(self, x: torch.Tensor, present: Optional[Sequence[bool]], *views: torch.Tensor) -> None:
        """The parent's sequence on x' - the map first, the reduced input gradient between the backward and the optimizer -
        and the backward runs whether or not a weight trains."""
        if self.lr == 0.0:
            super()._update(x, present)
            return
        raw, = views
        self._apply(raw, x, present)
        self.rt.pack_all(fused_current=True)
        logits, dlogits = self._entropy_objective(x, present)

        def input_step():
            try:
                self._input_step(raw, present)
            except MmttaError as exc:
                if "status -2" in str(exc):        # MMTTA_ERR_UNSUPPORTED: a first level the kernel does not gather
                    raise NotImplementedError(f"{self.plugin}: the model's first level is not supported: {exc}") from exc
                raise
        self._backward_and_step(dlogits, int(logits.shape[0]), fused=True, between=input_step, always_backward=True)

    def _records(self):
        """The parent's, and dL/dtheta of every step: one [C, row] row per replica (the map's ``grad`` table)."""
        if self.lr == 0.0:
            return self.records
        return self.records + ((self.record, f"{self.prefix}_grad", torch.float32, (self.rt.in_channels, self.row)),)

    def _final_logits(self, x_cl: torch.Tensor, x_step: torch.Tensor, present: Optional[Sequence[bool]]) -> torch.Tensor:
        """The eval-mode forward of x' at the final theta: the map runs once more, after the last step."""
        if self.lr > 0.0:
            self._apply(self._raw, x_cl, present)
        return self._forward(x_cl, present)

    @torch.no_grad()
    def adapt_volume(self, x: torch.Tensor, steps: Optional[int] = None) -> Dict[str, Any]:
        """``EntropyMinimizationTTA.adapt_volume`` with the fp32 volumes at hand for ``_stage``; at ``lr: 0`` the ``record``
        is zeros [steps, B, C, row]."""
        self._x_in = x.float()
        try:
            out = super().adapt_volume(x, steps)
        finally:
            self._x_in = None
        if self.lr == 0.0:
            out[self.record] = torch.zeros((len(out["losses"]), int(x.shape[0]), int(x.shape[1]), self.row), dtype=torch.float32,
                                           device=x.device)
        return out


@register_plugin("innorm_tta")
class InputNormTTA(InputMapTTA):
    """``method.innorm.lr`` (finite, >= 0, default 1e-2; 0: ``entmin_tta``), ``gamma`` (bool, default false: the power form of
    u), ``bound.log_scale`` ((0, 4], default 0.7), ``bound.shift`` ((0, 16], default 1.0) and ``bound.log_gamma`` ((0, 2],
    default 0.7): theta is clamped to +- its bound after every step.  theta's optimizer is Adam with torch's default betas
    and eps and no decay, whatever ``training.optimizer`` is.  Everything else is ``entmin_tta``'s, with one limit: every
    volume has its own theta, so a call takes at most ``method.group`` volumes."""
    plugin, prefix, row, record = "innorm_tta", "innorm", 4, "input_grad"

    def __init__(self, config: Any = None):
        super().__init__(config)
        s = method_block(config, "innorm")
        lr, gm = get_config(s, "lr", 1e-2), get_config(s, "gamma", False)
        bd = get_config(s, "bound", {}) or {}
        bs, bb, bg = get_config(bd, "log_scale", 0.7), get_config(bd, "shift", 1.0), get_config(bd, "log_gamma", 0.7)
        expect(is_number(lr) and lr >= 0.0, "method.innorm.lr", lr, "a finite number >= 0 (0: entmin_tta)")
        expect(isinstance(gm, bool), "method.innorm.gamma", gm, "a bool")
        for key, val, top in (("log_scale", bs, MAX_LOG_SCALE), ("shift", bb, MAX_SHIFT), ("log_gamma", bg, MAX_LOG_GAMMA)):
            expect(is_number(val) and 0.0 < val <= top, f"method.innorm.bound.{key}", val, f"a finite number in (0, {top:g}]")
        self.lr, self.gamma, self.bounds = float(lr), bool(gm), (float(bs), float(bb), float(bg))

    def _apply(self, raw: torch.Tensor, x: torch.Tensor, present: Optional[Sequence[bool]]) -> None:
        t = self._tables()
        ops.input_norm_apply(raw, x, t["theta"], t["range"], present=present, gamma=self.gamma)

    def _input_step(self, raw: torch.Tensor, present: Optional[Sequence[bool]]) -> None:
        """dL/dtheta from what the backward left, Adam's step on theta and the clamp: two launches."""
        t = self._tables()
        partial = self.rt.pool.flat("innorm_partial", ops.input_norm_grad_partials(raw), dtype=torch.float64)
        ops.input_norm_grad(raw, self._input_branches(), t["theta"], t["range"], partial, t["grad"], present=present, gamma=self.gamma,
                            exp_avg=t["exp_avg"], exp_avg_sq=t["exp_avg_sq"], step=t["step"], lr=self.lr, bounds=self.bounds)

    # ------------------------------------------------------------------ per volume
    @torch.no_grad()
    def adapt_volume(self, x: torch.Tensor, steps: Optional[int] = None) -> Dict[str, Any]:
        """``EntropyMinimizationTTA.adapt_volume`` plus ``input_grad`` [steps, B, C, 3] (dL/d(s, b, g) of every step; the g
        column is 0 with gamma off) and ``input_scale``, ``input_shift``, ``input_gamma`` [B, C]: exp(s), b, exp(g) at the end."""
        B, C = int(x.shape[0]), int(x.shape[1])
        out = super().adapt_volume(x, steps)
        out["input_grad"] = out["input_grad"][..., :3]
        if self.lr == 0.0:
            out["input_scale"] = torch.ones((B, C), dtype=torch.float32, device=x.device)
            out["input_shift"] = torch.zeros((B, C), dtype=torch.float32, device=x.device)
            out["input_gamma"] = torch.ones((B, C), dtype=torch.float32, device=x.device)
            return out
        theta = self._tables()["theta"].view(-1, C, 4)[:B]
        out["input_scale"] = torch.exp(theta[..., 0])
        out["input_shift"] = theta[..., 1].clone()
        out["input_gamma"] = torch.exp(theta[..., 2])
        return out
