"""Torch restatement of the input normaliser (``mmtta_input_norm_apply`` / ``mmtta_input_norm_grad``, plugin ``innorm_tta``) in
the dtype of its arguments - float64 for the references, float32 for the error yardsticks - and the oracle's adaptation
loop with the map in front of the model and a second Adam on theta.  No GPU code.

    u  = x                                                   gamma off
    u  = ((x - lo) / (hi - lo))^exp(g) (hi - lo) + lo        gamma on (hi > lo; t = 0 gives 0 with a zero derivative)
    x' = exp(s) u + b
"""
import copy

import torch

KEYS = ("losses",)


def channel_range(x):
    """(lo, hi) [B, C] of the raw volume x [B, C, D, H, W]."""
    flat = x.reshape(x.shape[0], x.shape[1], -1)
    return flat.min(-1).values, flat.max(-1).values


def _cols(theta, lo, hi):
    v = lambda a: a.reshape(a.shape[0], a.shape[1], 1, 1, 1)
    return v(theta[..., 0]), v(theta[..., 1]), v(theta[..., 2]), v(lo), v(hi - lo)


def normalised(x, lo, w):
    """t = (x - lo) / (hi - lo) where hi > lo, else 1 (a value whose logarithm is 0: the channel is left alone)."""
    safe = torch.where(w > 0, w, torch.ones_like(w))
    return torch.where(w > 0, (x - lo) / safe, torch.ones_like(x))


def apply_map(x, theta, lo, hi, gamma):
    """x' of x [B, C, D, H, W] under theta [B, C, 3] = (s, b, g); differentiable in theta."""
    s, b, g, l, w = _cols(theta, lo, hi)
    u = x
    if gamma:
        t = normalised(x, l, w)
        # t^gamma with the convention 0^gamma = 0 and a zero derivative there (torch.pow's gradient at 0 is nan for the exponent)
        tp = torch.where(t > 0, torch.exp(torch.exp(g) * torch.log(torch.where(t > 0, t, torch.ones_like(t)))), torch.zeros_like(t))
        u = torch.where(w > 0, tp * w + l, x)
    return torch.exp(s) * u + b


def derivatives(x, theta, lo, hi, gamma):
    """The analytic dx'/d(s, b, g), each [B, C, D, H, W]: exp(s) u, 1, exp(s) (hi - lo) t^gamma ln t gamma."""
    s, b, g, l, w = _cols(theta, lo, hi)
    zero = torch.zeros_like(x)
    if not gamma:
        return torch.exp(s) * x, torch.ones_like(x), zero
    t = normalised(x, l, w)
    pos = t > 0
    lt = torch.log(torch.where(pos, t, torch.ones_like(t)))
    gam = torch.exp(g)
    tp = torch.where(pos, torch.exp(gam * lt), zero)
    u = torch.where(w > 0, tp * w + l, x)
    return torch.exp(s) * u, torch.ones_like(x), torch.where(w > 0, torch.exp(s) * w * tp * lt * gam, zero)


def reduced_gradient(x, theta, lo, hi, gamma, weights, dys, keep):
    """autograd of sum_r sum conv3d(x' keep, W_r, stride 2, pad 1) dy_r with respect to theta -> [B, C, 3]; ``weights[r]``
    [B, c0, C, 3, 3, 3] (one set per item), ``dys[r]`` [B, c0, Do, Ho, Wo], ``keep`` [C] of 0 / 1."""
    th = theta.clone().requires_grad_(True)
    xp = apply_map(x, th, lo, hi, gamma) * keep.reshape(1, -1, 1, 1, 1)
    total = x.new_zeros(())
    for W, dy in zip(weights, dys):
        for n in range(x.shape[0]):
            total = total + (torch.nn.functional.conv3d(xp[n:n + 1], W[n], stride=2, padding=1) * dy[n:n + 1]).sum()
    total.backward()
    return th.grad.detach()


def gradient_scale(x, theta, lo, hi, gamma, weights, dys, keep):
    """A [B, C, 3]: the reduced gradient's sum over absolute values of W, dy and the derivative (the error bound's scale)."""
    d = derivatives(x, theta, lo, hi, gamma)
    out = x.new_zeros(x.shape[0], x.shape[1], 3)
    dxa = torch.zeros_like(x)
    for W, dy in zip(weights, dys):
        for n in range(x.shape[0]):
            dxa[n:n + 1] += torch.nn.functional.conv_transpose3d(dy[n:n + 1].abs(), W[n].abs(), stride=2, padding=1,
                                                                 output_padding=[(e + 1) % 2 for e in x.shape[2:]])
    dxa = dxa * keep.reshape(1, -1, 1, 1, 1)
    for k in range(3):
        out[..., k] = (dxa * d[k].abs()).flatten(2).sum(-1)
    return out


def adapt_reference(model, x, cfg, steps, softmax=False, missing=(), params="all", on_step=None):
    """``oracle.adapt_volume``'s loop (the oracle's model, ``select_params`` and optimizer factory unchanged; episodic) on
    x' = map(x; theta), with a second Adam (torch's default betas and eps, no decay) on theta and the clamp to its box, both
    gradients taken at the step's weights and the step's theta -> final logits (the eval forward of x' at the final theta)
    and the per-step records: ``losses``, ``input_grad`` [steps, 1, C, 3], ``theta`` [steps, 1, C, 3] after every step."""
    import oracle
    c = cfg["method"]["innorm"]
    gamma, bound = bool(c.get("gamma", False)), c.get("bound", {})
    box = torch.tensor([bound.get("log_scale", 0.7), bound.get("shift", 1.0), bound.get("log_gamma", 0.7)], dtype=x.dtype)
    source = copy.deepcopy(model.state_dict())
    named = oracle.select_params(model, params)
    chosen = {id(p) for _, p in named}
    frozen = [p for p in model.parameters() if id(p) not in chosen and p.requires_grad]
    for p in frozen:
        p.requires_grad_(False)
    opt = oracle.build_optimizer(named, cfg["training"]) if named else None
    present = oracle.tta.modality_mask(x.shape[1], missing, 0.0, None)
    lo, hi = channel_range(x)
    theta = torch.zeros(x.shape[0], x.shape[1], 3, dtype=x.dtype, requires_grad=True)
    opt_theta = torch.optim.Adam([theta], lr=float(c.get("lr", 1e-2)))
    rec = {"losses": [], "input_grad": [], "theta": []}
    model.train()
    for _ in range(int(steps)):
        if opt is not None:
            opt.zero_grad()
        opt_theta.zero_grad()
        xin = oracle.tta.apply_modality_mask(apply_map(x, theta, lo, hi, gamma), present)
        loss = oracle.entropy_loss(model(xin), softmax=softmax)
        loss.backward()
        if not gamma:
            theta.grad[..., 2] = 0
        for ch, p in enumerate(present):          # an absent channel has no gradient and keeps theta = 0
            if not p:
                theta.grad[:, ch] = 0
        if opt is not None:
            opt.step()
        opt_theta.step()
        with torch.no_grad():
            theta.copy_(torch.minimum(torch.maximum(theta, -box), box))
        rec["losses"].append(float(loss.item()))
        rec["input_grad"].append(theta.grad.detach().clone())
        rec["theta"].append(theta.detach().clone())
    model.eval()
    with torch.no_grad():
        logits = model(oracle.tta.apply_modality_mask(apply_map(x, theta, lo, hi, gamma), present))
    for p in frozen:
        p.requires_grad_(True)
    model.load_state_dict(source)
    if rec["theta"]:
        rec["input_grad"], rec["theta"] = torch.stack(rec["input_grad"]), torch.stack(rec["theta"])
    return logits, rec
