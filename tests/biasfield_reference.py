"""Torch restatement of the bias field (``mmtta_bias_field_apply`` / ``mmtta_bias_field_grad``, plugin ``biasfield_tta``) in the
dtype of its arguments - float64 for the references, float32 for the error yardsticks - and the oracle's adaptation loop with
the map in front of the model and a second Adam on theta.  No GPU code.

    F_c(z, y, x) = sum_k theta_ck phi_k(z, y, x)        phi_(a,b,c) = P_a(t_z) P_b(t_y) P_c(t_x), t_i = (2 i + 1) / n - 1
    x'_c         = (x_c - a_c) exp(F_c) + a_c           a_c = the channel's minimum (anchor "min") or 0 ("zero")

The terms with a + b + c <= order, by (a + b + c, a, b, c) ascending; P_0 .. P_3 the Legendre polynomials.
"""
import copy

import torch


def terms(order):
    out = [(a, b, c) for a in range(order + 1) for b in range(order + 1) for c in range(order + 1) if a + b + c <= order]
    return sorted(out, key=lambda t: (t[0] + t[1] + t[2], t[0], t[1], t[2]))


def legendre_tables(extents, dtype=torch.float64):
    """[T_d, T_h, T_w], T[a][i] = P_a(t_i) in float64 ([4, n] each), cast to ``dtype`` at the end (torch.float32: the one
    rounding of the tables the kernels read)."""
    out = []
    for n in extents:
        t = (2.0 * torch.arange(n, dtype=torch.float64) + 1.0) / n - 1.0
        out.append(torch.stack([torch.ones_like(t), t, (3 * t * t - 1) / 2, (5 * t * t * t - 3 * t) / 2]).to(dtype))
    return out


def basis(tables, order, dtype):
    """phi [K, D, H, W] from the tables' values, in ``dtype``."""
    td, th, tw = (t.to(dtype) for t in tables)
    return torch.stack([td[a][:, None, None] * th[b][None, :, None] * tw[c][None, None, :] for a, b, c in terms(order)])


def anchors(x, anchor):
    """a [B, C] of the raw volume x [B, C, D, H, W]."""
    lo = x.reshape(x.shape[0], x.shape[1], -1).min(-1).values
    return lo if anchor == "min" else torch.zeros_like(lo)


def log_field(theta, tables, order):
    """F [B, C, D, H, W] of theta [B, C, K]; differentiable in theta."""
    return torch.einsum("bck,kdhw->bcdhw", theta, basis(tables, order, theta.dtype))


def apply_field(x, theta, tables, order, anchor):
    """x' of x [B, C, D, H, W] under theta [B, C, K]; differentiable in theta."""
    a = anchors(x, anchor).reshape(x.shape[0], x.shape[1], 1, 1, 1)
    return (x - a) * torch.exp(log_field(theta, tables, order)) + a


def _conv_sum(xp, weights, dys):
    total = xp.new_zeros(())
    for W, dy in zip(weights, dys):
        for n in range(xp.shape[0]):
            total = total + (torch.nn.functional.conv3d(xp[n:n + 1], W[n], stride=2, padding=1) * dy[n:n + 1]).sum()
    return total


def reduced_gradient(x, theta, tables, order, anchor, weights, dys, keep):
    """autograd of sum_r sum conv3d(x' keep, W_r, stride 2, pad 1) dy_r with respect to theta -> [B, C, K]; ``weights[r]``
    [B, c0, C, 3, 3, 3] (one set per item), ``dys[r]`` [B, c0, Do, Ho, Wo], ``keep`` [C] of 0 / 1."""
    th = theta.clone().requires_grad_(True)
    xp = apply_field(x, th, tables, order, anchor) * keep.reshape(1, -1, 1, 1, 1)
    _conv_sum(xp, weights, dys).backward()
    return th.grad.detach()


def gradient_scale(x, theta, tables, order, anchor, weights, dys, keep):
    """A [B, C, K]: the reduced gradient's sum over absolute values of W, dy and the derivative (the error bound's scale)."""
    a = anchors(x, anchor).reshape(x.shape[0], x.shape[1], 1, 1, 1)
    de = ((x - a) * torch.exp(log_field(theta, tables, order))).abs()
    dxa = torch.zeros_like(x)
    for W, dy in zip(weights, dys):
        for n in range(x.shape[0]):
            dxa[n:n + 1] += torch.nn.functional.conv_transpose3d(dy[n:n + 1].abs(), W[n].abs(), stride=2, padding=1,
                                                                 output_padding=[(e + 1) % 2 for e in x.shape[2:]])
    dxa = dxa * keep.reshape(1, -1, 1, 1, 1)
    phi = basis(tables, order, x.dtype).abs()
    return torch.einsum("bcdhw,kdhw->bck", dxa * de, phi)


def adapt_reference(model, x, cfg, steps, softmax=False, missing=(), params="all"):
    """``oracle.adapt_volume``'s loop (the oracle's model, ``select_params`` and optimizer factory unchanged; episodic) on
    x' = field(x; theta), with a second Adam (torch's default betas and eps, no decay) on theta, the l2 term on the
    non-constant coefficients and the two-bound clamp, both gradients taken at the step's weights and the step's theta ->
    final logits (the eval forward of x' at the final theta) and the per-step records: ``losses``, ``field_grad``
    [steps, 1, C, K] (the l2 term included), ``theta`` [steps, 1, C, K] after every step.  The tables are the float32 values
    the kernels read, in the dtype of x."""
    import oracle
    c = cfg["method"]["biasfield"]
    order, anchor, l2 = int(c.get("order", 2)), c.get("anchor", "min"), float(c.get("l2", 0.0))
    bound = c.get("bound", {})
    K = len(terms(order))
    box = torch.full((K,), float(bound.get("field", 0.2)), dtype=x.dtype)
    box[0] = float(bound.get("gain", 0.7))
    tables = [t.to(x.dtype) for t in legendre_tables(x.shape[2:], torch.float32)]
    source = copy.deepcopy(model.state_dict())
    named = oracle.select_params(model, params)
    chosen = {id(p) for _, p in named}
    frozen = [p for p in model.parameters() if id(p) not in chosen and p.requires_grad]
    for p in frozen:
        p.requires_grad_(False)
    opt = oracle.build_optimizer(named, cfg["training"]) if named else None
    present = oracle.tta.modality_mask(x.shape[1], missing, 0.0, None)
    theta = torch.zeros(x.shape[0], x.shape[1], K, dtype=x.dtype, requires_grad=True)
    opt_theta = torch.optim.Adam([theta], lr=float(c.get("lr", 1e-2)))
    rec = {"losses": [], "field_grad": [], "theta": []}
    model.train()
    for _ in range(int(steps)):
        if opt is not None:
            opt.zero_grad()
        opt_theta.zero_grad()
        xin = oracle.tta.apply_modality_mask(apply_field(x, theta, tables, order, anchor), present)
        loss = oracle.entropy_loss(model(xin), softmax=softmax)
        loss.backward()
        with torch.no_grad():
            theta.grad[..., 1:] += 2.0 * l2 * theta[..., 1:]
        for ch, p in enumerate(present):          # an absent channel has no gradient and keeps theta = 0
            if not p:
                theta.grad[:, ch] = 0
        if opt is not None:
            opt.step()
        opt_theta.step()
        with torch.no_grad():
            theta.copy_(torch.minimum(torch.maximum(theta, -box), box))
        rec["losses"].append(float(loss.item()))
        rec["field_grad"].append(theta.grad.detach().clone())
        rec["theta"].append(theta.detach().clone())
    model.eval()
    with torch.no_grad():
        logits = model(oracle.tta.apply_modality_mask(apply_field(x, theta, tables, order, anchor), present))
    for p in frozen:
        p.requires_grad_(True)
    model.load_state_dict(source)
    if rec["theta"]:
        rec["field_grad"], rec["theta"] = torch.stack(rec["field_grad"]), torch.stack(rec["theta"])
    return logits, rec
