"""Torch restatement of sliding-window adaptation (``window_tta``, ``mmtta_window_views`` / ``mmtta_window_entropy_items`` /
``mmtta_window_blend``) for the tests: the window grid, the importance weights and their normalised tables in float64, the
crop as ``F.pad`` and slicing, the loss with autograd, the blend, and the adaptation loop on the oracle networks.  Pure torch,
any dtype, CPU.  Written from the method's text (multimodal_tta_amd/window.py), not from its code."""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

DEFAULTS = dict(overlap=0.5, mode="gaussian", sigma_scale=0.125, floor=1e-3, pad_value=0.0)


def axis_starts(n, r, overlap):
    """The starts along one axis: one start at -((r - n) // 2) where the axis is padded, else steps of the scan interval with
    the last window flush with the end."""
    if n < r:
        return [-((r - n) // 2)]
    interval = r if n == r else max(int(r * (1 - overlap)), 1)
    count = math.ceil((n - r) / interval) + 1
    return [min(i * interval, n - r) for i in range(count)]


def axis_weight(r, mode, sigma_scale, floor):
    if mode == "constant":
        return torch.ones(r, dtype=torch.float64)
    i = torch.arange(r, dtype=torch.float64)
    w = torch.exp(-(i - (r - 1) / 2) ** 2 / (2 * (sigma_scale * r) ** 2))
    return torch.clamp(w, min=floor)


def axis_table(n, r, starts, w):
    """float64 [len(starts), r]: w[i] over the sum of the weights of every window that covers position start + i; 0 outside
    [0, n)."""
    total = torch.zeros(n, dtype=torch.float64)
    for s in starts:
        for i in range(r):
            if 0 <= s + i < n:
                total[s + i] += w[i]
    table = torch.zeros(len(starts), r, dtype=torch.float64)
    for k, s in enumerate(starts):
        for i in range(r):
            if 0 <= s + i < n:
                table[k, i] = w[i] / total[s + i]
    return table


def grid(extents, roi, **spec):
    """The windows of a volume: extents, roi, starts per axis, origins [W_n][3] (W fastest), float64 tables per axis and the
    window weights a float64 [W_n, rd, rh, rw]."""
    s = dict(DEFAULTS, **spec)
    starts = [axis_starts(n, r, s["overlap"]) for n, r in zip(extents, roi)]
    tables = [axis_table(n, r, st, axis_weight(r, s["mode"], s["sigma_scale"], s["floor"])) for n, r, st in zip(extents, roi, starts)]
    origins = [(a, b, c) for a in starts[0] for b in starts[1] for c in starts[2]]
    return SimpleNamespace(extents=tuple(extents), roi=tuple(roi), starts=starts, origins=origins, tables=tables,
                           windows=len(origins), weights=window_weights(tables), pad_value=s["pad_value"])


def window_weights(tables):
    """a [W_n, rd, rh, rw] = A_d[kd][i] A_h[kh][j] A_w[kw][k] in the tables' dtype, ((d h) w) in that order."""
    td, th, tw = tables
    a = (td[:, None, None, :, None, None] * th[None, :, None, None, :, None]) * tw[None, None, :, None, None, :]
    return a.reshape(-1, td.shape[1], th.shape[1], tw.shape[1])


def covering(g):
    """int64 [D, H, W]: how many windows see every voxel of the volume."""
    count = torch.zeros(g.extents, dtype=torch.int64)
    for o in g.origins:
        lo = [max(o[a], 0) for a in range(3)]
        hi = [min(o[a] + g.roi[a], g.extents[a]) for a in range(3)]
        count[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] += 1
    return count


def inside(g):
    """bool [W_n, rd, rh, rw]: the window's voxel lies in the volume."""
    out = torch.zeros((g.windows, *g.roi), dtype=torch.bool)
    for w, o in enumerate(g.origins):
        idx = [(torch.arange(g.roi[a]) + o[a] >= 0) & (torch.arange(g.roi[a]) + o[a] < g.extents[a]) for a in range(3)]
        out[w] = idx[0][:, None, None] & idx[1][None, :, None] & idx[2][None, None, :]
    return out


def crop(x, g, pad_value=None):
    """x [G, C, D, H, W] -> [G * W_n, C, rd, rh, rw], item g * W_n + w = the crop at origin w: F.pad by the roi on every side
    with ``pad_value``, then slicing."""
    pad_value = g.pad_value if pad_value is None else pad_value
    rd, rh, rw = g.roi
    xp = F.pad(x, (rw, rw, rh, rh, rd, rd), value=pad_value)
    items = [xp[:, :, o[0] + rd:o[0] + 2 * rd, o[1] + rh:o[1] + 2 * rh, o[2] + rw:o[2] + 2 * rw] for o in g.origins]
    return torch.stack(items, 1).reshape(-1, x.shape[1], rd, rh, rw)


def window_loss(z, a, voxels, softmax):
    """z [G * W_n, R, rd, rh, rw], a [W_n, rd, rh, rw] -> L [G] = 1/(N R) sum_w sum_voxels a_w H_bern(sigmoid z_w) (softmax: 1/N
    and the categorical entropy), N = ``voxels`` of the unpadded volume.  Differentiable."""
    W = a.shape[0]
    zs = z.reshape(z.shape[0] // W, W, *z.shape[1:])
    if softmax:
        l = F.log_softmax(zs, 2)
        h = -(l.exp() * l).sum(2)
        return (h * a.to(z.dtype)).flatten(1).sum(1) / voxels
    h = -(torch.sigmoid(zs) * F.logsigmoid(zs) + torch.sigmoid(-zs) * F.logsigmoid(-zs))
    return (h * a.to(z.dtype).unsqueeze(1)).flatten(1).sum(1) / (voxels * zs.shape[2])


def loss_reference(z, a, voxels, softmax):
    """float64 autograd: the per-volume loss [G] and dL/dz (z's shape)."""
    z = z.double().detach().requires_grad_(True)
    loss = window_loss(z, a.double(), voxels, softmax)
    loss.sum().backward()
    return loss.detach(), z.grad


def blend(z, g, a=None):
    """z [G * W_n, R, rd, rh, rw] -> [G, R, D, H, W]: out(v) = sum_w a_w(v) z_w(v - o_w) in ascending window order, in z's
    dtype (``a``: the window weights, default the grid's float64 ones)."""
    a = (g.weights if a is None else a).to(z.dtype)
    W = g.windows
    zs = z.reshape(z.shape[0] // W, W, *z.shape[1:])
    out = torch.zeros((zs.shape[0], z.shape[1], *g.extents), dtype=z.dtype)
    for w, o in enumerate(g.origins):
        lo = [max(o[k], 0) for k in range(3)]
        hi = [min(o[k] + g.roi[k], g.extents[k]) for k in range(3)]
        src = tuple(slice(lo[k] - o[k], hi[k] - o[k]) for k in range(3))
        dst = tuple(slice(lo[k], hi[k]) for k in range(3))
        out[(slice(None), slice(None)) + dst] += a[w][src] * zs[(slice(None), w, slice(None)) + src]
    return out


def window_reference(model, x, train_cfg, steps, roi, params="all", softmax=False, missing=(), **spec):
    """The adaptation loop with torch autograd, one volume x [1, C, D, H, W]: the windows (of the volume with the ``missing``
    channels zeroed) are one batch on the one weight set, train-mode norms; the returned logits are the eval forward of the
    windows, blended."""
    import oracle
    from oracle.tta import select_params
    named = select_params(model, params)
    chosen = {id(p) for _, p in named}
    for p in model.parameters():
        p.requires_grad_(id(p) in chosen)
    opt = oracle.adam.build_optimizer(named, train_cfg)
    g = grid(tuple(x.shape[2:]), roi, **spec)
    keep = torch.tensor([0.0 if c in set(missing) else 1.0 for c in range(x.shape[1])], dtype=x.dtype).view(1, -1, 1, 1, 1)
    xv = crop(x * keep, g)
    a = g.weights.to(x.dtype)
    voxels = x.shape[2] * x.shape[3] * x.shape[4]
    out = {"losses": [], "windows": g.windows}
    model.train()
    for _ in range(steps):
        opt.zero_grad()
        loss = window_loss(model(xv), a, voxels, softmax)
        loss[0].backward()
        opt.step()
        out["losses"].append(float(loss[0].detach()))
    model.eval()
    with torch.no_grad():
        out["logits"] = blend(model(xv), g, a)
    for p in model.parameters():
        p.requires_grad_(True)
    return out
