"""Float64 NumPy restatement of the CRF-regularised entropy objective (``mmtta_crf_entropy_items``, plugin ``crf_tta``), shared by
``test_crf_host.py`` (which holds its analytic gradient to torch autograd) and ``test_hip_crf.py`` (which holds the kernels
to it), and a torch version of the loss for autograd.  One batch item, channels last: ``l`` [D, H, W, R], ``x`` [D, H, W, C].

    p      = sigmoid(l) per region, or softmax(l) over the last axis
    a_d    = shift(1, d) * exp(-sum_{c present} (x - shift(x, d))^2 / (2 sigma^2))          (sigma = 0: shift(1, d))
    phi_d  = potts:      sum_r [p (1 - q) + (1 - p) q]  (softmax head: 1 - sum_k p q),   q = shift(p, d)
             quadratic:  sum_k (p - q)^2
    P      = 1 / (2 n E) sum_d sum_voxels a_d phi_d,     H = mean entropy over the E elements,     L = H + weight * P

over the n = 6 / 18 / 26 offsets d; E = D H W R on the sigmoid head, D H W on the softmax head; a neighbour outside the
volume contributes nothing.  The gradient is the gather of the specification: g = dP/dp from the neighbours' p, then the
chain through the sigmoid or the softmax."""
import numpy as np

from lame_reference import offsets, shift, softmax_lastaxis

FORMS = ("potts", "quadratic")


def affinities(shape3, x, conn, sigma, present=None, dtype=np.float64):
    """[a_d for d in offsets(conn)], each [D, H, W, 1]."""
    ones = np.ones(tuple(shape3) + (1,), dtype=dtype)
    if sigma > 0:
        x = np.asarray(x, dtype=dtype)
        keep = [c for c in range(x.shape[-1]) if present is None or present[c]]
        x = x[..., keep]
    out = []
    for d in offsets(conn):
        a = shift(ones, d)
        if sigma > 0:
            a = a * np.exp(-((x - shift(x, d)) ** 2).sum(-1, keepdims=True) / dtype(2.0 * sigma * sigma))
        out.append(a)
    return out


def entropy_and_grad(l, softmax):
    """Per-element entropy h (sigmoid head [D,H,W,R], softmax head [D,H,W]) and dh/dl [D,H,W,R] (of the voxel's h)."""
    if softmax:
        m = l.max(-1, keepdims=True)
        lse = m + np.log(np.exp(l - m).sum(-1, keepdims=True))
        logp = l - lse
        p = np.exp(logp)
        h = -(p * logp).sum(-1)
        return h, -p * (logp + h[..., None])
    e = np.exp(-np.abs(l))
    p = np.where(l >= 0, 1 / (1 + e), e / (1 + e))
    h = np.maximum(l, 0) + np.log1p(e) - l * p
    return h, -l * p * (1 - p)


def crf(l, x, conn, weight, sigma, softmax, form, present=None, dtype=np.float64):
    """-> dict(H, P, L, dlogits) of one item.  ``dtype`` float32 restates the arithmetic in the kernels' precision (used to
    derive the tolerance, not to compare against); its sums are still taken in float64, as the kernels take theirs."""
    assert form in FORMS
    l = np.asarray(l, dtype=dtype)
    D, Hh, W, R = l.shape
    offs = offsets(conn)
    n = len(offs)
    E = D * Hh * W * (1 if softmax else R)
    aff = affinities((D, Hh, W), x, conn, sigma, present, dtype)
    if softmax:
        p = softmax_lastaxis(l)
    else:          # the stable form on both sides of 0
        e = np.exp(-np.abs(l))
        p = np.where(l >= 0, 1 / (1 + e), e / (1 + e)).astype(dtype)
    pair = 0.0
    g = np.zeros_like(p)
    for a, d in zip(aff, offs):
        q = shift(p, d)
        if form == "quadratic":
            phi = ((p - q) ** 2).sum(-1, keepdims=True)
            g += a * 2 * (p - q)
        elif softmax:
            phi = 1 - (p * q).sum(-1, keepdims=True)
            g += a * (-q)
        else:
            phi = (p * (1 - q) + (1 - p) * q).sum(-1, keepdims=True)
            g += a * (1 - 2 * q)
        pair += float((a * phi).astype(np.float64).sum())
    g = g / dtype(n * E)
    if softmax:
        dp = p * (g - (p * g).sum(-1, keepdims=True))
    else:
        dp = g * p * (1 - p)
    h, dh = entropy_and_grad(l, softmax)
    H = float(h.astype(np.float64).sum()) / E
    P = pair / (2.0 * n * E)
    return {"H": H, "P": P, "L": H + float(weight) * P, "dlogits": dh / dtype(E) + dtype(weight) * dp}


def crf_torch(l, x, conn, weight, sigma, softmax, form, present=None):
    """L, H and P of one item as torch scalars, differentiable in ``l`` ([D,H,W,R]); ``x`` [D,H,W,C] or None."""
    import torch
    import torch.nn.functional as F
    assert form in FORMS
    D, Hh, W, R = l.shape
    offs = offsets(conn)
    n = len(offs)
    E = D * Hh * W * (1 if softmax else R)

    def sh(a, d):
        pad = F.pad(a, (0, 0, 1, 1, 1, 1, 1, 1))
        return pad[1 + d[0]:1 + d[0] + D, 1 + d[1]:1 + d[1] + Hh, 1 + d[2]:1 + d[2] + W]

    ones = torch.ones(D, Hh, W, 1, dtype=l.dtype, device=l.device)
    if sigma > 0:
        keep = [c for c in range(x.shape[-1]) if present is None or present[c]]
        xs = x[..., keep].to(l.dtype)
    if softmax:
        logp = torch.log_softmax(l, -1)
        p = logp.exp()
        H = -(p * logp).sum() / E
    else:
        p = torch.sigmoid(l)
        H = (F.softplus(l) - l * p).sum() / E
    pair = l.new_zeros(())
    for d in offs:
        a = sh(ones, d)
        if sigma > 0:
            a = a * torch.exp(-((xs - sh(xs, d)) ** 2).sum(-1, keepdim=True) / (2.0 * sigma * sigma))
        q = sh(p, d)
        if form == "quadratic":
            phi = ((p - q) ** 2).sum(-1, keepdim=True)
        elif softmax:
            phi = 1 - (p * q).sum(-1, keepdim=True)
        else:
            phi = (p * (1 - q) + (1 - p) * q).sum(-1, keepdim=True)
        pair = pair + (a * phi).sum()
    P = pair / (2.0 * n * E)
    return H + weight * P, H, P
