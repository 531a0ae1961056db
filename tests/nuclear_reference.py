"""Float64 NumPy restatement of the entropy-minus-nuclear-norm objective (``mmtta_nuclear_entropy_items``, plugin ``bnm_tta``),
shared by ``test_nuclear_host.py`` (which holds its analytic gradient to torch autograd) and ``test_hip_nuclear.py`` (which
holds the kernels to it), and a torch version of the loss for autograd.  One batch item, channels last: ``l`` [D, H, W, R].

    p      = sigmoid(l) per region, or softmax(l) over the last axis
    boxes  of block = [bd, bh, bw] voxels from multiples of the block size (0, or an entry >= the extent: the whole extent;
           border boxes are smaller, nothing is padded)
    A      softmax head: per box the m x K matrix of the rows p_i (K = R);  sigmoid head: per (box, region) the m x 2 matrix
           of the rows (p_ir, 1 - p_ir)
    nu(A)  = sum_k sqrt(lambda_k + eps m) / sqrt(m min(m, K)),   lambda_k the eigenvalues of A^T A clamped at 0
    N      = 1 / Q sum_A nu(A),   H = mean entropy over the E elements,   L = entropy_weight * H - weight * N

with Q the number of matrices, E = D H W R on the sigmoid head and D H W on the softmax head.  The gradient is the
specification's: dN/dA = A M / Q with M = c V diag(1 / sqrt(lambda_k + eps m)) V^T, c = 1 / sqrt(m min(m, K)), then the chain
through the sigmoid or the softmax."""
import itertools

import numpy as np

from crf_reference import entropy_and_grad
from lame_reference import softmax_lastaxis


def boxes(shape3, block):
    """The slices (z, y, x) of every box, z-major."""
    axes = []
    for extent, b in zip(shape3, block):
        b = extent if (b == 0 or b >= extent) else int(b)
        axes.append([slice(s, min(s + b, extent)) for s in range(0, extent, b)])
    return list(itertools.product(*axes))


def _spectrum(A, eps, dtype):
    """nu(A) and M of one m x K matrix; the Gram products are taken in ``dtype``, their sums and the eigenproblem in float64."""
    m, K = A.shape
    G = np.empty((K, K))
    for a in range(K):
        for b in range(a, K):
            G[a, b] = G[b, a] = float((A[:, a] * A[:, b]).astype(np.float64).sum())
    lam, V = np.linalg.eigh(G)
    s = np.sqrt(np.maximum(lam, 0.0) + eps * m)
    c = 1.0 / np.sqrt(m * min(m, K))
    return c * float(s.sum()), c * (V / s) @ V.T


def nuclear(l, block, weight, entropy_weight, eps, softmax, dtype=np.float64):
    """-> dict(H, N, L, dlogits, dnuclear) of one item; ``dnuclear`` is dN/dl alone.  ``dtype`` float32 restates the per-voxel
    arithmetic in the kernels' precision (used to derive the tolerance, not to compare against); the Gram sums and the
    eigenvalues stay in float64, as the kernels keep them."""
    l = np.asarray(l, dtype=dtype)
    D, Hh, W, R = l.shape
    E = D * Hh * W * (1 if softmax else R)
    if softmax:
        p = softmax_lastaxis(l)
        q = None
    else:          # the stable form on both sides of 0, and 1 - p without the subtraction
        e = np.exp(-np.abs(l))
        p = np.where(l >= 0, 1 / (1 + e), e / (1 + e)).astype(dtype)
        q = np.where(l >= 0, e / (1 + e), 1 / (1 + e)).astype(dtype)
    bx = boxes((D, Hh, W), block)
    Q = len(bx) * (1 if softmax else R)
    g = np.zeros_like(p)          # softmax head: (A M)_i / Q;  sigmoid head: [(A M)_i0 - (A M)_i1] / Q
    total = 0.0
    for sl in bx:
        if softmax:
            A = p[sl].reshape(-1, R)
            nu, M = _spectrum(A, eps, dtype)
            total += nu
            g[sl] = ((A @ M.astype(dtype)) / dtype(Q)).reshape(p[sl].shape)
        else:
            for r in range(R):
                A = np.stack([p[sl][..., r].reshape(-1), q[sl][..., r].reshape(-1)], 1)
                nu, M = _spectrum(A, eps, dtype)
                total += nu
                AM = A @ M.astype(dtype)
                g[sl + (r,)] = ((AM[:, 0] - AM[:, 1]) / dtype(Q)).reshape(p[sl].shape[:3])
    if softmax:
        dn = p * (g - (p * g).sum(-1, keepdims=True))
    else:
        dn = g * p * q
    h, dh = entropy_and_grad(l, softmax)
    H = float(h.astype(np.float64).sum()) / E
    Nn = total / Q
    dlogits = dtype(entropy_weight) * dh / dtype(E) - dtype(weight) * dn
    return {"H": H, "N": Nn, "L": float(entropy_weight) * H - float(weight) * Nn, "dlogits": dlogits, "dnuclear": dn}


def nuclear_torch(l, block, weight, entropy_weight, eps, softmax):
    """L, H and N of one item as torch scalars, differentiable in ``l`` ([D,H,W,R])."""
    import torch
    import torch.nn.functional as F
    D, Hh, W, R = l.shape
    E = D * Hh * W * (1 if softmax else R)
    if softmax:
        logp = torch.log_softmax(l, -1)
        p = logp.exp()
        H = -(p * logp).sum() / E
    else:
        p = torch.sigmoid(l)
        H = (F.softplus(l) - l * p).sum() / E
    mats = {}          # matrices of equal m go through one batched eigvalsh
    for sl in boxes((D, Hh, W), block):
        if softmax:
            mats.setdefault(p[sl].numel() // R, []).append(p[sl].reshape(-1, R))
        else:
            for r in range(R):
                pr = p[sl][..., r].reshape(-1)
                mats.setdefault(pr.numel(), []).append(torch.stack([pr, 1 - pr], 1))
    total, Q = l.new_zeros(()), 0
    for m, group in mats.items():
        A = torch.stack(group)
        K = A.shape[-1]
        lam = torch.linalg.eigvalsh(A.transpose(1, 2) @ A).clamp_min(0)
        total = total + torch.sqrt(lam + eps * m).sum() / (m * min(m, K)) ** 0.5
        Q += len(group)
    N = total / Q
    return entropy_weight * H - weight * N, H, N
