"""Float64 NumPy restatement of LAME's output refinement (``mmtta_lame_refine``, plugin ``lame_tta``), shared by
``test_lame_host.py`` (which pins it with hand-computed cases) and ``test_hip_lame.py`` (which holds the kernels to it).

    l(0) = l0;   l(t+1) = l0 + lam * sum_d w_d * shift(y(l(t)), d),   y = tanh(l / 2) or softmax over the last axis
    w_d  = shift(1, d) * exp(-sum_{c present} (x - shift(x, d))^2 / (2 sigma^2)) / n      (sigma = 0: shift(1, d) / n)

over the n = 6 / 18 / 26 offsets d of the full neighbourhood; a neighbour outside the volume contributes nothing.  Arrays are
one batch item, channels last: ``l0`` [D, H, W, R], ``x`` [D, H, W, C]."""
import itertools

import numpy as np

L1_OF = {6: 1, 18: 2, 26: 3}


def offsets(conn):
    """All d in {-1, 0, 1}^3 without 0 with |d|_1 <= 1 / 2 / 3 for connectivity 6 / 18 / 26."""
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(abs(v) for v in d) <= L1_OF[conn]]


def shift(a, d):
    """a[z + dz, y + dy, x + dx] where that lies inside the volume, 0 elsewhere (trailing axes ride along)."""
    D, H, W = a.shape[:3]
    p = np.zeros((D + 2, H + 2, W + 2) + a.shape[3:], dtype=a.dtype)
    p[1:-1, 1:-1, 1:-1] = a
    return p[1 + d[0]:1 + d[0] + D, 1 + d[1]:1 + d[1] + H, 1 + d[2]:1 + d[2] + W]


def softmax_lastaxis(l):
    e = np.exp(l - l.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def lame(l0, x, conn, lam, sigma, T, softmax, present=None, dtype=np.float64):
    """T iterations from l0; ``present``: one flag per channel of x (default all).  ``dtype`` float32 restates the arithmetic
    of the kernels' precision (used to derive the tolerance, not to compare against)."""
    l0 = np.asarray(l0, dtype=dtype)
    offs = offsets(conn)
    ones = np.ones(l0.shape[:3] + (1,), dtype=dtype)
    if sigma > 0:
        x = np.asarray(x, dtype=dtype)
        keep = [c for c in range(x.shape[-1]) if present is None or present[c]]
        x = x[..., keep]
    w = []
    for d in offs:
        a = shift(ones, d)
        if sigma > 0:
            a = a * np.exp(-((x - shift(x, d)) ** 2).sum(-1, keepdims=True) / dtype(2.0 * sigma * sigma))
        w.append(a / dtype(len(offs)))
    l = l0.copy()
    for _ in range(T):
        y = softmax_lastaxis(l) if softmax else np.tanh(l / 2)
        l = l0 + dtype(lam) * sum(wd * shift(y, d) for wd, d in zip(w, offs))
    return l


def flipped(l0, l, softmax):
    """Elements whose hard prediction changed: sigmoid head 1[l >= 0] per (voxel, region), softmax head the FIRST arg max."""
    if softmax:
        return int((np.argmax(l, -1) != np.argmax(l0, -1)).sum())
    return int(((l >= 0) != (np.asarray(l0) >= 0)).sum())


def decision_gap(l, softmax):
    """The smallest distance of an element from its decision boundary: |l| (sigmoid head) or the top-2 gap (softmax head)."""
    if softmax:
        s = np.sort(l, -1)
        return float((s[..., -1] - s[..., -2]).min())
    return float(np.abs(l).min())
