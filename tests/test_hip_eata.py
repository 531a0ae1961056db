"""EATA adaptation (``eata_tta``) on the GPU: the weighted entropy, the pseudo-label loss, the Fisher accumulation and the
penalty pass against torch restatements, one eager step stage by stage against torch autograd, the Fisher estimate and the
plugin against an EATA restatement on the oracle networks, and the bitwise properties (grouped = one volume at a time =
eager, lambda = 0, the continual run).

Inputs of the kernel tests are seeded so that no element's entropy lies within 1e-5 of the margin (the rule DESIGN.md section
6 applies to the ReLU threshold): the keep masks must then agree exactly."""
import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from test_hip_sar import (BATCH, SECOND_TRIP, away_from_margin, entropy_elements, grad_buffer, keep_cl, run_filtered,
                          second_trip_logits, stage)
from test_hip_tta import SMALL, build_pair, root_cfg, volume

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- float64 restatements of the kernels
def weighted_reference(z: torch.Tensor, margin: float, softmax: bool):
    """Per item: loss, kept count, keep mask and d(loss)/dz in float64; c = exp(margin - H) carries no gradient."""
    z = z.double().detach().requires_grad_(True)
    H = entropy_elements(z, softmax)
    keep = H < margin
    c = torch.exp(margin - H).detach()
    losses, kept = [], []
    total = 0.0
    for n in range(z.shape[0]):
        k = keep[n]
        cnt = int(k.sum())
        kept.append(cnt)
        if cnt:
            ln = (c[n] * H[n])[k].sum() / cnt
            total = total + ln
            losses.append(float(ln))
        else:
            losses.append(float("nan"))
    if torch.is_tensor(total):
        total.backward()
        grad = z.grad
    else:
        grad = torch.zeros_like(z)
    return losses, kept, keep, grad


def run_weighted(z_cl, margin, softmax, dtype=torch.float32):
    from multimodal_tta_amd import ops
    n, d, h, w, r = z_cl.shape
    elems = n * d * h * w * (1 if softmax else r)
    g = grad_buffer(z_cl, dtype)
    keep = torch.full((elems,), 7, dtype=torch.uint8, device="cuda")
    partial = torch.empty(ops.entropy_weighted_partials(z_cl), dtype=torch.float64, device="cuda")
    loss = torch.full((n,), 123.0, device="cuda")
    kept = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    ops.entropy_weighted_items(z_cl, g, margin, keep, partial, loss, kept, softmax=softmax)
    torch.cuda.synchronize()
    return loss.cpu(), kept.cpu(), keep.cpu(), ops.from_cl(g.float()).cpu()


# (softmax, R, generic): the Bernoulli fast path, the generic Bernoulli kernel, the categorical head
HEADS = [(False, 3, False), (False, 4, False), (False, 1, False), (False, 3, True), (False, 4, True), (True, 3, False),
         (True, 4, False)]
SATURATED = [0.0, 20.0, -20.0, 90.0, -90.0, 1e4, -1e4]


@pytest.mark.parametrize("softmax,R,generic", HEADS)
@pytest.mark.parametrize("N", [1, 3])
def test_weighted_entropy_matches_float64_and_the_filtered_mask(softmax, R, generic, N):
    gen = torch.Generator().manual_seed(0)
    margin = 0.4 * math.log(R if softmax else 2.0)
    z = away_from_margin(torch.randn((N, R, 6, 7, 9), generator=gen) * 3.0, margin, softmax, gen)
    l_ref, k_ref, m_ref, g_ref = weighted_reference(z, margin, softmax)
    share = sum(k_ref) / float(m_ref.numel())
    print(f"kept share {share:.3f}")
    assert 0.2 <= share <= 0.8, "the filter is not exercised"
    z_cl = stage(z, generic)
    f_loss, f_kept, f_keep, _ = run_filtered(z_cl, margin, softmax)
    fp32 = None
    for dtype in ((torch.float32, torch.bfloat16) if (not softmax and not generic) else (torch.float32,)):
        loss, kept, keep, g = run_weighted(z_cl, margin, softmax, dtype=dtype)
        assert torch.equal(keep, keep_cl(m_ref, softmax)), "keep masks differ from float64"
        assert kept.tolist() == k_ref
        assert torch.equal(keep, f_keep) and torch.equal(kept, f_kept), "mask / count differ from mmtta_entropy_filtered_items"
        for a, b in zip(loss.tolist(), l_ref):
            assert abs(a - b) <= 1e-5 * abs(b), (a, b)
        if dtype == torch.float32:
            fp32 = g
            assert (g.double() - g_ref).abs().max().item() <= 2e-5 * g_ref.abs().max().item()
        else:
            want = fp32.to(torch.bfloat16).float()          # the fp32 result rounded, to 1 ulp of bf16 (2^-7 relative)
            assert ((g - want).abs() <= 2.0 ** -7 * want.abs()).all()
        assert torch.all(g[~(m_ref.unsqueeze(1).expand_as(g) if softmax else m_ref)] == 0)
    # the weight is in the loss: it differs from the plain filtered mean by the factor c > 1
    assert all(a > b for a, b in zip(loss.tolist(), f_loss.tolist()))


@functools.lru_cache(maxsize=None)
def second_trip_weighted_reference(softmax):
    z, margin = second_trip_logits(softmax)
    return weighted_reference(z, margin, softmax)


@pytest.mark.parametrize("softmax,generic,dtype", SECOND_TRIP)
def test_weighted_entropy_on_the_second_trip_of_the_walk(softmax, generic, dtype):
    """test_weighted_entropy_matches_float64_and_the_filtered_mask at test_hip_sar.SECOND_TRIP_SHAPE: more voxels than one
    launch has threads, two items."""
    z, margin = second_trip_logits(softmax)
    l_ref, k_ref, m_ref, g_ref = second_trip_weighted_reference(softmax)
    share = sum(k_ref) / float(m_ref.numel())
    print(f"kept share {share:.3f}")
    assert 0.2 <= share <= 0.8, "the filter is not exercised"
    z_cl = stage(z, generic)
    f_loss, f_kept, f_keep, _ = run_filtered(z_cl, margin, softmax)
    loss, kept, keep, g = run_weighted(z_cl, margin, softmax, dtype=dtype)
    assert torch.equal(keep, keep_cl(m_ref, softmax)), "keep masks differ from float64"
    assert kept.tolist() == k_ref
    assert torch.equal(keep, f_keep) and torch.equal(kept, f_kept), "mask / count differ from mmtta_entropy_filtered_items"
    for a, b in zip(loss.tolist(), l_ref):
        print(f"loss {a} vs {b}")
        assert abs(a - b) <= 1e-5 * abs(b), (a, b)
    if dtype == torch.float32:
        err = (g.double() - g_ref).abs().max().item() / g_ref.abs().max().item()
        print(f"gradient error {err:.2e} of the maximum")
        assert err <= 2e-5
    else:
        want = run_weighted(z_cl, margin, softmax)[3].to(torch.bfloat16).float()          # the fp32 result rounded
        assert ((g - want).abs() <= 2.0 ** -7 * want.abs()).all()
    assert torch.all(g[~(m_ref.unsqueeze(1).expand_as(g) if softmax else m_ref)] == 0)
    assert all(a > b for a, b in zip(loss.tolist(), f_loss.tolist()))


@pytest.mark.parametrize("softmax,R,generic,dtype", [(False, 3, False, torch.float32), (False, 3, False, torch.bfloat16),
                                                     (False, 3, True, torch.float32), (True, 4, False, torch.float32)])
def test_weighted_n_items_equal_n_single_item_calls(softmax, R, generic, dtype):
    gen = torch.Generator().manual_seed(5)
    N = 3
    margin = 0.6 * math.log(R if softmax else 2.0)
    z = torch.randn((N, R, 9, 8, 7), generator=gen) * 3.0
    together = run_weighted(stage(z, generic), margin, softmax, dtype=dtype)
    per = z[0:1].numel() // R * (1 if softmax else R)
    for n in range(N):
        one = run_weighted(stage(z[n:n + 1], generic), margin, softmax, dtype=dtype)
        assert torch.equal(one[0], together[0][n:n + 1]) and torch.equal(one[1], together[1][n:n + 1])
        assert torch.equal(one[2], together[2][n * per:(n + 1) * per])
        assert torch.equal(one[3], together[3][n:n + 1])


@pytest.mark.parametrize("softmax", [False, True])
def test_weighted_empty_filter_gives_nan_loss_and_zero_gradient(softmax):
    gen = torch.Generator().manual_seed(9)
    z = torch.randn((2, 3, 4, 5, 6), generator=gen) * 3.0
    loss, kept, keep, g = run_weighted(stage(z, False), 1e-30, softmax)
    assert torch.isnan(loss).all() and kept.tolist() == [0, 0]
    assert torch.all(keep == 0) and torch.all(g == 0)


def saturated_logits(N, R, gen):
    pick = torch.randint(0, len(SATURATED), (N, R, 5, 6, 7), generator=gen)
    return torch.tensor(SATURATED)[pick]


@pytest.mark.parametrize("softmax,R,generic", HEADS)
def test_weighted_entropy_is_finite_on_saturated_logits(softmax, R, generic):
    gen = torch.Generator().manual_seed(21)
    z = saturated_logits(2, R, gen)
    margin = 0.4 * math.log(R if softmax else 2.0)
    loss, kept, keep, g = run_weighted(stage(z, generic), margin, softmax)
    assert torch.isfinite(g).all() and torch.isfinite(loss).all() and (kept > 0).all()
    assert (loss >= 0).all() and (loss <= margin * math.exp(margin)).all()


# ----------------------------------------------------------------------------- pseudo-label loss
def pseudo_reference(z: torch.Tensor, softmax: bool):
    z = z.double().detach().requires_grad_(True)
    if softmax:
        per = F.cross_entropy(z, z.argmax(1), reduction="none").flatten(1).mean(1)
    else:
        per = F.binary_cross_entropy_with_logits(z, (z >= 0).double(), reduction="none").flatten(1).mean(1)
    per.sum().backward()
    return per.detach(), z.grad


def run_pseudo(z_cl, softmax, dtype=torch.float32):
    from multimodal_tta_amd import ops
    n = z_cl.shape[0]
    g = grad_buffer(z_cl, dtype)
    partial = torch.empty(ops.pseudo_label_partials(z_cl), dtype=torch.float64, device="cuda")
    loss = torch.full((n,), 123.0, device="cuda")
    ops.pseudo_label_loss_items(z_cl, g, partial, loss, softmax=softmax)
    torch.cuda.synchronize()
    return loss.cpu(), ops.from_cl(g.float()).cpu()


@pytest.mark.parametrize("softmax,R,generic", HEADS)
@pytest.mark.parametrize("N", [1, 3])
def test_pseudo_label_loss_matches_float64(softmax, R, generic, N):
    gen = torch.Generator().manual_seed(40 + R + N)
    z = torch.randn((N, R, 6, 7, 9), generator=gen) * 3.0
    l_ref, g_ref = pseudo_reference(z, softmax)
    z_cl = stage(z, generic)
    loss, g = run_pseudo(z_cl, softmax)
    assert ((loss.double() - l_ref).abs() <= 1e-5 * l_ref.abs()).all(), (loss, l_ref)
    assert (g.double() - g_ref).abs().max().item() <= 2e-5 * g_ref.abs().max().item()
    if not softmax and not generic:
        _, g16 = run_pseudo(z_cl, softmax, dtype=torch.bfloat16)
        want = g.to(torch.bfloat16).float()
        assert ((g16 - want).abs() <= 2.0 ** -7 * want.abs()).all()
    for n in range(N):          # N items = N calls, bit for bit
        l1, g1 = run_pseudo(stage(z[n:n + 1], generic), softmax)
        assert torch.equal(l1, loss[n:n + 1]) and torch.equal(g1, g[n:n + 1])


@functools.lru_cache(maxsize=None)
def second_trip_pseudo_reference(softmax):
    return pseudo_reference(second_trip_logits(softmax)[0], softmax)


@pytest.mark.parametrize("softmax,generic,dtype", SECOND_TRIP)
def test_pseudo_label_loss_on_the_second_trip_of_the_walk(softmax, generic, dtype):
    """test_pseudo_label_loss_matches_float64 at test_hip_sar.SECOND_TRIP_SHAPE."""
    z = second_trip_logits(softmax)[0]
    l_ref, g_ref = second_trip_pseudo_reference(softmax)
    z_cl = stage(z, generic)
    loss, g = run_pseudo(z_cl, softmax)
    print(f"loss {loss.tolist()} vs {l_ref.tolist()}")
    assert ((loss.double() - l_ref).abs() <= 1e-5 * l_ref.abs()).all(), (loss, l_ref)
    err = (g.double() - g_ref).abs().max().item() / g_ref.abs().max().item()
    print(f"gradient error {err:.2e} of the maximum")
    assert err <= 2e-5
    if dtype == torch.bfloat16:
        l16, g16 = run_pseudo(z_cl, softmax, dtype=dtype)
        want = g.to(torch.bfloat16).float()
        assert torch.equal(l16, loss) and ((g16 - want).abs() <= 2.0 ** -7 * want.abs()).all()
    for n in range(z.shape[0]):          # N items = N calls, bit for bit
        l1, g1 = run_pseudo(stage(z[n:n + 1], generic), softmax)
        assert torch.equal(l1, loss[n:n + 1]) and torch.equal(g1, g[n:n + 1])


@pytest.mark.parametrize("softmax,R,generic", HEADS)
def test_pseudo_label_loss_is_finite_on_saturated_logits(softmax, R, generic):
    gen = torch.Generator().manual_seed(22)
    z = saturated_logits(2, R, gen)
    if softmax:          # (no ties for the arg max: the restatement's choice among equal logits is not specified)
        z = z + torch.arange(R).view(1, R, 1, 1, 1) * 1e-3 * z.abs().clamp(min=1.0)
    l_ref, g_ref = pseudo_reference(z, softmax)
    loss, g = run_pseudo(stage(z, generic), softmax)
    assert torch.isfinite(loss).all() and torch.isfinite(g).all()
    assert ((loss.double() - l_ref).abs() <= 1e-5 * l_ref.abs() + 1e-12).all()
    assert (g.double() - g_ref).abs().max().item() <= 2e-5 * g_ref.abs().max().item()


# ----------------------------------------------------------------------------- Fisher span
def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("n,stride", [(1003, 1008), (4096 * 256 * 4 + 4 * 1003 + 3, 4096 * 256 * 4 + 4 * 1004)])
def test_fisher_accumulate_and_scale_are_bitwise_torch(n, stride):
    from multimodal_tta_amd import ops
    gen = torch.Generator().manual_seed(n % 97)
    sets = 3
    g = torch.randn((sets + 1, stride), generator=gen) * torch.tensor([1.0, 1e-3, 30.0, 1.0]).view(4, 1)
    f0 = torch.rand(stride, generator=gen)
    f = f0.clone().cuda()
    ops.fisher_accumulate_sets(f, g.cuda(), n, sets)
    torch.cuda.synchronize()
    want = f0[:n].clone()
    for s in range(sets):
        want = want + g[s, :n] * g[s, :n]
    assert torch.equal(bits(f.cpu()[:n]), bits(want)), "F + g * g in set order"
    assert torch.equal(f.cpu()[n:], f0[n:]), "elements past n moved"
    ops.fisher_scale(f, n, 3)
    torch.cuda.synchronize()
    assert torch.equal(bits(f.cpu()[:n]), bits(want / torch.tensor(3.0))), "F / N"
    assert torch.equal(f.cpu()[n:], f0[n:])


def test_fisher_penalty_matches_float64():
    from multimodal_tta_amd import ops
    gen = torch.Generator().manual_seed(3)
    replicas, stride, n, sets, lam = 4, 4104, 4000, 3, 750.0
    src = torch.randn(stride, generator=gen)
    w0 = src.unsqueeze(0) + torch.randn((replicas, stride), generator=gen) * torch.tensor([1e-3, 1e-1, 1.0, 1.0]).view(4, 1)
    fisher = torch.rand(stride, generator=gen) ** 4
    g0 = torch.randn((replicas, stride), generator=gen)
    w, g = w0.clone().cuda(), g0.clone().cuda()
    partial = torch.empty(ops.fisher_penalty_partials(n, sets), dtype=torch.float64, device="cuda")
    penalty = torch.full((replicas,), -1.0, device="cuda")
    ops.fisher_penalty_sets(w, g, fisher.cuda(), src.cuda(), n, sets, lam, partial, penalty)
    torch.cuda.synchronize()
    g, pen_dev, penalty = g.cpu(), penalty, penalty.cpu()
    assert torch.equal(w.cpu(), w0), "the weights moved"
    assert torch.equal(g[sets:], g0[sets:]) and torch.equal(g[:, n:], g0[:, n:]), "a gradient outside the sets / the span moved"
    assert torch.all(penalty[sets:] == -1.0)
    for s in range(sets):
        d = w0[s, :n].double() - src[:n].double()
        want = (g0[s, :n].double() + 2.0 * lam * fisher[:n].double() * d).float()
        assert ((g[s, :n] - want).abs() <= 1e-6 * want.abs() + 1e-7 * g0.abs().max()).all()
        p = lam * (fisher[:n].double() * d * d).sum().item()
        assert abs(penalty[s].item() - p) <= 1e-6 * p, (s, penalty[s].item(), p)
    assert penalty[0] < penalty[1] < penalty[2]
    # w == source: gradient values unchanged, penalty 0
    w = src.unsqueeze(0).repeat(replicas, 1).cuda()
    g = g0.clone().cuda()
    ops.fisher_penalty_sets(w, g, fisher.cuda(), src.cuda(), n, sets, lam, partial, pen_dev)
    torch.cuda.synchronize()
    assert torch.equal(g.cpu(), g0) and torch.all(pen_dev.cpu()[:sets] == 0)


# ----------------------------------------------------------------------------- the EATA restatement (torch autograd)
LAMBDA = 1e8          # the regulariser is visible at the reference's learning rate (2000, the paper's, is inert there)


def pseudo_loss(z, softmax):
    if softmax:
        return F.cross_entropy(z, z.argmax(1))
    return F.binary_cross_entropy_with_logits(z, (z >= 0).to(z.dtype))


def fisher_reference(model, xs, softmax=False):
    """F per parameter name from the volumes ``xs`` at the model's weights (a copy is used: its running statistics move)."""
    m = copy.deepcopy(model)
    m.train()
    fisher = {n: torch.zeros_like(p) for n, p in m.named_parameters()}
    for x in xs:
        m.zero_grad()
        pseudo_loss(m(x), softmax).backward()
        for n, p in m.named_parameters():
            if p.grad is not None:          # (a parameter the forward does not use has no gradient: F stays 0)
                fisher[n] = fisher[n] + p.grad * p.grad
    return {n: f / float(len(xs)) for n, f in fisher.items()}


def eata_reference(model, xs, train_cfg, steps, e_margin, lam, fisher, softmax=False, episodic=True):
    """EATA with torch autograd over the volumes ``xs`` in order: per volume the final logits and the per-step L, kept, P."""
    import oracle
    named = list(model.named_parameters())
    w0 = {n: p.detach().clone() for n, p in named}
    source = copy.deepcopy(model.state_dict())
    opt = oracle.adam.build_optimizer(named, train_cfg)
    out = []
    for x in xs:
        if episodic:
            model.load_state_dict(source)
            opt = oracle.adam.build_optimizer(named, train_cfg)
        rec = {"losses": [], "kept": [], "penalty": []}
        model.train()
        for _ in range(steps):
            opt.zero_grad()
            z = model(x)
            margin = e_margin * math.log(z.shape[1] if softmax else 2.0)
            H = entropy_elements(z, softmax)
            keep = H < margin
            c = torch.exp(margin - H).detach()
            loss = (c * H)[keep].mean()
            pen = lam * sum((fisher[n] * (p - w0[n]) ** 2).sum() for n, p in named) if lam > 0 else torch.zeros(())
            if int(keep.sum()):
                (loss + pen).backward()
            elif lam > 0:
                pen.backward()
            opt.step()
            rec["losses"].append(float(loss))
            rec["kept"].append(int(keep.sum()))
            rec["penalty"].append(float(pen))
        model.eval()
        with torch.no_grad():
            rec["logits"] = model(x)
        out.append(rec)
    return out


def eata_cfg(model_cfg, steps=3, lr=None, e_margin=0.8, lam=LAMBDA, **method):
    """``lr=None``: the configured learning rate (the reference's, 1e-5)."""
    from multimodal_tta_amd.config import compose
    cfg = root_cfg(model_cfg, steps=steps, lr=1e-3 if lr is None else lr, **method)
    if lr is None:
        cfg["training"]["optimizers"]["adam"]["lr"] = compose(overrides=["task=brats", "model=unet"])["training"]["optimizers"]["adam"]["lr"]
    cfg["method"]["name"] = "eata_tta"
    cfg["method"]["eata"] = {"e_margin": e_margin, "fisher_alpha": lam, "fisher": {"volumes": 2, "path": None}}
    return cfg


def masks_of(z, softmax):
    if softmax:
        return F.one_hot(z.argmax(1), z.shape[1]).permute(0, 4, 1, 2, 3)
    return torch.sigmoid(z) >= 0.5


def check_against_reference(z_hip, res, o32, o64, y, elements, softmax=False, bf16=False):
    """SAR's bounds (tests/test_hip_sar.py::check_against_reference), with P next to L.  fp32, at the reference's learning
    rate: per-step L and P within 1e-4 relative (+1e-6 / +1e-12) and kept within 1e-4 of the element count of the float64
    restatement, or 3x as far as the fp32 restatement sits from it; final logits within max(5e-3, 3x fp32's distance) of
    max|logits|; mask voxels differing only where the float64 logit is within that bound of the threshold; Dice 2e-3.  bf16:
    Tent's bf16 bounds against the fp32 restatement (L 1e-2 relative, kept 1e-2 of the elements, logits 3e-2, masks 1e-2,
    Dice 2e-2); P within 25 % of the fp32 restatement's (exactly 0 at the first step).  Adam's first steps move every element
    by about the learning rate whatever the size of its gradient, so P depends on the gradients' signs and the share of
    elements whose sign bf16 flips has no precision argument behind it; the bound is there to catch what is wrong by a
    factor - another lambda, a missing 2 in the pull, a sum over the wrong span - each of which moves P by 2x or more,
    while P is quadratic in a displacement whose relative error stays near the 3e-2 of the logits ((1 + 0.1)^2 - 1 = 0.21
    would already take a tenfold excess of that).  Returns the logit bound used."""
    import oracle
    steps = len(o32["losses"])
    losses, kept = res["losses"].cpu().reshape(-1).tolist(), res["kept"].cpu().reshape(-1).tolist()
    pens = res["penalty"].cpu().reshape(-1).tolist()

    def dice(m):
        return oracle.binary_dice_iou(m.to(torch.uint8), (y > 0.5).to(torch.uint8))[0]

    z32 = o32["logits"]
    if bf16:
        for t in range(steps):
            a, b = losses[t], o32["losses"][t]
            assert abs(a - b) <= 1e-2 * abs(b), f"step {t}: L {a} vs reference {b}"
            assert abs(kept[t] - o32["kept"][t]) <= 1e-2 * elements, f"step {t}: kept {kept[t]} vs {o32['kept'][t]}"
            b = o32["penalty"][t]
            assert math.isfinite(pens[t]) and abs(pens[t] - b) <= 0.25 * b, f"step {t}: P {pens[t]} vs reference {b}"
        err = (z_hip - z32).abs().max().item() / z32.abs().max().item()
        mism = (masks_of(z_hip, softmax) != masks_of(z32, softmax)).float().mean().item()
        ddice = (dice(masks_of(z_hip, softmax)) - dice(masks_of(z32, softmax))).abs().max().item()
        print(f"bf16: L {losses} kept {kept} P {pens} (fp32 {o32['penalty']}); logits {err:.2e}, masks {mism:.2e}, Dice {ddice:.2e}")
        assert err > 1e-6, "bf16 path not taken"
        assert err <= 3e-2 and mism <= 1e-2 and ddice <= 2e-2, (err, mism, ddice)
        return 3e-2
    for t in range(steps):
        a, b, c = losses[t], o32["losses"][t], o64["losses"][t]
        assert abs(a - c) <= max(1e-4 * abs(c) + 1e-6, 3.0 * abs(b - c)), f"step {t}: L {a}, fp32 {b}, fp64 {c}"
        a, b, c = kept[t], o32["kept"][t], o64["kept"][t]
        assert abs(a - c) <= max(1e-4 * elements, 3.0 * abs(b - c)), f"step {t}: kept {a}, fp32 {b}, fp64 {c}"
        a, b, c = pens[t], o32["penalty"][t], o64["penalty"][t]
        assert abs(a - c) <= max(1e-4 * abs(c) + 1e-12, 3.0 * abs(b - c)), f"step {t}: P {a}, fp32 {b}, fp64 {c}"
    z64 = o64["logits"]
    scale = z64.abs().max().item()
    e_ref = (z32.double() - z64).abs().max().item() / scale
    e_hip = (z_hip.double() - z64).abs().max().item() / scale
    bound = max(5e-3, 3.0 * e_ref)
    assert e_hip <= bound, f"HIP vs fp64 EATA {e_hip:.3e}; fp32 EATA vs fp64 EATA {e_ref:.3e}"
    m_hip, m32, m64 = masks_of(z_hip, softmax), masks_of(z32, softmax), masks_of(z64, softmax)
    if not softmax:
        near = z64.abs() <= bound * scale
        assert not torch.any((m_hip != m64) & ~near), "a mask voxel differs away from the threshold"
    d64 = dice(m64)
    dd_hip, dd_ref = (dice(m_hip) - d64).abs().max().item(), (dice(m32) - d64).abs().max().item()
    assert dd_hip <= max(2e-3, 3.0 * dd_ref), (dd_hip, dd_ref)
    print(f"L {losses} kept {kept} P {pens}; logits {e_hip:.2e} (fp32 {e_ref:.2e}), Dice {dd_hip:.2e}")
    return bound


def run_case(model_cfg, cfg, vols, steps, e_margin, lam, softmax=False, episodic=True, bf16=False, pair=None, R=3):
    """The plugin and the fp32 / float64 restatements over ``vols`` ([(x, y)]), F from the restatement's own estimate on
    volumes 10 and 11; returns the plugin's and the restatements' per-volume results."""
    from multimodal_tta_amd.registry import get_plugin
    ref, hip = pair if pair is not None else build_pair(model_cfg)
    fx = [volume(i, R=R)[0] for i in (10, 11)]
    ref64 = copy.deepcopy(ref).double()
    f32 = fisher_reference(ref, fx, softmax)
    f64 = fisher_reference(ref64, [x.double() for x in fx], softmax)
    o32 = eata_reference(ref, [x for x, _ in vols], cfg["training"], steps, e_margin, lam, f32, softmax, episodic)
    o64 = None if bf16 else eata_reference(ref64, [x.double() for x, _ in vols], cfg["training"], steps, e_margin, lam, f64,
                                           softmax, episodic)
    plug = get_plugin("eata_tta")(cfg).setup(hip, "cuda")
    plug.load_fisher({"volumes": 2, "fisher": f32})
    return plug, o32, o64


@pytest.mark.parametrize("e_margin", [0.8, 0.4])
def test_eata_matches_the_restatement(e_margin):
    cfg = eata_cfg(SMALL, steps=3, e_margin=e_margin, group=1)
    x, y = volume(0)
    plug, o32, o64 = run_case(SMALL, cfg, [(x, y)], 3, e_margin, LAMBDA)
    res = plug.adapt_volume(x.cuda())
    assert res["losses"].shape == (3,) and res["kept"].shape == (3,) and res["penalty"].shape == (3,)
    assert float(res["penalty"][0]) == 0.0 and float(res["penalty"][2]) > 0.0
    check_against_reference(plug.logits(res).cpu(), res, o32[0], o64[0], y, x[0, :3].numel())


@pytest.mark.parametrize("e_margin", [0.8, 0.4])
def test_eata_continual_run_matches_the_restatement_and_shows_the_regulariser(e_margin):
    """Three volumes x S = 3 with ``episodic: false``: weights, Adam state and the distance from the source carry over.  The
    float64 restatement with the case's lambda and with lambda = 0 must differ by at least 5x the logit bound on the last
    volume, so that a regulariser that did nothing would fail the comparison.  Measured on the CPU restatement (last volume,
    e_margin 0.8 / 0.4, of max|logits|): lambda 1e8 1.6e-2 / 1.1e-2, 1e9 2.6e-2 / 2.3e-2, 1e10 3.5e-2 / 3.3e-2 - against
    5 x 5e-3 = 2.5e-2 only 1e10 serves both margins (Adam's steps are about the learning rate per element whatever the
    gradient's size, so the distance grows slowly with lambda); the fp32 and float64 restatements stay 2e-6 apart there."""
    lam = 1e10
    cfg = eata_cfg(SMALL, steps=3, e_margin=e_margin, lam=lam, group=1, episodic=False)
    vols = [volume(i) for i in range(3)]
    plug, o32, o64 = run_case(SMALL, cfg, vols, 3, e_margin, lam, episodic=False)
    ref, _ = build_pair(SMALL)
    free = eata_reference(ref.double(), [x.double() for x, _ in vols], cfg["training"], 3, e_margin, 0.0, None, episodic=False)
    bound = 0.0
    for i, (x, y) in enumerate(vols):
        res = plug.adapt_volume(x.cuda())
        bound = check_against_reference(plug.logits(res).cpu(), res, o32[i], o64[i], y, x[0, :3].numel())
        if i > 0:
            assert float(res["penalty"][0]) > 0.0, "the weights were not carried into the next volume"
    z_reg, z_free = o64[-1]["logits"], free[-1]["logits"]
    moved = (z_reg - z_free).abs().max().item() / z_reg.abs().max().item()
    print(f"lambda {lam:g} against lambda 0 in float64: {moved:.3e} of max|logits| (logit bound {bound:.1e})")
    assert moved >= 5.0 * bound, f"the regulariser moves the logits by {moved:.3e} of their maximum, the logit bound is {bound:.1e}"


def test_eata_batchnorm_norm_sets_group_matches_the_restatement():
    G, e_margin = 3, 0.8
    cfg = eata_cfg(BATCH, steps=3, e_margin=e_margin, group=G, norm_sets=True)
    vols = [volume(i) for i in range(G)]
    plug, o32, o64 = run_case(BATCH, cfg, vols, 3, e_margin, LAMBDA)
    assert plug.group == G
    res = plug.adapt_volume(torch.cat([v[0] for v in vols]).cuda())
    assert res["losses"].shape == (3, G) and res["kept"].shape == (3, G) and res["penalty"].shape == (3, G)
    z = plug.logits(res).cpu()
    for g in range(G):
        x, y = vols[g]
        one = {k: res[k][:, g] for k in ("losses", "kept", "penalty")}
        check_against_reference(z[g:g + 1], one, o32[g], o64[g], y, x[0, :3].numel())


def test_eata_softmax_head_matches_the_restatement():
    e_margin = 0.8
    mcfg = dict(SMALL, num_classes=4)
    cfg = eata_cfg(mcfg, steps=3, e_margin=e_margin, group=1)
    cfg["training"]["criterion"]["softmax"] = True
    cfg["training"]["criterion"]["sigmoid"] = False
    x, y = volume(1, R=4)
    plug, o32, o64 = run_case(mcfg, cfg, [(x, y)], 3, e_margin, LAMBDA, softmax=True, R=4)
    assert plug.softmax
    res = plug.adapt_volume(x.cuda())
    check_against_reference(plug.logits(res).cpu(), res, o32[0], o64[0], y, x[0, 0].numel(), softmax=True)


def test_eata_deepfusion_matches_the_restatement():
    import oracle
    from multimodal_tta_amd.models import MultimodalUNetDeepFusion
    e_margin = 0.8
    mcfg = dict(name="unet_multimodal_deepfusion", num_modalities=4, num_classes=3, spatial_dims=3,
                channels=[4, 8, 16, 32, 64], strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)
    cfg = eata_cfg(mcfg, steps=3, e_margin=e_margin, group=1)
    torch.manual_seed(42)
    ref = oracle.MultimodalUNetDeepFusion(mcfg)
    hip = MultimodalUNetDeepFusion(mcfg)
    hip.load_state_dict(ref.state_dict())
    x, y = volume(2)
    plug, o32, o64 = run_case(mcfg, cfg, [(x, y)], 3, e_margin, LAMBDA, pair=(ref, hip))
    res = plug.adapt_volume(x.cuda())
    check_against_reference(plug.logits(res).cpu(), res, o32[0], o64[0], y, x[0, :3].numel())


def test_eata_bf16_tracks_the_restatement():
    e_margin = 0.8
    cfg = eata_cfg(SMALL, steps=3, e_margin=e_margin, group=1, precision="bf16")
    x, y = volume(5)
    plug, o32, _ = run_case(SMALL, cfg, [(x, y)], 3, e_margin, LAMBDA, bf16=True)
    res = plug.adapt_volume(x.cuda())
    assert float(res["penalty"][0]) == 0.0
    check_against_reference(plug.logits(res).cpu(), res, o32[0], None, y, x[0, :3].numel(), bf16=True)


# ----------------------------------------------------------------------------- the Fisher estimate
def test_fisher_estimate_matches_the_restatement_and_a_group_equals_one_at_a_time():
    """The estimate from two volumes against torch autograd.  The project's gradient bound is delta = 2e-3 of a tensor's
    maximum; an error delta max|g| in g moves g^2 by at most (2 delta + delta^2) max g^2, so F is held to
    4.1e-3 of its tensor's maximum.  Conv biases in front of an instance norm have an analytically zero gradient (max F <=
    1e-12 of the model's maximum in the restatement): those are held to 4.1e-3 of the model's maximum F."""
    from multimodal_tta_amd.registry import get_plugin
    ref, _ = build_pair(SMALL)
    xs = [volume(i)[0] for i in (10, 11)]
    want = fisher_reference(ref, xs)
    top = max(f.max().item() for f in want.values())
    states = {}
    for group in (2, 1):
        cfg = eata_cfg(SMALL, steps=1, group=group, tune_volumes=4)
        _, hip = build_pair(SMALL)
        plug = get_plugin("eata_tta")(cfg).setup(hip, "cuda")
        assert plug.needs_fisher
        n = plug.estimate_fisher([torch.cat(xs).cuda()] if group == 2 else [x.cuda() for x in xs])
        assert n == 2 and not plug.needs_fisher and plug.fisher_count == 2
        ar = plug.rt.arena
        assert torch.equal(ar.params_all.cpu(), ar.source.cpu().unsqueeze(0).expand(ar.replicas, -1)) and int(ar.step) == 0
        states[group] = plug.fisher_state()
        span = plug.fisher.clone()
        plug.load_fisher(states[group])          # the state round-trips through the parameter names
        assert torch.equal(plug.fisher, span)
    assert states[2]["volumes"] == 2 and set(states[2]["fisher"]) == set(want)
    worst, zeros = 0.0, 0
    for name, f in want.items():
        got = states[2]["fisher"][name]
        assert torch.equal(got, states[1]["fisher"][name]), f"{name}: the grouped estimate differs from one volume at a time"
        if f.max().item() <= 1e-12 * top:
            zeros += 1
            assert got.max().item() <= 4.1e-3 * top, name
            continue
        err = (got - f).abs().max().item() / f.max().item()
        worst = max(worst, err)
        assert err <= 4.1e-3, (name, err)
    print(f"Fisher estimate: worst tensor {worst:.2e} of its maximum; {zeros} analytically zero tensors")
    assert zeros == 17


# ----------------------------------------------------------------------------- one eager step, stage by stage
def test_one_eata_step_matches_torch_stage_by_stage(monkeypatch):
    """One eager step of the plugin away from the source (``episodic: false`` on a perturbed replica, so that the penalty is
    not zero), read at every stage against torch autograd on the same weights: logits 5e-4 of their maximum, the keep mask
    bit-exact where the float64 entropy is 1e-5 away from the margin, L 1e-5 relative on the recorded logits, the gradient
    before the penalty 2e-3 of each tensor's maximum, P 1e-5 relative, the gradient after the penalty by the kernel's bound
    and the weights after Adam's first step as in SAR's stage test."""
    import oracle
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.registry import get_plugin
    from test_hip_unet import feeds_norm
    e_margin, lam = 0.8, 1e6
    cfg = eata_cfg(SMALL, steps=1, lr=1e-3, e_margin=e_margin, lam=lam, group=1, use_graph=False, episodic=False)
    ref, hip = build_pair(SMALL)
    x, _ = volume(0)
    fisher = fisher_reference(ref, [volume(i)[0] for i in (10, 11)])
    plug = get_plugin("eata_tta")(cfg).setup(hip, "cuda")
    plug.load_fisher({"volumes": 2, "fisher": fisher})
    ar = plug.rt.arena
    nt = ar.n_train
    gen = torch.Generator().manual_seed(1)
    shift = torch.zeros(nt)
    for r in ar.refs:
        if r.trainable:          # (the alignment gaps between parameters stay at the source's zero)
            shift[r.offset:r.offset + r.numel] = torch.randn(r.numel, generator=gen) * 1e-3
    ar.params_all[0, :nt] += shift.cuda()
    w_start = ar.params_all[0, :nt].cpu()
    rec = {}
    weighted, pen, step = ops.entropy_weighted_items, ops.fisher_penalty_sets, plug.optimizer_step

    def spy_weighted(logits, dlogits, margin, keep, partial, loss, kept, softmax=False):
        weighted(logits, dlogits, margin, keep, partial, loss, kept, softmax=softmax)
        rec["z"], rec["keep"], rec["L"], rec["kept"] = ops.from_cl(logits).cpu(), keep.cpu().clone(), loss.cpu().clone(), kept.cpu().clone()
        rec["margin"] = margin

    def spy_pen(w, g, f, source, n, sets, lam_, partial, penalty):
        rec["g"], rec["n"], rec["sets"] = g[0, :nt].cpu(), n, sets
        pen(w, g, f, source, n, sets, lam_, partial, penalty)
        rec["P"] = penalty.cpu().clone()

    def spy_step(volumes=1, fused=False):
        rec["g_pen"] = ar.grads_all[0, :nt].cpu()
        step(volumes, fused=fused)

    monkeypatch.setattr(ops, "entropy_weighted_items", spy_weighted)
    monkeypatch.setattr(ops, "fisher_penalty_sets", spy_pen)
    monkeypatch.setattr(plug, "optimizer_step", spy_step)
    res = plug.adapt_volume(x.cuda())
    w_final = ar.params_all[0, :nt].cpu()
    assert rec["n"] == nt and rec["sets"] == 1 and abs(rec["margin"] - e_margin * math.log(2.0)) < 1e-12

    def flat(values):
        out = torch.zeros(nt)
        for r in ar.refs:
            if r.trainable:
                out[r.offset:r.offset + r.numel] = values[r.name].reshape(-1)
        return out

    named = dict(ref.named_parameters())
    w0 = {n: p.detach().clone() for n, p in named.items()}
    with torch.no_grad():
        for r in ar.refs:
            named[r.name].copy_(w_start[r.offset:r.offset + r.numel].view(r.shape))
    opt = oracle.adam.build_optimizer(list(named.items()), cfg["training"])
    ref.train()
    z = ref(x)
    m = e_margin * math.log(2.0)
    H = entropy_elements(z, False)
    keep = H < m
    L = (torch.exp(m - H).detach() * H)[keep].mean()
    L.backward()
    g_plain = flat({n: p.grad for n, p in named.items()})
    assert (rec["z"] - z.detach()).abs().max().item() <= 5e-4 * z.abs().max().item()
    H64 = entropy_elements(rec["z"].double(), False)
    safe = keep_cl((H64 - m).abs() >= 1e-5, False).bool()
    assert torch.equal(rec["keep"][safe], keep_cl(H64 < m, False)[safe]), "keep mask differs on margin-safe elements"
    own = weighted_reference(rec["z"], m, False)[0][0]
    print(f"L {rec['L'].item()}, restatement on the recorded logits {own}, torch end to end {L.item()}; kept {rec['kept'].item()}")
    assert abs(rec["L"].item() - own) <= 1e-5 * abs(own)
    assert abs(rec["L"].item() - L.item()) <= 1e-4 * abs(L.item())
    assert float(res["losses"][0]) == rec["L"].item() and int(res["kept"][0]) == rec["kept"].item()
    for r in ar.refs:
        if r.trainable:
            want = named[r.name].grad.reshape(-1)
            got = rec["g"][r.offset:r.offset + r.numel]
            if feeds_norm(ref, r.name):
                wscale = named[r.name[:-len("bias")] + "weight"].grad.abs().max().item()
                assert got.abs().max().item() <= 2e-3 * wscale and want.abs().max().item() <= 2e-3 * wscale, r.name
                continue
            assert (got - want).abs().max().item() <= 2e-3 * want.abs().max().item(), r.name
    f_flat, src = flat(fisher), flat(w0)
    d = w_start.double() - src.double()
    P = lam * (f_flat.double() * d * d).sum().item()
    print(f"P {rec['P'][0].item()}, float64 {P}")
    assert P > 0 and abs(rec["P"][0].item() - P) <= 1e-5 * P and float(res["penalty"][0]) == rec["P"][0].item()
    want = (rec["g"].double() + 2.0 * lam * f_flat.double() * d).float()
    assert ((rec["g_pen"] - want).abs() <= 1e-6 * want.abs() + 1e-7 * rec["g"].abs().max()).all()
    # torch end to end: the penalty through autograd, Adam's first step
    pen_t = lam * sum((fisher[n] * (p - w0[n]) ** 2).sum() for n, p in named.items())
    pen_t.backward()
    opt.step()
    w2 = flat({n: p.detach() for n, p in named.items()})
    moved = (w_final - w2).abs()
    assert not torch.equal(w_final, w_start)
    assert (moved <= 1e-6 * w2.abs() + 1e-7).float().mean().item() >= 0.99


# ----------------------------------------------------------------------------- bit for bit
def fisher_of(hip_cfg=SMALL):
    ref, _ = build_pair(hip_cfg)
    return {"volumes": 2, "fisher": fisher_reference(ref, [volume(i)[0] for i in (10, 11)])}


def test_eata_group_equals_one_volume_at_a_time_and_graph_equals_eager():
    from multimodal_tta_amd.registry import get_plugin
    G = 3
    vols = [volume(i)[0] for i in range(G)]
    state = fisher_of()
    keys = ("losses", "kept", "penalty")
    runs = {}
    for group, use_graph in ((G, True), (1, True), (G, False)):
        cfg = eata_cfg(SMALL, steps=3, lr=1e-3, e_margin=0.6, lam=1e4, group=group, tune_volumes=4, use_graph=use_graph)
        _, hip = build_pair(SMALL)
        plug = get_plugin("eata_tta")(cfg).setup(hip, "cuda")
        plug.load_fisher(state)
        if group == G:
            r = plug.adapt_volume(torch.cat(vols).cuda())
            runs[(group, use_graph)] = (plug.logits(r).cpu(),) + tuple(r[k].cpu() for k in keys)
        else:
            rs = []
            for v in vols:          # (the results are views of the plugin's buffers: read before the next volume)
                r = plug.adapt_volume(v.cuda())
                rs.append({"z": plug.logits(r).cpu(), **{k: r[k].cpu().clone() for k in keys}})
            runs[(group, use_graph)] = (torch.cat([r["z"] for r in rs]),) + tuple(torch.stack([r[k] for r in rs], 1) for k in keys)
    assert (runs[(G, True)][3][1:] > 0).all() and (runs[(G, True)][3][0] == 0).all(), "the penalty is not in the run"
    for a, b in zip(runs[(G, True)], runs[(1, True)]):
        assert torch.equal(a, b), "grouped run differs from one volume at a time"
    for a, b in zip(runs[(G, True)], runs[(G, False)]):
        assert torch.equal(a, b), "graph replay differs from eager launches"


def test_lambda_zero_needs_no_fisher_and_launches_no_penalty_pass(monkeypatch):
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.registry import get_plugin
    cfg = eata_cfg(SMALL, steps=2, lr=1e-3, lam=0.0, group=1)
    _, hip = build_pair(SMALL)
    plug = get_plugin("eata_tta")(cfg).setup(hip, "cuda")
    assert not plug.needs_fisher and plug.fisher is None

    def refuse(*a, **k):
        raise AssertionError("the penalty pass was launched")

    monkeypatch.setattr(ops, "fisher_penalty_sets", refuse)
    res = plug.adapt_volume(volume(0)[0].cuda())
    assert torch.all(res["penalty"] == 0) and torch.isfinite(res["losses"]).all() and (res["kept"] > 0).all()


def test_adapting_without_a_fisher_estimate_raises():
    from multimodal_tta_amd.ops import MmttaError
    from multimodal_tta_amd.registry import get_plugin
    cfg = eata_cfg(SMALL, steps=1, group=1)
    _, hip = build_pair(SMALL)
    plug = get_plugin("eata_tta")(cfg).setup(hip, "cuda")
    with pytest.raises(MmttaError, match="estimate_fisher.*method.eata.fisher.path"):
        plug.adapt_volume(volume(0)[0].cuda())
    with pytest.raises(MmttaError, match="stem.weight|missing|no entry"):
        plug.load_fisher({"volumes": 2, "fisher": {}})


@pytest.mark.parametrize("episodic", [True, False])
def test_episodic_false_carries_the_weights_to_the_next_volume(episodic):
    from multimodal_tta_amd.registry import get_plugin
    cfg = eata_cfg(SMALL, steps=2, lr=1e-3, lam=1e4, group=1, episodic=episodic)
    _, hip = build_pair(SMALL)
    plug = get_plugin("eata_tta")(cfg).setup(hip, "cuda")
    plug.load_fisher(fisher_of())
    span = plug.fisher.clone()
    first = plug.adapt_volume(volume(0)[0].cuda())
    assert float(first["penalty"][0]) == 0.0 and float(first["penalty"][1]) > 0.0
    second = plug.adapt_volume(volume(1)[0].cuda())
    if episodic:
        assert float(second["penalty"][0]) == 0.0
    else:
        assert float(second["penalty"][0]) > 0.0
    assert torch.equal(plug.fisher, span), "F moved while volumes adapted"


def test_seg_tta_eval_with_tta_eata_shares_one_fisher_span_and_sees_every_volume_once(tmp_path):
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_dataset_builder, get_evaluation_strategy

    def run(path=None):
        cfg = compose(overrides=["task=brats", "model=unet", "method=tta_eata", "method.steps=2", "method.lanes=2",
                                 "method.group=2", "method.eata.fisher.volumes=3"])
        cfg["model"] = dict(SMALL)
        cfg["method"]["eata"]["fisher"]["path"] = path
        cfg["dataset"]["synthetic"]["num_volumes"] = 7
        cfg["dataset"]["synthetic"]["shape"] = [32, 32, 32]
        cfg["training"]["eval_batch_size"] = 2
        _, hip = build_pair(SMALL)
        loader = get_dataset_builder("brats")(cfg).get_loader("test")
        strat = get_evaluation_strategy("seg_tta_eval")(cfg)
        m = strat.evaluate_epoch(hip, loader, torch.device("cuda"))
        return strat, m

    strat, m = run()
    assert type(strat.plugin).__name__ == "FisherRegularizedTTA" and len(strat.plugins) == 2
    assert strat.plugin.fisher_count == 3 and float(strat.plugin.fisher.max()) > 0.0
    assert all(p.fisher is strat.plugin.fisher for p in strat.plugins), "the lanes do not share one Fisher span"
    assert strat.last_table[:, 0].tolist() == [float(i) for i in range(7)], "every volume once and in order"
    assert {"et_dc", "tc_dc", "wt_dc", "avg_dc", "loss"} <= set(m) and 0.0 <= m["avg_dc"] <= 1.0
    path = str(tmp_path / "fisher.pt")
    torch.save(strat.plugin.fisher_state(), path)
    again, m2 = run(path)          # the same estimate from the file: the same evaluation
    assert torch.equal(again.plugin.fisher, strat.plugin.fisher) and again.plugin.fisher_count == 3
    assert torch.equal(again.last_table, strat.last_table) and m2 == m
