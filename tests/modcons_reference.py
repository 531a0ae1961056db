"""Torch restatement of the modality-consistency objective (``modcons_tta``, ``mmtta_modcons_loss_items``) for the tests:
the views as a masked copy, the per-volume terms with autograd (``.detach()`` makes the full view a teacher), the closed-form
gradients the kernels implement, and the adaptation loop on the oracle networks.  Pure torch, any dtype, CPU."""
import torch
import torch.nn.functional as F


def masked_views(x, keep_masks):
    """x [G,C,D,H,W] -> [G*V,C,D,H,W], item g*V+v = volume g with channel c kept iff bit c of keep_masks[v] (else +0)."""
    C = x.shape[1]
    views = []
    for m in keep_masks:
        keep = torch.tensor([bool((m >> c) & 1) for c in range(C)]).view(1, C, 1, 1, 1)
        views.append(torch.where(keep, x, torch.zeros_like(x)))
    return torch.stack(views, 1).reshape(-1, *x.shape[1:])


def hard(z, softmax):
    """(z >= 0) on the sigmoid head, the first arg max on the softmax head (torch.argmax returns the first maximum)."""
    return z.argmax(1) if softmax else z >= 0


def modcons_terms(z, V, softmax, detach=True):
    """z [G*V,R,D,H,W] (item g*V+v = view v of volume g) -> entropy [G], view_kl [G,V-1] (both differentiable) and disagree
    [G,V-1] (int64): H_g = mean H(p_0), K_g,v = mean KL(p_0 || p_v) with the elements (voxel, region) pairs (sigmoid head) or
    voxels (softmax head); ``detach``: p_0 enters the KL as a constant."""
    G = z.shape[0] // V
    zs = z.reshape(G, V, *z.shape[1:])
    z0 = zs[:, 0]
    t0 = z0.detach() if detach else z0
    if softmax:
        l0, lt = F.log_softmax(z0, 1), F.log_softmax(t0, 1)
        entropy = (-(l0.exp() * l0).sum(1)).flatten(1).mean(1)
    else:
        entropy = (-(torch.sigmoid(z0) * F.logsigmoid(z0) + torch.sigmoid(-z0) * F.logsigmoid(-z0))).flatten(1).mean(1)
    kls, dis = [], []
    for v in range(1, V):
        zv = zs[:, v]
        if softmax:
            kl = (lt.exp() * (lt - F.log_softmax(zv, 1))).sum(1)
        else:
            kl = (torch.sigmoid(t0) * (F.logsigmoid(t0) - F.logsigmoid(zv))
                  + torch.sigmoid(-t0) * (F.logsigmoid(-t0) - F.logsigmoid(-zv)))
        kls.append(kl.flatten(1).mean(1))
        dis.append((hard(zv.detach(), softmax) != hard(z0.detach(), softmax)).flatten(1).sum(1))
    return entropy, torch.stack(kls, 1), torch.stack(dis, 1)


def modcons_loss(z, V, softmax, weight=1.0, entropy_weight=1.0, detach=True):
    """Per-volume L_g = w_e H_g + lambda C_g [G] (differentiable), and the terms."""
    entropy, view_kl, disagree = modcons_terms(z, V, softmax, detach)
    consistency = view_kl.mean(1)
    return entropy_weight * entropy + weight * consistency, entropy, consistency, view_kl, disagree


def loss_reference(z, V, softmax, weight=1.0, entropy_weight=1.0, detach=True):
    """float64 autograd: dict of loss, entropy, consistency [G], view_kl, disagree [G,V-1] and grad (z's shape)."""
    z = z.double().detach().requires_grad_(True)
    loss, entropy, consistency, view_kl, disagree = modcons_loss(z, V, softmax, weight, entropy_weight, detach)
    loss.sum().backward()
    return {"loss": loss.detach(), "entropy": entropy.detach(), "consistency": consistency.detach(),
            "view_kl": view_kl.detach(), "disagree": disagree, "grad": z.grad}


def closed_form_grad(z, V, softmax, weight=1.0, entropy_weight=1.0, detach=True):
    """dL/dz as the kernels write it (the issue's formulas), in z's dtype:
        v >= 1:  lambda / ((V-1) n) (p_v - p_0)
        v == 0:  w_e / n dH/dz_0 + (detach ? 0 : lambda / ((V-1) n) sum_v dKL(p_0 || p_v)/dz_0)
                 Bernoulli dKL/dz_0 = p_0 (1 - p_0)(z_0 - z_v);  categorical p_0,k [(log p_0,k - log p_v,k) - KL_i]."""
    G = z.shape[0] // V
    zs = z.reshape(G, V, *z.shape[1:])
    z0 = zs[:, 0]
    n = z0[0].numel() // (z0.shape[1] if softmax else 1)
    cc = weight / ((V - 1) * n)
    g = torch.zeros_like(zs)
    if softmax:
        l0 = F.log_softmax(z0, 1)
        p0 = l0.exp()
        H = -(p0 * l0).sum(1, keepdim=True)
        g[:, 0] = entropy_weight / n * (-p0 * (l0 + H))
        for v in range(1, V):
            lv = F.log_softmax(zs[:, v], 1)
            g[:, v] = cc * (lv.exp() - p0)
            if not detach:
                d = l0 - lv
                g[:, 0] += cc * p0 * (d - (p0 * d).sum(1, keepdim=True))
    else:
        p0 = torch.sigmoid(z0)
        pq = p0 * torch.sigmoid(-z0)
        g[:, 0] = entropy_weight / n * (-z0 * pq)
        for v in range(1, V):
            g[:, v] = cc * (torch.sigmoid(zs[:, v]) - p0)
            if not detach:
                g[:, 0] += cc * pq * (z0 - zs[:, v])
    return g.reshape(z.shape)


def modcons_reference(model, x, train_cfg, steps, keep_masks, params="all", softmax=False, weight=1.0, entropy_weight=1.0,
                      detach=True):
    """The adaptation loop with torch autograd, one volume: the views (``keep_masks[0]`` = the present modalities) are one
    batch on the one weight set, train-mode norms; the returned logits are the eval forward of view 0."""
    import oracle
    from oracle.tta import select_params
    named = select_params(model, params)
    chosen = {id(p) for _, p in named}
    for p in model.parameters():
        p.requires_grad_(id(p) in chosen)
    opt = oracle.adam.build_optimizer(named, train_cfg)
    V = len(keep_masks)
    xv = masked_views(x, keep_masks)
    out = {"losses": [], "entropy": [], "consistency": [], "view_kl": [], "disagree": []}
    model.train()
    for _ in range(steps):
        opt.zero_grad()
        loss, entropy, consistency, view_kl, disagree = modcons_loss(model(xv), V, softmax, weight, entropy_weight, detach)
        loss[0].backward()
        opt.step()
        out["losses"].append(float(loss[0].detach()))
        out["entropy"].append(float(entropy[0].detach()))
        out["consistency"].append(float(consistency[0].detach()))
        out["view_kl"].append(view_kl[0].detach().clone())
        out["disagree"].append(disagree[0].clone())
    model.eval()
    with torch.no_grad():
        out["logits"] = model(xv[:1])
    for p in model.parameters():
        p.requires_grad_(True)
    return out
