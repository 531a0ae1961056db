"""DeYO adaptation (``deyo_tta``) on the GPU: the patch shuffle against a torch index restatement, the PLPD-weighted entropy
against a float64 restatement, the plugin against a DeYO restatement with torch autograd on the oracle networks, and the
bitwise properties (grouped = one volume at a time, graph = eager, N items = N calls).

The reference ships no adaptation code, so the semantics are restated here: per step z' = f(shuffle(x)) without gradient,
z = f(x), z''(v) = z' where the content of voxel v went, PLPD = p(z)[y^] - p(z'')[y^], keep = (H < e_margin ln K) and
(PLPD > threshold), a = exp(e_margin0 ln K - H) + exp(PLPD) without gradient, L = sum_keep a H / |keep|.

Inputs of the kernel tests are seeded so that no element lies within 1e-5 of either threshold in float64 (the rule DESIGN.md
section 6 applies to the ReLU threshold): masks and counts must then agree exactly."""
import copy
import functools
import math

import pytest
import torch

from test_hip_eata import HEADS, SATURATED, masks_of
from test_hip_sar import BATCH, SECOND_TRIP, SECOND_TRIP_SHAPE, entropy_elements, grad_buffer, keep_cl, run_filtered, stage
from test_hip_tta import SMALL, build_pair, root_cfg, volume

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- the shuffle, restated with torch indexing
def patch_index(shape, grid, perm):
    """idx [D*H*W] with shuffled.flat[v] = volume.flat[idx[v]]: destination slot j (row-major over the grid) holds source patch
    perm[j].  With the inverse permutation it is the un-shuffle: where the content of voxel v went."""
    D, H, W = shape
    gd, gh, gw = grid
    pd, ph, pw = D // gd, H // gh, W // gw
    z, y, x = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij")
    slot = ((z // pd) * gh + y // ph) * gw + x // pw
    s = torch.as_tensor(perm, dtype=torch.int64)[slot]
    sz, sy, sx = s // (gw * gh), (s // gw) % gh, s % gw
    return (((sz * pd + z % pd) * H + sy * ph + y % ph) * W + sx * pw + x % pw).reshape(-1)


def inverse(perm):
    inv = [0] * len(perm)
    for j, s in enumerate(perm):
        inv[s] = j
    return inv


def shuffle_ncdhw(x, grid, perms, invert=False):
    """[N,C,D,H,W] -> every item's patches permuted by its permutation (``invert``: the un-shuffle)."""
    out = torch.empty_like(x)
    for n, perm in enumerate(perms):
        idx = patch_index(x.shape[2:], grid, inverse(perm) if invert else perm)
        out[n] = x[n].flatten(1)[:, idx].view_as(x[n])
    return out


def random_perms(N, P, gen):
    return [torch.randperm(P, generator=gen).tolist() for _ in range(N)]


def device_table(perms):
    from multimodal_tta_amd import ops
    return ops.patch_table(perms).cuda()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [4, 2, 1])
@pytest.mark.parametrize("grid", [[2, 3, 2], [1, 2, 4], [4, 1, 1]])
def test_patch_shuffle_is_bit_exact_with_its_pad_lanes(grid, C, dtype):
    from multimodal_tta_amd import ops
    N, D, H, W, ldc = 3, 4, 6, 8, 4
    gen = torch.Generator().manual_seed(11 * C + grid[0])
    perms = random_perms(N, grid[0] * grid[1] * grid[2], gen)
    assert len({tuple(p) for p in perms}) == N, "a different permutation per item"
    base = torch.randn((N, D, H, W, ldc), generator=gen).to(dtype)
    x = ops.new_cl(N, D, H, W, C, "cuda", ldc=ldc, dtype=dtype)
    y = ops.new_cl(N, D, H, W, C, "cuda", ldc=ldc, dtype=dtype)
    xb, yb = (x if x._base is None else x._base), (y if y._base is None else y._base)
    xb.copy_(base)
    yb.fill_(float("nan"))
    ops.patch_shuffle(x, y, grid, device_table(perms))
    torch.cuda.synchronize()
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    got = yb.cpu().view(bits)
    for n in range(N):
        want = base[n].reshape(-1, ldc)[patch_index((D, H, W), grid, perms[n])].view(bits)      # whole rows, pad lanes included
        assert torch.equal(got[n].reshape(-1, ldc), want), f"item {n}"
    assert torch.equal(xb.cpu().view(bits), base.view(bits)), "the input moved"
    # the restatement on the logical tensor: shuffle, then un-shuffle, is the identity
    xs = shuffle_ncdhw(base[..., :C].permute(0, 4, 1, 2, 3).float(), grid, perms)
    assert torch.equal(ops.from_cl(y.float()).cpu(), xs)
    assert torch.equal(shuffle_ncdhw(xs, grid, perms, invert=True), base[..., :C].permute(0, 4, 1, 2, 3).float())


def test_patch_shuffle_refuses_an_in_place_call_and_a_bad_table():
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.ops import MmttaError
    x = ops.new_cl(1, 4, 4, 4, 4, "cuda")
    y = ops.new_cl(1, 4, 4, 4, 4, "cuda")
    table = device_table([[1, 0]])
    with pytest.raises(MmttaError, match="in-place"):
        ops.patch_shuffle(x, x, [2, 1, 1], table)
    with pytest.raises(MmttaError, match="table"):
        ops.patch_shuffle(x, y, [2, 2, 1], table)          # 4 patches, a table of 2
    with pytest.raises(MmttaError, match="table"):
        ops.patch_shuffle(x, y, [2, 1, 1], table.cpu())
    with pytest.raises(MmttaError, match="does not divide"):
        ops.patch_shuffle(x, y, [3, 1, 1], device_table([[1, 0, 2]]))


# ----------------------------------------------------------------------------- float64 restatement of the loss kernel
def plpd_elements(z, z2, softmax):
    """p(z)[y^] - p(z2)[y^] per element, y^ the hard prediction of z (the first arg max for the softmax head)."""
    if softmax:
        arg = z.argmax(1, keepdim=True)
        return (torch.softmax(z, 1).gather(1, arg) - torch.softmax(z2, 1).gather(1, arg)).squeeze(1)
    s = torch.where(z >= 0, 1.0, -1.0).to(z.dtype)
    return torch.sigmoid(z.abs()) - torch.sigmoid(s * z2)


def deyo_terms(z, zs, grid, perms, margin, margin0, thr, softmax):
    """H, PLPD, keep1, keep and the weight a (detached) of logits z against the shuffled volume's logits zs."""
    z2 = shuffle_ncdhw(zs.detach(), grid, perms, invert=True)
    H = entropy_elements(z, softmax)
    plpd = plpd_elements(z.detach(), z2, softmax)
    keep1 = H.detach() < margin
    keep = keep1 & (plpd > thr)
    a = (torch.exp(margin0 - H) + torch.exp(plpd)).detach()
    return H, plpd, keep1, keep, a


def deyo_kernel_reference(z, zs, grid, perms, margin, margin0, thr, softmax):
    """Per item: loss, kept, kept_entropy, keep mask and d(loss)/dz in float64."""
    z = z.double().detach().requires_grad_(True)
    H, _, keep1, keep, a = deyo_terms(z, zs.double(), grid, perms, margin, margin0, thr, softmax)
    losses, kept, kept_entropy = [], [], []
    total = 0.0
    for n in range(z.shape[0]):
        cnt = int(keep[n].sum())
        kept.append(cnt)
        kept_entropy.append(int(keep1[n].sum()))
        if cnt:
            ln = (a[n] * H[n])[keep[n]].sum() / cnt
            total = total + ln
            losses.append(float(ln.detach()))
        else:
            losses.append(float("nan"))
    if torch.is_tensor(total):
        total.backward()
        grad = z.grad
    else:
        grad = torch.zeros_like(z)
    return losses, kept, kept_entropy, keep, grad


def away_from_thresholds(z, zs, grid, perms, margin, thr, softmax, gen):
    """Resample the logits of the elements whose entropy lies within 1e-5 of the margin or whose PLPD within 1e-5 of the
    threshold (float64)."""
    for _ in range(20):
        H = entropy_elements(z.double(), softmax)
        plpd = plpd_elements(z.double(), shuffle_ncdhw(zs.double(), grid, perms, invert=True), softmax)
        near = ((H - margin).abs() < 1e-5) | ((plpd - thr).abs() < 1e-5)
        if not near.any():
            return z
        if softmax:
            near = near.unsqueeze(1).expand_as(z)
        z = torch.where(near, torch.randn(z.shape, generator=gen) * 3.0, z)
    raise AssertionError("could not seed the logits away from the thresholds")


def run_deyo(z_cl, zs_cl, grid, table, margin, margin0, thr, softmax, dtype=torch.float32):
    from multimodal_tta_amd import ops
    n, d, h, w, r = z_cl.shape
    elems = n * d * h * w * (1 if softmax else r)
    g = grad_buffer(z_cl, dtype)
    keep = torch.full((elems,), 7, dtype=torch.uint8, device="cuda")
    partial = torch.empty(ops.deyo_partials(z_cl), dtype=torch.float64, device="cuda")
    loss = torch.full((n,), 123.0, device="cuda")
    kept = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    kept_entropy = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    ops.deyo_loss_items(z_cl, zs_cl, g, grid, table, margin, margin0, thr, keep, partial, loss, kept, kept_entropy, softmax=softmax)
    torch.cuda.synchronize()
    return loss.cpu(), kept.cpu(), kept_entropy.cpu(), keep.cpu(), ops.from_cl(g.float()).cpu()


GRID = [2, 1, 3]          # of the (6, 7, 9) logits of the kernel tests
E_MARGIN, E_MARGIN0, THRESHOLD = 0.5, 0.4, 0.2


def kernel_case(softmax, R, N, seed=0):
    gen = torch.Generator().manual_seed(seed)
    lnk = math.log(R if softmax else 2.0)
    margin, margin0 = E_MARGIN * lnk, E_MARGIN0 * lnk
    perms = random_perms(N, GRID[0] * GRID[1] * GRID[2], gen)
    z = torch.randn((N, R, 6, 7, 9), generator=gen) * 3.0
    zs = torch.randn((N, R, 6, 7, 9), generator=gen) * 3.0
    z = away_from_thresholds(z, zs, GRID, perms, margin, THRESHOLD, softmax, gen)
    return z, zs, perms, margin, margin0


@pytest.mark.parametrize("softmax,R,generic", HEADS)
@pytest.mark.parametrize("N", [1, 3])
def test_deyo_loss_matches_float64_and_the_filtered_count(softmax, R, generic, N):
    """Loss 1e-5 relative, the gradient 2e-5 of its maximum, bf16 gradients within 2^-7 relative of the rounded fp32 ones, zero
    gradient off the mask, masks and both counts exact; kept_entropy is mmtta_entropy_filtered_items' kept, bit for bit.  The
    filters must be exercised: the entropy-kept share in [0.2, 0.8], the final share >= 0.2, the PLPD filter removing >= 5 % of
    all elements.  The restatement's figures for these inputs (entropy share / final share / removed): sigmoid heads
    0.48-0.51 / 0.31-0.33 / 17-18 %; softmax R = 3 0.59-0.64 / 0.45-0.52 / 12-14 %, R = 4 0.61 / 0.50-0.51 / 10-11 %."""
    z, zs, perms, margin, margin0 = kernel_case(softmax, R, N)
    l_ref, k_ref, k1_ref, m_ref, g_ref = deyo_kernel_reference(z, zs, GRID, perms, margin, margin0, THRESHOLD, softmax)
    elems = float(m_ref.numel())
    share1, share = sum(k1_ref) / elems, sum(k_ref) / elems
    print(f"entropy-kept share {share1:.3f}, final share {share:.3f}, removed by PLPD {share1 - share:.3f}")
    assert 0.2 <= share1 <= 0.8 and share >= 0.2 and share1 - share >= 0.05, "the filters are not exercised"
    z_cl, zs_cl, table = stage(z, generic), stage(zs, generic), device_table(perms)
    _, f_kept, f_keep, _ = run_filtered(z_cl, margin, softmax)
    fp32 = None
    for dtype in ((torch.float32, torch.bfloat16) if (not softmax and not generic) else (torch.float32,)):
        loss, kept, kept_entropy, keep, g = run_deyo(z_cl, zs_cl, GRID, table, margin, margin0, THRESHOLD, softmax, dtype=dtype)
        assert torch.equal(keep, keep_cl(m_ref, softmax)), "keep masks differ from float64"
        assert kept.tolist() == k_ref and kept_entropy.tolist() == k1_ref
        assert torch.equal(kept_entropy, f_kept), "kept_entropy differs from mmtta_entropy_filtered_items' kept"
        assert not torch.any(keep.bool() & ~f_keep.bool()), "an element was kept that the entropy filter drops"
        for a, b in zip(loss.tolist(), l_ref):
            assert abs(a - b) <= 1e-5 * abs(b), (a, b)
        if dtype == torch.float32:
            fp32 = g
            assert (g.double() - g_ref).abs().max().item() <= 2e-5 * g_ref.abs().max().item()
        else:
            want = fp32.to(torch.bfloat16).float()          # the fp32 result rounded, to 1 ulp of bf16 (2^-7 relative)
            assert ((g - want).abs() <= 2.0 ** -7 * want.abs()).all()
        assert torch.all(g[~(m_ref.unsqueeze(1).expand_as(g) if softmax else m_ref)] == 0)


SECOND_TRIP_GRID = [3, 1, 1]          # of the 81^3 logits of test_hip_sar.SECOND_TRIP_SHAPE


@functools.lru_cache(maxsize=None)
def second_trip_case(softmax):
    """kernel_case at SECOND_TRIP_SHAPE, and the float64 reference."""
    gen = torch.Generator().manual_seed(81)
    lnk = math.log(3 if softmax else 2.0)
    margin, margin0 = E_MARGIN * lnk, E_MARGIN0 * lnk
    perms = random_perms(SECOND_TRIP_SHAPE[0], 3, gen)
    z = torch.randn(SECOND_TRIP_SHAPE, generator=gen) * 3.0
    zs = torch.randn(SECOND_TRIP_SHAPE, generator=gen) * 3.0
    z = away_from_thresholds(z, zs, SECOND_TRIP_GRID, perms, margin, THRESHOLD, softmax, gen)
    return (z, zs, perms, margin, margin0) + deyo_kernel_reference(z, zs, SECOND_TRIP_GRID, perms, margin, margin0, THRESHOLD, softmax)


@pytest.mark.parametrize("softmax,generic,dtype", SECOND_TRIP)
def test_deyo_loss_on_the_second_trip_of_the_walk(softmax, generic, dtype):
    """test_deyo_loss_matches_float64_and_the_filtered_count at test_hip_sar.SECOND_TRIP_SHAPE: more voxels than one launch has
    threads, two items, three patches along D."""
    z, zs, perms, margin, margin0, l_ref, k_ref, k1_ref, m_ref, g_ref = second_trip_case(softmax)
    elems = float(m_ref.numel())
    share1, share = sum(k1_ref) / elems, sum(k_ref) / elems
    print(f"entropy-kept share {share1:.3f}, final share {share:.3f}, removed by PLPD {share1 - share:.3f}")
    assert 0.2 <= share1 <= 0.8 and share >= 0.2 and share1 - share >= 0.05, "the filters are not exercised"
    z_cl, zs_cl, table = stage(z, generic), stage(zs, generic), device_table(perms)
    _, f_kept, f_keep, _ = run_filtered(z_cl, margin, softmax)
    loss, kept, kept_entropy, keep, g = run_deyo(z_cl, zs_cl, SECOND_TRIP_GRID, table, margin, margin0, THRESHOLD, softmax, dtype=dtype)
    assert torch.equal(keep, keep_cl(m_ref, softmax)), "keep masks differ from float64"
    assert kept.tolist() == k_ref and kept_entropy.tolist() == k1_ref
    assert torch.equal(kept_entropy, f_kept), "kept_entropy differs from mmtta_entropy_filtered_items' kept"
    assert not torch.any(keep.bool() & ~f_keep.bool()), "an element was kept that the entropy filter drops"
    for a, b in zip(loss.tolist(), l_ref):
        print(f"loss {a} vs {b}")
        assert abs(a - b) <= 1e-5 * abs(b), (a, b)
    if dtype == torch.float32:
        err = (g.double() - g_ref).abs().max().item() / g_ref.abs().max().item()
        print(f"gradient error {err:.2e} of the maximum")
        assert err <= 2e-5
    else:
        want = run_deyo(z_cl, zs_cl, SECOND_TRIP_GRID, table, margin, margin0, THRESHOLD, softmax)[4].to(torch.bfloat16).float()
        assert ((g - want).abs() <= 2.0 ** -7 * want.abs()).all()
    assert torch.all(g[~(m_ref.unsqueeze(1).expand_as(g) if softmax else m_ref)] == 0)


@pytest.mark.parametrize("softmax,R,generic,dtype", [(False, 3, False, torch.float32), (False, 3, False, torch.bfloat16),
                                                     (False, 3, True, torch.float32), (True, 4, False, torch.float32)])
def test_deyo_n_items_equal_n_single_item_calls(softmax, R, generic, dtype):
    N = 3
    z, zs, perms, margin, margin0 = kernel_case(softmax, R, N, seed=5)
    args = (margin, margin0, THRESHOLD, softmax)
    together = run_deyo(stage(z, generic), stage(zs, generic), GRID, device_table(perms), *args, dtype=dtype)
    per = z[0:1].numel() // R * (1 if softmax else R)
    for n in range(N):
        one = run_deyo(stage(z[n:n + 1], generic), stage(zs[n:n + 1], generic), GRID, device_table(perms[n:n + 1]), *args, dtype=dtype)
        for i in (0, 1, 2, 4):
            assert torch.equal(one[i], together[i][n:n + 1]), (n, i)
        assert torch.equal(one[3], together[3][n * per:(n + 1) * per])


def saturated_logits(N, R, gen):
    pick = torch.randint(0, len(SATURATED), (N, R, 6, 7, 9), generator=gen)
    return torch.tensor(SATURATED)[pick]


@pytest.mark.parametrize("softmax,R,generic", HEADS)
def test_deyo_loss_is_finite_on_saturated_logits(softmax, R, generic):
    gen = torch.Generator().manual_seed(21)
    z, zs = saturated_logits(2, R, gen), saturated_logits(2, R, gen)
    lnk = math.log(R if softmax else 2.0)
    perms = random_perms(2, 6, gen)
    loss, kept, kept_entropy, keep, g = run_deyo(stage(z, generic), stage(zs, generic), GRID, device_table(perms), E_MARGIN * lnk,
                                                 E_MARGIN0 * lnk, THRESHOLD, softmax)
    assert torch.isfinite(g).all() and torch.isfinite(loss).all() and (kept > 0).all() and (kept <= kept_entropy).all()
    # a <= e^margin0 + e, H < margin on the mask
    assert (loss >= 0).all() and (loss <= E_MARGIN * lnk * (math.exp(E_MARGIN0 * lnk) + math.e)).all()


@pytest.mark.parametrize("softmax,R,generic", HEADS)
def test_the_identity_permutation_on_equal_logits_keeps_nothing(softmax, R, generic):
    """PLPD = p(z)[y^] - p(z)[y^] = 0 exactly: nothing passes the threshold 0.2; NaN loss, zero gradient, while the entropy
    count is the filtered entry point's."""
    gen = torch.Generator().manual_seed(9)
    z = torch.randn((2, R, 6, 7, 9), generator=gen) * 3.0
    lnk = math.log(R if softmax else 2.0)
    z_cl = stage(z, generic)
    table = device_table([list(range(6))] * 2)
    loss, kept, kept_entropy, keep, g = run_deyo(z_cl, z_cl, GRID, table, E_MARGIN * lnk, E_MARGIN0 * lnk, THRESHOLD, softmax)
    assert torch.isnan(loss).all() and kept.tolist() == [0, 0] and torch.all(keep == 0) and torch.all(g == 0)
    assert torch.equal(kept_entropy, run_filtered(z_cl, E_MARGIN * lnk, softmax)[1]) and (kept_entropy > 0).all()
    # ... and everything below the entropy margin at a threshold below 0
    _, kept, kept_entropy, _, _ = run_deyo(z_cl, z_cl, GRID, table, E_MARGIN * lnk, E_MARGIN0 * lnk, -0.5, softmax)
    assert torch.equal(kept, kept_entropy)


# ----------------------------------------------------------------------------- the DeYO restatement (torch autograd)
PATCHES = [2, 2, 2]


def bf16_proxy(model):
    """A copy with its convolution weights rounded to bf16: the reference-side proxy of the bf16 path's operand rounding."""
    m = copy.deepcopy(model)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 5:
                p.copy_(p.to(torch.bfloat16).to(p.dtype))
    return m


def deyo_reference(model, xs, ordinals, train_cfg, steps, e_margin, e_margin0, thr, patches=PATCHES, seed=0, softmax=False,
                   missing=()):
    """DeYO with torch autograd over the volumes ``xs`` (episodic): per volume the final logits and the per-step L, kept,
    kept_entropy."""
    import oracle
    from multimodal_tta_amd.deyo import draw_permutation
    named = list(model.named_parameters())
    source = copy.deepcopy(model.state_dict())
    P = patches[0] * patches[1] * patches[2]
    out = []
    for x, ordinal in zip(xs, ordinals):
        model.load_state_dict(source)
        opt = oracle.adam.build_optimizer(named, train_cfg)
        if missing:
            keep_c = torch.ones(x.shape[1], dtype=x.dtype)
            keep_c[list(missing)] = 0.0
            x = x * keep_c.view(1, -1, 1, 1, 1)
        perms = [draw_permutation(seed, ordinal, P)]
        x_shuf = shuffle_ncdhw(x, patches, perms)
        rec = {"losses": [], "kept": [], "kept_entropy": []}
        model.train()
        for _ in range(steps):
            opt.zero_grad()
            with torch.no_grad():
                zs = model(x_shuf)
            z = model(x)
            lnk = math.log(z.shape[1] if softmax else 2.0)
            H, _, keep1, keep, a = deyo_terms(z, zs, patches, perms, e_margin * lnk, e_margin0 * lnk, thr, softmax)
            cnt = int(keep.sum())
            loss = (a * H)[keep].sum() / cnt if cnt else torch.full((), float("nan"))
            if cnt:
                loss.backward()
            opt.step()
            rec["losses"].append(float(loss.detach()))
            rec["kept"].append(cnt)
            rec["kept_entropy"].append(int(keep1.sum()))
        model.eval()
        with torch.no_grad():
            rec["logits"] = model(x)
        out.append(rec)
    return out


def deyo_cfg(model_cfg, steps=3, lr=None, e_margin=0.8, e_margin0=0.6, thr=0.05, patches=PATCHES, seed=0, **method):
    """``lr=None``: the configured learning rate (the reference's, 1e-5)."""
    from multimodal_tta_amd.config import compose
    cfg = root_cfg(model_cfg, steps=steps, lr=1e-3 if lr is None else lr, **method)
    if lr is None:
        cfg["training"]["optimizers"]["adam"]["lr"] = compose(overrides=["task=brats", "model=unet"])["training"]["optimizers"]["adam"]["lr"]
    cfg["method"]["name"] = "deyo_tta"
    cfg["method"]["deyo"] = {"e_margin": e_margin, "e_margin0": e_margin0, "plpd_threshold": thr, "patches": list(patches),
                             "seed": seed}
    return cfg


def check_against_reference(z_hip, res, o32, o64, y, elements, softmax=False, bf16=False, o16=None):
    """EATA's bounds (tests/test_hip_eata.py::check_against_reference) with the two counts in P's place.  fp32, at the
    reference's learning rate: per-step L within 1e-4 relative (+1e-6) and both counts within 1e-4 of the element count of
    the float64 restatement, or 3x as far as the fp32 restatement sits from it; final logits within max(5e-3, 3x fp32's
    distance) of max|logits|; mask voxels differing only where the float64 logit is within that bound of the threshold; Dice
    2e-3.  The float64 restatement must show the PLPD filter at work: kept_entropy - kept >= 1 % of the elements at every step
    (100x the count tolerance).  bf16: against the fp32 restatement L 1e-2 relative, kept_entropy 1e-2 of the elements,
    logits 3e-2, masks 1e-2, Dice 2e-2; kept - the difference of two forwards decides it - within max(1e-2 of the elements,
    3 d), d the distance in kept between the fp32 restatement and the same restatement with its input and convolution weights
    rounded to bf16 (``o16``)."""
    import oracle
    steps = len(o32["losses"])
    losses, kept = res["losses"].cpu().reshape(-1).tolist(), res["kept"].cpu().reshape(-1).tolist()
    kent = res["kept_entropy"].cpu().reshape(-1).tolist()

    def dice(m):
        return oracle.binary_dice_iou(m.to(torch.uint8), (y > 0.5).to(torch.uint8))[0]

    z32 = o32["logits"]
    if bf16:
        for t in range(steps):
            a, b = losses[t], o32["losses"][t]
            assert abs(a - b) <= 1e-2 * abs(b), f"step {t}: L {a} vs reference {b}"
            assert abs(kent[t] - o32["kept_entropy"][t]) <= 1e-2 * elements, f"step {t}: kept_entropy {kent[t]} vs {o32['kept_entropy'][t]}"
            d = abs(o16["kept"][t] - o32["kept"][t])
            print(f"step {t}: kept {kept[t]}, fp32 restatement {o32['kept'][t]}, bf16-rounded restatement {o16['kept'][t]} (d = {d}), "
                  f"observed distance {abs(kept[t] - o32['kept'][t])} of {elements} elements")
            assert abs(kept[t] - o32["kept"][t]) <= max(1e-2 * elements, 3.0 * d), f"step {t}: kept {kept[t]} vs {o32['kept'][t]} (d = {d})"
        err = (z_hip - z32).abs().max().item() / z32.abs().max().item()
        mism = (masks_of(z_hip, softmax) != masks_of(z32, softmax)).float().mean().item()
        ddice = (dice(masks_of(z_hip, softmax)) - dice(masks_of(z32, softmax))).abs().max().item()
        print(f"bf16: L {losses} kept {kept} kept_entropy {kent}; logits {err:.2e}, masks {mism:.2e}, Dice {ddice:.2e}")
        assert err > 1e-6, "bf16 path not taken"
        assert err <= 3e-2 and mism <= 1e-2 and ddice <= 2e-2, (err, mism, ddice)
        return 3e-2
    for t in range(steps):
        gap = (o64["kept_entropy"][t] - o64["kept"][t]) / float(elements)
        print(f"step {t}: float64 restatement keeps {o64['kept_entropy'][t] / float(elements):.4f} by entropy, "
              f"{o64['kept'][t] / float(elements):.4f} after the PLPD filter")
        assert gap >= 0.01, f"step {t}: the PLPD filter removes {gap:.4f} of the elements: the case does not exercise it"
        a, b, c = losses[t], o32["losses"][t], o64["losses"][t]
        assert abs(a - c) <= max(1e-4 * abs(c) + 1e-6, 3.0 * abs(b - c)), f"step {t}: L {a}, fp32 {b}, fp64 {c}"
        for name, got in (("kept", kept), ("kept_entropy", kent)):
            a, b, c = got[t], o32[name][t], o64[name][t]
            assert abs(a - c) <= max(1e-4 * elements, 3.0 * abs(b - c)), f"step {t}: {name} {a}, fp32 {b}, fp64 {c}"
    z64 = o64["logits"]
    scale = z64.abs().max().item()
    e_ref = (z32.double() - z64).abs().max().item() / scale
    e_hip = (z_hip.double() - z64).abs().max().item() / scale
    bound = max(5e-3, 3.0 * e_ref)
    assert e_hip <= bound, f"HIP vs fp64 DeYO {e_hip:.3e}; fp32 DeYO vs fp64 DeYO {e_ref:.3e}"
    m_hip, m32, m64 = masks_of(z_hip, softmax), masks_of(z32, softmax), masks_of(z64, softmax)
    if not softmax:
        near = z64.abs() <= bound * scale
        assert not torch.any((m_hip != m64) & ~near), "a mask voxel differs away from the threshold"
    d64 = dice(m64)
    dd_hip, dd_ref = (dice(m_hip) - d64).abs().max().item(), (dice(m32) - d64).abs().max().item()
    assert dd_hip <= max(2e-3, 3.0 * dd_ref), (dd_hip, dd_ref)
    print(f"L {losses} kept {kept} kept_entropy {kent}; logits {e_hip:.2e} (fp32 {e_ref:.2e}), Dice {dd_hip:.2e}")
    return bound


def run_case(model_cfg, cfg, x, ordinal=0, softmax=False, bf16=False, pair=None, missing=()):
    """The plugin's result for the volume ``x`` and the fp32 / float64 (bf16: fp32 / bf16-rounded) restatements."""
    from multimodal_tta_amd.registry import get_plugin
    ref, hip = pair if pair is not None else build_pair(model_cfg)
    d = cfg["method"]["deyo"]
    args = (cfg["training"], cfg["method"]["steps"], d["e_margin"], d["e_margin0"], d["plpd_threshold"])
    kw = dict(patches=d["patches"], seed=d["seed"], softmax=softmax, missing=missing)
    if bf16:
        other = deyo_reference(bf16_proxy(ref), [x.to(torch.bfloat16).float()], [ordinal], *args, **kw)[0]
    else:
        other = deyo_reference(copy.deepcopy(ref).double(), [x.double()], [ordinal], *args, **kw)[0]
    o32 = deyo_reference(ref, [x], [ordinal], *args, **kw)[0]
    plug = get_plugin("deyo_tta")(cfg).setup(hip, "cuda")
    res = plug.adapt_volume(x.cuda(), ordinals=[ordinal])
    return plug, res, o32, other


@pytest.mark.parametrize("index", [0, 1])
def test_deyo_matches_the_restatement(index):
    """32^3, S = 3, the reference's learning rate, patches [2, 2, 2], e_margin 0.8, e_margin0 0.6, plpd_threshold 0.05, group 1.
    Float64 restatement, entropy-kept / finally kept share of the elements at steps 0, 1, 2: volume 0 0.1072 / 0.0565,
    0.1074 / 0.0567, 0.1072 / 0.0569; volume 1 0.1046 / 0.0586, 0.1043 / 0.0587, 0.1043 / 0.0589."""
    cfg = deyo_cfg(SMALL, steps=3, group=1)
    x, y = volume(index)
    plug, res, o32, o64 = run_case(SMALL, cfg, x, ordinal=index)
    assert res["losses"].shape == (3,) and res["kept"].shape == (3,) and res["kept_entropy"].shape == (3,)
    check_against_reference(plug.logits(res).cpu(), res, o32, o64, y, x[0, :3].numel())


# The further cases run at the first plpd_threshold of (0.05, 0.02, 0.0) at which the float64 restatement removes >= 1 % of the
# elements at every step.  A lower threshold removes less, so the first one decides; all three cases meet it at 0.05.
def test_deyo_softmax_head_matches_the_restatement():
    """R = 4, volume 1, plpd_threshold 0.05.  Float64 restatement, entropy-kept / finally kept share of the voxels at steps 0,
    1, 2: 0.1828 / 0.1185, 0.1833 / 0.1196, 0.1841 / 0.1207."""
    mcfg = dict(SMALL, num_classes=4)
    cfg = deyo_cfg(mcfg, steps=3, group=1, thr=0.05)
    cfg["training"]["criterion"]["softmax"] = True
    cfg["training"]["criterion"]["sigmoid"] = False
    x, y = volume(1, R=4)
    plug, res, o32, o64 = run_case(mcfg, cfg, x, ordinal=1, softmax=True)
    assert plug.softmax
    check_against_reference(plug.logits(res).cpu(), res, o32, o64, y, x[0, 0].numel(), softmax=True)


def test_deyo_missing_modality_matches_the_restatement():
    """``missing_modalities: [1]``: the mask applies to both forwards.  Volume 3, plpd_threshold 0.05.  Float64 restatement,
    entropy-kept / finally kept share at steps 0, 1, 2: 0.1090 / 0.0623, 0.1087 / 0.0624, 0.1087 / 0.0626."""
    cfg = deyo_cfg(SMALL, steps=3, group=1, thr=0.05, missing_modalities=[1])
    x, y = volume(3)
    plug, res, o32, o64 = run_case(SMALL, cfg, x, ordinal=3, missing=[1])
    check_against_reference(plug.logits(res).cpu(), res, o32, o64, y, x[0, :3].numel())


def test_deyo_deepfusion_matches_the_restatement():
    """The family batch of the shuffled volume is a second pool buffer the runtime reads for the shuffled forward only.
    plpd_threshold 0.05, volume 1.  The deep-fusion network is less confident: the entropy filter keeps under 3 % of the
    elements, so the volume had to be chosen - with the float64 restatement - for the 1 % condition.  Entropy-kept / finally
    kept share at steps 0, 1, 2 on volume 1: 0.0270 / 0.0164, 0.0273 / 0.0168, 0.0274 / 0.0170 (1.04 - 1.06 % removed);
    volume 4 removes 1.01 - 1.02 %, volumes 0, 2, 3, 5 and 6 0.89 - 0.99 % at step 0 and fall short."""
    import oracle
    from multimodal_tta_amd.models import MultimodalUNetDeepFusion
    mcfg = dict(name="unet_multimodal_deepfusion", num_modalities=4, num_classes=3, spatial_dims=3,
                channels=[4, 8, 16, 32, 64], strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)
    cfg = deyo_cfg(mcfg, steps=3, group=1, thr=0.05)
    torch.manual_seed(42)
    ref = oracle.MultimodalUNetDeepFusion(mcfg)
    hip = MultimodalUNetDeepFusion(mcfg)
    hip.load_state_dict(ref.state_dict())
    x, y = volume(1)
    plug, res, o32, o64 = run_case(mcfg, cfg, x, ordinal=1, pair=(ref, hip))
    assert plug.rt.family_key == "xm", "the family batch's key was not restored"
    check_against_reference(plug.logits(res).cpu(), res, o32, o64, y, x[0, :3].numel())


def test_deyo_bf16_tracks_the_restatement():
    """bf16 precision against the fp32 restatement (volume 5).  ``kept`` is held to max(1e-2 of the elements, 3 d): see
    ``check_against_reference``; d and the observed distance are printed per step.  Measured at steps 0, 1, 2 of 98304
    elements: d = 2, 14, 12 (the bf16-rounded restatement keeps 5442, 5500, 5520 where the fp32 one keeps 5440, 5486, 5508),
    observed distance 8, 13, 9 (the plugin keeps 5432, 5499, 5517) - the floor of 983 elements is the bound in force."""
    cfg = deyo_cfg(SMALL, steps=3, group=1, precision="bf16")
    x, y = volume(5)
    plug, res, o32, o16 = run_case(SMALL, cfg, x, ordinal=5, bf16=True)
    check_against_reference(plug.logits(res).cpu(), res, o32, None, y, x[0, :3].numel(), bf16=True, o16=o16)


# ----------------------------------------------------------------------------- bit for bit
def test_deyo_group_equals_one_volume_at_a_time_and_graph_equals_eager():
    from multimodal_tta_amd.registry import get_plugin
    G = 3
    vols = [volume(i)[0] for i in range(G)]
    ordinals = [7, 0, 300]
    keys = ("losses", "kept", "kept_entropy")
    runs = {}
    for group, use_graph in ((G, True), (1, True), (G, False)):
        cfg = deyo_cfg(SMALL, steps=3, lr=1e-3, group=group, tune_volumes=4, use_graph=use_graph)
        _, hip = build_pair(SMALL)
        plug = get_plugin("deyo_tta")(cfg).setup(hip, "cuda")
        if group == G:
            r = plug.adapt_volume(torch.cat(vols).cuda(), ordinals=ordinals)
            runs[(group, use_graph)] = (plug.logits(r).cpu(),) + tuple(r[k].cpu() for k in keys)
        else:
            rs = []
            for v, o in zip(vols, ordinals):          # (the results are views of the plugin's buffers: read before the next volume)
                r = plug.adapt_volume(v.cuda(), ordinals=[o])
                rs.append({"z": plug.logits(r).cpu(), **{k: r[k].cpu().clone() for k in keys}})
            runs[(group, use_graph)] = (torch.cat([r["z"] for r in rs]),) + tuple(torch.stack([r[k] for r in rs], 1) for k in keys)
    _, losses, kept, kent = runs[(G, True)]
    assert torch.isfinite(losses).all() and (kept > 0).all() and (kept < kent).all(), "the PLPD filter is not in the run"
    for a, b in zip(runs[(G, True)], runs[(1, True)]):
        assert torch.equal(a, b), "grouped run differs from one volume at a time"
    for a, b in zip(runs[(G, True)], runs[(G, False)]):
        assert torch.equal(a, b), "graph replay differs from eager launches"


def test_the_ordinal_selects_the_permutation_and_the_default_counts_volumes():
    from multimodal_tta_amd.registry import get_plugin
    cfg = deyo_cfg(SMALL, steps=1, lr=1e-3, group=1)
    _, hip = build_pair(SMALL)
    plug = get_plugin("deyo_tta")(cfg).setup(hip, "cuda")
    x = volume(0)[0].cuda()
    first = {k: plug.adapt_volume(x)[k].cpu().clone() for k in ("kept", "kept_entropy")}          # ordinal 0
    second = {k: plug.adapt_volume(x)[k].cpu().clone() for k in ("kept", "kept_entropy")}         # ordinal 1
    again = {k: plug.adapt_volume(x, ordinals=[0])[k].cpu().clone() for k in ("kept", "kept_entropy")}
    assert torch.equal(first["kept_entropy"], second["kept_entropy"]), "the entropy filter does not see the shuffle"
    assert not torch.equal(first["kept"], second["kept"]), "another ordinal drew the same shuffle"
    assert torch.equal(first["kept"], again["kept"])


# ----------------------------------------------------------------------------- refusals
def test_deyo_refuses_modality_dropout_running_statistics_and_a_grid_that_does_not_divide():
    from multimodal_tta_amd.registry import get_plugin
    cfg = deyo_cfg(SMALL, steps=1, group=1, moddrop={"enabled": True, "p": 0.5, "seed": 0})
    with pytest.raises(NotImplementedError, match="method.moddrop.enabled"):
        get_plugin("deyo_tta")(cfg)
    cfg = deyo_cfg(BATCH, steps=1, group=1)
    _, hip = build_pair(BATCH)
    with pytest.raises(NotImplementedError, match="model.norm"):
        get_plugin("deyo_tta")(cfg).setup(hip, "cuda")
    cfg = deyo_cfg(SMALL, steps=1, group=1, patches=[3, 2, 2])
    _, hip = build_pair(SMALL)
    plug = get_plugin("deyo_tta")(cfg).setup(hip, "cuda")
    with pytest.raises(ValueError, match="method.deyo.patches"):
        plug.adapt_volume(volume(0)[0].cuda())
