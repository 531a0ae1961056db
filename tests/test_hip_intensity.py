"""Intensity-augmented views on the GPU (``mmtta_intensity_range``, ``mmtta_augment_views`` and the two plugins that stage
them): the channel ranges against ``torch.amin`` / ``torch.amax``; the views against a torch restatement - bit for bit where
the arithmetic is exactly specified (identity, scale and shift, constant and absent channels, a group against its volumes
one at a time), within a bound measured from torch's own fp32 evaluation where it goes through pow / log / cos (gamma,
noise); the noise against its moments; ``memo_tta`` and ``cotta_tta`` with intensity views against their torch-autograd
restatements fed the restated views, with the bounds of tests/test_hip_memo.py and tests/test_hip_cotta.py; and the bitwise
properties (a group = one volume at a time, the defaults = the block absent).  The measured figures of the gamma and noise
comparisons are recorded in DESIGN.md section 6."""
import copy
import math

import numpy as np
import pytest
import torch

import test_hip_cotta as tc
import test_hip_memo as tm
from test_cotta_host import philox4x32_10
from test_hip_tta import SMALL, build_pair, volume

pytestmark = pytest.mark.gpu

IDENTITY = (1.0, 1.0, 0.0, 0.0)
ALL_ON = dict(scale=0.1, shift=0.1, gamma=0.3, noise_std=0.05)


# ----------------------------------------------------------------------------- the restatement
def flip_dims(mask):
    """torch.flip dimensions of a mirror mask (bit 0 = W, 1 = H, 2 = D) on one channels-last item [D,H,W,C]."""
    return [dim for bit, dim in ((4, 0), (2, 1), (1, 2)) if mask & bit]


def noise_restated(nvox, seed, ordinal, view, dtype=torch.float64):
    """n [4, nvox] of channel quad 0: Philox at the counter (i, (0 << 8) | view, ordinal, 1); words (0, 1) -> channels 0, 1 as
    R cos(theta), R sin(theta) with R = sqrt(-2 ln(((w0 >> 8) + 1) 2^-24)), theta = 2 pi (w1 >> 8) 2^-24; words (2, 3) ->
    channels 2, 3.  ``dtype``: the arithmetic (float64: the restatement; float32: torch's own fp32 evaluation of it)."""
    i = np.arange(nvox, dtype=np.uint64)
    w = [torch.from_numpy((x >> np.uint32(8)).astype(np.int64)) for x in philox4x32_10((i, view, ordinal, 1), (seed & 0xFFFFFFFF, seed >> 32))]
    out = []
    for wa, wb in ((w[0], w[1]), (w[2], w[3])):
        u = (wa + 1).to(dtype) * 2.0 ** -24
        theta = (2 * math.pi) * (wb.to(dtype) * 2.0 ** -24)
        r = torch.sqrt(-2 * torch.log(u))
        out += [r * torch.cos(theta), r * torch.sin(theta)]
    return torch.stack(out)


def transform_restated(item, C, rows, lo, hi, noise=None):
    """One view of one volume in the volume's own frame: item [D,H,W,4] (the arithmetic runs in its dtype), rows [C,4] =
    (g, a, b, sigma) per channel, lo / hi [C] the channel ranges, noise [4, D*H*W] or None.  Gamma, then * a, then + b,
    then + sigma n, each operation rounded on its own; identity rows, constant channels and pad lanes pass."""
    out = item.clone()
    dt = item.dtype
    for c in range(C):
        g, a, b, s = (torch.tensor(float(v), dtype=dt) for v in rows[c])
        if tuple(float(v) for v in rows[c]) == IDENTITY or not float(hi[c]) > float(lo[c]):
            continue
        val = item[..., c]
        l, h = lo[c].to(dt), hi[c].to(dt)
        if float(g) != 1.0:
            val = torch.pow((val - l) / (h - l), g) * (h - l) + l
        val = val * a
        val = val + b
        if float(s) > 0:
            val = val + s * noise[c].to(dt).reshape(val.shape)
        out[..., c] = val
    return out


def views_restated(base, C, masks, table, seed, ordinals, dtype=torch.float32):
    """base [G,D,H,W,4] -> [G*V,D,H,W,4] in ``dtype`` arithmetic: item g*V+v = view v of volume g (transformed, then mirrored)."""
    G, V = base.shape[0], len(masks)
    nvox = base[0, ..., 0].numel()
    out = []
    for g in range(G):
        item = base[g].to(dtype)
        lo, hi = item.reshape(-1, 4).amin(0), item.reshape(-1, 4).amax(0)
        for v, m in enumerate(masks):
            noisy = v > 0 and bool((table[g, v, :, 3] > 0).any())
            # (the noise is a float64 draw rounded to the arithmetic's type; the float32 evaluation of the draw itself is
            # what test_noise measures)
            noise = noise_restated(nvox, seed, ordinals[g], v) if noisy else None
            t = item if v == 0 else transform_restated(item, C, table[g, v], lo, hi, noise)
            out.append(torch.flip(t, flip_dims(m)) if m else t)
    return torch.stack(out)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def make_base(G, D, H, W, C, dtype, seed, pad=float("nan")):
    gen = torch.Generator().manual_seed(seed)
    base = torch.randn((G, D, H, W, 4), generator=gen).to(dtype)
    base[..., C:] = pad          # the pad lanes are poisoned
    return base


def run_kernels(base, C, masks, table, seed, ordinals):
    """-> (views [G*V,D,H,W,4] pad lanes included, ranges [G,C,2]) from mmtta_intensity_range + mmtta_augment_views."""
    from multimodal_tta_amd import ops
    G, D, H, W, _ = base.shape
    V = len(masks)
    x = ops.new_cl(G, D, H, W, C, "cuda", ldc=4, dtype=base.dtype)
    xb = x if x._base is None else x._base
    xb.copy_(base)
    y = ops.new_cl(G * V, D, H, W, C, "cuda", ldc=4, dtype=base.dtype)
    yb = y if y._base is None else y._base
    yb.fill_(float("nan"))
    rng = torch.full((G * C * 2,), float("nan"), device="cuda")
    partial = torch.full((ops.intensity_range_partials(x),), float("nan"), device="cuda")
    ops.intensity_range(x, partial, rng)
    th = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32))
    ords = torch.from_numpy(np.array(ordinals, dtype=np.uint32).view(np.int32)).cuda()
    ops.augment_views(x, y, masks, th, th.cuda(), rng, seed, ords)
    torch.cuda.synchronize()
    assert torch.equal(bits(xb.cpu()), bits(base)), "the input was written"
    return yb.cpu(), rng.cpu().view(G, C, 2)


def identity_table(G, V, C):
    return np.tile(np.array(IDENTITY, dtype=np.float32), (G, V, C, 1))


def spec(mirror_axes, **kw):
    from multimodal_tta_amd.intensity import parse_intensity
    return parse_intensity(kw, list(mirror_axes), "method.memo.intensity")


# ----------------------------------------------------------------------------- 1. range
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("shape", [(5, 6, 7), (20, 24, 28)])          # one workgroup, and 53 of them
def test_range_equals_amin_amax(dtype, C, shape):
    from multimodal_tta_amd import ops
    G = 3
    base = make_base(G, *shape, C, dtype, 31 + C + shape[0])
    base[1, ..., 0] = 0.25          # a constant channel
    x = ops.new_cl(G, *shape, C, "cuda", ldc=4, dtype=dtype)
    (x if x._base is None else x._base).copy_(base)
    out = torch.full((G, C, 2), float("nan"), device="cuda")
    partial = torch.full((ops.intensity_range_partials(x),), float("nan"), device="cuda")
    ops.intensity_range(x, partial, out)
    torch.cuda.synchronize()
    want = base[..., :C].float()
    assert torch.equal(out[..., 0].cpu(), want.amin((1, 2, 3))) and torch.equal(out[..., 1].cpu(), want.amax((1, 2, 3)))
    assert out[1, 0, 0].item() == out[1, 0, 1].item() == 0.25


# ----------------------------------------------------------------------------- 2. identity = mirror_views
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,masks", [(4, [0, 2, 1, 3]), (2, [0, 4, 0, 4, 0, 4, 0, 4]), (3, [0, 0]), (1, [0])])
def test_identity_table_gives_the_bits_of_mirror_views(dtype, C, masks):
    from multimodal_tta_amd import ops
    G, (D, H, W) = 2, (5, 6, 7)
    base = make_base(G, D, H, W, C, dtype, 5 + C, pad=3.5)
    got, _ = run_kernels(base, C, masks, identity_table(G, len(masks), C), 0, [0, 1])
    x = ops.new_cl(G, D, H, W, C, "cuda", ldc=4, dtype=dtype)
    (x if x._base is None else x._base).copy_(base)
    y = ops.new_cl(G * len(masks), D, H, W, C, "cuda", ldc=4, dtype=dtype)
    yb = y if y._base is None else y._base
    yb.fill_(float("nan"))
    ops.mirror_views(x, y, masks)
    torch.cuda.synchronize()
    assert torch.equal(bits(got), bits(yb.cpu()))


# ----------------------------------------------------------------------------- 3. scale and shift, bit for bit
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [2, 4])
def test_scale_and_shift_are_two_separately_rounded_operations(dtype, C):
    """flip(x) * a + b: in fp32 the product is rounded, then the sum (an fma would differ in a share of the elements); with
    bf16 storage the fp32 value is rounded to nearest even once."""
    G, masks, (D, H, W) = 2, [0, 2, 1, 3], (6, 10, 12)
    base = make_base(G, D, H, W, C, dtype, 77 + C)
    rng = np.random.default_rng(C)
    table = identity_table(G, 4, C)
    table[:, 1:, :, 1] = rng.uniform(0.9, 1.1, (G, 3, C))
    table[:, 1:, :, 2] = rng.uniform(-0.1, 0.1, (G, 3, C))
    table[1, 2, 0] = IDENTITY          # one identity channel inside a transformed view
    got, _ = run_kernels(base, C, masks, table, 0, [0, 1])
    x32 = base.float()
    fused = 0
    for g in range(G):
        for v, m in enumerate(masks):
            want = x32[g].clone()
            for c in range(C):
                if v > 0 and tuple(table[g, v, c]) != IDENTITY:
                    a, b = torch.tensor(table[g, v, c, 1]), torch.tensor(table[g, v, c, 2])
                    want[..., c] = x32[g, ..., c] * a + b
                    fused += int((torch.addcmul(b, x32[g, ..., c], a) != want[..., c]).sum())
            want = (torch.flip(want, flip_dims(m)) if m else want).to(dtype)
            # pad lanes: the input's bits (NaN payload and all), moved with the row
            pad = torch.flip(base[g], flip_dims(m)) if m else base[g]
            want[..., C:] = pad[..., C:]
            assert torch.equal(bits(got[g * 4 + v]), bits(want)), (g, v)
    assert fused > 0, "the inputs do not tell a fused multiply-add from two operations"


# ----------------------------------------------------------------------------- 4. constant and absent channels
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_constant_and_absent_channels_pass_bit_for_bit(dtype):
    from multimodal_tta_amd.intensity import view_parameters
    G, C, (D, H, W) = 2, 4, (6, 8, 10)
    cfg = spec(["h"], copies=2, per_channel=True, seed=3, **ALL_ON)
    masks = cfg.view_axes
    base = make_base(G, D, H, W, C, dtype, 91)
    base[..., 1] = 0.37          # constant: hi == lo
    base[0, ..., 1] = -0.0       # ... with a sign bit to keep
    present = [True, True, False, True]          # channel 2 is absent: the host gives it identity rows
    table = view_parameters(cfg, [6, 2], C, present)
    assert (table[:, 1:, 1, 3] > 0).all() and (table[:, 1:, 1, 2] != 0).all(), "the constant channel's rows are not the identity"
    got, _ = run_kernels(base, C, masks, table, cfg.seed, [6, 2])
    for g in range(G):
        for v, m in enumerate(masks):
            want = torch.flip(base[g], flip_dims(m)) if m else base[g]
            for c in (1, 2):
                assert torch.equal(bits(got[g * 4 + v][..., c]), bits(want[..., c])), (g, v, c)
            for c in (0, 3):
                assert (v == 0) == torch.equal(bits(got[g * 4 + v][..., c]), bits(want[..., c])), (g, v, c)


# ----------------------------------------------------------------------------- 5. gamma
def test_gamma_against_float64():
    """The bound is not fixed in advance: torch's own fp32 evaluation of the formula is measured against the float64
    restatement on the same inputs, and the kernel is allowed 4 x that, floored at 4 fp32 ulp of the channel's range (the
    device's exp2 / log2 forms against libm)."""
    G, C, masks, (D, H, W) = 2, 4, [0, 2, 0, 1], (16, 20, 24)
    base = make_base(G, D, H, W, C, torch.float32, 123, pad=0.0)
    rng = np.random.default_rng(9)
    table = identity_table(G, 4, C)
    table[:, 1:, :, 0] = np.exp(rng.uniform(-0.5, 0.5, (G, 3, C)))
    got, ranges = run_kernels(base, C, masks, table, 0, [0, 1])
    w64 = views_restated(base, C, masks, table, 0, [0, 1], torch.float64)
    w32 = views_restated(base, C, masks, table, 0, [0, 1], torch.float32)
    assert torch.equal(w64[::4].float(), base[:, ...]) and torch.equal(got[::4], base)
    worst = []
    for g in range(G):
        for c in range(C):
            lo, hi = ranges[g, c]
            ulp = float(np.spacing(np.float32(hi - lo)))
            ref = w64[g * 4 + 1:g * 4 + 4, ..., c]
            e_torch = (w32[g * 4 + 1:g * 4 + 4, ..., c].double() - ref).abs().max().item()
            e_hip = (got[g * 4 + 1:g * 4 + 4, ..., c].double() - ref).abs().max().item()
            bound = max(4 * e_torch, 4 * ulp)
            print(f"gamma, volume {g} channel {c}: range {float(hi - lo):.4f} (ulp {ulp:.2e}); torch fp32 {e_torch:.2e} "
                  f"({e_torch / ulp:.2f} ulp), kernel {e_hip:.2e} ({e_hip / ulp:.2f} ulp), bound {bound:.2e}")
            worst.append((e_hip, bound))
    assert all(e <= b for e, b in worst), worst
    # the ends of the range: t = 0 gives 0 * (hi - lo) + lo = lo exactly; t = 1 gives 1 * (hi - lo) + lo, which in fp32 is
    # the rounded sum of the rounded difference (hi itself only up to that rounding)
    for g in range(G):
        for v in range(1, 4):
            for c in range(C):
                col = got[g * 4 + v][..., c]
                lo, hi = ranges[g, c]
                assert col.min().item() == lo.item(), (g, v, c)
                assert col.max().item() == ((hi - lo) + lo).item(), (g, v, c)


# ----------------------------------------------------------------------------- 6. noise
def test_noise_against_float64_and_its_moments():
    """n = (y - x) / sigma with g, a, b at identity.  Against the float64 restatement of the draw: the bound is 4 x the
    distance of torch's own fp32 evaluation (the draw in fp32, then x + sigma n and the same read-back), floored at 4 fp32 ulp
    of max |y| over sigma - the rounding of y = x + sigma n is part of what is read back.  Against its moments over N samples:
    |mean| <= 6 / sqrt(N) and |std - 1| <= 6 / sqrt(2 N) (six standard errors of the mean and of the standard deviation of N
    standard normals)."""
    C, masks, S, seed, ordinal = 4, [0, 1, 0, 1], 64, 0x1234567890ABCDEF, 77
    base = make_base(1, S, S, S, C, torch.float32, 55)
    sigma = np.float32(0.1)
    table = identity_table(1, 4, C)
    table[:, 1:, :, 3] = sigma
    got, _ = run_kernels(base, C, masks, table, seed, [ordinal])
    x = base[0].double()
    nvox = S ** 3
    samples = []
    for v in (1, 2, 3):
        y = got[v]
        y = torch.flip(y, flip_dims(masks[v])) if masks[v] else y          # back to the volume's own frame
        n = (y.double() - x) / float(sigma)
        n64 = noise_restated(nvox, seed, ordinal, v).T.reshape(S, S, S, 4)
        n32 = noise_restated(nvox, seed, ordinal, v, torch.float32).T.reshape(S, S, S, 4)
        y32 = base[0] + torch.tensor(sigma) * n32
        e_torch = ((y32.double() - x) / float(sigma) - n64).abs().max().item()
        e_hip = (n - n64).abs().max().item()
        floor = 4 * float(np.spacing(np.float32(y.abs().max().item()))) / float(sigma)
        bound = max(4 * e_torch, floor)
        N = n.numel()
        mean, std = n.mean().item(), n.std().item()
        print(f"noise, view {v}: torch fp32 {e_torch:.2e}, kernel {e_hip:.2e}, bound {bound:.2e} (floor {floor:.2e}); "
              f"mean {mean:+.2e} (<= {6 / math.sqrt(N):.2e}), std - 1 {std - 1:+.2e} (<= {6 / math.sqrt(2 * N):.2e})")
        assert e_hip <= bound, (v, e_hip, bound)
        assert abs(mean) <= 6 / math.sqrt(N) and abs(std - 1) <= 6 / math.sqrt(2 * N), (v, mean, std)
        samples.append(n.reshape(-1))
    # every view, every channel draws its own numbers: sample correlations of independent normals, six standard errors
    N = samples[0].numel()
    for a in range(3):
        for b in range(a + 1, 3):
            assert abs((samples[a] * samples[b]).mean().item()) <= 6 / math.sqrt(N)
    ch = samples[0].reshape(-1, 4)
    for a in range(4):
        for b in range(a + 1, 4):
            assert abs((ch[:, a] * ch[:, b]).mean().item()) <= 6 / math.sqrt(nvox)
    # another ordinal or seed draws other numbers
    for s2, o2 in ((seed, ordinal + 1), (seed + 1, ordinal)):
        other, _ = run_kernels(base, C, masks, table, s2, [o2])
        assert (other[1] != got[1])[..., :C].float().mean().item() > 0.99


# ----------------------------------------------------------------------------- 7. grouped = one at a time
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_g_volumes_equal_g_single_volume_calls(dtype):
    from multimodal_tta_amd.intensity import view_parameters
    G, C, (D, H, W), ordinals = 3, 4, (6, 10, 12), [5, 9, 2]
    cfg = spec(["h"], copies=2, per_channel=True, seed=8, **ALL_ON)
    base = make_base(G, D, H, W, C, dtype, 19)
    table = view_parameters(cfg, ordinals, C)
    got, ranges = run_kernels(base, C, cfg.view_axes, table, cfg.seed, ordinals)
    assert not torch.equal(bits(got[1]), bits(got[5]))
    for g in range(G):
        one, r1 = run_kernels(base[g:g + 1], C, cfg.view_axes, view_parameters(cfg, [ordinals[g]], C), cfg.seed, [ordinals[g]])
        assert torch.equal(bits(one), bits(got[g * 4:(g + 1) * 4])), g
        assert torch.equal(r1[0], ranges[g])
    # ... and the views are the restatement's, within fp32 / bf16 rounding of pow and the draw (1e-5 of the largest value;
    # the exact comparisons are tests 3 to 6)
    want = views_restated(base, C, cfg.view_axes, table, cfg.seed, ordinals)
    tol = (2.0 ** -7 if dtype == torch.bfloat16 else 1e-5) * want[..., :C].abs().max().item()
    assert (got[..., :C].float() - want[..., :C]).abs().max().item() <= tol


# ----------------------------------------------------------------------------- 8. the plugins against their restatements
def restated_input_views(x, plug, ordinals):
    """x [G,C,D,H,W] fp32 -> the views the plugin stages, restated: [G*V,C,D,H,W] fp32."""
    from multimodal_tta_amd.intensity import view_parameters
    C = x.shape[1]
    assert C == 4
    table = view_parameters(plug.intensity, ordinals, C)
    v = views_restated(x.permute(0, 2, 3, 4, 1).contiguous(), C, plug.view_axes, table, plug.intensity.seed, ordinals)
    return v.permute(0, 4, 1, 2, 3).contiguous()


def intensity_cfg(make, axes, intensity, **kw):
    cfg = make(SMALL, axes, **kw)
    cfg["method"][cfg["method"]["name"][:-4]]["intensity"] = dict(intensity)
    return cfg


@pytest.mark.parametrize("axes,intensity,ensemble", [
    (["h"], dict(copies=2, **ALL_ON), False),
    ([], dict(copies=2, scale=0.1, shift=0.1), False),
    (["h"], dict(copies=2, per_channel=True, seed=5, **ALL_ON), True),          # the ensemble: the mean over the augmented views
])
def test_memo_with_intensity_views_matches_the_restatement(monkeypatch, axes, intensity, ensemble):
    """``memo_tta`` against tests/test_hip_memo.py's MEMO restatement fed the restated views, with that file's bounds
    (``check_against_reference``)."""
    from multimodal_tta_amd.registry import get_plugin
    cfg = intensity_cfg(tm.memo_cfg, axes, intensity, steps=3, ensemble=ensemble, group=1)
    ref, hip = build_pair(SMALL)
    ref0 = copy.deepcopy(ref)
    x, y = volume(0)
    plug = get_plugin("memo_tta")(cfg).setup(hip, "cuda")
    assert plug.views == len(plug.view_axes) == 2 * (1 << len(axes)) and not plug.rt.fused_layers
    xv = restated_input_views(x, plug, [7])
    assert not torch.equal(xv[0], xv[plug.views // 2]), "the copies are identical"
    monkeypatch.setattr(tm, "memo_views", lambda x_, masks: xv.to(x_.dtype))
    out_ref = tm.memo_reference(ref, x, cfg["training"], 3, plug.view_axes, ensemble=ensemble)
    res = plug.adapt_volume(x.cuda(), ordinals=[7])
    assert res["losses"].shape == (3,)
    # the staged views are the restated ones (the exact comparisons are the kernel tests above)
    staged = plug.rt.pool.cl("x_views", plug.views, 32, 32, 32, 4, ldc=4, zero=True, dtype=torch.float32)
    assert (staged.permute(0, 4, 1, 2, 3).cpu() - xv).abs().max().item() <= 1e-5 * xv.abs().max().item()
    tm.check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref, ref0, x, y, cfg, plug.view_axes, ensemble=ensemble)


def test_cotta_with_intensity_views_matches_the_restatement(monkeypatch):
    """``cotta_tta`` with ``copies: 2`` against tests/test_hip_cotta.py's CoTTA restatement, its teacher fed the restated
    views, with that file's bounds (``check_against_reference``)."""
    from multimodal_tta_amd.registry import get_plugin
    cfg = intensity_cfg(tc.cotta_cfg, ["h"], dict(copies=2, seed=11, **ALL_ON), steps=3, group=1)
    ref, hip = build_pair(SMALL)
    x, y = volume(0)
    plug = get_plugin("cotta_tta")(cfg).setup(hip, "cuda")
    assert plug.views == 4 and plug.view_axes == [0, 2, 0, 2]
    xv = restated_input_views(x, plug, [3])
    monkeypatch.setattr(tc, "memo_views", lambda x_, masks: xv.to(x_.dtype))
    args = dict(alpha=0.9, restore_p=0.2, seed=0, ordinals=[3])
    o64, _ = tc.cotta_reference(copy.deepcopy(ref).double(), [x.double()], cfg["training"], 3, plug.view_axes, tc.layout_of(plug), **args)
    out_ref, _ = tc.cotta_reference(ref, [x], cfg["training"], 3, plug.view_axes, tc.layout_of(plug), **args)
    res = plug.adapt_volume(x.cuda(), ordinals=[3])
    tc.check_against_reference(plug.logits(res).cpu(), res["losses"], out_ref[0], o64[0], y)
    # the draws do not meet: the restore count is the restore mask's, whatever the views drew
    n_train = plug.rt.arena.n_train
    for t in range(3):
        assert int(res["restored"][t]) == int(tc.restore_mask(n_train, 0, t + 1, 3, 0.2).sum())


# ----------------------------------------------------------------------------- 9. bit for bit
@pytest.mark.parametrize("method", ["memo", "cotta"])
def test_a_group_equals_one_volume_at_a_time(method):
    from multimodal_tta_amd.registry import get_plugin
    make = tm.memo_cfg if method == "memo" else tc.cotta_cfg
    G, ordinals = 2, [8, 3]
    vols = [volume(i)[0] for i in range(G)]
    runs = {}
    for group in (G, 1):
        cfg = intensity_cfg(make, ["w"], dict(copies=2, per_channel=True, **ALL_ON), steps=3, lr=1e-3, group=group, tune_volumes=4)
        _, hip = build_pair(SMALL)
        plug = get_plugin(f"{method}_tta")(cfg).setup(hip, "cuda")
        if group == G:
            r = plug.adapt_volume(torch.cat(vols).cuda(), ordinals=ordinals)
            runs[group] = (plug.logits(r).cpu(), r["losses"].cpu())
        else:
            zs, ls = [], []
            for v, o in zip(vols, ordinals):
                r = plug.adapt_volume(v.cuda(), ordinals=[o])
                zs.append(plug.logits(r).cpu())
                ls.append(r["losses"].cpu())
            runs[group] = (torch.cat(zs), torch.stack(ls, 1))
            # the ordinal enters the draw: another one gives another result
            r = plug.adapt_volume(vols[0].cuda(), ordinals=[ordinals[0] + 1])
            assert not torch.equal(r["losses"].cpu(), ls[0])
    for a, b in zip(runs[G], runs[1]):
        assert torch.equal(a, b), "grouped run differs from one volume at a time"


def test_memo_default_ordinals_count_the_volumes_served():
    from multimodal_tta_amd.registry import get_plugin
    cfg = intensity_cfg(tm.memo_cfg, [], dict(copies=2, noise_std=0.1), steps=1, lr=1e-3, group=1)
    _, hip = build_pair(SMALL)
    plug = get_plugin("memo_tta")(cfg).setup(hip, "cuda")
    x = volume(0)[0].cuda()
    served = [plug.adapt_volume(x)["losses"].cpu().clone() for _ in range(3)]
    given = [plug.adapt_volume(x, ordinals=[o])["losses"].cpu().clone() for o in (0, 1, 2)]
    for a, b in zip(served, given):
        assert torch.equal(a, b)
    assert not torch.equal(given[0], given[1])
    with pytest.raises(ValueError, match="ordinals"):
        plug.adapt_volume(x, ordinals=[1, 2])


# ----------------------------------------------------------------------------- 10. the off state
@pytest.mark.parametrize("method", ["memo", "cotta"])
def test_the_defaults_are_the_block_absent_bit_for_bit(monkeypatch, method):
    """With the block at its defaults nothing new runs: the mirror pass stages the views, and both plugins return the bits of
    a run of the same process whose config has no ``intensity`` block (the config of the parent commit)."""
    from multimodal_tta_amd import ops
    from multimodal_tta_amd.config import compose
    from multimodal_tta_amd.registry import get_plugin

    def never(*a, **k):
        raise AssertionError("an intensity kernel ran with the block off")

    monkeypatch.setattr(ops, "augment_views", never)
    monkeypatch.setattr(ops, "intensity_range", never)
    make = tm.memo_cfg if method == "memo" else tc.cotta_cfg
    defaults = dict(compose(overrides=["task=brats", "model=unet", f"method=tta_{method}"])["method"][method]["intensity"])
    x = torch.cat([volume(0)[0], volume(1)[0]]).cuda()
    outs = []
    for block in (None, defaults):
        cfg = make(SMALL, ["h", "w"], steps=2, lr=1e-3, group=2)
        if block is not None:
            cfg["method"][method]["intensity"] = block
        assert ("intensity" in cfg["method"][method]) == (block is not None)
        _, hip = build_pair(SMALL)
        plug = get_plugin(f"{method}_tta")(cfg).setup(hip, "cuda")
        assert plug.views == 4 and not plug.intensity.active
        r = plug.adapt_volume(x)
        outs.append((plug.logits(r).cpu(), r["losses"].cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
