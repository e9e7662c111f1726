"""The device math functions of csrc/aon_common.h -- sin_f32 (and with it the reduction cos_f32 shares), sigmoid_f32, softplus_f32 --
against fp64 over their whole argument range, through stage entry points that return the function's value itself:

  * ops.pos_enc(x, 0, 1) = [x, sin_f32(x), sin_f32(fl(x + fp32(pi/2)))]
  * ops.composite_raw with S = 1, raw_sigma = 1, black background: the only interval is the 1e10-long last one, alpha = 1 - expf(-1e10)
    = 1 and the transmittance before it is 1, so comp_rgb = 1 * activated colour = sigmoid_f32(raw) (act 1), and for act 2
    fl(fl(sigmoid_f32(raw) * rgb_scale) - rgb_shift)
  * ops.composite_raw with S = 2, act 2, t = [0, delta], d = (1, 0, 0): weights[:, 0] = 1 - expf(-fl(softplus_f32(fl(x + bias)) * delta))

Inputs are fp32 bit patterns: every normal binade, both signs, the zeros, the denormal range's ends, the fp32 values next to multiples of
pi/2 (the reduction's worst cancellation), and the non-finite values with a defined result.  Every test prints its worst error."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HALF_PI_F32 = np.float32(1.57079637050628662109375)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(dev):
    from aon_amd import ops as _ops

    return _ops


def binade_patterns():
    """Positive fp32 values: for every normal binade 1,024 evenly spaced mantissas and the binade's first and last value."""
    ex = np.arange(1, 255, dtype=np.uint32)[:, None] << 23
    man = np.concatenate([np.arange(1024, dtype=np.uint32) * 8192, np.array([0x7FFFFF], dtype=np.uint32)])[None, :]
    return (ex | man).reshape(-1).view(np.float32)


def both_signs(a):
    return np.concatenate([a, -a])


def near_multiples_of_half_pi():
    """The fp32 nearest to k pi/2: every k <= 2^20, then 2^16 evenly spaced k in every binade of the argument above (long double: k is
    exact below 2^64; where an fp32 ulp exceeds pi/2 -- from 2^24 on -- every value is next to a multiple anyway)."""
    half_pi = np.longdouble(math.pi) / 2 + np.longdouble(6.123233995736766e-17)   # fp64 pi/2 and what it lacks: pi/2 to the long double
    parts = [(np.arange(1, (1 << 20) + 1, dtype=np.float64).astype(np.longdouble) * half_pi).astype(np.float32)]
    top = float(parts[0][-1])
    frac = (np.arange(1 << 16, dtype=np.float64) / (1 << 16)).astype(np.longdouble)
    for e in range(20, 128):
        k = np.rint(np.longdouble(2.0) ** e * (1 + frac) / half_pi)
        with np.errstate(over="ignore"):
            v = (k * half_pi).astype(np.float32)
        parts.append(v[(v > top) & np.isfinite(v)])
    return np.concatenate(parts)


def pad3(a, fill=0.0):
    """(m,) -> (ceil(m/3), 3) fp32 tensor"""
    m = (-len(a)) % 3
    return torch.from_numpy(np.concatenate([a, np.full(m, fill, dtype=np.float32)]).reshape(-1, 3))


SIN_RANGES = [(0, 19), (19, 20), (20, 21), (21, 22), (22, 24), (24, 32), (32, 128)]


def test_sin_f32_every_binade(ops, dev):
    """sin_f32 against numpy's float64 sin of the same fp32 argument (the shifted column: of the fp32 sum).  Bars: 1.5e-7 absolute for
    |arg| < 2^19 (the bar tests/test_hip_parity.py::test_pos_enc holds at |arg| <= 3072), 4 * 2^-24 absolute from 2^19 on (4 ulp at 1:
    the bound OpenCL sets for sin).  Measured on an MI355X: 9.27e-8 below 2^19, at most 9.30e-8 in every range above.  The Cody-Waite
    reduction alone misses the second bar from the binade [2^20, 2^21) on (on the device: 2.9e-7 there, 2.1e-4 in [2^22, 2^24), 9e15 in
    [2^24, 2^32))."""
    den = np.array([0.0, 1e-45, 1.1754942e-38], dtype=np.float32)   # +0, the smallest and the largest denormal
    x = both_signs(np.concatenate([binade_patterns(), near_multiples_of_half_pi(), den]))
    xt = pad3(x)
    out = ops.pos_enc(xt.to(dev), 0, 1).cpu().numpy()
    xs = xt.numpy()
    assert np.array_equal(out[:, :3].view(np.uint32), xs.view(np.uint32))
    arg = np.concatenate([xs, xs + HALF_PI_F32], axis=1).reshape(-1)       # fp32 sum, as the kernel forms it
    got = out[:, 3:].reshape(-1).astype(np.float64)
    err = np.abs(got - np.sin(arg.astype(np.float64)))
    err[np.isnan(err)] = np.inf      # a NaN for a finite argument misses every bar
    mag = np.abs(arg.astype(np.float64))
    failed = []
    for lo, hi in SIN_RANGES:
        sel = (mag < 2.0 ** hi) & ((mag >= 2.0 ** lo) if lo else True)
        bar = 1.5e-7 if hi <= 19 else 4 * 2.0 ** -24
        worst = err[sel].max()
        i = np.flatnonzero(sel)[err[sel].argmax()]
        print(f"sin_f32, |arg| in [{'0' if not lo else f'2^{lo}'}, 2^{hi}): {int(sel.sum())} values, worst abs error {worst:.3e} at arg {arg[i]!r} "
              f"(got {got[i]!r}), bar {bar:.3e}, ratio {worst / bar:.3g}")
        if not worst <= bar:
            failed.append((lo, hi, worst))
    assert not failed, failed
    # sin(+-0) = 0, and the denormals come back to within the bar (already covered); the non-finite arguments give NaN, as torch.sin does
    bad = torch.tensor([[float("inf"), float("-inf"), float("nan")]])
    o = ops.pos_enc(bad.to(dev), 0, 1).cpu()
    assert torch.isnan(o[:, 3:]).all() and torch.isnan(torch.sin(bad)).all()


# ------------------------------------------------------------------------------------------------ sigmoid_f32
def _sigmoid64(x):
    x = x.astype(np.float64)
    with np.errstate(over="ignore"):
        return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


@pytest.mark.parametrize("act", [1, 2])
def test_sigmoid_f32_whole_range(ops, dev, act):
    """comp_rgb of a one-sample ray is the activated colour.  act 1 (sigmoid_f32 itself): 2^-23 absolute against fp64 -- the hardware exp2
    at 1 ulp reaches the result times e / (1 + e)^2 <= 1/4 (2^-25), the rounding of the product x log2(e) at most 1e-8 (aon_common.h),
    the reciprocal after its Newton step and the final rounding half an ulp each (2^-25 + 2^-25 below 1).  act 2: the same bar times
    rgb_scale, plus the two fp32 roundings of fl(fl(s * scale) - shift), 2^-24 each for values up to 1.002.  x < -87: the function returns
    0 for a true value below 1.7e-38.  Monotone non-decreasing over the sorted inputs."""
    x = np.concatenate([np.linspace(-110.0, 110.0, 1 << 20).astype(np.float32), both_signs(binade_patterns()),
                        both_signs(np.array([0.0, 1e-45, 1.1754942e-38], dtype=np.float32))])
    x = np.sort(x, kind="stable")
    xt = pad3(x, fill=float(x[-1]))
    n = xt.shape[0]
    raw = torch.cat([xt, torch.ones(n, 1)], 1).reshape(n, 1, 4)
    t = torch.ones(n, 1)
    d = torch.tensor([[0.0, 0.0, 1.0]]).repeat(n, 1)
    opts = ops.RenderOpts() if act == 2 else None
    comp, acc, _, _ = ops.composite_raw(raw.to(dev), t.to(dev), d.to(dev), False, act=act, want_weights=False, opts=opts)
    got = comp.cpu().numpy().reshape(-1)
    xs = xt.numpy().reshape(-1)
    assert (acc.cpu() == 1).all()
    want = _sigmoid64(xs)
    bar = 2.0 ** -23
    if act == 2:
        scale, shift = np.float64(np.float32(1.002)), np.float64(np.float32(0.001))
        want = want * scale - shift
        bar = 2.0 ** -23 * scale + 2 * 2.0 ** -24
    err = np.abs(got.astype(np.float64) - want)
    i = err.argmax()
    print(f"sigmoid_f32 (act {act}): {len(xs)} values, worst abs error {err[i]:.3e} at x = {xs[i]!r}, bar {bar:.3e}, ratio {err[i] / bar:.3g}; "
          f"worst in [-20, 20]: {err[np.abs(xs) <= 20].max():.3e}")
    assert err.max() <= bar
    low = got[xs < -87.0]
    if act == 1:
        assert (low >= 0).all() and (low <= 1.2e-38).all()
    else:
        assert (low == np.float32(-np.float32(0.001))).all()
    drops = np.flatnonzero(np.diff(got) < 0)
    print(f"sigmoid_f32 (act {act}): {len(drops)} decreasing steps over the sorted inputs" + (f", first at x = {xs[drops[0]]!r} -> {xs[drops[0] + 1]!r}: "
          f"{got[drops[0]]!r} -> {got[drops[0] + 1]!r}" if len(drops) else ""))
    assert len(drops) == 0
    # +inf -> 1, -inf -> 0, NaN -> NaN (act 2: through scale and shift)
    bad = torch.tensor([float("inf"), float("-inf"), float("nan"), 1.0]).reshape(1, 1, 4)
    c = ops.composite_raw(bad.to(dev), t[:1].to(dev), d[:1].to(dev), False, act=act, want_weights=False, opts=opts)[0].cpu()[0]
    one, zero = (1.0, 0.0) if act == 1 else (float(np.float32(np.float32(1.002) - np.float32(0.001))), float(-np.float32(0.001)))
    assert c[0].item() == one and c[1].item() == zero and math.isnan(c[2].item())


# ------------------------------------------------------------------------------------------------ softplus_f32
@pytest.mark.parametrize("bias", [-1.0, 0.3])
def test_softplus_f32_whole_range(ops, dev, bias):
    """weights[:, 0] of a two-sample ray with t = [0, delta], delta = fp32(1 / softplus64(a)), a = fl(x + fp32(bias)) the kernel's own fp32
    argument: w = 1 - expf(-fl(sg * delta)) with sg = softplus_f32(a), near 1 - 1/e for every a.  Truth: 1 - exp(-softplus64(a) delta) in
    fp64, softplus64 with torch's threshold (a > 20: a).  Bar: sg may be off by eps = 2.5e-7 + 2^-24 |min(a, 0)| relative (the bar of
    tests/test_hip_mesh.py, and the rounding of the exponent's product |a| log2(e), which the hardware exp2 turns into a relative error
    of that size); the product sg * delta ~ 1 inherits it and reaches w times d/dp (1 - e^-p) = e^-1; then the three roundings of the
    chain itself, 2^-24 (product), 2^-23 (expf), 2^-25 (the subtraction, result in [0.5, 1)):
        |w - truth| <= e^-1 eps + 2^-24 + 2^-23 + 2^-25.
    Arguments: a in [-85, 100] (below, 1 / softplus overflows fp32), dense in [19, 21] around torch's threshold and around 0."""
    b32 = np.float32(bias)
    target = np.concatenate([np.linspace(-85.0, 100.0, 60001), np.linspace(19.0, 21.0, 40001), np.linspace(-0.01, 0.01, 20001),
                             np.array([0.0, 20.0, np.nextafter(np.float32(20), np.float32(21)), np.nextafter(np.float32(20), np.float32(19))])])
    x = (target - np.float64(b32)).astype(np.float32)
    a = (x + b32).astype(np.float32)                       # fl(raw + sigma_bias)
    a64 = a.astype(np.float64)
    sp = np.where(a64 > 20.0, a64, np.maximum(a64, 0.0) + np.log1p(np.exp(-np.abs(a64))))
    delta = (1.0 / sp).astype(np.float32)
    assert np.isfinite(delta).all() and (delta > 0).all()
    n = len(x)
    raw = torch.zeros(n, 2, 4)
    raw[:, 0, 3] = torch.from_numpy(x)
    t = torch.zeros(n, 2)
    t[:, 1] = torch.from_numpy(delta)
    d = torch.tensor([[1.0, 0.0, 0.0]]).repeat(n, 1)
    opts = ops.RenderOpts(density_bias=bias)
    w = ops.composite_raw(raw.to(dev), t.to(dev), d.to(dev), False, act=2, opts=opts)[2].cpu().numpy()[:, 0].astype(np.float64)
    truth = -np.expm1(-sp * delta.astype(np.float64))
    eps = 2.5e-7 + 2.0 ** -24 * np.abs(np.minimum(a64, 0.0))
    bar = math.exp(-1.0) * eps + 2.0 ** -24 + 2.0 ** -23 + 2.0 ** -25
    ratio = np.abs(w - truth) / bar
    for name, sel in (("[-85, -20)", a64 < -20), ("[-20, 19)", (a64 >= -20) & (a64 < 19)), ("[19, 21]", (a64 >= 19) & (a64 <= 21)), ("(21, 100]", a64 > 21)):
        i = np.flatnonzero(sel)[ratio[sel].argmax()]
        print(f"softplus_f32 (bias {bias}), a in {name}: worst |w - truth| {abs(w[i] - truth[i]):.3e} at a = {a[i]!r}, bar {bar[i]:.3e}, ratio {ratio[i]:.3g}; "
              f"as a relative error of softplus: {abs(w[i] - truth[i]) * math.e:.3e}")
    assert ratio.max() <= 1.0
    # below -88 softplus is under 6.1e-39: with delta = 1 the weight is at most 1e-37 (and not negative)
    tl = np.linspace(-100.0, -88.0, 1201)
    xl = (tl - np.float64(b32)).astype(np.float32)
    rawl = torch.zeros(len(xl), 2, 4)
    rawl[:, 0, 3] = torch.from_numpy(xl)
    tt = torch.tensor([[0.0, 1.0]]).repeat(len(xl), 1)
    wl = ops.composite_raw(rawl.to(dev), tt.to(dev), d[: len(xl)].to(dev), False, act=2, opts=opts)[2].cpu().numpy()[:, 0]
    print(f"softplus_f32 (bias {bias}), a in [-100, -88]: largest weight {wl.max():.3e}")
    assert (wl >= 0).all() and (wl <= 1e-37).all()


# ------------------------------------------------------------------------------------------------ cos_f32 above 2^19
def test_cos_f32_at_large_arguments_through_the_ray_gradients(dev, monkeypatch):
    """cos_f32 has no stage call; its accurate form runs in the ray-gradient kernels (csrc/aon_ray_grad.hip), as the derivative of the
    encoding at the forward's own fp32 argument.  A frozen vanilla network at degrees (14, 24, 4) -- the articulated kernels stop at
    max_deg_point = 16 -- with one level, deterministic samples and rays whose points are EXACT in fp32 and fp64 alike: rays_d = (0, 0, 1),
    rays_o on a grid of 1/16, t = 2 + 4 i / 64, so x = o + t d has a dozen bits and 2^l x is exact for every level.  The arguments reach
    2^23 |x| (up to 2^24: five of the ten levels lie above 2^19 for |x| >= 1), and the only rounding in them is the fp32 sum
    fl(2^l x + fp32(pi/2)), which is part of the function (ulp 2 at 2^24: in fp64 that column would be another function).  d loss /
    d rays_o against tests/test_hip_vanilla_ray_grads.py's fp64 oracle, its encoding taken at those fp32 arguments (value and derivative:
    a straight-through rounding), under that file's bar: as close to the truth as the oracle's fp32 autograd, factor 5, floor 1e-4.  A
    wrong quadrant or sign of cos_f32 in any level moves the gradient by its whole size: the levels' weights 2^l cos(arg) are of
    the same order."""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_hip_vanilla_ray_grads as vrg
    from oracle import nerf_oracle as orc

    model = vrg._model(dev, num_levels=1, min_deg_point=14, max_deg_point=24, deg_view=4)
    n = 24
    gen = torch.Generator().manual_seed(5)
    o = torch.randint(-12, 13, (n, 3), generator=gen).float() / 16
    o[:, 2] -= 4
    d = torch.tensor([[0.0, 0.0, 1.0]]).repeat(n, 1)
    rays = {"rays_o": o, "rays_d": d, "viewdirs": d.clone()}
    target = torch.rand(n, 3, generator=gen)
    x = o[:, None, :] + (2 + 4 * torch.arange(65) / 64)[None, :, None] * d[:, None, :]
    assert torch.equal(x.double(), o.double()[:, None, :] + (2 + 4 * torch.arange(65).double() / 64)[None, :, None] * d.double()[:, None, :])
    big = (x.abs() * 2.0 ** 23 >= 2.0 ** 19).float().mean().item()
    hip, _ = vrg._hip_grads(model, dev, rays, target, None, None, randomized=False, which=("rays_o",))
    hip = {"rays_o": hip["rays_o"].cpu()}
    assert torch.isfinite(hip["rays_o"]).all() and hip["rays_o"].abs().max() > 0
    ref32 = vrg._oracle_grads(model, rays, target, None, None, torch.float32, randomized=False)

    def pos_enc_at_fp32_arguments(p, min_deg, max_deg):
        scales = torch.tensor([2.0 ** l for l in range(min_deg, max_deg)], dtype=p.dtype)
        xb = (p[..., None, :] * scales[:, None]).reshape(*p.shape[:-1], -1)
        arg = torch.cat([xb, xb + orc.HALF_PI_F32], dim=-1)
        arg = arg + (arg.detach().float().to(p.dtype) - arg.detach())
        return torch.cat([p, torch.sin(arg)], dim=-1)

    monkeypatch.setattr(orc, "pos_enc", pos_enc_at_fp32_arguments)
    truth = vrg._oracle_grads(model, rays, target, None, None, torch.float64, randomized=False)
    print(f"cos_f32 through the vanilla ray gradients, degrees (14, 24): {big:.0%} of the top level's arguments are >= 2^19; |truth| "
          f"{truth['rays_o'].norm().item():.3e}, |hip - truth| {(hip['rays_o'].double() - truth['rays_o']).norm().item():.3e}, |ref32 - truth| "
          f"{(ref32['rays_o'].double() - truth['rays_o']).norm().item():.3e}")
    vrg._yardstick().assert_as_close_as_fp32(hip, {"rays_o": truth["rays_o"]}, {"rays_o": ref32["rays_o"]}, "cos_f32 at large arguments",
                                             factor=5.0, floor=1e-4)
