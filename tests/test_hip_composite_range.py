"""The compositing kernels, forward and backward, on the adversarial rays of tests/_composite_truth.py: opaque shells, empty rays, zero and
denormal densities, the softplus threshold, saturated colours, repeated and log-spaced t, |d| of 1e-3 / 1e3 / 0, and S = 1, 2, 65, 193, 300
(300: the eight-block instance of composite_bwd_kernel).  At the stage level both sides see the same fp32 inputs: nothing is ill-conditioned.

  forward   per ray |hip - truth| <= base + 3 |oracle32 - truth| (the pattern of tests/test_hip_fuzz.py), base the stage bars of
            tests/test_hip_parity.py: 2e-6 for rgb and acc, 1e-6 for the weights, 2e-6 max t of the ray for the depth; truth: long double
  backward  per element |got - truth| <= 2^-23 |truth| + 2^-40 max over the ray of |truth|, and exact zeros where the truth is exactly
            zero -- what "the correctly rounded derivative at the forward's fp32 inputs" (csrc/aon_composite_grad.h) means, with a floor
            for the cancellation inside the fp64 evaluation.  tests/test_composite_truth_cpu.py shows a plain float64 evaluation at 0.5.
            The truth is taken at the correctly rounded norm |d|, as torch.norm gives it.
  scene     the same rows as a one-object scene list and as a two-object interleave, against tests/_scene_grad_ref.composite_torch
            (round32=True) in fp64, under the same bars.

The ray-gradient reduce kernel (csrc/aon_ray_grad.hip) has no stage call that takes raw and t -- tests/test_hip_ray_grads.py drives it
through the whole frozen-network call only -- so it is not among the kernels here.  Every test prints its worst ratio to its bar."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _composite_truth as ct  # noqa: E402
import _scene_grad_ref as gref  # noqa: E402
from oracle import nerf_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(dev):
    from aon_amd import ops as _ops

    return _ops


_BATCH = {}


def batch(S, act):
    """the shared rows and their long-double forward truth, computed once"""
    if (S, act) not in _BATCH:
        b = ct.adversarial_batch(S, act)
        b["truth"] = {w: ct.composite(b["raw"], b["t"], b["d"], w, act) for w in (False, True)}
        _BATCH[S, act] = b
    return _BATCH[S, act]


def activated32(raw, act):
    """the reference's fp32 activations of a raw record (model.py:186-187, model_autodecoder.py:321-323)"""
    if act == 1:
        return torch.sigmoid(raw[..., :3]), torch.relu(raw[..., 3:])
    if act == 2:
        return torch.sigmoid(raw[..., :3]) * (1 + 2 * 0.001) - 0.001, torch.nn.functional.softplus(raw[..., 3:] + (-1.0))
    return raw[..., :3], raw[..., 3:]


def thin_rows(b, act):
    """(n,) bool: rays on which at least nine in ten of the finite intervals have an optical depth sigma delta < 1e-3 -- their transmittance
    is a long product of factors just below 1 (a property of the inputs: activation and fp32 intervals as tests/_composite_truth.py forms
    them; for two lists, of the first)"""
    _, _, sg, _ = ct.activate(b["raw"][: ct.N_RAYS], act, None, np.float64)
    x = (sg * ct.intervals32(b["t"][: ct.N_RAYS], b["d"]))[:, :-1]
    return (x < 1e-3).mean(1) >= 0.9 if x.shape[1] else np.zeros(x.shape[0], bool)


THIN_CAUSE = ("thin rays at S >= 193: the transmittance is a product of ~S factors fl(1 - alpha + 1e-10) = expf(-sigma delta) just below 1, and "
              "the device expf is low by 0.11-0.12 ulp on average for arguments in [1e-7, 1e-3] (measured through weights = 1 - expf(-x) of a "
              "two-sample ray, 200,000 arguments a decade; the host's fp32 exp is centred: -0.006), so the product drifts by 7e-9 per sample: the "
              "weights of an almost empty 193 / 300-sample ray end 1.4e-6 / 3.3e-6 from the truth (bar 1e-6 + 3 x 3e-8 / 2.7e-7).  A centred "
              "factor changes the forward's bits, which tests/golden pins (g24, g30)")


def forward_ratios(got, truth, ref32, t, rows):
    """got / ref32: (rgb, acc, weights, depth) fp32 arrays; truth: the long-double dict; rows: (n,) bool, the rays that count
    -> {name: (worst err / bar over those rays, ray, its err, its |oracle32 - truth|)}"""
    n = t.shape[0]
    tmax = np.abs(t).max(1).astype(np.float64)
    out = {}
    for name, g, r, base in (("rgb", got[0], ref32[0], 2e-6), ("acc", got[1], ref32[1], 2e-6), ("weights", got[2], ref32[2], 1e-6),
                             ("depth", got[3], ref32[3], 2e-6 * tmax)):
        if g is None:
            continue
        tr = truth[name].reshape(n, -1)
        g64, r64 = np.asarray(g, np.float64).reshape(n, -1), np.asarray(r, np.float64).reshape(n, -1)
        if name == "depth":   # helper.py:182: NaN -> +inf, exactly there
            nan = np.isnan(tr.astype(np.float64))
            assert np.array_equal(np.isposinf(g64), nan)
            g64, r64, tr = (np.where(nan, 0, x) for x in (g64, r64, tr))
        assert np.isfinite(g64).all(), name
        err = np.abs(g64 - tr).max(1).astype(np.float64)
        spread = np.abs(r64 - tr).max(1).astype(np.float64)
        ratio = np.where(rows, err / (base + 3 * spread), 0.0)
        i = int(ratio.argmax())
        out[name] = (float(ratio[i]), i, float(err[i]), float(spread[i]))
    return out


def oracle32(b, act, white):
    raw, t, d = (torch.from_numpy(b[k]) for k in ("raw", "t", "d"))
    rgb, sig = activated32(raw, act)
    return [x.numpy() for x in orc.volumetric_rendering(rgb, sig, t, d, white)]


# ------------------------------------------------------------------------------------------------ the two known deviations
class ExpfDrift(Exception):
    """a thin ray's output outside the forward bar, in one of the (entry point, act, output) combinations THIN_KNOWN names"""


class NativeRoot(Exception):
    """a ray with a scaled direction outside the backward bar against the correctly rounded norm, and inside it against a neighbour"""


ROOT_CAUSE = ("the kernels take the square root of the norm |d| on the hardware unit (HIP's __fsqrt_rn is the native v_sqrt_f32 unless the "
              "correctly rounded device operations are asked for: ray_norm_f32 in csrc/aon_ray_core.h, composite_kernel in csrc/aon_render.hip), "
              "one ulp from the correctly rounded root torch.norm returns.  On some of the rays with |d| = 1e-3 or 1e3 the two differ, every interval moves "
              "by an ulp and the gradients end 1.04-2.2 (scene: up to 5.3) times the bar from the truth at the rounded norm; against the truth at "
              "the neighbouring norm they are at 0.50.  A correctly rounded root changes the bits tests/golden pins (g24, g30)")
# which outputs exceed the forward bar on the thin rays, measured on an MI355X; everything else on those rays is asserted
THIN_KNOWN = {(193, "thin"): {("composite_raw", 2, "weights")},
              (300, "thin"): {("composite_raw", 1, "weights"), ("composite_raw", 2, "weights"), ("volumetric_rendering", 0, "weights")},
              ("scene", 2, 2, 300): {"acc", "depth"}}
_XFAIL_THIN = pytest.mark.xfail(strict=True, raises=ExpfDrift, reason=THIN_CAUSE)
_XFAIL_ROOT = pytest.mark.xfail(strict=True, raises=NativeRoot, reason=ROOT_CAUSE)


def scaled_direction(b):
    """(n,) bool: the rays whose direction is not a unit vector: |d| = 1e-3 or 1e3 (six rows; d = 0 has the root 0 on any unit)"""
    dn = ct.norm32(b["d"])
    return (dn > 0) & ((dn < 0.5) | (dn > 2.0))


def test_device_expf_of_small_arguments(ops, dev):
    """How THIN_CAUSE's figure is obtained: weights[:, 0] of a two-sample ray with t = [0, 1], d = (0, 0, 1) and act 0 is 1 - expf(-sigma),
    and 1 - w recovers expf(-sigma) exactly (a difference of two fp32 values in [0.5, 1]).  Asserted: the library's bound of one ulp.
    Printed: the mean signed error a decade.  Measured on an MI355X: -0.107, -0.119, -0.119, -0.113 ulp for [1e-7, 1e-6) .. [1e-4, 1e-3)."""
    rng = np.random.RandomState(0)
    for lo in (-7, -6, -5, -4):
        x = (10.0 ** (rng.rand(50000) + lo)).astype(np.float32)
        n = len(x)
        den = torch.zeros(n, 2, 1)
        den[:, 0, 0] = torch.from_numpy(x)
        t, d = torch.tensor([[0.0, 1.0]]).repeat(n, 1), torch.tensor([[0.0, 0.0, 1.0]]).repeat(n, 1)
        w = ops.volumetric_rendering(torch.zeros(n, 2, 3).to(dev), den.to(dev), t.to(dev), d.to(dev), False)[2].cpu().numpy()[:, 0].astype(np.float64)
        err = ((1.0 - w) - np.exp(-x.astype(np.float64))) / 2.0 ** -24
        print(f"expf(-x), x in [1e{lo}, 1e{lo + 1}): mean signed error {err.mean():+.3f} ulp, largest {np.abs(err).max():.3f}")
        assert np.abs(err).max() <= 1.0


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("S,rows", [(S, r) for S in ct.SIZES for r in ("ordinary", "thin") if (S, r) not in THIN_KNOWN]
                         + [pytest.param(193, "thin", marks=_XFAIL_THIN), pytest.param(300, "thin", marks=_XFAIL_THIN)])
def test_composite_forward_on_the_adversarial_rows(ops, dev, S, rows):
    """ops.composite_raw (acts 1 and 2, the packed kernel; S = 65 and 193 are its compile-time instances, the others the run-time one),
    ops.volumetric_rendering (act 0, the unpacked kernel) and, at S = 65, ops.composite_pdf (the fused coarse level).  Every ray is in one
    of two cases: "thin" (thin_rows) or "ordinary".  Measured on an MI355X: ordinary rays at most 0.94 of the bar (the weights of the opaque ray
    under |d| = 1e-3 at S = 193; 0.41 up to S = 65); thin rays 0.40 at S = 65, and at S = 193 / 300 their weights at 1.31 / 1.81 of it
    (THIN_CAUSE).  The expected failure covers the combinations of THIN_KNOWN only: any other output outside the bar fails the test."""
    worst = {}
    for act in (0, 1, 2):
        b = batch(S, act)
        raw, t, d = (torch.from_numpy(b[k]).to(dev) for k in ("raw", "t", "d"))
        for white in (False, True):
            ref = oracle32(b, act, white)
            if act == 0:
                calls = {"volumetric_rendering": ops.volumetric_rendering(raw[..., :3].contiguous(), raw[..., 3:].contiguous(), t, d, white)}
            else:
                calls = {"composite_raw": ops.composite_raw(raw, t, d, white, act=act)}
                if S == 65:
                    calls["composite_pdf"] = ops.composite_pdf(raw, t, d, white, act=act, want_weights=True)[:4]
            for name, (comp, acc, w, depth) in calls.items():
                got = [x.cpu().numpy() for x in (comp, acc, w, depth)]
                mask = thin_rows(b, act) == (rows == "thin")
                for k, v in forward_ratios(got, b["truth"][white], ref, b["t"], mask).items():
                    if v[0] >= worst.get((name, act, k), (0.0,))[0]:
                        worst[name, act, k] = v + (b["labels"][v[1]], white)
    for key, v in sorted(worst.items()):
        print(f"S = {S}, {rows} rays: {key[0]} act {key[1]} {key[2]}: worst err / (base + 3 |oracle32 - truth|) = {v[0]:.3f} (ray {v[1]}, {v[4]!r}, white {v[5]}: "
              f"err {v[2]:.2e}, oracle32 {v[3]:.2e})")
    over = {k for k, v in worst.items() if v[0] > 1.0}
    assert over <= THIN_KNOWN.get((S, rows), set()), {k: worst[k] for k in over}
    if over:
        raise ExpfDrift(sorted(over))


@pytest.mark.parametrize("S", ct.SIZES)
def test_fully_extreme_rays(ops, dev, S):
    """The rays adversarial_batch softens for the backward bar, whole: all three colour channels of every sample at +-20 / +-90, and
    raw_sigma + bias = -80 / -100 at every sample (ct.extreme_rows).  Forward: the bar of the test above (acts 1 and 2).  Backward: every
    output finite, the padded tail zero, the two density rows exactly zero under relu; the ratio to the backward bar is printed (every
    gradient of such a ray is tiny -- fp32 denormals, alphas below the fp64 cancellation of 1 - exp(-x), or, with one colour at every sample,
    density gradients that cancel down to the last sample's transmittance -- so the bar's floor, 2^-40 of the ray's largest, is below
    fp64's own rounding: see adversarial_batch; measured 0.2 .. 8e6)."""
    for act in (1, 2):
        b = ct.extreme_rows(S)
        n = len(b["labels"])
        raw, t, d, g_rgb = (torch.from_numpy(b[k]).to(dev) for k in ("raw", "t", "d", "g_rgb"))
        for white in (False, True):
            truth = ct.composite(b["raw"], b["t"], b["d"], white, act, None, b["g_rgb"])
            got = [x.cpu().numpy() for x in ops.composite_raw(raw, t, d, white, act=act)]
            fr = forward_ratios(got, truth, oracle32(b, act, white), b["t"], np.ones(n, bool))
            assert max(v[0] for v in fr.values()) <= 1.0, fr
            out = ops.composite_bwd(raw, t, d, g_rgb, None, None, white, act, ops.padded_samples(n * S) + 128).cpu().numpy()
            gb = out[: n * S].reshape(n, S, 4)
            assert np.isfinite(out).all() and (out[n * S:] == 0).all()
            if act == 1:      # relu of a negative raw_sigma at every sample: an empty ray, every gradient exactly 0
                assert (gb[4:] == 0).all() and (truth["d_raw"][4:] == 0).all()
            r = ct.backward_ratio(gb, truth["d_raw"]).reshape(n, -1).max(1)
            print(f"fully extreme rays, S = {S}, act {act}, white {white}: forward {({k: round(v[0], 3) for k, v in fr.items()})}; backward ratio per ray "
                  f"{dict(zip(b['labels'], np.round(r, 2).tolist()))}")


@pytest.mark.parametrize("act", [1, 2])
def test_infinite_colours_give_the_activation_limits(ops, dev, act):
    """A colour record at +-inf: the forward colour is the activation's limit exactly (act 1: 1 / 0; act 2: fl(scale - shift) / -shift)
    and its gradient exactly 0; everything else stays finite."""
    b = ct.inf_colour_rows()
    raw, t, d, g = (torch.from_numpy(b[k]).to(dev) for k in ("raw", "t", "d", "g_rgb"))
    comp = ops.composite_raw(raw, t, d, False, act=act)[0].cpu().numpy()
    scale, shift = np.float32(1 + 2 * 0.001), np.float32(0.001)
    hi, lo = (np.float32(1), np.float32(0)) if act == 1 else (np.float32(scale - shift), np.float32(-shift))
    assert comp[0, 0] == hi and comp[1, 0] == lo and np.isfinite(comp).all(), comp
    n, S = b["t"].shape
    d_raw = ops.composite_bwd(raw, t, d, g, None, None, False, act, ops.padded_samples(n * S)).cpu().numpy()[: n * S].reshape(n, S, 4)
    assert (d_raw[..., 0] == 0).all() and np.isfinite(d_raw).all() and (d_raw[:, 0, 1:3] != 0).all()


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("S,act", [pytest.param(S, act, marks=_XFAIL_ROOT) if S in (2, 65, 300) else (S, act) for S in ct.SIZES for act in (0, 1, 2)])
def test_composite_backward_on_the_adversarial_rows(ops, dev, S, act):
    """ops.composite_bwd, both backgrounds, with and without g_acc / g_depth, against the truth at the correctly rounded norm.  Measured on
    an MI355X: every ray at 0.50 of the bar at most, except some of the six with |d| = 1e-3 or 1e3 at S = 2, 65 and 300 (ROOT_CAUSE; at S = 1 and 193
    the hardware root of those directions is the rounded one).  The expected failure is that deviation alone: every other ray is asserted
    against the bar, and those six rays must meet it against the truth at the rounded norm or at one of its two fp32 neighbours
    (ct.norm_candidates, one norm for the whole ray) -- else the test fails."""
    b = batch(S, act)
    n = ct.N_RAYS
    short = scaled_direction(b)
    raw, t, d, g_rgb, g_acc, g_depth = (torch.from_numpy(b[k]).to(dev) for k in ("raw", "t", "d", "g_rgb", "g_acc", "g_depth"))
    Np = ops.padded_samples(n * S) + 128
    worst, where, worst_short, worst_any, off = 0.0, None, 0.0, 0.0, 0
    for white in (False, True):
        for extra in (False, True):
            ga, gd = (g_acc, g_depth) if extra else (None, None)
            out = ops.composite_bwd(raw, t, d, g_rgb, ga, gd, white, act, Np).cpu().numpy()
            assert (out[n * S:] == 0).all()                                   # the padded tail
            got = out[: n * S].reshape(n, S, 4)
            truths = [ct.composite(b["raw"], b["t"], b["d"], white, act, None, b["g_rgb"], b["g_acc"] if extra else None,
                                   b["g_depth"] if extra else None, dn=dn)["d_raw"] for dn in ct.norm_candidates(b["d"])]
            truth = truths[0]
            assert np.isfinite(got).all()
            assert (got[truth == 0] == 0).all(), sorted({b["labels"][i] for i in np.nonzero((truth == 0) & (got != 0))[0]})
            ratio = ct.backward_ratio(got, truth).reshape(n, -1).max(1)
            off += int((ratio > 1.0).sum())
            worst_short = max(worst_short, float(ratio[short].max()))
            worst_any = max(worst_any, float(ct.backward_ratio_any_norm(got, truths)[short].max()))
            rest = np.where(short, 0.0, ratio)
            i = int(rest.argmax())
            if rest[i] > worst:
                worst, where = float(rest[i]), (b["labels"][i], i, white, extra)
    print(f"composite_bwd S = {S}, act {act}: worst |got - truth| / (2^-23 |truth| + 2^-40 max_ray |truth|) = {worst:.3f} at {where}; rays with "
          f"|d| = 1e-3 or 1e3: {worst_short:.3f} ({worst_any:.3f} against the best of the rounded norm and its neighbours); {off} ray evaluations outside the bar")
    assert worst <= 1.0 and worst_any <= 1.0
    if worst_short > 1.0:
        raise NativeRoot(worst_short)


# ------------------------------------------------------------------------------------------------ scene kernels
def _pairs(ops, dev, n, K):
    """n rays that each cross all K objects: object k's rows are k n .. k n + n - 1 (the object-major layout of ops.scene_pairs)"""
    slot = (torch.arange(n, dtype=torch.int32)[:, None] + n * torch.arange(K, dtype=torch.int32)[None, :]).contiguous()
    P = n * K
    z3, z1 = torch.zeros(P, 3, device=dev), torch.zeros(P, device=dev)
    offsets = torch.arange(K + 1, dtype=torch.int64) * n
    return ops.ScenePairs(n, K, offsets.to(dev), [n] * K, slot.to(dev), torch.arange(P, dtype=torch.int32, device=dev) % n, z3, z3, z3, z1, z1), slot.numpy()


def _scene_case(S, act, K):
    """the rows as K lists a ray: list 0 the batch itself; list 1 the batch of another seed (other t: the lists interleave), directions
    of list 0 (a scene ray has one world direction)"""
    parts = [ct.adversarial_batch(S, act, seed=k) for k in range(K)]
    b = dict(parts[0])
    b["raw"] = np.concatenate([p["raw"] for p in parts])
    b["t"] = np.concatenate([p["t"] for p in parts])
    return b


_SCENE = [(1, 1, 2), (1, 2, 2), (1, 1, 65), (1, 2, 65), (1, 2, 193), (1, 1, 300), (1, 2, 300), (2, 2, 65), (2, 1, 300), (2, 2, 300)]


@pytest.mark.parametrize("K,act,S", [c if c == (1, 2, 193) else pytest.param(*c, marks=_XFAIL_ROOT) for c in _SCENE])
def test_scene_composite_and_backward_on_the_adversarial_rows(ops, dev, K, act, S):
    """ops.scene_composite on the ordinary rays, and ops.scene_composite_bwd on every ray (a scene list ends with an interval of 0; the scene
    calls start at S = 2).  The forward of the thin rays: the next test.  The expected failure is ROOT_CAUSE on the backward of the rays
    with |d| = 1e-3 or 1e3, as in the one-object test, and nothing else."""
    _scene(ops, dev, K, act, S, "ordinary", True)


@pytest.mark.parametrize("K,act,S", [pytest.param(*c, marks=_XFAIL_THIN) if ("scene",) + c in THIN_KNOWN else c for c in _SCENE])
def test_scene_composite_forward_on_the_thin_rows(ops, dev, K, act, S):
    """Measured on an MI355X: at most 0.97 of the bar, except acc (1.50) and depth (1.03) of the 600 merged samples of two interleaved act-2
    lists (THIN_CAUSE): the expected failure covers those two outputs only."""
    _scene(ops, dev, K, act, S, "thin", False)


def _scene(ops, dev, K, act, S, rows, backward):
    b = _scene_case(S, act, K)
    n = ct.N_RAYS
    short = scaled_direction(b)
    pairs, slot = _pairs(ops, dev, n, K)
    raw, t, d, g_rgb, g_acc, g_depth = (torch.from_numpy(b[k]).to(dev) for k in ("raw", "t", "d", "g_rgb", "g_acc", "g_depth"))
    g_obj = torch.from_numpy(np.random.RandomState(S + K).randn(n, K).astype(np.float32))
    worst_f, worst_b, where, worst_short, worst_any = {}, 0.0, None, 0.0, 0.0
    mask = thin_rows(b, act) == (rows == "thin")

    def note(name, ratio):
        ratio = np.where(mask, ratio, 0.0)
        i = int(ratio.argmax())
        if ratio[i] >= worst_f.get(name, (0.0,))[0]:
            worst_f[name] = (float(ratio[i]), b["labels"][i])

    for white in (False, True):
        with torch.no_grad():
            t64 = gref.composite_torch(torch.from_numpy(b["raw"].astype(np.float64)), b["t"], slot, b["d"], white, None, act, True)
            t32 = gref.composite_torch(torch.from_numpy(b["raw"]), b["t"], slot, b["d"], white, None, act, True)
        rgb, acc, depth, obj_acc, w = ops.scene_composite(raw, t, pairs, d, white, act=act)
        tmax = np.abs(b["t"]).reshape(K, n, S).max((0, 2))
        for name, g, base in (("rgb", rgb, 2e-6), ("acc", acc, 2e-6), ("depth", depth, 2e-6 * tmax), ("obj_acc", obj_acc, 2e-6)):
            g64 = g.cpu().numpy().astype(np.float64).reshape(n, -1)
            assert np.isfinite(g64).all(), name
            err = np.abs(g64 - t64[name].numpy().reshape(n, -1)).max(1)
            spread = np.abs(t32[name].numpy().astype(np.float64).reshape(n, -1) - t64[name].numpy().reshape(n, -1)).max(1)
            note(name, err / (base + 3 * spread))
        werr = np.abs(w.cpu().numpy().astype(np.float64) - t64["weights"].numpy()).reshape(K, n, S).max((0, 2))
        wspread = np.abs(t32["weights"].numpy().astype(np.float64) - t64["weights"].numpy()).reshape(K, n, S).max((0, 2))
        note("weights", werr / (1e-6 + 3 * wspread))
        for extra in ((False, True) if backward else ()):
            ga, gd, go = (g_acc, g_depth, g_obj.to(dev)) if extra else (None, None, None)
            got = ops.scene_composite_bwd(raw, t, pairs, d, g_rgb, ga, gd, go, white, act=act).cpu().numpy()

            def truth_for(sel, dirs):
                """(len(sel), K S, 4): the rays `sel` under the directions dirs"""
                g = gref.composite_grads(b["raw"], b["t"], slot[sel], dirs[sel], white, b["g_rgb"][sel], b["g_acc"][sel] if extra else None,
                                         b["g_depth"][sel] if extra else None, g_obj.numpy()[sel] if extra else None, None, act).numpy()
                return g.reshape(K, n, S, 4).transpose(1, 0, 2, 3).reshape(n, K * S, 4)[sel]

            got = got.reshape(K, n, S, 4).transpose(1, 0, 2, 3).reshape(n, K * S, 4)      # a ray's elements: its K lists
            truth = truth_for(np.arange(n), b["d"])
            assert np.isfinite(got).all()
            assert (got[truth == 0] == 0).all()
            ratio = ct.backward_ratio(got, truth).reshape(n, -1).max(1)
            sel = np.flatnonzero(short)
            best = ratio[sel].copy()
            for dn in ct.norm_candidates(b["d"])[1:]:      # (sqrt(fl(x x)) = x in fp32: a direction (dn, 0, 0) has the norm dn)
                dirs = np.stack([dn, np.zeros_like(dn), np.zeros_like(dn)], 1)
                best = np.minimum(best, ct.backward_ratio(got[sel], truth_for(sel, dirs)).reshape(len(sel), -1).max(1))
            worst_short, worst_any = max(worst_short, float(ratio[sel].max())), max(worst_any, float(best.max()))
            rest = np.where(short, 0.0, ratio)
            i = int(rest.argmax())
            if rest[i] > worst_b:
                worst_b, where = float(rest[i]), (b["labels"][i], i, white, extra)
    print(f"scene K = {K}, act {act}, S = {S}, {rows} rays: forward worst err / bar {({k: (round(v[0], 3), v[1]) for k, v in worst_f.items()})}; backward worst "
          f"ratio {worst_b:.3f} at {where}; rays with |d| = 1e-3 or 1e3: {worst_short:.3f} ({worst_any:.3f} against the best of the rounded norm and its neighbours)")
    assert backward or mask.any()
    over = {k for k, v in worst_f.items() if v[0] > 1.0}
    assert over <= (THIN_KNOWN.get(("scene", K, act, S), set()) if rows == "thin" else set()), {k: worst_f[k] for k in over}
    assert worst_b <= 1.0 and worst_any <= 1.0
    if over:
        raise ExpfDrift(sorted(over))
    if worst_short > 1.0:
        raise NativeRoot(worst_short)
