"""The rays a sharp-field comparison leaves out, classified instead of ignored.

Vanilla NeRF's last interval is 1e10 long (helper.py:163), so the far sample's alpha is a step function of the sign of its raw sigma:
where that sigma sits within rounding of zero, two correct evaluations may land on different sides of the step.  The end-to-end tests
therefore hold only rays with a robust far-plane margin to their tight bars.  This module checks the others: the fp64 oracle is run on
them with the last alpha of each level forced to 0 or 1 (the four (coarse, fine) combinations) and unforced, and each ray's HIP
(rgb, acc, depth) at every level must match ONE combination -- the same one for both levels -- within the calling test's bar.  A
compositing kernel that mishandles the far interval (any alpha other than 0 or 1 there, a wrong interval length) matches none.

A ray matches a branch when |hip - oracle64| <= bar + widen * |oracle32 - oracle64| for every compared quantity at every level, both
oracle runs forced to that branch.  ``widen=1`` is what a test that holds HIP to the fp32 oracle within ``bar`` implies (triangle
inequality); a test that widens its bar by 3x the reference's own fp32-vs-fp64 spread passes ``widen=3``.
"""
import itertools

import torch

from oracle import nerf_oracle as orc  # noqa: E402  (checker only)

QUANTITIES = ("rgb", "acc", "depth")


def _per_ray(x):
    return x.abs().amax(dim=-1) if x.dim() > 1 else x.abs()


def _take(kw, idx):
    """The per-ray arguments of orc.nerf_forward restricted to the rays ``idx``; the others unchanged."""
    out = dict(kw)
    for k in ("t_rand", "u"):
        if out.get(k) is not None:
            out[k] = out[k][idx]
    if out.get("noise") is not None:
        out["noise"] = [z[idx] for z in out["noise"]]
    return out


def _f64(kw):
    out = {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in kw.items()}
    if out.get("noise") is not None:
        out["noise"] = [z.double() for z in out["noise"]]
    return out


def check_far_branch(hip, sd, rays, drop, bars, randomized, white_bkgd, near, far, widen=1.0, label="", **kw):
    """hip: per level (rgb, acc, depth) of ALL rays (CPU tensors); sd, rays (CPU fp32): the oracle's inputs for all rays; drop: (n,) bool,
    the rays the test's tight comparison skipped; bars: per level a (rgb, acc, depth) triple of bars (None: not compared); kw: the other
    arguments of orc.nerf_forward (per-ray draws t_rand / u / noise are restricted to the dropped rays here).  Asserts that every
    dropped ray matches a branch and returns {"dropped", "unforced", "flipped", "unmatched"} (also printed)."""
    idx = torch.nonzero(drop)[:, 0]
    counts = {"dropped": int(idx.numel()), "unforced": 0, "flipped": 0, "unmatched": 0}
    if idx.numel() == 0:
        print(f"far-plane branch {label}: no dropped rays")
        return counts
    levels = len(hip)
    r = {k: rays[k][idx] for k in ("rays_o", "rays_d", "viewdirs")}
    kw = _take(kw, idx)
    sd64, r64, kw64 = {k: v.double() for k, v in sd.items()}, {k: v.double() for k, v in r.items()}, _f64(kw)
    got = [[hip[lvl][q][idx] for q in range(3)] for lvl in range(levels)]

    def matches(far_alpha):
        with torch.no_grad():
            o32 = orc.nerf_forward(sd, r, randomized, white_bkgd, near, far, num_levels=levels, far_alpha=far_alpha, **kw)
            o64 = orc.nerf_forward(sd64, r64, randomized, white_bkgd, near, far, num_levels=levels, far_alpha=far_alpha, **kw64)
        ok = torch.ones(idx.numel(), dtype=torch.bool)
        for lvl in range(levels):
            for q in range(3):
                if bars[lvl][q] is None:
                    continue
                err = _per_ray(got[lvl][q].double() - o64[lvl][q])
                spread = _per_ray(o32[lvl][q].double() - o64[lvl][q])
                ok &= err <= bars[lvl][q] + widen * spread
        return ok

    unforced = matches(None)
    any_branch = unforced.clone()
    for combo in itertools.product((0.0, 1.0), repeat=levels):
        any_branch |= matches(list(combo))
    counts["unforced"] = int(unforced.sum())
    counts["flipped"] = int((any_branch & ~unforced).sum())
    counts["unmatched"] = int((~any_branch).sum())
    print(f"far-plane branch {label}: {counts['dropped']} dropped rays -- {counts['unforced']} on the reference's branch, "
          f"{counts['flipped']} on a flipped branch, {counts['unmatched']} on none")
    if counts["unmatched"]:
        bad = idx[~any_branch][:8].tolist()
        detail = [(i, [tuple(float(_per_ray(hip[lvl][q][i:i + 1])) for q in range(3)) for lvl in range(levels)]) for i in bad]
        raise AssertionError(f"{label}: {counts['unmatched']} of {counts['dropped']} far-plane rays match no branch of the oracle, e.g. {detail}")
    return counts
