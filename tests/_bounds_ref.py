"""An independent numpy restatement of the per-ray bounds convention, as _occ_ref.py is for the occupancy grid:
the ray-box limits, the fix-up with its `live` rule, and the per-ray stratified t.  fp32 throughout, one rounding per operation."""
import numpy as np

F = np.float32


def _box(box):
    if np.isscalar(box):
        half = box / 2
        return np.full(3, -1 * half, F), np.full(3, 1 * half, F)
    return np.asarray(box[0], F).reshape(3), np.asarray(box[1], F).reshape(3)


def _tmax(a, b):
    """torch.max of two tensors: NaN if either is NaN"""
    out = np.where(a < b, b, a)
    return np.where(np.isnan(a) | np.isnan(b), F(np.nan), out).astype(F)


def _tmin(a, b):
    out = np.where(b < a, b, a)
    return np.where(np.isnan(a) | np.isnan(b), F(np.nan), out).astype(F)


def ray_limits_box(o, d, box):
    """-> (near, far), (n,) fp32 each: the slab test of the reference, (-1, -2) for the rays it rejects; its NaNs kept."""
    o, d = np.asarray(o, F), np.asarray(d, F)
    lo, hi = _box(box)
    with np.errstate(all="ignore"):
        inv = (F(1) / d).astype(F)
        neg = inv < 0
        t0 = ((np.where(neg, hi, lo).astype(F) - o).astype(F) * inv).astype(F)   # entry per axis
        t1 = ((np.where(neg, lo, hi).astype(F) - o).astype(F) * inv).astype(F)   # exit per axis
        valid = ~((t0[:, 0] > t1[:, 1]) | (t0[:, 1] > t1[:, 0]))
        tmin, tmax = _tmax(t0[:, 0], t0[:, 1]), _tmin(t1[:, 0], t1[:, 1])
        valid &= ~((tmin > t1[:, 2]) | (t0[:, 2] > tmax))
        tmin, tmax = _tmax(tmin, t0[:, 2]), _tmin(tmax, t1[:, 2])
    return np.where(valid, tmin, F(-1)).astype(F), np.where(valid, tmax, F(-2)).astype(F)


def ray_limits(o, d, box):
    """-> (near, far, live): invalid rays (not far > near) take min(near) / max(far) of the valid ones when there is one; negatives are
    clamped to 0; live = valid and far > near after the clamp."""
    near, far = ray_limits_box(o, d, box)
    with np.errstate(all="ignore"):
        valid = far > near
        if valid.any():
            near = np.where(valid, near, near[valid].min()).astype(F)
            far = np.where(valid, far, far[valid].max()).astype(F)
        near = np.where(near < 0, F(0), near).astype(F)
        far = np.where(far < 0, F(0), far).astype(F)
        live = valid & (far > near)
    return near, far, live.astype(np.uint8)


def linspace01(steps):
    """torch.linspace(0, 1, steps) in fp32: step * i below the middle, 1 - step * (steps - 1 - i) as ONE fused multiply-add above it (the
    product and the sum are exact in fp64 here, so fp64 arithmetic rounded once is the fused result)."""
    step = F(1) / F(steps - 1)
    i = np.arange(steps)
    low = (step * i.astype(F)).astype(F)
    high = (1.0 - np.float64(step) * (steps - 1 - i).astype(np.float64)).astype(F)
    return np.where(i < steps // 2, low, high).astype(F)


def sample_t(near, far, S, lindisp=False, t_rand=None):
    """helper.sample_along_rays with (n,) near / far -> (n, S) t"""
    near, far = np.asarray(near, F).reshape(-1, 1), np.asarray(far, F).reshape(-1, 1)
    s = linspace01(S)[None, :]
    one_minus = (F(1) - s).astype(F)
    with np.errstate(all="ignore"):
        if lindisp:
            inv_n, inv_f = (F(1) / near).astype(F), (F(1) / far).astype(F)
            t = (F(1) / ((inv_n * one_minus).astype(F) + (inv_f * s).astype(F)).astype(F)).astype(F)
        else:
            t = ((near * one_minus).astype(F) + (far * s).astype(F)).astype(F)
        if t_rand is not None:
            mids = (F(0.5) * (t[:, 1:] + t[:, :-1]).astype(F)).astype(F)
            upper = np.concatenate([mids, t[:, -1:]], -1)
            lower = np.concatenate([t[:, :1], mids], -1)
            t = (lower + ((upper - lower).astype(F) * np.asarray(t_rand, F)).astype(F)).astype(F)
    return t
