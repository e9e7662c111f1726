"""numpy reference of the early-ray-termination convention, written from the convention, not from the kernels:

* eps in [0, 1), rounds of R >= 1 sample indices; tau_stop = fp32(-log(eps)) computed in fp64 from the fp32 value of eps and rounded once;
  eps == 0: +inf (off);
* a level of S samples has ceil(S / R) rounds, round k covers [kR, min(S, (k+1)R)) of every ray;
* per ray tau (fp32, 0) and stop (int32, S).  After round k a ray with stop == S adds sigma_i * delta_i of the round's samples in ascending
  i, one sequential fp32 chain (multiply rounded, add rounded, no fma), and stops with stop = (k+1)R when tau >= tau_stop.  NaN never stops;
* the last round (the one that holds sample S-1 and its 1e10 interval) decides nothing;
* sigma_i: the activated density (relu(raw), or softplus(raw + sigma_bias)), 0 for a sentinel; delta_i = (t[i+1] - t[i]) * ||d||, each
  operation rounded to fp32, ||d|| = sqrt((dx dx + dy dy) + dz dz); delta_{S-1} = 1e10 * ||d||;
* a sample i >= stop of its ray is dead (sentinel record); a live one goes through the grid lookup of section 4.9.
"""
from __future__ import annotations

import numpy as np


def tau_stop(eps) -> np.float32:
    e = np.float64(np.float32(eps))
    if e == 0.0:
        return np.float32(np.inf)
    return np.float32(-np.log(e))


def num_rounds(S: int, R: int) -> int:
    return -(-S // R)


def dir_norm(d) -> np.ndarray:
    d = np.asarray(d, dtype=np.float32)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return np.sqrt(((x * x).astype(np.float32) + (y * y).astype(np.float32)).astype(np.float32) + (z * z).astype(np.float32), dtype=np.float32)


def deltas(t, d) -> np.ndarray:
    """(n, S) fp32 interval lengths as the compositing kernel forms them."""
    t = np.asarray(t, dtype=np.float32)
    dn = dir_norm(d)[:, None]
    out = np.empty_like(t)
    out[:, :-1] = ((t[:, 1:] - t[:, :-1]).astype(np.float32) * dn).astype(np.float32)
    out[:, -1] = (np.float32(1e10) * dn[:, 0]).astype(np.float32)
    return out


def relu_sigma(raw_sigma) -> np.ndarray:
    """fp32 relu; -inf (a sentinel) gives exactly 0."""
    return np.maximum(np.asarray(raw_sigma, dtype=np.float32), np.float32(0))


def sigma64(raw_sigma, act: str, sigma_bias: float = -1.0) -> np.ndarray:
    """fp64 activated density for the tolerance checks: 'relu' or 'softplus' (softplus(raw + sigma_bias); -inf gives 0)."""
    r = np.asarray(raw_sigma, dtype=np.float64)
    if act == "relu":
        return np.maximum(r, 0.0)
    x = r + np.float64(np.float32(sigma_bias))
    with np.errstate(over="ignore"):
        return np.where(x > 30.0, x, np.log1p(np.exp(np.minimum(x, 30.0))))


def stops(sigma, delta, eps, R: int) -> np.ndarray:
    """(n, S) fp32 sigma (already 0 where the grid is empty) and delta -> (n,) int32 stop indices, vectorised over rays."""
    sigma = np.asarray(sigma, dtype=np.float32)
    delta = np.asarray(delta, dtype=np.float32)
    n, S = sigma.shape
    ts = tau_stop(eps)
    tau = np.zeros(n, dtype=np.float32)
    stop = np.full(n, S, dtype=np.int32)
    for k in range(num_rounds(S, R)):
        s0, s1 = k * R, min(S, (k + 1) * R)
        if s1 == S:
            break   # the last round decides nothing
        live = stop == S
        for i in range(s0, s1):
            p = (sigma[:, i] * delta[:, i]).astype(np.float32)
            tau = np.where(live, (tau + p).astype(np.float32), tau)
        with np.errstate(invalid="ignore"):
            hit = live & (tau >= ts)
        stop[hit] = s1
    return stop


def boundary_tau64(sigma, delta, R: int) -> np.ndarray:
    """fp64 optical depth at every deciding round boundary: (n, B) with column k = sum over i < (k+1)R, B = the rounds before the last."""
    sigma = np.asarray(sigma, dtype=np.float64)
    delta = np.asarray(delta, dtype=np.float64)
    S = sigma.shape[1]
    cum = np.cumsum(sigma * delta, axis=1)
    ends = [min(S, (k + 1) * R) for k in range(num_rounds(S, R))]
    ends = [e for e in ends if e < S]
    return cum[:, [e - 1 for e in ends]] if ends else np.zeros((sigma.shape[0], 0))


def live_mask(stop, S: int) -> np.ndarray:
    """(n, S) bool: sample i of a ray is live iff i < stop."""
    return np.arange(S)[None, :] < np.asarray(stop)[:, None]
