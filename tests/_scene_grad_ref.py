"""The merged scene composite of tests/_scene_ref.composite_ref restated in torch, so that autograd gives its derivative with respect to raw
(DESIGN.md section 4.18): the merge order of a ray from np.lexsort over (i, object, t), then gather, an exclusive cumprod and plain sums.

``round32=True`` is the function the HIP kernels evaluate: the interval lengths delta = fl(fl(t_{i+1} - t_i) * |d|), the norm and
raw + sigma_bias are formed in fp32 (they are part of the function), everything else in raw's dtype.  ``round32=False`` forms them in the
dtype too, which is composite_ref's own arithmetic (tests/test_scene_grad_cpu.py compares the two forwards at 1e-12)."""
import numpy as np
import torch

import _scene_ref as sref

F = np.float32


def _activate(raw, opts, act, round32):
    dt = raw.dtype
    c, w = raw[..., :3], raw[..., 3]
    if act == 0:
        return c, w
    if act == 1:
        return torch.sigmoid(c), torch.relu(w)
    scale, shift, bias = (float(F(x)) for x in (1 + 2 * opts["rgb_padding"], opts["rgb_padding"], opts["density_bias"]))
    if round32:      # xs = fl32(raw + bias): raw plus a constant, so d xs / d raw = 1
        w32 = w.detach().to(torch.float32)
        with np.errstate(all="ignore"):
            xs32 = torch.from_numpy((w32.numpy().astype(F) + F(bias)).astype(F))
        shift_w = torch.where(torch.isfinite(w32), xs32.to(dt) - w.detach(), torch.full_like(w.detach(), bias))
        xs = w + shift_w
    else:
        xs = w + bias
    return torch.sigmoid(c) * scale - shift, torch.nn.functional.softplus(xs, beta=1.0, threshold=20.0)


def deltas(t, slot, dirs, dtype, round32=True):
    """(P, S) interval lengths: (t_{i+1} - t_i) |d| of the pair's WORLD ray, 0 at the last sample of a list"""
    t, dirs = np.asarray(t, F), np.asarray(dirs, F)
    P, S = t.shape
    ray_of = np.zeros(P, np.int64)
    r, k = np.nonzero((np.asarray(slot) >= 0) & (np.asarray(slot) < P))
    ray_of[np.asarray(slot)[r, k]] = r
    nd = np.float32 if round32 else np.float64
    d = dirs.astype(nd)
    norm = np.sqrt(((d[:, 0] * d[:, 0]).astype(nd) + (d[:, 1] * d[:, 1]).astype(nd)).astype(nd) + (d[:, 2] * d[:, 2]).astype(nd)).astype(nd)
    out = np.zeros((P, S), nd)
    tt = t.astype(nd)
    out[:, :-1] = ((tt[:, 1:] - tt[:, :-1]).astype(nd) * norm[ray_of][:, None]).astype(nd)
    return torch.from_numpy(out.astype(np.float64)).to(dtype)


def merge_index(t, slot_row, P):
    """flat indices p * S + i of one ray's live samples in ascending (t, object, i), and the object of each"""
    t = np.asarray(t, F)
    S = t.shape[1]
    ps, ks = [], []
    for k, p in enumerate(slot_row):
        if 0 <= int(p) < P:
            ps.append(int(p))
            ks.append(k)
    if not ps:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    pp = np.repeat(np.asarray(ps), S)
    kk = np.repeat(np.asarray(ks), S)
    ii = np.tile(np.arange(S), len(ps))
    order = np.lexsort((ii, kk, t[pp, ii]))
    return (pp * S + ii)[order], kk[order]


def composite_torch(raw, t, slot, dirs, white, opts=None, act=2, round32=True):
    """raw: torch (P, S, 4), fp64 or fp32, may require grad; t (P, S), slot (n, K), dirs (n, 3): arrays of fp32 / int32 values.
    -> dict(rgb (n, 3), acc (n,), depth (n,), obj_acc (n, K), weights (P, S)) in raw's dtype, differentiable with respect to raw."""
    opts = sref.DEFAULT_ACT if opts is None else opts
    dt = raw.dtype
    t, slot = np.asarray(t, F), np.asarray(slot)
    n, K = slot.shape
    P, S = t.shape
    c, sigma = _activate(raw, opts, act, round32)
    alpha = (1.0 - torch.exp(-(sigma * deltas(t, slot, dirs, dt, round32)))).reshape(-1)
    c = c.reshape(-1, 3)
    tt = torch.from_numpy(t.astype(np.float64)).to(dt).reshape(-1)
    rgb, acc, depth, obj = [], [], [], []
    weights = torch.zeros(P * S, dtype=dt)
    for r in range(n):
        idx, kk = merge_index(t, slot[r], P)
        if len(idx) == 0:
            rgb.append(torch.full((3,), 1.0 if white else 0.0, dtype=dt))
            acc.append(torch.zeros((), dtype=dt)); depth.append(torch.zeros((), dtype=dt)); obj.append(torch.zeros(K, dtype=dt))
            continue
        idx_t = torch.from_numpy(idx)
        a = alpha[idx_t]
        f = (1.0 - a) + 1e-10
        T = torch.cat([torch.ones(1, dtype=dt), torch.cumprod(f, 0)[:-1]])
        w = a * T
        s_w = w.sum()
        col = (w[:, None] * c[idx_t]).sum(0)
        rgb.append(col + (1.0 - s_w) if white else col)
        acc.append(s_w)
        depth.append((w * tt[idx_t]).sum())
        obj.append(torch.zeros(K, dtype=dt).index_add(0, torch.from_numpy(kk), w))
        weights = weights.index_add(0, idx_t, w)
    return dict(rgb=torch.stack(rgb), acc=torch.stack(acc), depth=torch.stack(depth), obj_acc=torch.stack(obj), weights=weights.reshape(P, S))


def composite_grads(raw, t, slot, dirs, white, g_rgb, g_acc=None, g_depth=None, g_obj_acc=None, opts=None, act=2):
    """d (sum of g . output) / d raw in fp64 on the fp32 inputs -> (P, S, 4) fp64 tensor; rows no slot entry names get zeros"""
    x = torch.as_tensor(np.asarray(raw, F).astype(np.float64)).requires_grad_(True)
    out = composite_torch(x, t, slot, dirs, white, opts, act, True)
    loss = (out["rgb"] * torch.as_tensor(np.asarray(g_rgb, np.float64))).sum()
    for key, g in (("acc", g_acc), ("depth", g_depth), ("obj_acc", g_obj_acc)):
        if g is not None:
            loss = loss + (out[key] * torch.as_tensor(np.asarray(g, np.float64))).sum()
    if not loss.requires_grad:      # no live pair at all
        return torch.zeros_like(x)
    g, = torch.autograd.grad(loss, x)
    return g


def scene_level_oracle(sd, prefix, pr, t, latents, rays_d, white, dtype, degrees=(0, 10, 4), opts=None):
    """One level of a scene around the oracle's network: pr = the pairs (tests/_scene_ref.pairs_ref's dict, or the same arrays read back from
    ops.scene_pairs), t (P, S) fp32 -- data, shared with the implementation under test --, latents one dict per object and sd the state dict,
    both of torch tensors of `dtype` that may require grad.  orc.art_mlp per object segment, then composite_torch."""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import nerf_oracle as orc

    po, pd, pv = (torch.from_numpy(np.asarray(pr[k], F)).to(dtype) for k in ("o", "d", "v"))
    tt = torch.from_numpy(np.asarray(t, F)).to(dtype)
    pos = orc.cast_rays(tt, po, pd)
    venc = orc.pos_enc(pv, 0, degrees[2])
    parts = []
    for k, lat in enumerate(latents):
        a, b = int(pr["offsets"][k]), int(pr["offsets"][k + 1])
        if b > a:
            rr, rs = orc.art_mlp(sd, prefix, pos[a:b], venc[a:b], lat, degrees[0], degrees[1])
            parts.append(torch.cat([rr, rs], -1))
    raw = torch.cat(parts) if parts else torch.zeros((0, t.shape[1], 4), dtype=dtype)
    return composite_torch(raw, t, pr["slot"], rays_d, white, opts)
