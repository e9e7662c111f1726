"""The per-list merged composite of tests/_scene_lists_ref.composite_ref restated in torch, so that autograd gives its derivative with respect
to raw, in the manner of tests/_scene_grad_ref.py: every list is read by its own (act, opts, open_end), the merge
order of a ray comes from np.lexsort over (i, list, t), then gather, an exclusive cumprod and plain sums.

``round32=True`` is the function the HIP kernel evaluates: the interval lengths -- delta = fl(fl(t_{i+1} - t_i) * |d|), and for the last
sample of an open list fl(1e10f * |d|) --, the norm and raw + sigma_bias are formed in fp32 (they are part of the function), everything else
in raw's dtype.  ``round32=False`` forms them in the dtype too, which is composite_ref's own arithmetic."""
import numpy as np
import torch

import _scene_grad_ref as gref

F = np.float32


def list_deltas(t, slot, dirs, lists, dtype, round32=True):
    """(P, S) interval lengths of every row `slot` names: (t_{i+1} - t_i) |d| of the row's WORLD ray; the last one 0 for a closed list and
    1e10f |d| for an open one.  Rows nobody names get zeros."""
    t, dirs, slot = np.asarray(t, F), np.asarray(dirs, F), np.asarray(slot)
    P, S = t.shape
    nd = np.float32 if round32 else np.float64
    d = dirs.astype(nd)
    norm = np.sqrt(((d[:, 0] * d[:, 0]).astype(nd) + (d[:, 1] * d[:, 1]).astype(nd)).astype(nd) + (d[:, 2] * d[:, 2]).astype(nd)).astype(nd)
    out = np.zeros((P, S), nd)
    tt = t.astype(nd)
    far = nd(F(1e10))
    for k, (_act, _opts, open_end) in enumerate(lists):
        live = (slot[:, k] >= 0) & (slot[:, k] < P)
        rows, nr = slot[live, k], norm[live]
        out[rows, :-1] = ((tt[rows, 1:] - tt[rows, :-1]).astype(nd) * nr[:, None]).astype(nd)
        if open_end:
            out[rows, -1] = (far * nr).astype(nd)
    return torch.from_numpy(out.astype(np.float64)).to(dtype)


def composite_torch(raw, t, slot, dirs, white, lists, round32=True):
    """raw: torch (P, S, 4), fp64 or fp32, may require grad; t (P, S), slot (n, K), dirs (n, 3): arrays of fp32 / int32 values; lists: K
    tuples (act, opts or None, open_end) as tests/_scene_lists_ref.composite_ref takes them.
    -> dict(rgb (n, 3), acc (n,), depth (n,), obj_acc (n, K), weights (P, S)) in raw's dtype, differentiable with respect to raw."""
    dt = raw.dtype
    t, slot = np.asarray(t, F), np.asarray(slot)
    n, K = slot.shape
    P, S = t.shape
    assert len(lists) == K
    c, sigma = torch.zeros((P, S, 3), dtype=dt), torch.zeros((P, S), dtype=dt)
    for k, (act, opts, _open) in enumerate(lists):
        rows = slot[:, k][(slot[:, k] >= 0) & (slot[:, k] < P)]
        if len(rows):
            idx = torch.from_numpy(rows.astype(np.int64))
            # (activated on ALL rows and then picked: an element keeps its place in the vectorised loops, so homogeneous lists give
            # _scene_grad_ref.composite_torch's bits)
            ck, sk = gref._activate(raw, gref.sref.DEFAULT_ACT if opts is None else opts, act, round32)
            c, sigma = c.index_copy(0, idx, ck[idx]), sigma.index_copy(0, idx, sk[idx])
    alpha = (1.0 - torch.exp(-(sigma * list_deltas(t, slot, dirs, lists, dt, round32)))).reshape(-1)
    c = c.reshape(-1, 3)
    tt = torch.from_numpy(t.astype(np.float64)).to(dt).reshape(-1)
    rgb, acc, depth, obj = [], [], [], []
    weights = torch.zeros(P * S, dtype=dt)
    for r in range(n):
        idx, kk = gref.merge_index(t, slot[r], P)
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


def loss_of(out, g_rgb, g_acc=None, g_depth=None, g_obj_acc=None):
    loss = (out["rgb"] * torch.as_tensor(np.asarray(g_rgb, np.float64)).to(out["rgb"].dtype)).sum()
    for key, g in (("acc", g_acc), ("depth", g_depth), ("obj_acc", g_obj_acc)):
        if g is not None:
            loss = loss + (out[key] * torch.as_tensor(np.asarray(g, np.float64)).to(out[key].dtype)).sum()
    return loss


def composite_grads(raw, t, slot, dirs, white, lists, g_rgb, g_acc=None, g_depth=None, g_obj_acc=None):
    """d (sum of g . output) / d raw in fp64 on the fp32 inputs -> (P, S, 4) fp64 tensor; rows no slot entry names get zeros"""
    x = torch.as_tensor(np.asarray(raw, F).astype(np.float64)).requires_grad_(True)
    loss = loss_of(composite_torch(x, t, slot, dirs, white, lists, True), g_rgb, g_acc, g_depth, g_obj_acc)
    if not loss.requires_grad:      # no live row at all
        return torch.zeros_like(x)
    g, = torch.autograd.grad(loss, x)
    return g


def scene_level_oracle(sd, prefix, bg_sd, bg_prefix, pr, t, latents, rays_d, white, dtype, degrees=(0, 10, 4), opts=None):
    """One level of a scene + backdrop around the oracle's two networks, in the manner of _scene_grad_ref.scene_level_oracle: pr = the pairs
    WITH the backdrop's list last (tests/_scene_lists_ref.with_background_ref's dict, or the same arrays read back from
    ops.ScenePairs.with_background), t (P + n, S) fp32 -- data, shared with the implementation under test --, latents one dict per object,
    sd / bg_sd the two state dicts, all of torch tensors of `dtype` that may require grad.  orc.art_mlp per object segment, orc.nerf_mlp on
    the backdrop's rows, then composite_torch with K articulated closed lists and one vanilla open one."""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import nerf_oracle as orc

    K = len(latents)
    po, pd, pv = (torch.from_numpy(np.asarray(pr[k], F)).to(dtype) for k in ("o", "d", "v"))
    tt = torch.from_numpy(np.asarray(t, F)).to(dtype)
    pos = orc.cast_rays(tt, po, pd)
    venc, venc_art = orc.pos_enc(pv, 0, 4), orc.pos_enc(pv, 0, degrees[2])      # the backdrop's degrees are the defaults
    parts = []
    for k in range(K + 1):
        a, b = int(pr["offsets"][k]), int(pr["offsets"][k + 1])
        if b <= a:
            continue
        if k < K:
            rr, rs = orc.art_mlp(sd, prefix, pos[a:b], venc_art[a:b], latents[k], degrees[0], degrees[1])
        else:
            rr, rs = orc.nerf_mlp(bg_sd, bg_prefix, orc.pos_enc(pos[a:b], 0, 10), venc[a:b])
        parts.append(torch.cat([rr, rs], -1))
    raw = torch.cat(parts)
    lists = [(2, opts, False)] * K + [(1, None, True)]
    out = composite_torch(raw, t, pr["slot"], rays_d, white, lists)
    out["raw"] = raw
    return out
