"""An independent numpy restatement of the per-list merged composite (include/aon_hip_scene_lists.h), in the style
of _scene_ref.py: every list of a scene carries its own activation (none / vanilla / articulated) and end rule (closed, or the reference's
1e10-long last interval), the merge is a plain sort by (t, list, i) and a serial loop in fp32 or fp64; and the whole render around the
oracle with the vanilla oracle network as the last list."""
import numpy as np

import _scene_ref as sref

F = np.float32
ACT_NONE, ACT_VANILLA, ACT_ARTICULATED = 0, 1, 2


def activate_list(raw, act, opts, dtype):
    """raw (..., 4) of ONE list -> (rgb (..., 3), sigma (...)) in `dtype`"""
    raw = np.asarray(raw).astype(dtype)
    if act == ACT_ARTICULATED:
        return sref.activate(raw, sref.DEFAULT_ACT if opts is None else opts, dtype)
    if act == ACT_VANILLA:
        with np.errstate(all="ignore"):
            rgb = (dtype(1) / (dtype(1) + np.exp(-raw[..., :3])).astype(dtype)).astype(dtype)
        return rgb, np.maximum(raw[..., 3], dtype(0)).astype(dtype)
    return raw[..., :3].copy(), raw[..., 3].copy()


def composite_ref(raw, t, slot, dirs, white, lists, dtype=np.float64):
    """raw (P, S, 4), t (P, S), slot (n, K), dirs (n, 3) world, lists: K tuples (act, opts or None, open_end)
    -> dict(rgb (n, 3), acc, depth (n,), obj_acc (n, K), weights (P, S)).  Sample i of list k: sigma / rgb by lists[k]'s activation,
    delta = (t_{i+1} - t_i) N, the last one 0 or -- open_end -- 1e10 N (the fp32 constant 1e10f, times N, then sigma times that)."""
    raw, t, slot, dirs = np.asarray(raw), np.asarray(t).astype(dtype), np.asarray(slot), np.asarray(dirs).astype(dtype)
    n, K = slot.shape
    P, S = t.shape
    assert len(lists) == K
    rgb_s, sigma = np.zeros((P, S, 3), dtype), np.zeros((P, S), dtype)
    for k, (act, opts, _open) in enumerate(lists):
        rows = slot[:, k][slot[:, k] >= 0]
        if len(rows):
            rgb_s[rows], sigma[rows] = activate_list(raw[rows], act, opts, dtype)
    norm = np.sqrt(((dirs[:, 0] * dirs[:, 0]).astype(dtype) + (dirs[:, 1] * dirs[:, 1]).astype(dtype)).astype(dtype)
                   + (dirs[:, 2] * dirs[:, 2]).astype(dtype)).astype(dtype)
    out = dict(rgb=np.zeros((n, 3), dtype), acc=np.zeros(n, dtype), depth=np.zeros(n, dtype), obj_acc=np.zeros((n, K), dtype),
               weights=np.zeros((P, S), dtype))
    one, eps, far = dtype(1), dtype(1e-10), dtype(F(1e10))
    for r in range(n):
        keys = sref.merge_order(t, slot[r])
        T = one
        rgb, acc, depth = np.zeros(3, dtype), dtype(0), dtype(0)
        for tv, k, i, p in keys:
            if i < S - 1:
                delta = dtype((t[p, i + 1] - tv) * norm[r])
            else:
                delta = dtype(far * norm[r]) if lists[k][2] else dtype(0)
            with np.errstate(all="ignore"):
                alpha = dtype(one - np.exp(dtype(-(sigma[p, i] * delta))))
            w = dtype(alpha * T)
            T = dtype(T * dtype(dtype(one - alpha) + eps))
            rgb = (rgb + (w * rgb_s[p, i]).astype(dtype)).astype(dtype)
            acc = dtype(acc + w)
            depth = dtype(depth + dtype(w * tv))
            out["obj_acc"][r, k] = dtype(out["obj_acc"][r, k] + w)
            out["weights"][p, i] = w
        if white:
            rgb = (rgb + dtype(one - acc)).astype(dtype)
        out["rgb"][r], out["acc"][r], out["depth"][r] = rgb, acc, depth
    return out


def with_background_ref(pr, rays, near, far):
    """pairs_ref's dict (or None: no objects) extended by the backdrop's list: n rows after the objects', world rays, slot column P + r"""
    n = len(rays["rays_o"])
    if pr is None:
        pr = dict(offsets=np.zeros(1, np.int64), slot=np.zeros((n, 0), np.int32), ray=np.zeros(0, np.int32), o=np.zeros((0, 3), F),
                  d=np.zeros((0, 3), F), v=np.zeros((0, 3), F), near=np.zeros(0, F), far=np.zeros(0, F))
    P = int(pr["offsets"][-1])
    rows = np.arange(n, dtype=np.int32)
    bound = lambda x: np.broadcast_to(np.asarray(x, F).reshape(-1), (n,)).astype(F)   # noqa: E731
    return dict(offsets=np.concatenate([pr["offsets"], [P + n]]).astype(np.int64), slot=np.concatenate([pr["slot"], (rows + P)[:, None]], 1).astype(np.int32),
                ray=np.concatenate([pr["ray"], rows]), o=np.concatenate([pr["o"], np.asarray(rays["rays_o"], F)]),
                d=np.concatenate([pr["d"], np.asarray(rays["rays_d"], F)]), v=np.concatenate([pr["v"], np.asarray(rays["viewdirs"], F)]),
                near=np.concatenate([pr["near"], bound(near)]), far=np.concatenate([pr["far"], bound(far)]))


def render_scene_ref(sd, objects, latents, rays, white, bg_sd, bg_near, bg_far, num_levels=2, num_coarse=64, num_fine=128, opts=None,
                     dtype=np.float64, return_raw=False):
    """_scene_ref.render_scene_ref with the vanilla oracle network `bg_sd` as the last list: objects [(pose, box)] (may be empty), latents one
    dict per object, rays dict of (n, 3) arrays, bg_near / bg_far numbers or (n,) arrays.  The pairs in fp32, then per row the oracle's
    sample_along_rays / art_mlp or nerf_mlp / sample_pdf in torch at `dtype`, merged by composite_ref; the fine draws of every list come
    from the merged weights.  -> [dict per level] as composite_ref (with "raw" and "t" added when return_raw)."""
    import os
    import sys

    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import nerf_oracle as orc

    td = torch.float64 if dtype == np.float64 else torch.float32
    K = len(objects)
    pr = with_background_ref(sref.pairs_ref(rays["rays_o"], rays["rays_d"], rays["viewdirs"], objects) if K else None, rays, bg_near, bg_far)
    sdt, bgt = {k: v.to(td) for k, v in sd.items()}, {k: v.to(td) for k, v in bg_sd.items()}
    po, pd, pv = (torch.from_numpy(pr[k]).to(td) for k in ("o", "d", "v"))
    near, far = (torch.from_numpy(pr[k]).to(td)[:, None] for k in ("near", "far"))
    lists = [(ACT_ARTICULATED, opts, False)] * K + [(ACT_VANILLA, None, True)]
    levels, t, weights = [], None, None
    for level in range(num_levels):
        prefix = "coarse_mlp." if level == 0 else "fine_mlp."
        if level == 0:
            t, pos = orc.sample_along_rays(po, pd, num_coarse, near, far, False)
        else:
            mids = 0.5 * (t[..., 1:] + t[..., :-1])
            t, pos = orc.sample_pdf(mids, weights[..., 1:-1], po, pd, t, num_fine, False)
        raw = torch.zeros(t.shape + (4,), dtype=td)
        venc = orc.pos_enc(pv, 0, 4)
        for k in range(K + 1):
            a, b = int(pr["offsets"][k]), int(pr["offsets"][k + 1])
            if b <= a:
                continue
            if k < K:
                lat = {key: val.to(td) for key, val in latents[k].items()}
                rr, rs = orc.art_mlp(sdt, prefix, pos[a:b], venc[a:b], lat)
            else:
                rr, rs = orc.nerf_mlp(bgt, prefix, orc.pos_enc(pos[a:b], 0, 10), venc[a:b])
            raw[a:b] = torch.cat([rr, rs], -1)
        out = composite_ref(raw.numpy(), t.numpy(), pr["slot"], rays["rays_d"], white, lists, dtype)
        weights = torch.from_numpy(out["weights"]).to(td)
        if return_raw:
            out["raw"], out["t"], out["bg_rows"] = raw.numpy(), t.numpy(), slice(int(pr["offsets"][K]), int(pr["offsets"][K + 1]))
        levels.append(out)
    return levels
