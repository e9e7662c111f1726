"""An independent numpy restatement of the scene contract (include/aon_hip_scene.h), as _bounds_ref.py is for the
per-ray bounds: the ray-object pairs in fp32 with one rounding per operation, the merged composite as a plain sort by (t, object, i) and a
serial loop in fp32 or fp64, and the whole render around the oracle's own network, samplers and inverse CDF."""
import numpy as np

import _bounds_ref as bref

F = np.float32


def object_rays(o, d, v, pose):
    """o' = R^T (o - c), d' = R^T d, v' = R^T v: component a as ((R[0][a] x_0) + R[1][a] x_1) + R[2][a] x_2, every operation rounded to fp32"""
    pose = np.asarray(pose, F).reshape(3, 4)
    R, c = pose[:, :3], pose[:, 3]

    def rt(x):
        cols = []
        for a in range(3):
            s = ((R[0, a] * x[:, 0]).astype(F) + (R[1, a] * x[:, 1]).astype(F)).astype(F)
            cols.append((s + (R[2, a] * x[:, 2]).astype(F)).astype(F))
        return np.stack(cols, -1)
    o, d, v = np.asarray(o, F), np.asarray(d, F), np.asarray(v, F)
    return rt((o - c[None, :]).astype(F)), rt(d), rt(v)


def pairs_ref(o, d, v, objects):
    """objects: [(pose (3, 4), box)] -> dict(offsets (K + 1,) int64, slot (n, K) int32, ray (P,) int32, o / d / v (P, 3), near / far (P,)):
    live pairs object-major, ascending ray index inside an object."""
    n, K = len(o), len(objects)
    slot = np.full((n, K), -1, np.int32)
    offsets = np.zeros(K + 1, np.int64)
    rows = {k: [] for k in ("ray", "o", "d", "v", "near", "far")}
    for k, (pose, box) in enumerate(objects):
        oo, od, ov = object_rays(o, d, v, pose)
        near, far = bref.ray_limits_box(oo, od, box)
        with np.errstate(all="ignore"):
            valid = far > near
            near = np.where(near < 0, F(0), near).astype(F)
            far = np.where(far < 0, F(0), far).astype(F)
            live = valid & (far > near)
        idx = np.nonzero(live)[0]
        slot[idx, k] = offsets[k] + np.arange(len(idx))
        offsets[k + 1] = offsets[k] + len(idx)
        for key, val in (("ray", idx.astype(np.int32)), ("o", oo[idx]), ("d", od[idx]), ("v", ov[idx]), ("near", near[idx]), ("far", far[idx])):
            rows[key].append(val)
    out = {key: np.concatenate(val) for key, val in rows.items()}
    out.update(offsets=offsets, slot=slot)
    return out


def activate(raw, opts, dtype):
    """articulated activations: sigma = softplus(raw + sigma_bias), rgb = sigmoid(raw) * rgb_scale - rgb_shift, the three scalars as fp32"""
    scale, shift, bias = (dtype(F(x)) for x in (1 + 2 * opts["rgb_padding"], opts["rgb_padding"], opts["density_bias"]))
    raw = np.asarray(raw).astype(dtype)
    x = (raw[..., 3] + bias).astype(dtype)
    with np.errstate(all="ignore"):
        sigma = (np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))).astype(dtype)
        rgb = ((dtype(1) / (dtype(1) + np.exp(-raw[..., :3]))).astype(dtype) * scale).astype(dtype) - shift
    return rgb.astype(dtype), sigma


def merge_order(t, slot_row):
    """the samples of one ray's live lists as (t, object, i, row), ascending by the key (t, object, i)"""
    keys = []
    for k, p in enumerate(slot_row):
        if int(p) >= 0:
            keys += [(t[int(p), i], k, i, int(p)) for i in range(t.shape[1])]
    keys.sort(key=lambda q: (q[0], q[1], q[2]))
    return keys


DEFAULT_ACT = {"rgb_padding": 0.001, "density_bias": -1.0}


def composite_ref(raw, t, slot, dirs, white, opts=None, dtype=np.float64):
    """raw (P, S, 4), t (P, S), slot (n, K), dirs (n, 3) world -> dict(rgb (n, 3), acc, depth (n,), obj_acc (n, K), weights (P, S)).  A plain
    sort of the ray's samples by (t, object, i) and one serial loop; every operation in `dtype`."""
    opts = DEFAULT_ACT if opts is None else opts
    raw, t, slot, dirs = np.asarray(raw), np.asarray(t).astype(dtype), np.asarray(slot), np.asarray(dirs).astype(dtype)
    n, K = slot.shape
    P, S = t.shape
    rgb_s, sigma = activate(raw, opts, dtype)
    norm = np.sqrt(((dirs[:, 0] * dirs[:, 0]).astype(dtype) + (dirs[:, 1] * dirs[:, 1]).astype(dtype)).astype(dtype)
                   + (dirs[:, 2] * dirs[:, 2]).astype(dtype)).astype(dtype)
    out = dict(rgb=np.zeros((n, 3), dtype), acc=np.zeros(n, dtype), depth=np.zeros(n, dtype), obj_acc=np.zeros((n, K), dtype),
               weights=np.zeros((P, S), dtype))
    one, eps = dtype(1), dtype(1e-10)
    for r in range(n):
        keys = merge_order(t, slot[r])
        T = one
        rgb, acc, depth = np.zeros(3, dtype), dtype(0), dtype(0)
        for tv, k, i, p in keys:
            delta = dtype((t[p, i + 1] - tv) * norm[r]) if i < S - 1 else dtype(0)
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


def over_composite(layers, white, dtype=np.float64):
    """Front-to-back over-compositing of objects rendered ALONE on a black background: layers = one (near (n,), rgb (n, 3), acc (n,)) per
    object, near = NaN where the ray misses it (rgb = acc = 0 there); per ray the objects are taken in ascending near -> (rgb, acc)."""
    n = len(layers[0][1])
    near = np.stack([np.where(np.isnan(l[0]), np.inf, l[0]) for l in layers], 1)
    order = np.argsort(near, axis=1, kind="stable")
    rgb, T = np.zeros((n, 3), dtype), np.ones(n, dtype)
    for j in range(len(layers)):
        for r in range(n):
            k = order[r, j]
            rgb[r] += T[r] * layers[k][1][r].astype(dtype)
            T[r] *= 1 - dtype(layers[k][2][r])
    acc = 1 - T
    if white:
        rgb = rgb + (1 - acc)[:, None]
    return rgb, acc


def render_scene_ref(sd, objects, latents, rays, white, num_levels=2, num_coarse=64, num_fine=128, opts=None, dtype=np.float64):
    """The whole render around the oracle: objects [(pose, box)], latents one dict per object, rays dict of (n, 3) arrays.  The pairs in fp32
    (they decide which lists exist), then per pair the oracle's sample_along_rays / art_mlp / sample_pdf in torch at `dtype`, merged by
    composite_ref; the fine draws come from the merged weights.  -> [dict per level] as composite_ref."""
    import os
    import sys

    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import nerf_oracle as orc

    td = torch.float64 if dtype == np.float64 else torch.float32
    pr = pairs_ref(rays["rays_o"], rays["rays_d"], rays["viewdirs"], objects)
    sdt = {k: v.to(td) for k, v in sd.items()}
    po, pd, pv = (torch.from_numpy(pr[k]).to(td) for k in ("o", "d", "v"))
    near, far = (torch.from_numpy(pr[k]).to(td)[:, None] for k in ("near", "far"))
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
        for k in range(len(objects)):
            a, b = int(pr["offsets"][k]), int(pr["offsets"][k + 1])
            if b > a:
                lat = {key: val.to(td) for key, val in latents[k].items()}
                rr, rs = orc.art_mlp(sdt, prefix, pos[a:b], venc[a:b], lat)
                raw[a:b] = torch.cat([rr, rs], -1)
        out = composite_ref(raw.numpy(), t.numpy(), pr["slot"], rays["rays_d"], white, opts, dtype)
        weights = torch.from_numpy(out["weights"]).to(td)
        levels.append(out)
    return levels
