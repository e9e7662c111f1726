"""SHA-256 of every gradient of one training step (articulated config-5 step and the vanilla 4096-ray step, seeded inputs): an A/B aid for
changes that must not move a bit -- run it with two builds of the library (AON_HIP_LIB=... selects an alternative build) and diff.
    python tools/grad_hash.py > a.txt;  AON_HIP_LIB=articulated-object-nerf_amd/libaon_hip_prev.so python tools/grad_hash.py > b.txt;  diff a.txt b.txt
--frozen: the outputs of the frozen networks' backwards instead (aon_art_render_bwd_latents, aon_art_render_bwd_inputs with and without the
latents wanted, aon_render_bwd_inputs) on 37 rays: one and two levels, the default sample counts and (39, 32), both stream forms, and two
levels at (64, 224): a fine level of 289 samples, the 8-block form of the reduce kernel.
--composite: every kernel that differentiates or orders the composite (csrc/aon_composite_grad.h, csrc/aon_scene_merge.h) on seeded inputs made
here -- aon_composite_bwd, aon_scene_composite and aon_scene_composite_bwd at the block edges (64 / 65, 256 / 257 samples, K * S = 4096), all
three activations, both backgrounds, the optional gradients given and null, twins tied in t, sentinel records, dead slot entries -- and
the --frozen set.  `--composite --write COMMIT` writes tests/golden/g30_composite_hashes.json
(tests/test_hip_arena.py::test_composite_bits_are_pinned); COMMIT names the commit the library in use was built from.
--fit: the trajectories of the five fits on a frozen network (fit_latents, both fit_pose, fit_scene_codes, fit_scene_poses) on small seeded
cases: per case the (steps,) losses, every returned code and every returned pose.  `--fit --write COMMIT` writes
tests/golden/g31_fit_hashes.json (tests/test_hip_arena.py::test_fit_bits_are_pinned); COMMIT names the commit whose fit code ran."""
import hashlib
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def h(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def hashes(n=4096):
    """-> ordered list of (label, 16-hex-digit hash) for the articulated and the vanilla step on n seeded rays."""
    out = []
    _run(n, lambda *a: out.append((" ".join(a[:-1]), a[-1])))
    return out


def composite_hashes():
    """-> ordered list of (label, 16-hex-digit hash): the --composite set."""
    out = []
    emit = lambda *a: out.append((" ".join(a[:-1]), a[-1]))   # noqa: E731
    _run_composite(emit)
    _run_frozen(emit)
    return out


def fit_hashes():
    """-> ordered list of (label, 16-hex-digit hash): the --fit set."""
    out = []
    _run_fit(lambda *a: out.append((" ".join(a[:-1]), a[-1])))
    return out


def main():
    if "--fit" in sys.argv:
        got = fit_hashes()
        if "--write" in sys.argv:
            import json

            commit = sys.argv[sys.argv.index("--write") + 1]
            path = os.path.join(ROOT, "tests", "golden", "g31_fit_hashes.json")
            json.dump({"note": "sha256[:16] of the losses, codes and poses of fit_latents, both fit_pose, fit_scene_codes and fit_scene_poses on "
                               "seeded cases on gfx950, written by `python tools/grad_hash.py --fit --write <library_commit>` with the fit "
                               "code of library_commit", "library_commit": commit, "hashes": dict(got)}, open(path, "w"), indent=0)
            print("wrote", path, len(got))
            return
        for label, digest in got:
            print(label, digest)
        return
    if "--composite" in sys.argv:
        got = composite_hashes()
        if "--write" in sys.argv:
            import json

            commit = sys.argv[sys.argv.index("--write") + 1]
            path = os.path.join(ROOT, "tests", "golden", "g30_composite_hashes.json")
            json.dump({"note": "sha256[:16] of the outputs of aon_composite_bwd, aon_scene_composite, aon_scene_composite_bwd and the frozen networks' "
                               "backwards on seeded inputs on gfx950, written by `AON_HIP_LIB=<library built from library_commit> python "
                               "tools/grad_hash.py --composite --write <library_commit>`", "library_commit": commit, "hashes": dict(got)},
                      open(path, "w"), indent=0)
            print("wrote", path, len(got))
            return
        for label, digest in got:
            print(label, digest)
        return
    if "--write" in sys.argv:     # tests/golden/g24_gradient_hashes.json (tests/test_hip_arena.py::test_gradient_bits_are_pinned)
        import json

        path = os.path.join(ROOT, "tests", "golden", "g24_gradient_hashes.json")
        json.dump({"n_rays": 4096, "note": "sha256[:16] of every gradient of the seeded articulated / vanilla 4096-ray steps on gfx950 (tools/grad_hash.py)",
                   "hashes": dict(hashes(4096))}, open(path, "w"), indent=0)
        print("wrote", path)
        return
    if "--frozen" in sys.argv:
        _run_frozen(lambda *a: print(*a))
        return
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    _run(n, lambda *a: print(*a))


def _run(n, emit):
    import aon_amd.synthetic as syn
    from aon_amd.models.code_library import CodeLibraryArticulated
    from aon_amd.models.vanilla_nerf.helper import train_loss
    from aon_amd.models.vanilla_nerf.model import NeRF
    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

    dev = torch.device("cuda:0")
    rays = {k: v.to(dev) for k, v in syn.random_rays(n, seed=11).items()}
    target = syn.seeded_uniform(12, n, 3).to(dev)
    tr, u = syn.seeded_uniform(13, n, 65).to(dev), syn.seeded_uniform(14, n, 128).to(dev)
    model = NeRF_AE_Art().to(dev)
    model.load_state_dict(syn.make_art_state_dict(seed=0, density_scale=30.0))
    lib = CodeLibraryArticulated(types.SimpleNamespace(N_max_objs=1, N_obj_code_length=128)).to(dev)
    lib.load_state_dict(syn.make_code_library_state(seed=0, n_max_objs=1))
    lat = lib({"instance_id": torch.tensor([0], device=dev), "articulation_id": torch.tensor([3], device=dev)})
    out = model(rays, True, True, 2.0, 6.0, lat, t_rand=tr, u=u)
    loss, _ = train_loss(out, target, (lat["density"], lat["color"], lat["articulation"]), 1e-4)
    loss.backward()
    emit("art loss", h(loss))
    for k, p in list(model.named_parameters()) + [("lib." + k, p) for k, p in lib.named_parameters()]:
        emit("art", k, h(p.grad))
    van = NeRF().to(dev)
    van.load_state_dict(syn.make_nerf_state_dict(seed=0, density_scale=30.0))
    out = van(rays, True, True, 2.0, 6.0, t_rand=tr, u=u)
    loss, _ = train_loss(out, target)
    loss.backward()
    emit("van loss", h(loss))
    for k, p in van.named_parameters():
        emit("van", k, h(p.grad))


def _run_frozen(emit, n=37):
    import aon_amd.synthetic as syn
    from aon_amd import ops

    dev = torch.device("cuda:0")
    r = syn.random_rays(n, seed=11)
    o, d, v = (r[k].to(dev) for k in ("rays_o", "rays_d", "viewdirs"))
    nets = {}
    for art, sd in ((True, syn.make_art_state_dict(seed=0, density_scale=2.0)), (False, syn.make_nerf_state_dict(seed=0, density_scale=30.0))):
        nets[art] = [{k[len(p):]: t.to(dev) for k, t in sd.items() if k.startswith(p)} for p in ("coarse_mlp.", "fine_mlp.")]
    lat = {k: (0.2 * syn.seeded_uniform(30 + i, 1, w) - 0.1).to(dev) for i, (k, w) in enumerate(ops._LATENT_KEYS)}
    g_rgb = [(syn.seeded_uniform(142 + l, n, 3) - 0.5).to(dev) for l in range(2)]
    g_acc, g_depth = (syn.seeded_uniform(144, n) - 0.5).to(dev), (syn.seeded_uniform(145, n) - 0.5).to(dev)
    before = ops.bottleneck_fold()
    try:
        for fold in (True, False):
            ops.set_bottleneck_fold(fold)
            art_pk = {"fwd": [ops.pack_art_mlp(p) for p in nets[True]], "small": [ops.art_prepare(p, lat) for p in nets[True]],
                      "bwd": [ops.pack_art_mlp_bwd(p) for p in nets[True]]}
            van_pk = {"fwd": [ops.pack_vanilla_mlp(p) for p in nets[False]], "bwd": [ops.pack_vanilla_mlp_bwd(p) for p in nets[False]]}
            for k in (1, 2):
                for counts in ({}, dict(num_coarse_samples=39, num_fine_samples=32), dict(num_fine_samples=224)):
                    if k == 1 and counts.get("num_fine_samples") == 224:
                        continue      # (the long fine level is the case)
                    nc, nf = counts.get("num_coarse_samples", 64), counts.get("num_fine_samples", 128)
                    t_rand, u = syn.seeded_uniform(140, n, nc + 1).to(dev), (syn.seeded_uniform(141, n, nf).to(dev) if k == 2 else None)
                    tag = f"{'folded' if fold else 'literal'} L{k} {nc}+{nf}"
                    up = (True, k, g_rgb[:k], [None] * (k - 1) + [g_acc], [g_depth] + [None] * (k - 1))   # white_bkgd, levels, the upstream gradients

                    def forward(pk, art):
                        sm = pk["small"] if art else [None, None]
                        return ops.render_fwd_train(pk["fwd"][0], pk["fwd"][1] if k == 2 else None, o, d, v, 2.0, 6.0, True, k, t_rand, u, small_c=sm[0],
                                                    small_f=sm[1] if k == 2 else None, opts=ops.RenderOpts(**counts))

                    for which in ("latents", "inputs", "inputs_nolatents"):
                        _, ws, geometry = forward(art_pk, True)
                        head = (ws, art_pk["bwd"][:k], art_pk["small"][:k])
                        if which == "latents":
                            g_lat, g_rays = ops.art_render_bwd_latents(*head, d, *up, nets[True][:k], geometry=geometry), ()
                        else:
                            g_lat, *g_rays = ops.art_render_bwd_inputs(*head, o, d, v, *up, nets[True][:k], geometry=geometry, want_latents=which == "inputs")
                        ops.pool_give(ws)
                        for key, g in (g_lat or {}).items():
                            emit("art", which, tag, key, h(g))
                        for name, g in zip(("g_rays_o", "g_rays_d", "g_viewdirs"), g_rays):
                            emit("art", which, tag, name, h(g))
                    _, ws, geometry = forward(van_pk, False)
                    g_rays = ops.render_bwd_inputs(ws, van_pk["bwd"][:k], van_pk["fwd"][:k], o, d, v, *up, nets[False][:k], geometry=geometry)
                    ops.pool_give(ws)
                    for name, g in zip(("g_rays_o", "g_rays_d", "g_viewdirs"), g_rays):
                        emit("van", "inputs", tag, name, h(g))
    finally:
        ops.set_bottleneck_fold(before)


def _unit(seed, *shape):
    import aon_amd.synthetic as syn

    return syn.seeded_uniform(seed, *shape)


def _raw(seed, act, *shape):
    """records (…, 4) in [-2, 2); a raw density that is used as it is (act 0) is not negative"""
    raw = 4.0 * _unit(seed, *shape, 4) - 2.0
    if act == 0:
        raw[..., 3] = raw[..., 3].abs()
    return raw


def _scene_case(kind, n, K, S, seed):
    """-> (slot (n, K), P, t (P, S) ascending in [2, 6], rays_d): about a third of the pairs dead, ray 0 without a pair, ray 1 with all K,
    rows object-major and ascending with the ray as aon_scene_pairs lays them out"""
    live = _unit(seed, n, K) < 0.67
    live[0], live[1] = False, True
    if kind == "twins":
        live[:] = True
    flat = live.T.reshape(-1)
    rows = torch.cumsum(flat.to(torch.int64), 0) - 1
    slot = torch.where(flat, rows, torch.full_like(rows, -1)).reshape(K, n).T.contiguous().to(torch.int32)
    P = int(flat.sum())
    t = 2.0 + 4.0 * torch.sort(_unit(seed + 1, P, S), dim=1).values
    if kind == "twins":         # object 1's lists are object 0's, t for t
        t[n:] = t[:n]
    if kind == "dead_slot":     # entries that name no row: -1 already; a row past the pairs is dead too (ray 0 still has no pair)
        slot[0, 0], slot[0, 1] = P + 5, P
    return slot, P, t.contiguous(), (_unit(seed + 2, n, 3) - 0.5).contiguous()


def _run_composite(emit):
    from aon_amd import ops

    dev = torch.device("cuda:0")
    for n, S in ((5, 2), (5, 64), (5, 65), (37, 193), (3, 257), (3, 512)):
        t = (2.0 + 4.0 * torch.sort(_unit(200 + S, n, S), dim=1).values).to(dev)
        dirs = (_unit(201 + S, n, 3) - 0.5).to(dev)
        g_rgb, g_acc, g_depth = ((_unit(202 + S + i, *sh) - 0.5).to(dev) for i, sh in enumerate(((n, 3), (n,), (n,))))
        for act in (0, 1, 2):
            raw = _raw(210 + S + act, act, n * S).to(dev)
            for white in (True, False):
                for given in (True, False):
                    d_raw = ops.composite_bwd(raw, t, dirs, g_rgb, g_acc if given else None, g_depth if given else None, white, act, n * S)
                    emit("composite_bwd", f"n{n} S{S} act{act}", "white" if white else "black", "all" if given else "rgb_only", "d_raw", h(d_raw))
    sizes = [("plain", n, K, S) for n, K, S in ((5, 2, 2), (5, 2, 3), (37, 3, 65), (9, 5, 13), (20, 16, 193), (7, 16, 256))]
    for kind, n, K, S in sizes + [("twins", 9, 2, 17), ("sentinel", 9, 5, 13), ("dead_slot", 37, 3, 65)]:
        slot, P, t, dirs = _scene_case(kind, n, K, S, 300 + 7 * K + S)
        pairs = types.SimpleNamespace(n=n, K=K, P=P, slot=slot.to(dev))
        t, dirs = t.to(dev), dirs.to(dev)
        g = [(_unit(310 + K + S + i, *sh) - 0.5).to(dev) for i, sh in enumerate(((n, 3), (n,), (n,), (n, K)))]
        for act in (0, 1, 2):
            raw = _raw(320 + K + S + act, act, P, S)
            if kind == "sentinel":
                mask = _unit(330 + act, P, S) < 0.3
                mask[1] = True      # a whole list
                raw[mask] = torch.tensor([0.0, 0.0, 0.0, float("-inf")])
            raw = raw.to(dev)
            for white in (True, False):
                tag = (kind, f"n{n} K{K} S{S} act{act}", "white" if white else "black")
                outs = ops.scene_composite(raw, t, pairs, dirs, white, act=act)
                for name, x in zip(("rgb", "acc", "depth", "obj_acc", "weights"), outs):
                    emit("scene_composite", *tag, name, h(x))
                for given in (True, False):
                    extra = dict(g_acc=g[1], g_depth=g[2], g_obj_acc=g[3]) if given else {}
                    d_raw = ops.scene_composite_bwd(raw, t, pairs, dirs, g[0], white_bkgd=white, act=act, **extra)
                    emit("scene_composite_bwd", *tag, "all" if given else "rgb_only", "d_raw", h(d_raw))


def _run_fit(emit):
    """Single object: the default networks at both levels (65 / 193 samples), two 6 x 8 views (48 rays).  Scenes: K = 2, an 8 x 12 frame, one
    level of 33 samples, degrees (0, 3, 2), the density bias lowered by 2, two batches of the same rays with different targets.  The targets
    are seeded noise: nothing is to be recovered, every step has a gradient."""
    import numpy as np

    import aon_amd.synthetic as syn
    from aon_amd import ops
    from aon_amd.models.vanilla_nerf.model import LitNeRF
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    dev = torch.device("cuda:0")
    keys = [k for k, _ in ops._LATENT_KEYS]

    def emit_codes(tag, codes):
        for k in keys:
            emit(tag, k, h(codes[k]))

    def art(**kw):
        lit = LitNeRF_AutoDecoder(hparams={"N_max_objs": 2}, near=2.0, far=6.0, white_bkgd=True, **kw).to(dev)
        lit.code_library.load_state_dict(syn.make_code_library_state(seed=0, n_max_objs=2))
        return lit

    # ---- one object
    H, W = 6, 8
    focal = syn.focal_from_fovy(H)
    cams = [syn.look_at_pose(azim_deg=a) for a in (20.0, 75.0)]
    targets = [syn.seeded_uniform(400 + v, H * W, 3).to(dev) for v in range(2)]
    batches = []
    for c2w, target in zip(cams, targets):
        ro, vd = ops.raygen(c2w, H, W, focal, device=dev)
        batches.append({"rays_o": ro, "rays_d": vd, "viewdirs": vd, "target": target})
    views = [{"directions": ops.ray_directions(H, W, focal, device=dev).reshape(-1, 3), "target": target} for target in targets]
    for tag, kw, steps in (("fit_latents randomized", dict(randomized=True), 4), ("fit_latents ray_box", dict(randomized=False, ray_box=2.0), 3)):
        lit = art(**kw)
        lit.model.load_state_dict(syn.make_art_state_dict(seed=2, density_scale=10.0))
        codes, losses = lit.fit_latents(batches, steps, lr=5e-3, init=(1, 3), seed=3)
        emit(tag, "losses", h(losses))
        emit_codes(tag, codes)
    lit = art(randomized=False)
    lit.model.load_state_dict(syn.make_art_state_dict(seed=2, density_scale=10.0))
    for tag, kw in (("art fit_pose", dict(lr=5e-3)), ("art fit_pose codes", dict(lr=(2e-3, 5e-3), fit_codes=True))):
        poses, codes, losses = lit.fit_pose(views, 5, codes=(1, 3), poses=cams, seed=3, **kw)     # view 0 takes 3 steps, view 1 takes 2
        emit(tag, "losses", h(losses))
        for v, p in enumerate(poses):
            emit(tag, f"pose{v}", h(p))
        emit_codes(tag, codes)
    van = LitNeRF(randomized=False, near=2.0, far=6.0, white_bkgd=True).to(dev)
    van.model.load_state_dict(syn.make_nerf_state_dict(seed=0, density_scale=30.0))
    poses, losses = van.fit_pose(views, 5, lr=5e-3, poses=cams, seed=3)
    emit("van fit_pose", "losses", h(losses))
    for v, p in enumerate(poses):
        emit("van fit_pose", f"pose{v}", h(p))

    # ---- scenes
    degrees = dict(min_deg_point=0, max_deg_point=3, deg_view=2)
    lit = art(randomized=False, model_kwargs=dict(num_levels=1, num_coarse_samples=32, **degrees))
    sd = syn.make_art_state_dict(seed=2, density_scale=30.0, **degrees)
    sd["coarse_mlp.density_layer.bias"] = sd["coarse_mlp.density_layer.bias"] - 2.0
    lit.model.load_state_dict(sd)

    def pose(seed, centre):      # tests/test_hip_scene.py::pose
        w = np.random.default_rng(seed).normal(size=3)
        R = ops.so3_exp(torch.tensor(w / np.linalg.norm(w) * (0.3 + 0.2 * seed % 2.5), dtype=torch.float64)).float()
        return torch.cat([R, torch.tensor(centre, dtype=torch.float32)[:, None]], 1)

    H, W = 8, 12
    placements = [(0, 4, pose(1, (0.35, 0.0, 0.0)), 1.6), (1, 11, pose(2, (-0.45, 0.1, 0.1)), 1.4)]
    rays = {k: v.to(dev) for k, v in syn.make_rays(H, W, syn.look_at_pose(4.0, 30.0, 30.0), syn.focal_from_fovy(H, 30.0)).items()}
    frames = [{**rays, "target": syn.seeded_uniform(410 + b, H * W, 3).to(dev)} for b in range(2)]
    for tag, kw in (("fit_scene_codes", {}), ("fit_scene_codes articulation", dict(fit_keys=("articulation",)))):
        codes, losses = lit.fit_scene_codes(frames, placements, 4, lr=5e-3, **kw)
        emit(tag, "losses", h(losses))
        for j, c in enumerate(codes):
            emit_codes(f"{tag} obj{j}", c)
    for tag, lr, fit_codes in (("fit_scene_poses", 2e-3, False), ("fit_scene_poses codes", (2e-3, 5e-3), True)):
        poses, codes, losses = lit.fit_scene_poses(frames, placements, 4, lr, fit_codes=fit_codes)
        emit(tag, "losses", h(losses))
        for j, (p, c) in enumerate(zip(poses, codes)):
            emit(f"{tag} obj{j}", "pose", h(p))
            emit_codes(f"{tag} obj{j}", c)


if __name__ == "__main__":
    main()
