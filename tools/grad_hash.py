"""SHA-256 of every gradient of one training step (articulated config-5 step and the vanilla 4096-ray step, seeded inputs): an A/B aid for
changes that must not move a bit -- run it with two builds of the library (AON_HIP_LIB=... selects an alternative build) and diff.
    python tools/grad_hash.py > a.txt;  AON_HIP_LIB=articulated-object-nerf_amd/libaon_hip_prev.so python tools/grad_hash.py > b.txt;  diff a.txt b.txt
--frozen: the outputs of the frozen networks' backwards instead (aon_art_render_bwd_latents, aon_art_render_bwd_inputs with and without the
latents wanted, aon_render_bwd_inputs) on 37 rays: one and two levels, the default sample counts and (39, 32), both stream forms."""
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


def main():
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
                for counts in ({}, dict(num_coarse_samples=39, num_fine_samples=32)):
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


if __name__ == "__main__":
    main()
