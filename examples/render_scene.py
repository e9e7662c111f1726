"""Several instances of one trained category-level model in ONE frame: train ``LitNeRF_AutoDecoder`` briefly on the
synthetic multi-instance set of examples/run_autodecoder.py, place three instances at different articulations and poses -- two of them with
overlapping boxes -- and write the image, the depth map and the instance mask (argmax of the per-object opacity, background where the
accumulated opacity is small).

    python examples/render_scene.py --synthetic /tmp/multi --img_wh 32 24 --steps 300
    python examples/render_scene.py --synthetic /tmp/multi --steps 300 --render_wh 160 120 --out ckpts/scene_demo
    python examples/render_scene.py --synthetic /tmp/multi --steps 300 --occupancy      # skip the empty space inside every object's box

    python examples/render_scene.py --synthetic /tmp/multi --steps 300 --background     # ... in front of a vanilla NeRF as the backdrop

--occupancy renders the same three images with one occupancy grid per distinct (instance, articulation) and prints,
per object, the share of its fine samples that reached the network and the PSNR of its pixels against the exact frame.
--background trains a small ``LitNeRF`` on the synthetic single scene for --background-steps steps and renders the
three instances in front of it (``scene.SceneBackground``), with or without --occupancy; the mask's last colour is the backdrop.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from examples.run_autodecoder import collate  # noqa: E402


def rotation_z(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)


def placement(instance, articulation, turn_deg, centre, box):
    return instance, articulation, torch.cat([rotation_z(turn_deg), torch.tensor(centre, dtype=torch.float32)[:, None]], 1), box


def train_backdrop(args, dev):
    """A small vanilla LitNeRF trained on the synthetic single scene -> scene.SceneBackground over that scene's near / far"""
    from aon_amd import scene
    from aon_amd.datasets.sapien import SapienDataset, write_synthetic_scene
    from aon_amd.models.vanilla_nerf.model import LitNeRF

    root = write_synthetic_scene(os.path.join(args.synthetic or args.out, "backdrop"), n_train=8, n_val=1, img_wh=tuple(args.img_wh))
    train = SapienDataset(root, "train", tuple(args.img_wh), white_back=True, device=dev)
    lit = LitNeRF({"chunk": 65536, "img_wh": tuple(args.img_wh), "run_max_steps": args.background_steps}, near=train.near, far=train.far,
                  white_bkgd=True).to(dev)
    opt = lit.configure_optimizers()
    gen = torch.Generator(device=dev).manual_seed(0)
    step = 0
    while step < args.background_steps:
        for batch in train.train_batches(2048, generator=gen):
            lit.fit_step({k: v.unsqueeze(0) for k, v in batch.items()}, step, opt)
            step += 1
            if step >= args.background_steps:
                break
    lit.finish_fit()
    return scene.SceneBackground(lit.model.eval(), float(train.near), float(train.far))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root_dir", default=None)
    ap.add_argument("--synthetic", default=None, help="write a small synthetic multi-instance tree here and train on it")
    ap.add_argument("--img_wh", type=int, nargs=2, default=(32, 24), help="training resolution")
    ap.add_argument("--render_wh", type=int, nargs=2, default=(96, 72), help="resolution of the scene frame")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--out", default="ckpts/scene_demo")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--occupancy", action="store_true", help="render through per-object occupancy grids and compare with the exact frame")
    ap.add_argument("--occ_resolution", type=int, default=64, help="cells per axis of the grids (over [-1, 1]^3, which encloses the boxes)")
    ap.add_argument("--background", action="store_true", help="render the instances in front of a vanilla NeRF trained on the synthetic single scene")
    ap.add_argument("--background-steps", type=int, default=300, help="training steps of the backdrop's LitNeRF")
    args = ap.parse_args()
    import random as _random
    _random.seed(args.seed); np.random.seed(args.seed); torch.manual_seed(args.seed)

    from PIL import Image

    import aon_amd.synthetic as syn
    from aon_amd import ops
    from aon_amd.datasets.sapien_multi import SapienDatasetMulti, write_synthetic_multi_scene
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    if args.synthetic:
        args.root_dir = write_synthetic_multi_scene(args.synthetic, n_instances=2, n_degrees=3, n_views=60, img_wh=tuple(args.img_wh))
    assert args.root_dir, "--root_dir or --synthetic"
    dev = torch.device("cuda:0")
    train = SapienDatasetMulti(args.root_dir, "train", img_wh=tuple(args.img_wh), white_back=True, device=dev)
    lit = LitNeRF_AutoDecoder({"chunk": 65536, "img_wh": tuple(args.img_wh), "run_max_steps": args.steps, "N_max_objs": len(train.ids),
                               "N_obj_code_length": 128}).to(dev)
    lit.setup(train)
    opt = lit.configure_optimizers()
    for step in range(args.steps):
        lit.fit_step(collate(train[step], dev), step, opt)
    lit.finish_fit()

    background = None
    if args.background:
        background = train_backdrop(args, dev)

    # three instances in one frame: 0 and 1 stand close enough for their boxes to overlap, the third stands apart
    placements = [placement(0, 0, 0.0, (-0.45, -0.3, 0.0), 1.6),
                  placement(1 % len(train.ids), 8, 40.0, (0.45, 0.35, 0.1), 1.6),
                  placement(0, 16, -70.0, (-0.2, 1.9, -0.2), 1.6)]
    Wr, Hr = args.render_wh
    ro, vd = ops.raygen(syn.look_at_pose(5.0, 35.0, 30.0), Hr, Wr, syn.focal_from_fovy(Hr, 40.0), device=dev)
    batch = {"rays_o": ro, "rays_d": vd, "viewdirs": vd}
    occ_rep = None
    if args.occupancy:
        exact = lit.render_scene(batch, placements, background=background)
        out = lit.render_scene(batch, placements, occupancy=dict(bounds=(-1.0, 1.0), resolution=args.occ_resolution), background=background)
        S_fine = lit.model.num_coarse_samples + lit.model.num_fine_samples + 1
        pairs = ops.scene_pairs(ro, vd, vd, [(p[2], p[3]) for p in placements])
        owner = exact["obj_acc"][:, :3].argmax(1)
        occ_rep = []
        for k, (count, run) in enumerate(zip(pairs.counts, out["occupied"].tolist())):
            mine = (owner == k) & (exact["acc"] > 0.5)
            mse = float(((out["rgb"][mine] - exact["rgb"][mine]) ** 2).mean()) if bool(mine.any()) else 0.0
            occ_rep.append({"object": k, "fine_samples_run": int(run), "fine_samples": count * S_fine,
                            "share_run": round(run / max(count * S_fine, 1), 4), "psnr_to_exact_db": round(-10 * np.log10(max(mse, 1e-12)), 2)})
            print(f"object {k}: {occ_rep[-1]['share_run']:.1%} of its fine samples reached the network, PSNR to the exact frame {occ_rep[-1]['psnr_to_exact_db']:.1f} dB")
    else:
        out = lit.render_scene(batch, placements, background=background)
    rgb, acc, depth, obj_acc = (out[k].cpu() for k in ("rgb", "acc", "depth", "obj_acc"))
    seen = acc > 0.5
    mask = torch.where(seen, obj_acc.argmax(1) + 1, torch.zeros_like(acc, dtype=torch.int64))     # 0 = background, k + 1 = placement k
    os.makedirs(args.out, exist_ok=True)
    Image.fromarray((rgb.clamp(0, 1).reshape(Hr, Wr, 3).numpy() * 255).astype(np.uint8), "RGB").save(os.path.join(args.out, "scene_rgb.png"))
    d = depth / acc.clamp(min=1e-6)
    d = torch.where(seen, (d - d[seen].min()) / (d[seen].max() - d[seen].min()).clamp(min=1e-6), torch.ones_like(d)) if seen.any() else torch.ones_like(d)
    Image.fromarray((d.reshape(Hr, Wr).numpy() * 255).astype(np.uint8), "L").save(os.path.join(args.out, "scene_depth.png"))
    palette = np.array([[255, 255, 255], [230, 60, 60], [60, 160, 230], [70, 190, 90], [150, 150, 150]], np.uint8)   # (the last: the backdrop)
    Image.fromarray(palette[mask.reshape(Hr, Wr).numpy()], "RGB").save(os.path.join(args.out, "scene_mask.png"))
    rep = {"trained_steps": args.steps, "frame": [Wr, Hr], "pixels_per_object": [int((mask == k + 1).sum()) for k in range(3)],
           "background_pixels": int((mask == 0).sum()), "files": [os.path.join(args.out, f) for f in ("scene_rgb.png", "scene_depth.png", "scene_mask.png")]}
    if background is not None:
        rep["backdrop_pixels"] = int((mask == 4).sum())
        rep["backdrop_steps"] = args.background_steps
    if occ_rep is not None:
        rep["occupancy"] = occ_rep
    print(json.dumps(rep))
    return rep


if __name__ == "__main__":
    main()
