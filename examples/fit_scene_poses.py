"""Recover where several objects ARE from ONE observed frame: train ``LitNeRF_AutoDecoder`` briefly on the synthetic
multi-instance set of examples/run_autodecoder.py, render three placements as in examples/render_scene.py, perturb their three poses by a
small rotation and translation, fit them back on the frozen network with ``fit_scene_poses`` -- the codes are known, gradients reach the
poses -- and print every object's rotation and translation error before and after.

    python examples/fit_scene_poses.py --synthetic /tmp/multi --img_wh 32 24 --steps 300
    python examples/fit_scene_poses.py --synthetic /tmp/multi --steps 300 --fit_steps 300 --render_wh 48 36
    python examples/fit_scene_poses.py --synthetic /tmp/multi --steps 300 --background  # ... in front of a vanilla NeRF as the frozen backdrop
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from examples.render_scene import placement, train_backdrop  # noqa: E402
from examples.run_autodecoder import collate  # noqa: E402


def pose_errors(p, q):
    """(rotation angle in degrees, translation distance) between two (3, 4) poses"""
    p, q = p.detach().cpu().double(), q.detach().cpu().double()
    c = torch.clamp((torch.trace(p[:, :3] @ q[:, :3].T) - 1.0) / 2.0, -1.0, 1.0)
    return float(torch.rad2deg(torch.acos(c))), float((p[:, 3] - q[:, 3]).norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root_dir", default=None)
    ap.add_argument("--synthetic", default=None, help="write a small synthetic multi-instance tree here and train on it")
    ap.add_argument("--img_wh", type=int, nargs=2, default=(32, 24), help="training resolution")
    ap.add_argument("--render_wh", type=int, nargs=2, default=(32, 24), help="resolution of the observed frame (one chunk: its planes live until the backward)")
    ap.add_argument("--steps", type=int, default=300, help="training steps")
    ap.add_argument("--fit_steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--degrees", type=float, default=2.0, help="rotation of the perturbation")
    ap.add_argument("--shift", type=float, default=0.05, help="translation of the perturbation")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--background", action="store_true", help="the observed frame shows the objects in front of a vanilla NeRF trained on the synthetic "
                    "single scene, and the fit renders them in front of that frozen backdrop (DESIGN.md section 4.22)")
    ap.add_argument("--background-steps", type=int, default=300, help="training steps of the backdrop's LitNeRF")
    ap.add_argument("--out", default="fit_scene_out", help="where the backdrop's synthetic scene is written without --synthetic")
    args = ap.parse_args()
    import random as _random
    _random.seed(args.seed); np.random.seed(args.seed); torch.manual_seed(args.seed)

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

    layout = [placement(0, 0, 0.0, (-0.45, -0.3, 0.0), 1.6), placement(1 % len(train.ids), 8, 40.0, (0.45, 0.35, 0.1), 1.6),
              placement(0, 16, -70.0, (-0.2, 1.9, -0.2), 1.6)]
    Wr, Hr = args.render_wh
    ro, vd = ops.raygen(syn.look_at_pose(5.0, 35.0, 30.0), Hr, Wr, syn.focal_from_fovy(Hr, 40.0), device=dev)
    batch = {"rays_o": ro, "rays_d": vd, "viewdirs": vd}
    background = train_backdrop(args, dev) if args.background else None
    batch["target"] = lit.render_scene(batch, layout, background=background)["rgb"].clone()
    gen = torch.Generator().manual_seed(args.seed + 1)
    start = []
    for iid, art, pose, box in layout:
        axis, move = torch.randn(3, generator=gen, dtype=torch.float64), torch.randn(3, generator=gen, dtype=torch.float64)
        corr = torch.cat([axis / axis.norm() * np.deg2rad(args.degrees), move / move.norm() * args.shift])
        start.append((iid, art, ops.apply_pose_correction(torch.as_tensor(pose, dtype=torch.float64), corr).float(), box))
    poses, _, losses = lit.fit_scene_poses([batch], start, args.fit_steps, args.lr, background=background)
    before = [pose_errors(s[2], torch.as_tensor(t[2])) for s, t in zip(start, layout)]
    after = [pose_errors(p, torch.as_tensor(t[2])) for p, t in zip(poses, layout)]
    for j, (b, a) in enumerate(zip(before, after)):
        print(f"object {j}: rotation error {b[0]:.3f} -> {a[0]:.3f} degrees, translation error {b[1]:.4f} -> {a[1]:.4f}")
    rep = {"trained_steps": args.steps, "fit_steps": args.fit_steps, "frame": [Wr, Hr], "loss_first": float(losses[0]), "loss_last": float(losses[-1]),
           "pose_error_before": [[round(x, 4) for x in b] for b in before], "pose_error_after": [[round(x, 4) for x in a] for a in after]}
    if background is not None:
        rep["backdrop_steps"] = args.background_steps
    print(json.dumps(rep))
    return rep


if __name__ == "__main__":
    main()
