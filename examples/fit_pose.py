"""Camera pose of an observed view, refined on the FROZEN network: train ``LitNeRF_AutoDecoder`` briefly on the
synthetic scene, take a view between two training views (the observation is the trained model's own render from that pose: the example
shows the optimiser, not the scene generator), perturb its pose by a small rotation and translation and recover it with ``fit_pose``
(gradients of rays_o / rays_d / viewdirs through the HIP backward, one 6-vector stepped by aon_adam_step).  Prints the rotation and
translation error before and after.

    python examples/fit_pose.py --synthetic /tmp/scene_art --img_wh 32 24 --steps 300 --fit-steps 150
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from examples.run_autodecoder import collate  # noqa: E402


def pose_errors(p, q):
    """(rotation angle in degrees, translation distance) between two (3, 4) poses."""
    R = p[:3, :3].double().cpu() @ q[:3, :3].double().cpu().T
    return math.degrees(math.acos(max(-1.0, min(1.0, (R.trace().item() - 1.0) / 2.0)))), (p[:3, 3].double().cpu() - q[:3, 3].double().cpu()).norm().item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root_dir", default=None)
    ap.add_argument("--synthetic", default=None, help="write a small synthetic multi-instance tree here and train on it")
    ap.add_argument("--img_wh", type=int, nargs=2, default=(32, 24))
    ap.add_argument("--steps", type=int, default=300, help="training steps of the whole model before the fit")
    ap.add_argument("--fit-steps", type=int, default=150)
    ap.add_argument("--lr", type=float, default=3e-3)
    ap.add_argument("--state", type=int, nargs=2, default=(0, 1), metavar=("INSTANCE", "ARTICULATION"))
    ap.add_argument("--rotation-deg", type=float, default=2.0)
    ap.add_argument("--translation", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import random as _random
    _random.seed(args.seed); np.random.seed(args.seed); torch.manual_seed(args.seed)

    import aon_amd.synthetic as syn
    from aon_amd import ops
    from aon_amd.datasets.sapien_multi import SapienDatasetMulti, write_synthetic_multi_scene
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    n_views = 60
    if args.synthetic:
        args.root_dir = write_synthetic_multi_scene(args.synthetic, n_instances=2, n_degrees=3, n_views=n_views, img_wh=tuple(args.img_wh))
    assert args.root_dir, "--root_dir or --synthetic"
    dev = torch.device("cuda:0")
    train = SapienDatasetMulti(args.root_dir, "train", img_wh=tuple(args.img_wh), white_back=True, device=dev)
    lit = LitNeRF_AutoDecoder({"chunk": 65536, "img_wh": tuple(args.img_wh), "run_max_steps": args.steps, "N_max_objs": len(train.ids),
                               "N_obj_code_length": 128}).to(dev)
    lit.setup(train)
    opt = lit.configure_optimizers()
    for step in range(args.steps):      # 1. train briefly
        lit.fit_step(collate(train[step], dev), step, opt)
    lit.finish_fit()
    lit.randomized = False              # the fit samples deterministically
    print(json.dumps({"trained_steps": args.steps, "train_psnr_fine": lit.logged["train/psnr1"][-1]}), flush=True)

    # 2. a view half-way between two training views of the synthetic scene (look-at poses on the radius-4 sphere), seen by the trained model
    w, h = args.img_wh
    true = syn.look_at_pose(4.0, 360.0 * 7.5 / n_views + 3.0 * args.state[0], 30.0)
    dirs = ops.ray_directions(h, w, syn.focal_from_fovy(h), device=dev).reshape(-1, 3)
    codes = lit._initial_latents(tuple(args.state), dev)
    with torch.no_grad():
        o, d = ops.rays_from_pose(dirs, true.to(dev))
        target = lit.model({"rays_o": o.contiguous(), "rays_d": d, "viewdirs": d}, False, lit.white_bkgd, lit.near, lit.far, codes)[-1][0].clone()
    # 3. perturb the pose: a rotation about a fixed axis and a translation along another
    axis = torch.tensor([0.6, -0.64, 0.48], dtype=torch.float64)
    shift = torch.tensor([0.6, -0.48, 0.64], dtype=torch.float64)
    corr = torch.cat([math.radians(args.rotation_deg) * axis / axis.norm(), args.translation * shift / shift.norm()])
    start = ops.apply_pose_correction(true.double(), corr).float()
    # 4. recover it
    poses, _, losses = lit.fit_pose([{"directions": dirs, "target": target}], args.fit_steps, lr=args.lr, codes=codes, poses=[start], seed=args.seed)
    e0, e1 = pose_errors(start, true), pose_errors(poses[0], true)
    losses = losses.tolist()
    out = {"state": tuple(args.state), "fit_steps": args.fit_steps, "loss_first": losses[0], "loss_last": losses[-1],
           "rotation_error_deg": {"before": e0[0], "after": e1[0]}, "translation_error": {"before": e0[1], "after": e1[1]}}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
