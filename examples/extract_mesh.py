"""Mesh extraction from a trained model: density grid on the GPU (one fused HIP launch), GPU marching cubes, binary PLY output.

    python examples/extract_mesh.py --synthetic /tmp/scene --steps 300 --resolution 128                  # train a small vanilla scene first
    python examples/extract_mesh.py --synthetic /tmp/scene_art --steps 60 --resolution 128 --articulated # one PLY per articulation state
    python examples/extract_mesh.py --ckpt ckpts/demo/last.ckpt --resolution 256 --color                 # a checkpoint written by run_*.py

Without --ckpt the training example (run_single_scene.py, or run_autodecoder.py with --articulated) runs first in a child process and its
last.ckpt is loaded.  Writes mesh.ply (vanilla) or mesh_art_00.ply .. mesh_art_18.ply (the 19 interpolated articulation codes of the test
epoch) and mesh.json with V, F, timings and the grid's largest density to --out_dir.  The synthetic demo scenes (soft 2-D discs) hold
little geometry after a few hundred steps, so the default iso levels (mesh.DEFAULT_THRESHOLD_*) may find no surface there: the example then
says so, and --threshold below the printed density_max gives a mesh."""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", default=None, help="checkpoint of run_single_scene.py / run_autodecoder.py (else train one first)")
    ap.add_argument("--synthetic", default=None, help="scene directory for the training run (see the training examples)")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--articulated", action="store_true")
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--bounds", type=float, nargs=2, default=(-1.2, 1.2), help="the cube [lo, hi]^3 to mesh")
    ap.add_argument("--threshold", type=float, default=None, help="iso level (default: mesh.DEFAULT_THRESHOLD_*)")
    ap.add_argument("--instance", type=int, default=0)
    ap.add_argument("--color", action="store_true", help="per-vertex colour from the network")
    ap.add_argument("--out_dir", default="ckpts/mesh")
    args = ap.parse_args()

    import aon_amd  # noqa: F401
    from aon_amd.mesh import extract_mesh, write_ply
    from aon_amd.utils import load_checkpoint

    os.makedirs(args.out_dir, exist_ok=True)
    t_train = 0.0
    if args.ckpt is None:
        if not args.synthetic:
            raise SystemExit("give --ckpt, or --synthetic DIR to train a small model first")
        exp = os.path.join(args.out_dir, "train")
        script = "run_autodecoder.py" if args.articulated else "run_single_scene.py"
        t0 = time.perf_counter()
        subprocess.run([sys.executable, os.path.join(ROOT, "examples", script), "--synthetic", args.synthetic, "--steps", str(args.steps),
                        "--exp_dir", exp], check=True)
        t_train = time.perf_counter() - t0
        args.ckpt = os.path.join(exp, "last.ckpt")

    dev = torch.device("cuda:0")
    state = torch.load(args.ckpt, map_location="cpu", weights_only=False)["state_dict"]
    if args.articulated:
        from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

        n_obj, code_len = state["code_library.embedding_instance_shape.weight"].shape
        lit = LitNeRF_AutoDecoder({"N_max_objs": n_obj, "N_obj_code_length": code_len})
    else:
        from aon_amd.models.vanilla_nerf.model import LitNeRF

        lit = LitNeRF({})
    load_checkpoint(args.ckpt, lit)
    lit = lit.to(dev)

    bounds = tuple(args.bounds)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if args.articulated:
        meshes = lit.extract_meshes(args.instance, args.resolution, bounds=bounds, threshold=args.threshold, color=args.color)
    else:
        meshes = [extract_mesh(lit.model, bounds, args.resolution, threshold=args.threshold, color=args.color)]
    torch.cuda.synchronize()
    t_mesh = time.perf_counter() - t0
    files = []
    for i, m in enumerate(meshes):
        name = f"mesh_art_{i:02d}.ply" if args.articulated else "mesh.ply"
        write_ply(os.path.join(args.out_dir, name), m)
        files.append({"file": name, "V": int(m.verts.shape[0]), "F": int(m.faces.shape[0])})
    if args.articulated:   # the grid of the first articulation state
        lat = lit.code_library({"instance_id": torch.tensor([args.instance], device=dev), "articulation_id": torch.tensor([0], device=dev)},
                               is_test=True)
        density_max = float(lit.model.density_grid(bounds, args.resolution, lat).max())
    else:
        density_max = float(lit.model.density_grid(bounds, args.resolution).max())
    rec = {"ckpt": args.ckpt, "resolution": args.resolution, "bounds": bounds, "articulated": args.articulated, "meshes": files,
           "extract_s": t_mesh, "train_s": t_train, "density_max": density_max}
    if all(f["F"] == 0 for f in files):
        print(f"no surface at the iso level: the grid's density peaks at {density_max:.3g}; pass a lower --threshold", file=sys.stderr)
    with open(os.path.join(args.out_dir, "mesh.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
