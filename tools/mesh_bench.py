"""Time mesh extraction on seeded networks at 128^3, 256^3 and 512^3 and print one JSON line per measurement:

  * grid evaluation, vanilla and articulated (ops.density_grid: one fused launch), with the achieved fraction of the fp32 matrix peak on the
    executed FLOPs (2 x MACs of the chunks the kernel runs: 491,776 per point vanilla, 541,696 articulated);
  * the per-point route a user had before: ops.pos_enc + ops.mlp_fwd_enc (vanilla) / ops.art_mlp_fwd_pos (articulated) in chunks of
    2^20 points -- the whole network including the view branch;
  * marching cubes on the vanilla grid (ops.marching_cubes: count + emit, three launches each), with its bytes moved per second against
    the HBM peak (grid read twice, workspace written and read, vertices and faces written);
  * the whole extract_mesh (grid + marching cubes, no colour).

Times are device-event times per call (median of --reps after a warm-up); for the kernels alone run the script under
`rocprofv3 --kernel-trace --stats -- python tools/mesh_bench.py` and read density_grid_kernel / art_density_grid_kernel / mc_*_kernel.

    python tools/mesh_bench.py [--res 128 256 512] [--reps 3] [--route-max 512]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import aon_amd.synthetic as syn  # noqa: E402
from aon_amd import ops  # noqa: E402
from aon_amd.mesh import extract_mesh  # noqa: E402

PEAK_FP32_MATRIX = 157.3e12   # MI355X, FLOP/s
PEAK_HBM = 8.0e12             # B/s
MACS_VANILLA = 60 * 32 * 256 + 256                                  # trunk chunks 0..59 + density head
MACS_ART = 12 * 32 * 128 + 60 * 32 * 256 + 3 * 128 + 128 * 3 + 256   # + deformation MLP (VALU layers included)
BOUNDS = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / 1e3)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--route-max", type=int, default=512, help="largest resolution at which the per-point route is timed")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench needs a GPU")
    dev = torch.device("cuda:0")
    from aon_amd.models.code_library import CodeLibraryArticulated
    from aon_amd.models.vanilla_nerf.model import NeRF
    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art
    import types

    nerf = NeRF().to(dev)
    nerf.load_state_dict(syn.make_nerf_state_dict(seed=0, density_scale=30.0))
    art = NeRF_AE_Art().to(dev)
    art.load_state_dict(syn.make_art_state_dict(seed=0, density_scale=30.0))
    lib = CodeLibraryArticulated(types.SimpleNamespace(N_max_objs=2, N_obj_code_length=128)).to(dev)
    lib.load_state_dict(syn.make_code_library_state(seed=0, n_max_objs=2))
    with torch.no_grad():
        lat = lib({"instance_id": torch.tensor([0], device=dev), "articulation_id": torch.tensor([2], device=dev)}, is_test=True)
    pv = nerf.fine_mlp.packed()
    pa, sa = art.fine_mlp.packed(), art.fine_mlp.prepared(lat)

    for N in args.res:
        P = N ** 3
        dims = (N, N, N)
        t = timed(lambda: ops.density_grid(pv, dims, *BOUNDS, ops.ACT_VANILLA), args.reps)
        print(json.dumps({"what": "grid_vanilla", "res": N, "s": t, "fp32_matrix_fraction": 2 * MACS_VANILLA * P / t / PEAK_FP32_MATRIX}), flush=True)
        t = timed(lambda: ops.density_grid(pa, dims, *BOUNDS, ops.ACT_ARTICULATED, small=sa), args.reps)
        print(json.dumps({"what": "grid_articulated", "res": N, "s": t, "fp32_matrix_fraction": 2 * MACS_ART * P / t / PEAK_FP32_MATRIX}), flush=True)
        grid = ops.density_grid(pv, dims, *BOUNDS, ops.ACT_VANILLA)
        level = float(torch.quantile(grid.reshape(-1)[:: max(1, P // 1_000_000)], 0.8).item())
        verts, faces = ops.marching_cubes(grid, level, *BOUNDS)
        t = timed(lambda: ops.marching_cubes(grid, level, *BOUNDS), args.reps)
        moved = 2 * (4 * P + 4 * P + 4 * P) + 12 * (verts.shape[0] + faces.shape[0])   # two passes: grid + flags/offsets each, then the outputs
        print(json.dumps({"what": "marching_cubes", "res": N, "s": t, "V": verts.shape[0], "F": faces.shape[0], "level": level,
                          "GB_per_s": moved / t / 1e9, "hbm_fraction": moved / t / PEAK_HBM}), flush=True)
        t = timed(lambda: extract_mesh(nerf, BOUNDS, N, threshold=level), args.reps)
        print(json.dumps({"what": "extract_mesh_vanilla", "res": N, "s": t}), flush=True)
        if N <= args.route_max:
            def route(articulated):
                chunk = 1 << 20
                out = torch.empty(P, device=dev)
                vd = torch.zeros(chunk, 3, device=dev)
                vd[:, 2] = 1
                venc = ops.pos_enc(vd, 0, 4)
                for b in range(0, P, chunk):
                    e = min(P, b + chunk)
                    pts = ops.grid_points(dims, *BOUNDS, b, e, device=dev)
                    if articulated:
                        raw = ops.art_mlp_fwd_pos(pa, sa, pts[:, None, :].contiguous(), venc[: e - b].contiguous())
                    else:
                        raw = ops.mlp_fwd_enc(pv, ops.pos_enc(pts[:, None, :].contiguous(), 0, 10), venc[: e - b].contiguous())
                    out[b:e] = raw[:, 0, 3]
                return out
            t = timed(lambda: route(False), max(1, args.reps - 2))
            print(json.dumps({"what": "per_point_route_vanilla", "res": N, "s": t}), flush=True)
            t = timed(lambda: route(True), max(1, args.reps - 2))
            print(json.dumps({"what": "per_point_route_articulated", "res": N, "s": t}), flush=True)


if __name__ == "__main__":
    main()
