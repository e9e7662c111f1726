"""Early ray termination on the occupancy renders on a 640x480 frame, one JSON line per field:

  * frame time (median of --reps, device-synchronised wall time) of the exact render, the grid-only render (render_fwd_occ) and grid + stop
    (render_fwd_stop at --eps) for every round size of --rounds, whole-frame calls and calls of --chunk rays (the eval harness's chunk);
  * coarse / fine samples run through the MLP, the share of rays that stop, PSNR of each frame to the exact one;
  * round overhead: grid + stop on an EMPTY grid (every round marked, scanned, emitted and -- no ray ever stops -- its depth taken, no MLP
    work) minus its profiled sampling and compositing launches, per round and as a share of the dense frame.

Fields: the synthetic weights made sparse by synthetic.sparsify_nerf_ ("sparse", density scale 30, the field of section 4.9), the same with
the density scale --opaque-scale ("opaque": surfaces a ray cannot see through), and the synthetic scene trained by
examples/run_single_scene.py for --steps steps ("trained"; --no-trained skips it).  For the kernels alone run it under
`rocprofv3 --kernel-trace --stats -- python tools/early_stop_bench.py` and read occ_mark_kernel<1> / occ_scan_kernel<1> /
occ_emit_kernel<1> / occ_depth_kernel and the mlp_fwd_kernel instances.

    python tools/early_stop_bench.py [--reps 5] [--eps 1e-3] [--rounds 16 32 48 64] [--chunk 3840] [--steps 300] [--no-trained]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import aon_amd.synthetic as syn  # noqa: E402
from aon_amd import ops  # noqa: E402
from aon_amd.occupancy import build_occupancy  # noqa: E402
from occupancy_bench import H, W, NEAR, FAR, frame_time, profiled  # noqa: E402


def sparse_nerf(dev, density_scale):
    from aon_amd.models.vanilla_nerf.model import NeRF

    model = NeRF().to(dev)
    model.load_state_dict(syn.make_nerf_state_dict(seed=0, density_scale=density_scale))
    return syn.sparsify_nerf_(model, 0.8, 4.0)


def chunked(call, n, chunk):
    """`call(b, e)` over ray ranges of `chunk` rays -> the fine rgb of the frame, summed occupied counts, the fine stop column (or None)"""
    rgb, occ, stop = [], torch.zeros(2, dtype=torch.int64), []
    for b in range(0, n, chunk):
        out = call(b, min(n, b + chunk))
        rgb.append(out[0][1][0])
        if len(out) > 1:
            occ += out[1].cpu()
        if len(out) > 2:
            stop.append(out[2][:, 1])
    return torch.cat(rgb), [int(x) for x in occ.tolist()], torch.cat(stop) if stop else None


def psnr(a, b):
    mse = torch.mean((a - b) ** 2).item()
    return float("inf") if mse == 0 else round(-10 * math.log10(mse), 2)


def bench(name, model, bound, args, dev):
    ro, vd = ops.raygen(syn.look_at_pose(), H, W, syn.focal_from_fovy(H), device=dev)
    pc, pf = model.coarse_mlp.packed(), model.fine_mlp.packed()
    grid = build_occupancy(model, (-bound, bound))
    empty = ops.occupancy_grid(torch.zeros(5, 5, 5, device=dev), -bound, bound, 0.01, 0)
    n = ro.shape[0]
    samples = [n * 65, n * 193]
    rec = {"field": name, "frame": f"{W}x{H}", "eps": args.eps, "occupied_cells": round(grid.occupied_fraction(), 4), "samples": samples}
    with torch.no_grad():
        for label, chunk in (("frame", n), (f"chunk{args.chunk}", args.chunk)):
            exact = lambda b, e: (ops.render_fwd(pc, pf, ro[b:e], vd[b:e], vd[b:e], NEAR, FAR, True),)  # noqa: E731
            accel = lambda b, e: ops.render_fwd_occ(pc, pf, ro[b:e], vd[b:e], vd[b:e], NEAR, FAR, True, grid)  # noqa: E731
            ref_rgb, _, _ = chunked(exact, n, chunk)
            g_rgb, g_occ, _ = chunked(accel, n, chunk)
            r = {"ms_exact": round(frame_time(lambda: chunked(exact, n, chunk), args.reps) * 1e3, 3),
                 "ms_grid": round(frame_time(lambda: chunked(accel, n, chunk), args.reps) * 1e3, 3),
                 "grid_ran": g_occ, "grid_psnr": psnr(g_rgb, ref_rgb), "stop": {}}
            for R in args.rounds:
                both = lambda b, e: ops.render_fwd_stop(pc, pf, ro[b:e], vd[b:e], vd[b:e], NEAR, FAR, True, grid, args.eps, R)  # noqa: E731
                s_rgb, s_occ, s_stop = chunked(both, n, chunk)
                r["stop"][str(R)] = {"ms": round(frame_time(lambda: chunked(both, n, chunk), args.reps) * 1e3, 3), "ran": s_occ,
                                     "rays_stopped": round(float((s_stop < 193).float().mean()), 4), "psnr": psnr(s_rgb, ref_rgb)}
            rec[label] = r
        # round overhead on the whole frame: an empty grid lists nothing and stops nobody, so every round's mark / scan / emit / depth runs
        for R in args.rounds:
            blank = lambda: ops.render_fwd_stop(pc, pf, ro, vd, vd, NEAR, FAR, True, empty, args.eps, R)  # noqa: E731
            t_blank = frame_time(blank, args.reps)
            p = profiled(blank)
            staged = sum(p[k][0] for k in ("sample_t", "composite", "composite_pdf", "mlp_fwd"))
            rounds = -(-65 // R) + -(-193 // R)
            over = t_blank * 1e3 - staged
            rec.setdefault("round_overhead", {})[str(R)] = {"rounds": rounds, "ms": round(over, 3), "ms_per_round": round(over / rounds, 4),
                                                            "share_of_dense_frame": round(over / rec["frame"]["ms_exact"], 4)}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--rounds", type=int, nargs="+", default=[16, 32, 48, 64])
    ap.add_argument("--chunk", type=int, default=3840)
    ap.add_argument("--opaque-scale", type=float, default=300.0)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--no-trained", action="store_true")
    ap.add_argument("--exp_dir", default="ckpts/occupancy_bench")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    bench("sparse", sparse_nerf(dev, 30.0), 4.0, args, dev)
    bench("opaque", sparse_nerf(dev, args.opaque_scale), 4.0, args, dev)
    if not args.no_trained:
        from render_occupancy import train_or_load

        lit, _ = train_or_load(steps=args.steps, exp_dir=args.exp_dir)
        bench("trained", lit.model, 1.5, args, dev)


if __name__ == "__main__":
    main()
