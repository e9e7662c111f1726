"""Step time of the ray-gradient step on a frozen vanilla network beside the full training step of the same build:
NeRF.forward + loss + backward with the rays as leaves and the network frozen (autograd.RenderVanillaInputs) against the same forward with
the parameters trainable (autograd.RenderVanilla), alternating runs, HIP events around each run, then one run of each with the library's
per-kernel-class timers (aon_profile_class).  In the frozen step the weight-gradient class holds the two ray-gradient launches.

    python tools/vanilla_pose_bench.py --rays 4096 --steps 10 --runs 4 --out profiles/vanilla_pose_bench.json
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12    # bytes / s, MI355X
VALU_PEAK = 78.6e12  # fp32 flop / s, MI355X, one fused multiply-add per lane and clock (no packed fp32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed run")
    ap.add_argument("--runs", type=int, default=4, help="timed runs per mode (alternating)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import aon_amd.synthetic as syn
    from aon_amd import ops
    from aon_amd.models.vanilla_nerf import helper
    from aon_amd.models.vanilla_nerf.model import NeRF

    dev = torch.device("cuda:0")
    model = NeRF().to(dev)
    model.load_state_dict(syn.make_nerf_state_dict(seed=0, density_scale=30.0))
    H, W = 480, 640
    ro, vd = ops.raygen(syn.look_at_pose(), H, W, syn.focal_from_fovy(H), device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    idx = torch.randint(0, H * W, (args.rays,), device=dev, generator=g)
    o, d = ro[idx].contiguous(), vd[idx].contiguous()
    target = torch.rand(args.rays, 3, device=dev, generator=g)
    t_rand = torch.rand(args.rays, model.num_coarse_samples + 1, device=dev, generator=g)
    u = torch.rand(args.rays, model.num_fine_samples, device=dev, generator=g)

    def run(frozen, steps):
        model.requires_grad_(not frozen)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            lo, ld = (o.clone().requires_grad_(True), d.clone().requires_grad_(True)) if frozen else (o, d)
            out = model({"rays_o": lo, "rays_d": ld, "viewdirs": ld}, True, True, 2.0, 6.0, t_rand=t_rand, u=u)
            loss, _ = helper.train_loss(out, target)
            loss.backward()
            model.zero_grad(set_to_none=True)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / steps, loss.detach()

    for frozen in (False, True):
        run(frozen, args.warmup)
    times = {True: [], False: []}
    last = {}
    for _ in range(args.runs):
        for frozen in (False, True):
            ms, loss = run(frozen, args.steps)
            times[frozen].append(ms)
            last[frozen] = loss
    classes = {}
    for frozen in (False, True):
        ops.profile_begin()
        run(frozen, args.steps)
        ops.profile_end()
        classes[frozen] = {k: round(v[0] / args.steps, 4) for k, v in ops.profile_classes().items() if v[1]}
    model.requires_grad_(True)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    S = (model.num_coarse_samples + 1, model.num_coarse_samples + 1 + model.num_fine_samples)
    samples = sum(args.rays * s for s in S)
    macs = samples * (63 * 512 + 27 * 128)                       # the sample kernel's multiply-adds
    plane_bytes = samples * (256 + 256 + 128) * 4                # dZ0, dZ5, dZ_v0
    rec_bytes = samples * 128 * 2                                # records written, then read by the reduce kernel
    rg_ms = next((v for k, v in classes[True].items() if "wgrad" in k.lower()), None)
    out = {"rays_per_step": args.rays, "steps_per_run": args.steps, "runs": args.runs,
           "ms_per_step_full": [round(x, 3) for x in times[False]], "ms_per_step_ray_grads": [round(x, 3) for x in times[True]],
           "median_ms_full": round(med[False], 3), "median_ms_ray_grads": round(med[True], 3), "loss_bit_equal": bool(torch.equal(last[True], last[False])),
           "classes_ms_per_step_full": classes[False], "classes_ms_per_step_ray_grads": classes[True],
           "ray_grad_launches_ms": rg_ms, "sample_kernel_macs": macs, "sample_kernel_plane_bytes": plane_bytes, "record_bytes": rec_bytes,
           "ray_grad_fraction_of_valu_peak": None if not rg_ms else round(2 * macs / (rg_ms * 1e-3) / VALU_PEAK, 4),
           "ray_grad_fraction_of_hbm_peak": None if not rg_ms else round((plane_bytes + rec_bytes) / (rg_ms * 1e-3) / HBM_PEAK, 4),
           "scratch_GB_full": round(ops.lib.aon_train_scratch_bytes_ex(args.rays, 0, 2, None) / 2 ** 30, 3),
           "scratch_GB_ray_grads": round(ops.lib.aon_train_scratch_bytes_inputs_vanilla(args.rays, 2, None) / 2 ** 30, 3)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
