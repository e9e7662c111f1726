"""Benchmark of the hot path: full-frame NeRF render throughput in rays/s (65 coarse + 193 fine network
evaluations per ray), BASELINE.json's metric on its config 2 (Sapien single-scene 640x480, 1x MI355X), and the
weak-scaled multi-GPU form of it (config 3: every rank renders a 640x480 frame of ray batches, rendered pixels
are exchanged with one RCCL all-gather).

    python bench.py --gpus 1 --steps 3 --warmup 1 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One step = one pass of NeRF.forward over one synthetic 307,200-ray frame per GPU, inputs already resident in HBM.
Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the steps and prints the headline; `--full` adds
everything else: the live roofline of the timed region, clock / power samples, the informational legs (configs 1, 3, 4
and 5, non-default constructor arguments) and the CPU baseline with its PSNR check.  `--dump-outputs DIR` writes the
last timed step's outputs (both levels' rgb / acc / depth) as DIR/<name>.npy; the inputs are seeded, so two builds of
the project can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FLOP_PER_SAMPLE = 1_186_816          # reference-literal MACs x 2 of one NeRFMLP evaluation
EVALS_PER_RAY = 65 + 193
PEAK_FP32_MATRIX_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense fp32 matrix peak
PEAK_FP32_MATRIX_MEASURED_TFLOPS = 155.0   # the same guide's MEASURED ceiling of that instruction (a register-resident MFMA loop on all 256 CUs)
PEAK_HBM_TBS = 8.0                   # MI355X_MICROARCH.md: HBM3E
# articulated network: reference-literal MACs per sample, and the MACs the kernels execute once the latent
# columns are folded into per-call biases (128*(128+32) + 2*256*128 + 128*128 = 102,400 fewer)
ART_MAC_LITERAL = 794_880
ART_MAC_FWD = ART_MAC_LITERAL - 102_400
ART_MAC_BWD_CHAIN = ART_MAC_FWD - 128 * 3 - 128 * 27      # no data gradient into the raw position / the view encoding
ART_MAC_WGRAD = ART_MAC_FWD                                # latent-column weight gradients are outer products of bias gradients
VAN_MAC = 593_408
VAN_MAC_BWD_CHAIN = VAN_MAC - 2 * 256 * 63 - 128 * 27     # no data gradient into the encodings
# Round 5: bottleneck_layer (256 -> 256, no activation) folded into views_linear[0] (include/aon_hip.h, aon_set_bottleneck_fold): the
# kernels execute 65,536 fewer MACs per sample in the forward, in the backward chain and in the weight gradients alike.  `executed`
# figures below subtract them when the fold is on (default); `reference_literal` figures never do.
FOLD_MAC = 256 * 256
# ... and the first view layer's view-encoding columns (27 -> 128, a constant of the ray) enter as a per-ray bias in the whole-path FORWARD
# kernels (aon_set_view_bias): the 14 two-deep MFMA steps of that chunk -- 28 columns, one of them padding -- are no longer executed.
VIEW_BIAS_MAC = 128 * 28


def executed(mac: int, fold: bool, view_bias: bool = False) -> int:
    return mac - (FOLD_MAC if fold else 0) - (VIEW_BIAS_MAC if fold and view_bias else 0)

# algorithmic HBM bytes per ray of the per-ray kernels: compositing reads float4(rgb, sigma) + t per sample and
# the direction, writes rgb/acc/depth (+ the 65 weights at the coarse level); the inverse CDF reads t (65) and 63 weights and
# writes 193 sorted t values
BYTES_COMPOSITE_COARSE = 65 * 20 + 12 + 20 + 65 * 4
BYTES_COMPOSITE_FINE = 193 * 20 + 12 + 20
BYTES_SAMPLE_PDF = 65 * 4 + 63 * 4 + 193 * 4
BYTES_COARSE_FUSED = 65 * 20 + 12 + 20 + 193 * 4   # fused coarse level: records + t + dir in, outputs + t_fine out (weights stay in registers)


def cpu_baseline(sd, rays_cpu, budget_s=20.0):
    """The oracle (plain-PyTorch restatement of the reference path) timed on the host cores on a bounded sample:
    reference-sized chunks of 3840 rays (opt.py:103) of the same frame, one small warm-up, then chunks until
    ~budget_s seconds have been spent (at least one, at most five)."""
    from oracle import nerf_oracle as orc

    n = rays_cpu["rays_o"].shape[0]
    chunk = 3840
    ncpu = os.cpu_count() or 1
    with torch.no_grad():
        # give the CPU its best shot: torch's intra-op pool is not fastest at one thread per logical core on a
        # many-core host, so probe a few pool sizes on a small batch and keep the fastest
        warm = {k: v[n // 2: n // 2 + 512] for k, v in rays_cpu.items()}
        best, threads = None, ncpu
        for cand in sorted({c for c in (8, 16, 32, 64, 128, ncpu) if c <= ncpu}):
            torch.set_num_threads(cand)
            orc.nerf_forward(sd, {k: v[:64] for k, v in warm.items()}, False, True, 2.0, 6.0)
            t0 = time.perf_counter()
            orc.nerf_forward(sd, warm, False, True, 2.0, 6.0)
            dt = time.perf_counter() - t0
            if best is None or dt < best:
                best, threads = dt, cand
        torch.set_num_threads(threads)
        done, t0, outs, starts = 0, time.perf_counter(), [], []
        start = n // 2 - chunk  # middle of the frame: rays that actually hit the scene volume
        while done < 5:
            s = start + done * chunk
            sl = {k: v[s:s + chunk] for k, v in rays_cpu.items()}
            outs.append(orc.nerf_forward(sd, sl, False, True, 2.0, 6.0)[1][0])
            starts.append(s)
            done += 1
            if time.perf_counter() - t0 > budget_s:
                break
        dt = time.perf_counter() - t0
    phys, model_name = host_cpu()
    return {"value": done * chunk / dt, "unit": "rays/s", "cores": phys, "threads": threads, "logical_cpus": ncpu, "cpu": model_name, "kind": "port",
            "sample": f"{done} x 3840-ray chunks of the same 640x480 frame, fp32, torch {torch.__version__} CPU, {dt:.1f} s; "
                      f"torch intra-op threads = {threads} (fastest of a probe over 8..{ncpu}) on a host with {phys} physical cores",
            "form": "oracle/nerf_oracle.py: searchsorted restatement of the inverse CDF, bit-identical to and faster than helper.py:232-238's "
                    "(N,64,128) mask/max/min form -- a conservative (fast) CPU baseline"}, \
        torch.cat(outs), (starts[0], starts[0] + done * chunk)


def host_cpu():
    """(physical cores, model name) of the host, from lscpu; falls back to os.cpu_count()."""
    import subprocess

    try:
        txt = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        kv = {l.split(":", 1)[0].strip(): l.split(":", 1)[1].strip() for l in txt.splitlines() if ":" in l}
        return int(kv["Core(s) per socket"]) * int(kv["Socket(s)"]), kv.get("Model name", "?")
    except Exception:
        return os.cpu_count() or 1, "?"


class GpuStateSampler:
    """Shader clock and package power of this rank's GPU, sampled with rocm-smi about once a second WHILE a timed region runs (a host
    thread; nothing is enqueued on the GPU).  Informational: the config-5 training loop draws ~1.25 kW at 2.39 GHz, close to the board's
    limit, and boxes of the pool were seen running whole calls 12-14 % slower with no other difference (34.6 instead of 30.4 ms per step,
    round 6) -- a line that carries the clock it was measured at explains itself."""

    def __init__(self, index: int, enabled: bool = True):
        import threading

        self.index, self.samples, self._stop, self.enabled = index, [], threading.Event(), enabled     # (rank 0 only: one sampler per node)
        self._thread = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        import re
        import subprocess

        self._stop.wait(0.15)     # (the first sample a moment into the region, not at its idle edge)
        while not self._stop.is_set():
            try:
                out = subprocess.run(["rocm-smi", "-d", str(self.index), "--showclocks", "--showpower"], capture_output=True, text=True, timeout=5).stdout
                sclk = re.search(r"sclk clock level: \d+: \((\d+)Mhz\)", out)
                power = re.search(r"Power \(W\): ([0-9.]+)", out)
                if sclk:
                    self.samples.append((int(sclk.group(1)), float(power.group(1)) if power else None))
            except Exception:
                return
            self._stop.wait(0.3)

    def __enter__(self):
        if self.enabled:
            self._thread.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        if self.enabled:
            self._thread.join(timeout=6)

    def summary(self):
        if not self.samples:
            return None
        clk = sorted(c for c, _ in self.samples)
        pw = sorted(p for _, p in self.samples if p is not None)
        return {"samples": len(clk), "sclk_mhz_median": clk[len(clk) // 2], "sclk_mhz_min": clk[0], "sclk_mhz_max": clk[-1],
                "power_w_median": pw[len(pw) // 2] if pw else None, "source": "rocm-smi --showclocks --showpower, ~2 samples/s during the timed region"}


def mfma_roofline(kernel, ms, launches, samples, mac_executed, mac_literal):
    """Roofline object of an MFMA-bound kernel class from live HIP-event totals: executed and reference-literal FLOP rates."""
    if ms <= 0 or launches <= 0:
        return None
    ex = samples * mac_executed * 2 / (ms * 1e-3) / 1e12
    lit = samples * mac_literal * 2 / (ms * 1e-3) / 1e12
    return {"bound": "mfma", "kernel": kernel, "achieved": ex, "peak": PEAK_FP32_MATRIX_TFLOPS, "unit": "TFLOP/s", "frac": ex / PEAK_FP32_MATRIX_TFLOPS,
            "achieved_reference_literal": lit, "frac_reference_literal": lit / PEAK_FP32_MATRIX_TFLOPS, "traffic": None,
            "launches": launches, "avg_launch_ms": ms / launches, "samples": samples,
            "flop_per_sample_executed": 2 * mac_executed, "flop_per_sample_reference_literal": 2 * mac_literal}


def hbm_roofline(kernel, ms, launches, nbytes):
    if ms <= 0 or launches <= 0:
        return None
    tbs = nbytes / (ms * 1e-3) / 1e12
    return {"bound": "hbm", "kernel": kernel, "achieved": tbs * 1e3, "peak": PEAK_HBM_TBS * 1e3, "unit": "GB/s", "frac": tbs / PEAK_HBM_TBS,
            "traffic": None, "launches": launches, "avg_launch_us": ms / launches * 1e3, "algorithmic_bytes": nbytes,
            "algorithmic_bytes_per_launch": nbytes / launches}


def per_ray_rooflines(classes):
    """HBM rooflines of the per-ray kernels of a two-level render from the profile classes (composite launches come in
    coarse / fine pairs over the same rays)."""
    out = {}
    fused_ms, fused_launches, fused_rays = classes.get("composite_pdf", (0.0, 0, 0))
    if fused_launches:   # the coarse level is ONE kernel: compositing + inverse CDF + merge
        out["coarse_fused"] = hbm_roofline("aon::composite_kernel<true,true> (coarse compositing + inverse CDF + merge)", fused_ms, fused_launches,
                                           fused_rays * BYTES_COARSE_FUSED)
    ms, launches, rays = classes["composite"]
    if launches and fused_launches:
        out["composite"] = hbm_roofline("aon::composite_kernel<true,false> (fine level, 193 samples)", ms, launches, rays * BYTES_COMPOSITE_FINE)
    elif launches:
        out["composite"] = hbm_roofline("aon::composite_kernel (coarse + fine launches)", ms, launches, rays / 2 * (BYTES_COMPOSITE_COARSE + BYTES_COMPOSITE_FINE))
    ms, launches, rays = classes["sample_pdf"]
    if launches:
        out["sample_pdf"] = hbm_roofline("aon::sample_pdf_kernel", ms, launches, rays * BYTES_SAMPLE_PDF)
    ms, launches, rays = classes.get("sample_t", (0.0, 0, 0))
    if launches:   # deterministic stratified t: a pure write of 65 floats per ray
        out["sample_t"] = hbm_roofline("aon::sample_t4_kernel (stratified t, 65 per ray)", ms, launches, rays * 65 * 4)
    return out


def render_leg(dev, kind, H, W, steps=3):
    """Informational (never `value`): BASELINE config 1 (`kind` "config1": vanilla, coarse level only, 320x240 -- the reference's
    own CPU-runnable case) or config 4 ("art": articulated NeRF_AE_Art render, 320x240) on this rank's GPU, with the dominant
    kernel's roofline from live HIP events."""
    try:
        import types

        import aon_amd.synthetic as syn
        from aon_amd import ops
        from aon_amd.datasets.ray_utils import get_frame_rays

        ro, vd = get_frame_rays(H, W, syn.focal_from_fovy(H), syn.look_at_pose(), device=dev)
        rays = {"rays_o": ro, "rays_d": vd, "viewdirs": vd}
        if kind == "config1":
            from aon_amd.models.vanilla_nerf.model import NeRF

            model = NeRF(num_levels=1).to(dev)
            model.load_state_dict(syn.make_nerf_state_dict(seed=0, density_scale=30.0))
            call = lambda: model(rays, False, True, syn.NEAR, syn.FAR)
            evals, mac_ex, mac_lit = 65, executed(VAN_MAC, ops.bottleneck_fold(), ops.view_bias_enabled()), VAN_MAC
            name = "aon::mlp_fwd_kernel<true,false,fold> (fused encode+MLP, fp32 MFMA)"
            work = f"vanilla NeRF {W}x{H}, 65 coarse evals/ray only (num_levels=1), {H * W} rays"
        else:
            from aon_amd.models.code_library import CodeLibraryArticulated
            from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

            model = NeRF_AE_Art().to(dev)
            model.load_state_dict(syn.make_art_state_dict(seed=0, density_scale=30.0))
            lib = CodeLibraryArticulated(types.SimpleNamespace(N_max_objs=1, N_obj_code_length=128)).to(dev)
            lib.load_state_dict(syn.make_code_library_state(0, 1))
            with torch.no_grad():
                lat = lib({"instance_id": torch.tensor([0], device=dev), "articulation_id": torch.tensor([3], device=dev)})
            call = lambda: model(rays, False, True, syn.NEAR, syn.FAR, lat)
            evals, mac_ex, mac_lit = EVALS_PER_RAY, executed(ART_MAC_FWD, ops.bottleneck_fold(), ops.view_bias_enabled()), ART_MAC_LITERAL
            name = "aon::art_mlp_fwd_kernel<true,false,fold> (deformation + trunk + view branch, latents folded into biases, fp32 MFMA)"
            work = f"articulated NeRF_AE_Art {W}x{H}, 65 coarse + 193 fine evals/ray, {H * W} rays"
        with torch.no_grad():
            call()
            torch.cuda.synchronize()
            ops.profile_begin()
            t0 = time.perf_counter()
            for _ in range(steps):
                call()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / steps
            ms, launches, samples = ops.profile_end()
        res = {"workload": work, "value": H * W / dt, "unit": "rays/s", "ms_per_frame": dt * 1e3, "steps": steps, "evals_per_ray": evals,
               "bottleneck_fold": bool(ops.bottleneck_fold()), "roofline": mfma_roofline(name, ms, launches, samples, mac_ex, mac_lit)}
        if kind != "config1":
            res["hbm_kernels"] = pmc_traffic_ray_kernels(per_ray_rooflines(ops.profile_classes()), rays_per_launch=H * W)
        return res
    except Exception as e:  # informational leg: never take the headline down with it
        return {"error": f"{type(e).__name__}: {e}"}


def other_constructor_leg(dev, H=240, W=320, steps=3):
    """Informational (never `value`): the drop-in classes built with NON-default constructor arguments on a 320x240
    frame -- NeRF(max_deg_point=6, deg_view=2) on the fused kernels (zero-weight slots) and on the layer-wise GEMM engine, and a
    default network with 32 + 64 samples and lindisp (runtime sampler options on the fused kernels)."""
    try:
        import aon_amd.synthetic as syn
        from aon_amd.datasets.ray_utils import get_frame_rays
        from aon_amd.models.vanilla_nerf.model import NeRF

        ro, vd = get_frame_rays(H, W, syn.focal_from_fovy(H), syn.look_at_pose(), device=dev)
        rays = {"rays_o": ro, "rays_d": vd, "viewdirs": vd}

        def timed(model):
            with torch.no_grad():
                model(rays, False, True, syn.NEAR, syn.FAR)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    model(rays, False, True, syn.NEAR, syn.FAR)
                torch.cuda.synchronize()
            return H * W / ((time.perf_counter() - t0) / steps)

        gk = dict(min_deg_point=0, max_deg_point=6, deg_view=2)
        m = NeRF(**gk).to(dev)
        m.load_state_dict(syn.make_general_nerf_state_dict(7, **gk))
        out = {"workload": f"vanilla NeRF {W}x{H}, {H * W} rays, non-default constructor arguments", "unit": "rays/s",
               "degrees_0_6_2_fused_padded_slots": timed(m)}
        m._fused_inference = False
        out["degrees_0_6_2_layerwise_engine"] = timed(m)
        m2 = NeRF(num_coarse_samples=32, num_fine_samples=64, lindisp=True).to(dev)
        m2.load_state_dict(syn.make_nerf_state_dict(seed=0, density_scale=30.0))
        out["default_net_32c_64f_lindisp"] = timed(m2)
        out["evals_per_ray_32c_64f"] = 33 + 97
        return out
    except Exception as e:  # informational leg: never take the headline down with it
        return {"error": f"{type(e).__name__}: {e}"}


def _pmc_file(kind="render"):
    """The newest committed rocprofv3 PMC summary: kind "render" = profiles/rNN_pmc.json (counters of THIS command's headline region),
    "train" = profiles/rNN_train_pmc.json (counters of the config-5 training step, tools/pmc_wgrad.sh); or (None, None)."""
    import glob
    import re

    pat = r"r\d+_pmc\.json" if kind == "render" else r"r\d+_train_pmc\.json"
    paths = [p for p in glob.glob(os.path.join(ROOT, "profiles", "*_pmc.json")) if re.fullmatch(pat, os.path.basename(p))]
    for path in sorted(paths, reverse=True):
        try:
            return json.load(open(path)), os.path.relpath(path, ROOT)
        except Exception:
            continue
    return None, None


def _pmc_bytes(pmc, needle):
    """HBM bytes per launch of the kernel whose name contains `needle`: FETCH_SIZE / WRITE_SIZE are in KiB, and on gfx950
    FETCH_SIZE counts half the bytes of a wide coalesced read (MI355X_MICROARCH.md, HBM section), hence the factor 2."""
    k = next(v for name, v in pmc.items() if needle in name)
    return (2.0 * k["FETCH_SIZE"]["avg_per_dispatch"] + k["WRITE_SIZE"]["avg_per_dispatch"]) * 1024.0


COMMITTED = "committed (rocprofv3 PMC passes, separate --pmc runs; not measured in this run)"


def _pmc_mfma_busy(pmc, needle):
    """MFMA busy fraction of the kernel whose name contains `needle`: SQ_VALU_MFMA_BUSY_CYCLES over 4 SIMDs x SQ_BUSY_CU_CYCLES (cycles
    over cycles: independent of the clock the counter pass ran at), or None."""
    try:
        k = next(v for name, v in pmc.items() if needle in name)
        return k["SQ_VALU_MFMA_BUSY_CYCLES"]["avg_per_dispatch"] / (4.0 * k["SQ_BUSY_CU_CYCLES"]["avg_per_dispatch"])
    except Exception:
        return None


def pmc_traffic():
    """HBM bytes per launch (and the MFMA busy fraction) of the dominant kernel from the committed rocprofv3 PMC passes of this same
    command.  bench.py cannot run the profiler on itself, so this is the last committed measurement, not a live one; null when no profile
    is present."""
    pmc, src = _pmc_file()
    try:
        return {"traffic": _pmc_bytes(pmc, "mlp_fwd_kernel"), "traffic_unit": "B/launch", "traffic_source": src,
                "mfma_busy": _pmc_mfma_busy(pmc, "mlp_fwd_kernel"), "mfma_busy_source": src,
                "traffic_provenance": COMMITTED + ": " + "tools/profile_round.sh, this same command"}
    except Exception:
        return {"traffic": None, "traffic_provenance": "none (no committed PMC summary found)"}


RAY_KERNEL_NEEDLES = (("coarse_fused", "composite_kernel<true, true, 65>"), ("composite", "composite_kernel<true, false, 193>"),
                      ("sample_t", "sample_t4_kernel"), ("sample_pdf", "sample_pdf_kernel"))
PROFILED_FRAME_RAYS = 640 * 480    # the frame of the profiled command (tools/profile_round.sh runs bench.py's default workload)


def pmc_traffic_ray_kernels(hbm, rays_per_launch=PROFILED_FRAME_RAYS):
    """Same for the per-ray kernels (`hbm_kernels`).  The committed counters are of frame-sized launches (307,200 rays); a leg whose
    launches cover another number of rays (the 320x240 legs) gets the profiled bytes PER RAY times its own rays -- these kernels move
    a fixed number of bytes per ray -- and says so."""
    pmc, src = _pmc_file()
    for key, needle in RAY_KERNEL_NEEDLES:
        if key in hbm and hbm[key] is not None:
            try:
                b = _pmc_bytes(pmc, needle) * rays_per_launch / PROFILED_FRAME_RAYS
                how = "" if rays_per_launch == PROFILED_FRAME_RAYS else f"; scaled per ray from the profiled {PROFILED_FRAME_RAYS}-ray launch to {rays_per_launch} rays"
                hbm[key].update({"traffic": b, "traffic_unit": "B/launch", "traffic_source": src, "traffic_provenance": COMMITTED + how})
            except Exception:
                hbm[key]["traffic_provenance"] = "none (kernel not in the committed PMC summary)"
    return hbm


TRAIN_KERNEL_NEEDLES = {"mlp_fwd": "art_mlp_fwd_kernel<true, true", "bwd_chain": "art_bwd_chain_kernel", "wgrad": "wgrad_grouped_kernel"}


def pmc_traffic_train(kernels, launches_per_step):
    """HBM bytes of the training step's kernel classes from profiles/rNN_train_pmc.json (the same 4096-ray articulated step,
    tools/pmc_wgrad.sh): per launch (average over the class's launches of a step) and per step; -> (bytes per step of the three
    classes + the head reductions, source) or (None, None)."""
    pmc, src = _pmc_file("train")
    total = 0.0
    try:
        for key, needle in TRAIN_KERNEL_NEEDLES.items():
            if key in kernels:
                b = _pmc_bytes(pmc, needle)
                kernels[key].update({"traffic": b, "traffic_unit": "B/launch (average over the class's launches)", "traffic_per_step": b * launches_per_step[key],
                                     "traffic_source": src, "traffic_provenance": COMMITTED + ": tools/pmc_wgrad.sh, the same 4096-ray step"})
                total += b * launches_per_step[key]
        head = _pmc_bytes(pmc, "head_wgrad_kernel")
        total += head * launches_per_step["wgrad"]
        hk = next(v for name, v in pmc.items() if "head_wgrad_kernel" in name)
        dur_s = hk["FETCH_SIZE"]["avg_duration_ns"] * 1e-9
        head_roof = {"bound": "hbm", "kernel": "aon::head_wgrad_kernel (head / bias / first-deformation-layer reductions: plane rows x one 16-byte record per sample, fp64 sums)",
                     "traffic": head, "traffic_unit": "B/launch", "avg_launch_us": dur_s * 1e6, "achieved": head / dur_s / 1e9, "peak": PEAK_HBM_TBS * 1e3, "unit": "GB/s",
                     "frac": head / dur_s / 1e12 / PEAK_HBM_TBS, "traffic_source": src,
                     "traffic_provenance": COMMITTED + ": duration and bytes both from that profile (the kernel has no timer class of its own)"}
        return total, src, head_roof
    except Exception:
        return None, None, None


def train_leg(dev, rank, world, distributed, steps=24, n_rays=4096):
    """Informational only (never `value`): BASELINE config 5 per GPU -- articulated NeRF_AE_Art + code library, 4096 rays,
    randomized sampling, loss of model_autodecoder.py:395-477, HIP forward+backward, ONE flat gradient all-reduce over RCCL
    when world > 1 (parallel.allreduce_gradients), Adam.  Returns a dict for the JSON line (or {"error": ...})."""
    try:
        import types

        import aon_amd.synthetic as syn
        from aon_amd import ops
        from aon_amd.models.code_library import CodeLibraryArticulated
        from aon_amd.models.vanilla_nerf.helper import train_loss
        from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art
        from aon_amd.parallel import allreduce_gradients

        model = NeRF_AE_Art().to(dev)
        model.load_state_dict(syn.make_art_state_dict(seed=0, density_scale=30.0))
        lib = CodeLibraryArticulated(types.SimpleNamespace(N_max_objs=1, N_obj_code_length=128)).to(dev)
        lib.load_state_dict(syn.make_code_library_state(seed=0, n_max_objs=1))
        both = torch.nn.ModuleList([model, lib])
        from aon_amd.models.vanilla_nerf.model import build_adam
        opt = build_adam([model, lib], 5e-4)   # the harness's optimizer (LitNeRF_AutoDecoder.configure_optimizers): Adam(betas=(0.9, 0.999)) as ONE launch on a parameter arena
        batch = {"instance_id": torch.tensor([0], device=dev), "articulation_id": torch.tensor([3], device=dev)}
        H, W = 480, 640
        ro, vd = ops.raygen(syn.look_at_pose(4.0, 30.0 + 45.0 * rank, 30.0), H, W, syn.focal_from_fovy(H), device=dev)
        g = torch.Generator(device=dev).manual_seed(rank)
        idx = torch.randint(0, H * W, (n_rays,), device=dev, generator=g)
        rays = {"rays_o": ro[idx].contiguous(), "rays_d": vd[idx].contiguous(), "viewdirs": vd[idx].contiguous()}
        target = torch.rand(n_rays, 3, device=dev, generator=g)

        ar_marks = []

        def step():
            opt.zero_grad(set_to_none=True)
            latents = lib(batch)
            out = model(rays, True, True, syn.NEAR, syn.FAR, latents)
            # the harness's loss lines (LitNeRF_AutoDecoder.training_step): loss1 + loss0 + 1e-4 * the latent regulariser, two launches
            loss, _ = train_loss(out, target, (latents["density"], latents["color"], latents["articulation"]), 1e-4)
            loss.backward()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            allreduce_gradients(both)     # a no-op at world size 1
            e1.record()
            ar_marks.append((e0, e1))
            opt.step()
            return loss

        def fence():
            torch.cuda.synchronize()
            if distributed:
                dist.barrier()
                torch.cuda.synchronize()

        def timed(profile=False):
            for _ in range(4):   # untimed steps: the first allocates the 26 GB of workspaces of a step from the driver; the clock settles over the next ones
                step()
            fence()
            if profile:
                ops.profile_begin()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = step()
            fence()
            t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
            if profile:
                ops.profile_end()
            if distributed:
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return t.item() / steps, float(loss.detach()), ops.profile_classes() if profile else None

        # the step as the product runs it (round 4: merged launches on ONE stream -- forward coarse(A) | fine(A)+coarse(B) | fine(B), one
        # backward chain launch for both levels, then the levels' weight gradients), no kernel-class timers
        train_state = GpuStateSampler(dev.index or 0, enabled=rank == 0)
        train_state.__enter__()     # (spans the product pass and the per-class pass below: ~0.8 s of the same load)
        dt, loss, _ = timed()
        # gradient exchange as this rank saw it (HIP events; includes waiting for the slowest rank's backward), min / max over ranks
        ar = torch.tensor([sum(a.elapsed_time(b) for a, b in ar_marks[-steps:]) / steps], dtype=torch.float64, device=dev)
        ar_all = [ar.clone() for _ in range(world)]
        if distributed:
            dist.all_gather(ar_all, ar)
        ar_all = torch.cat(ar_all).cpu()
        # per-kernel-class durations from a second pass with the library's HIP-event timers on (and the round-3 stream overlap
        # switches off: they only matter when the merged forms are disabled)
        ops.set_bwd_overlap(False)
        ops.set_fwd_overlap(False)      # likewise the forward's two ray halves
        try:
            dt_serial, _, classes = timed(profile=True)
        finally:
            ops.set_bwd_overlap(True)
            ops.set_fwd_overlap(True)
            train_state.__exit__(None, None, None)
        samples = n_rays * EVALS_PER_RAY
        fold = bool(ops.bottleneck_fold())
        mac_f, mac_c, mac_w = executed(ART_MAC_FWD, fold, ops.view_bias_enabled()), executed(ART_MAC_BWD_CHAIN, fold), executed(ART_MAC_WGRAD, fold)
        mac_lit, mac_ex = 3 * ART_MAC_LITERAL, mac_f + mac_c + mac_w
        kernels = {}
        for key, name, mac in (("mlp_fwd", "aon::art_mlp_fwd_kernel<true,true,fold> (training forward: + activation planes, ReLU bits)", mac_f),
                               ("bwd_chain", "aon::art_bwd_chain_kernel<fold> (data-gradient chain + gradient planes)", mac_c),
                               ("wgrad", "aon::wgrad_grouped_kernel (all layers of a level in one launch) + heads + second stage + un-fold + latent outer products", mac_w)):
            ms, launches, units = classes[key]
            r = mfma_roofline(name, ms, launches, samples * steps, mac, ART_MAC_LITERAL)   # units are padded samples: price the real ones
            if r is not None:
                r["ms_per_step"] = ms / steps
                kernels[key] = r
        other_ms = sum(classes[k][0] for k in ("composite", "sample_pdf", "composite_pdf", "composite_bwd", "sample_t") if k in classes) / steps
        step_traffic, traffic_src, head_bytes = pmc_traffic_train(kernels, {k: v["launches"] / steps for k, v in kernels.items()})
        res = {"workload": f"articulated NeRF_AE_Art training step, {n_rays} rays/GPU, fwd+bwd" + (" + RCCL gradient all-reduce (6.4 MB, one bucket)" if world > 1 else "") + " + Adam (" + type(opt).__name__ + ": one launch on the parameter arena)",
               "ms_per_step": dt * 1e3, "rays_per_s": world * n_rays / dt, "steps": steps, "loss": loss, "gpu_state": train_state.summary(), "bottleneck_fold": fold, "view_bias": bool(ops.view_bias_enabled()),
               "allreduce_ms": {"min": ar_all.min().item(), "max": ar_all.max().item(), "per_rank": ar_all.tolist(),
                                "note": "parallel.allreduce_gradients per step, HIP events on the launch stream; 0 at world size 1 (no-op); "
                                        "includes the wait for the slowest rank's backward"},
               "roofline": {"bound": "mfma", "unit": "TFLOP/s", "peak": PEAK_FP32_MATRIX_TFLOPS,
                            "achieved": samples * mac_ex * 2 / dt / 1e12, "frac": samples * mac_ex * 2 / dt / 1e12 / PEAK_FP32_MATRIX_TFLOPS,
                            "achieved_reference_literal": samples * mac_lit * 2 / dt / 1e12,
                            "frac_reference_literal": samples * mac_lit * 2 / dt / 1e12 / PEAK_FP32_MATRIX_TFLOPS,
                            "flop_per_ray_executed": 2 * mac_ex * EVALS_PER_RAY, "flop_per_ray_reference_literal": 2 * mac_lit * EVALS_PER_RAY,
                            "note": "whole step (kernels + Adam + harness) priced against the fp32-matrix peak; executed = MACs the kernels issue "
                                    "(latent columns folded into biases; bottleneck_layer folded into views_linear[0] when bottleneck_fold; the forward's "
                                    "view-encoding chunk replaced by a per-ray bias when view_bias), "
                                    "reference-literal = 3 x the forward MACs of SURVEY R10",
                            "kernels": kernels, "per_ray_kernels_ms_per_step": other_ms,
                            "kernel_ms_per_step": sum(k["ms_per_step"] for k in kernels.values()) + other_ms,
                            "kernels_measured_on": "a second pass of the same schedule with the library's per-kernel-class HIP-event timers on "
                                                   f"({dt_serial * 1e3:.2f} ms per step); forward = 3 merged launches per step, chain = 1 launch "
                                                   "for both levels, wgrad = 1 grouped launch per level",
                            "traffic": step_traffic, "traffic_unit": "B/step (forward + chain + weight gradients + head reductions)", "traffic_source": traffic_src,
                            "traffic_provenance": (COMMITTED + ": tools/pmc_wgrad.sh, the same 4096-ray step") if step_traffic else "none (no committed training PMC summary found)",
                            "hbm_kernels": {"head_reductions": head_bytes}}}
        return res
    except Exception as e:  # informational leg: never take the headline down with it
        return {"error": f"{type(e).__name__}: {e}"}


DUMP_LIMIT_BYTES = 60 * 2**20   # --dump-outputs stays under 64 MB in all, .npy headers included


def dump_outputs(outdir, arrays):
    """Write each tensor of `arrays` as outdir/<name>.npy in float32 (float64 stays float64).  Over DUMP_LIMIT_BYTES in all, every
    array keeps the same fixed, seeded sample of its rows (sorted, so a row of one array still pairs with the same row of another)."""
    import numpy as np

    os.makedirs(outdir, exist_ok=True)
    arrays = {k: v.detach().cpu() for k, v in arrays.items()}
    arrays = {k: v if v.dtype == torch.float64 else v.float() for k, v in arrays.items()}
    total = sum(v.numel() * v.element_size() for v in arrays.values())
    for name, v in arrays.items():
        if total > DUMP_LIMIT_BYTES and v.dim() > 0 and v.shape[0] > 1:
            keep = max(1, v.shape[0] * DUMP_LIMIT_BYTES // total)
            v = v[torch.randperm(v.shape[0], generator=torch.Generator().manual_seed(0))[:keep].sort().values]
        np.save(os.path.join(outdir, name + ".npy"), v.contiguous().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--full", action="store_true", help="also measure everything beyond the headline: live roofline of the timed region, "
                    "clock / power samples, the informational legs and the CPU baseline (the --no-* options below select among them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's outputs as DIR/<name>.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(with --full) skip the CPU baseline and its PSNR check")
    ap.add_argument("--no-alt", action="store_true", help="(no-op since round 3: the split-bf16 engine was removed; kept for old command lines)")
    ap.add_argument("--sharded-leg", action="store_true", help="kept for old command lines: with --full the sharded-frame leg always runs")
    ap.add_argument("--no-sharded-leg", action="store_true", help="(with --full) skip the informational BASELINE config 3 leg (one frame sharded over the ranks + RCCL all-gather)")
    ap.add_argument("--no-train-leg", action="store_true", help="(with --full) skip the extra (informational) articulated training-step timing")
    ap.add_argument("--no-extra-legs", action="store_true", help="(with --full) skip the informational BASELINE config 1 / config 4 render legs")
    ap.add_argument("--literal", action="store_true", help="A/B: aon_set_bottleneck_fold(0) -- the reference-literal two-layer bottleneck + view layer of rounds 1-4")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 or "RANK" in os.environ:  # launched by torch.distributed.run: exercise the RCCL path even at N=1
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run"
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    import aon_amd.synthetic as syn
    from aon_amd import ops
    from aon_amd.datasets.ray_utils import get_frame_rays
    from aon_amd.models.vanilla_nerf.model import NeRF
    from aon_amd.parallel import all_gather_pixels

    if args.literal:
        ops.set_bottleneck_fold(False)
    fold = bool(ops.bottleneck_fold())
    H, W = args.height, args.width
    n_rays = H * W
    sd = syn.make_nerf_state_dict(seed=0, density_scale=30.0)
    model = NeRF().to(dev)
    model.load_state_dict(sd)
    # weak scaling: rank r renders its own frame (pose r of a ring around the object)
    c2w = syn.look_at_pose(4.0, 30.0 + 45.0 * rank, 30.0)
    rays_o, viewdirs = get_frame_rays(H, W, syn.focal_from_fovy(H), c2w, device=dev)
    rays = {"rays_o": rays_o, "rays_d": viewdirs, "viewdirs": viewdirs}

    distributed = dist.is_available() and dist.is_initialized()

    marks = []   # per timed step: (begin, rendered, gathered) events on torch's current stream (recording is asynchronous)
    last = {}    # what the latest step handed back: both levels of this rank's frame, and the gathered fine level

    def step():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        out = model(rays, False, True, syn.NEAR, syn.FAR)
        ev[1].record()
        res = all_gather_pixels(out[1], counts=[n_rays] * world) if distributed else out[1]   # one RCCL all-gather of 20 B/ray; (world*n, .) rank-major
        ev[2].record()
        marks.append(ev)
        last["levels"], last["gathered"] = out, res
        return res

    def fence():
        torch.cuda.synchronize()
        if distributed:
            dist.barrier()
            torch.cuda.synchronize()

    with torch.no_grad():
        for _ in range(args.warmup):
            step()
        fence()
        marks.clear()
        if args.full:   # the library's per-kernel-class HIP-event timers: the live roofline of this region
            ops.profile_begin()
        with GpuStateSampler(local_rank, enabled=rank == 0 and args.full) as gpu_state:
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fine = step()
            fence()
            dt = time.perf_counter() - t0
        if args.full:
            mlp_ms, mlp_launches, mlp_samples = ops.profile_end()
            headline_classes = ops.profile_classes()

    if args.dump_outputs and rank == 0:
        arrays = {}
        for lvl, name in enumerate(("coarse", "fine")):
            arrays.update({f"{name}_{k}": v for k, v in zip(("rgb", "acc", "depth"), last["levels"][lvl])})
        if distributed:
            arrays.update({f"gathered_fine_{k}": v for k, v in zip(("rgb", "acc", "depth"), last["gathered"])})
        dump_outputs(args.dump_outputs, arrays)

    dt_local = dt
    t = torch.tensor([dt], dtype=torch.float64, device=dev)
    if distributed:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = t.item()
    # Self-diagnosis of a multi-GPU run (outside the timed region): who took part, and where each rank's time went.  `render_ms`
    # = NeRF.forward of this rank's frame, `gather_ms` = the all-gather INCLUDING the wait for the slowest rank to arrive.
    render_ms = sum(e[0].elapsed_time(e[1]) for e in marks) / max(len(marks), 1)
    gather_ms = sum(e[1].elapsed_time(e[2]) for e in marks) / max(len(marks), 1)
    mine = torch.tensor([1.0, rank, render_ms, gather_ms, dt_local / args.steps * 1e3], dtype=torch.float64, device=dev)
    per_rank = [mine.clone() for _ in range(world)]
    if distributed:
        dist.all_gather(per_rank, mine)
    per_rank = torch.stack(per_rank).cpu()
    diag = {"ranks_seen": int(per_rank[:, 0].sum().item()), "world": world, "device": torch.cuda.get_device_name(dev),
            "render_ms": {"min": per_rank[:, 2].min().item(), "max": per_rank[:, 2].max().item(), "per_rank": per_rank[:, 2].tolist()},
            "gather_ms": {"min": per_rank[:, 3].min().item(), "max": per_rank[:, 3].max().item(), "per_rank": per_rank[:, 3].tolist()},
            "step_ms_host_clock": {"min": per_rank[:, 4].min().item(), "max": per_rank[:, 4].max().item()},
            "note": "HIP events on the launch stream per timed step; gather_ms includes waiting for the slowest rank, so "
                    "max(render_ms) + min(gather_ms) ~ ms_per_step; the efficiency of the weak-scaled value is ~ N=1's ms_per_step / ms_per_step"}
    n1_frame_ms = per_rank[:, 2].mean().item()   # one rank rendering one whole frame alone: the N = 1 reference of the sharded leg

    # BASELINE config 3 literally (informational, never `value`): ONE 640x480 frame, contiguous ray ranges sharded over the
    # ranks, fine-level pixels all-gathered (RCCL) -- strong scaling of a single frame, where `value` above is weak scaling.
    sharded = None
    if args.full and not args.no_sharded_leg:
        own_group = False
        # RCCL prints a version banner on C-level stdout when it comes up; this script's stdout carries ONE JSON line, so file
        # descriptor 1 points at stderr while the leg runs (the banner would otherwise land behind the JSON at exit)
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            from aon_amd.parallel import render_frame_sharded

            if not distributed:   # plain `python bench.py` at N = 1: bring RCCL up for this leg so the all-gather is the real collective
                import socket

                with socket.socket() as sk:
                    sk.bind(("127.0.0.1", 0))
                    port = sk.getsockname()[1]
                os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
                dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
                own_group = True
            focal0, c2w0 = syn.focal_from_fovy(H), syn.look_at_pose(4.0, 30.0, 30.0)
            raygen = lambda h, w, f, c, b, e: get_frame_rays(h, w, f, c, b, e, device=dev)
            with torch.no_grad():
                render_frame_sharded(model, H, W, focal0, c2w0, syn.NEAR, syn.FAR, True, raygen, force=True)
                fence()
                ts = time.perf_counter()
                for _ in range(args.steps):
                    frame = render_frame_sharded(model, H, W, focal0, c2w0, syn.NEAR, syn.FAR, True, raygen, force=True)
                fence()
                tsd = torch.tensor([time.perf_counter() - ts], dtype=torch.float64, device=dev)
                # where a rank's time goes: its shard alone (raygen + render, no collective), timed after the frames above
                from aon_amd.parallel import shard_range
                b0, e0 = shard_range(n_rays, rank, world)
                sh0, sh1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                sh0.record()
                for _ in range(args.steps):
                    ro_s, vd_s = raygen(H, W, focal0, c2w0, b0, e0)
                    model({"rays_o": ro_s, "rays_d": vd_s, "viewdirs": vd_s}, False, True, syn.NEAR, syn.FAR)
                sh1.record()
                fence()
                shard_ms = torch.tensor([sh0.elapsed_time(sh1) / args.steps], dtype=torch.float64, device=dev)
            shard_all = [shard_ms.clone() for _ in range(world)]
            if distributed:
                dist.all_reduce(tsd, op=dist.ReduceOp.MAX)
                dist.all_gather(shard_all, shard_ms)
            shard_all = torch.cat(shard_all).cpu()
            dts = tsd.item() / args.steps
            sharded = {"workload": f"BASELINE config 3: one {W}x{H} frame, contiguous ray ranges sharded over {world} rank(s), raygen on the GPU, "
                                   "fine-level pixels all-gathered over RCCL (the collective runs at world size 1 too)",
                       "ms_per_frame": dts * 1e3, "rays_per_s": n_rays / dts, "frame_rows": int(frame[0].shape[0]), "world": world,
                       "collective": "all_gather_into_tensor (nccl = RCCL), 20 B/ray",
                       "n1_frame_ms": n1_frame_ms,
                       "efficiency_vs_n1": n1_frame_ms / world / (dts * 1e3),
                       "shard_render_ms": {"min": shard_all.min().item(), "max": shard_all.max().item(), "per_rank": shard_all.tolist()},
                       "exchange_and_skew_ms": dts * 1e3 - shard_all.max().item(),
                       "note": "efficiency_vs_n1 = (a whole frame rendered by ONE rank in this same run: the mean render_ms of the weak-scaled "
                               "leg) / world / ms_per_frame; exchange_and_skew_ms = ms_per_frame - the slowest rank's shard rendered alone"}
        except Exception as e:  # informational leg
            sharded = {"error": f"{type(e).__name__}: {e}"}
        finally:
            if own_group and dist.is_initialized():
                dist.destroy_process_group()
            try:
                import ctypes

                ctypes.CDLL(None).fflush(None)   # the C library's buffered banner goes out while fd 1 is still stderr
            except Exception:
                pass
            os.dup2(saved_fd, 1)
            os.close(saved_fd)

    train = train_leg(dev, rank, world, distributed) if args.full and not args.no_train_leg else None
    # BASELINE configs 1 and 4 on this rank's GPU (informational, never `value`)
    extra = args.full and not args.no_extra_legs
    config1 = render_leg(dev, "config1", 240, 320) if extra else None
    art_render = render_leg(dev, "art", 240, 320) if extra else None
    other_ctor = other_constructor_leg(dev) if extra else None

    if rank == 0:
        rays_per_s = world * n_rays * args.steps / dt
        res = {
            "metric": "rays/sec (64c+128f samples)", "value": rays_per_s, "unit": "rays/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": f"sapien-single-scene vanilla NeRF full-frame render {W}x{H}, 65 coarse + 193 fine evals/ray, "
                                   f"{n_rays} rays per GPU per step, randomized=False, white_bkgd=True",
                       "rays_per_gpu": n_rays, "evals_per_ray": EVALS_PER_RAY,
                       "exchange": "RCCL all_gather of (rgb,acc,depth)=20 B/ray" if world > 1 else "none"},
            "multi_gpu": diag,
            "bottleneck_fold": fold,
            "view_bias": bool(ops.view_bias_enabled()),
        }
        if args.full:   # the live roofline of the timed region, its clock / power samples, the informational legs and the CPU baseline
            flop_ex = 2 * executed(VAN_MAC, fold, ops.view_bias_enabled())       # what the kernel executes per network evaluation
            mlp_tflops = mlp_samples * flop_ex / (mlp_ms * 1e-3) / 1e12 if mlp_ms > 0 else 0.0
            mlp_tflops_lit = mlp_samples * FLOP_PER_SAMPLE / (mlp_ms * 1e-3) / 1e12 if mlp_ms > 0 else 0.0
            res.update({
                "gpu_state": gpu_state.summary(),
                "roofline": {"bound": "mfma", "kernel": "aon::mlp_fwd_kernel<true,false,fold,view-bias> (fused encode+MLP, fp32 MFMA)",
                             "achieved": mlp_tflops, "peak": PEAK_FP32_MATRIX_TFLOPS, "unit": "TFLOP/s",
                             "frac": mlp_tflops / PEAK_FP32_MATRIX_TFLOPS, "traffic": None,
                             "peak_measured": PEAK_FP32_MATRIX_MEASURED_TFLOPS, "frac_of_peak_measured": mlp_tflops / PEAK_FP32_MATRIX_MEASURED_TFLOPS,
                             "achieved_reference_literal": mlp_tflops_lit, "frac_reference_literal": mlp_tflops_lit / PEAK_FP32_MATRIX_TFLOPS,
                             "launches": mlp_launches, "avg_launch_ms": mlp_ms / max(mlp_launches, 1),
                             "flop_per_sample": flop_ex, "flop_per_sample_reference_literal": FLOP_PER_SAMPLE,
                             "note": "achieved / frac price the FLOPs the kernel EXECUTES (bottleneck_layer folded into views_linear[0] when bottleneck_fold: "
                                     "65,536 MACs per sample fewer than the reference's graph; the view-encoding columns of that layer as a per-ray bias when "
                                     "view_bias: 3,584 fewer); *_reference_literal price the reference's 1,186,816 FLOP per "
                                     "sample against the same time and can exceed the executed fraction",
                             "whole_path_frac": rays_per_s / world * EVALS_PER_RAY * flop_ex / (PEAK_FP32_MATRIX_TFLOPS * 1e12),
                             "whole_path_frac_reference_literal": rays_per_s / world * EVALS_PER_RAY * FLOP_PER_SAMPLE / (PEAK_FP32_MATRIX_TFLOPS * 1e12)},
            })
            res["roofline"].update(pmc_traffic())
            res["hbm_kernels"] = pmc_traffic_ray_kernels(per_ray_rooflines(headline_classes))   # the non-GEMM kernels of the same timed region (>= 50 % of HBM peak each)
            if config1 is not None:
                res["config1"] = config1
            if art_render is not None:
                res["art_render"] = art_render
            if other_ctor is not None:
                res["other_constructor_arguments"] = other_ctor
            if sharded is not None:
                res["sharded_frame"] = sharded
            if train is not None:
                res["train_step"] = train
            # the informational legs' headline scalars, where the driver's parser keeps them (they survived only in the truncated tail)
            lifted = {}
            if train is not None and "error" not in train:
                lifted.update({"config5_train_step_ms": train["ms_per_step"], "config5_train_step_frac_executed": train["roofline"]["frac"],
                               "config5_train_step_frac_reference_literal": train["roofline"]["frac_reference_literal"],
                               "config5_train_rays_per_s": train["rays_per_s"]})
            if config1 is not None and "error" not in config1:
                lifted.update({"config1_rays_per_s": config1.get("value"), "config1_frac_executed": (config1.get("roofline") or {}).get("frac")})
            if art_render is not None and "error" not in art_render:
                lifted.update({"config4_art_render_rays_per_s": art_render.get("value"), "config4_art_render_frac_executed": (art_render.get("roofline") or {}).get("frac")})
            if sharded is not None and "error" not in sharded:
                lifted.update({"config3_sharded_frame_rays_per_s": sharded["rays_per_s"]})
            res["config"]["informational"] = lifted
            if world == 1 and not args.no_cpu_baseline:
                rays_cpu = {k: v.cpu() for k, v in rays.items()}
                base, ref_rgb, (a, b) = cpu_baseline(sd, rays_cpu)
                res["cpu_baseline"] = base
                mse = torch.mean((fine[0][:n_rays][a:b].cpu() - ref_rgb) ** 2).item()
                res["psnr_vs_oracle_db"] = float(-10.0 * torch.log10(torch.tensor(max(mse, 1e-20))))
                res["speedup_vs_cpu"] = rays_per_s / base["value"]
        print(json.dumps(res), flush=True)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
