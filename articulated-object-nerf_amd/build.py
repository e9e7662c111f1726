"""Build libaon_hip.so (gfx950) in-tree with hipcc.  No torch extension machinery: the library is a plain
C-ABI shared object (include/aon_hip.h) loaded with ctypes.

    python articulated-object-nerf_amd/build.py [--force]
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
# experiments: AON_BUILD_TAG=x builds build_x/ -> libaon_hip_x.so next to the product library (select it with AON_HIP_LIB)
_TAG = os.environ.get("AON_BUILD_TAG", "")
OBJ = os.path.join(PKG, "build" + ("_" + _TAG if _TAG else ""))
LIB = os.path.join(PKG, "libaon_hip" + ("_" + _TAG if _TAG else "") + ".so")
SOURCES = ["aon_mlp.hip", "aon_mlp_art.hip", "aon_train.hip", "aon_train_art.hip", "aon_train_latent.hip", "aon_ray_grad.hip", "aon_render.hip", "aon_gmlp.hip", "aon_fold.hip", "aon_optim.hip", "aon_metrics.hip", "aon_mesh.hip", "aon_occ.hip", "aon_bounds.hip", "aon_scene.hip", "aon_scene_occ.hip", "aon_scene_grad.hip", "aon_scene_pose.hip", "aon_scene_lists.hip", "aon_scene_lists_grad.hip", "aon_capi.hip", "aon_capi_render.hip", "aon_capi_train.hip", "aon_capi_gmlp.hip"]
HEADERS = [os.path.join(CSRC, "aon_common.h"), os.path.join(CSRC, "aon_params.h"), os.path.join(CSRC, "aon_launch.h"), os.path.join(CSRC, "aon_capi_util.h"), os.path.join(CSRC, "aon_mlp_core.h"), os.path.join(CSRC, "aon_pass.h"), os.path.join(CSRC, "aon_wgrad.h"), os.path.join(CSRC, "aon_art_common.h"), os.path.join(CSRC, "aon_ray_core.h"), os.path.join(CSRC, "aon_composite_grad.h"), os.path.join(CSRC, "aon_scene_merge.h"), os.path.join(CSRC, "aon_gmlp.h"), os.path.join(CSRC, "aon_fold.h"), os.path.join(CSRC, "aon_occ_lookup.h"),
           os.path.join(os.path.dirname(PKG), "include", "aon_hip.h"), os.path.join(os.path.dirname(PKG), "include", "aon_hip_inputs.h"),
           os.path.join(os.path.dirname(PKG), "include", "aon_hip_scene.h"), os.path.join(os.path.dirname(PKG), "include", "aon_hip_scene_occ.h"),
           os.path.join(os.path.dirname(PKG), "include", "aon_hip_scene_grad.h"), os.path.join(os.path.dirname(PKG), "include", "aon_hip_scene_pose.h"),
           os.path.join(os.path.dirname(PKG), "include", "aon_hip_scene_lists.h"),
           os.path.join(os.path.dirname(PKG), "include", "aon_hip_scene_lists_grad.h")]
# -ffp-contract=off: the stage kernels reproduce the reference's un-fused mul/add sequences; FMAs are explicit.
# Every file takes the same flags: the one per-file choice ever kept (rounds 1-3: a sched_barrier per MFMA step pinning the A-fragment
# prefetch in aon_train.hip) spilled 3.5 KB per lane once the chain took two segments (round 4) and is gone (profiles/LAB_NOTEBOOK.md).
FLAGS = (os.environ.get("AON_EXTRA_FLAGS", "").split()) + ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unused-lambda-capture"]


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm with gfx950 support)")


def _stale(target: str, deps: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(OBJ, exist_ok=True)
    cc = hipcc()
    jobs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, src.replace(".hip", ".o"))
        cmd = [cc, *FLAGS, "-c", s, "-o", o]
        # an object is also stale when it was built with other flags (AON_EXTRA_FLAGS experiments must not reuse objects)
        stamp = o + ".cmd"
        same_cmd = os.path.exists(stamp) and open(stamp).read() == " ".join(cmd)
        if force or not same_cmd or _stale(o, [s] + HEADERS):
            jobs.append(cmd)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True, timeout=1800)
        with open(cmd[-1] + ".cmd", "w") as f:
            f.write(" ".join(cmd))

    with ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(run, jobs))
    objs = [os.path.join(OBJ, s.replace(".hip", ".o")) for s in SOURCES]
    if force or jobs or _stale(LIB, objs):
        run([cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs])
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
