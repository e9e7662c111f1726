"""ctypes binding of libaon_hip.so (C ABI declared in include/aon_hip.h).

There is NO fallback: if the shared library is missing or fails to load, importing this module raises, and so
does every op built on it.  Build it with ``python articulated-object-nerf_amd/build.py`` (hipcc, gfx950).
"""
from __future__ import annotations

import ctypes as C
import os

# torch FIRST: it carries its own copy of the HIP runtime (torch/lib/libamdhip64.so), and the process must run on ONE runtime --
# the one that owns torch's allocations and streams.  Loading libaon_hip.so before torch binds it to /opt/rocm's copy instead, and
# its first launch on torch's memory fails with "no ROCm-capable device is detected" (seen when __graft_entry__.build() and
# smoke() ran in one process on a GPU box).
import torch  # noqa: F401

_PKG = os.path.dirname(os.path.abspath(__file__))
# AON_HIP_LIB: an alternative build of the SAME library (A/B experiments, tools/kernel_bench.py); never a different backend
LIB_PATH = os.environ.get("AON_HIP_LIB") or os.path.join(_PKG, "libaon_hip.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: the HIP kernels are the product path and there is no CPU/eager fallback. "
        "Build them with `python articulated-object-nerf_amd/build.py` (needs /opt/rocm/bin/hipcc)."
    )

lib = C.CDLL(LIB_PATH)

_p, _i, _l, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float
# The whole-path forwards (one C call from rays to composited levels) share one argument list, csrc/aon_capi_util.h's PathCall, between a
# network prefix and the suffixes of the form
_PATH = ([_p, _p, _p, _l]          # rays_o, rays_d, viewdirs, n_rays
         + [_f, _f, _i, _i]        # near, far, white_bkgd, num_levels
         + [_p, _p, _l]            # t_rand, u, u_stride
         + [_p] * 6                # rgb, acc, depth of the coarse and of the fine level
         + [_p, _l, _p])           # workspace, workspace_bytes, stream
_VANILLA, _ART, _GENERAL = [_p] * 2, [_p] * 4, [_p] * 3   # packed c/f | packed, small c/f | aon_mlp_geometry, parameter arrays c/f
_OPTS, _OCC, _STOP, _BOUNDS = [_p], [_p, _p], [_f, _i, _p], [_p]   # opts | grid, tally | eps, round_samples, stop map | aon_ray_bounds
# The whole-path backwards share csrc/aon_capi_util.h's BwdCall: its two runs stand either side of the network's own arrays
_BWD = ([_p, _l, _i, _i] + [_p] * 3,     # rays_d, n_rays, white_bkgd, num_levels | g_rgb, g_acc, g_depth (host arrays of device pointers)
        [_p, _l, _p, _l, _p])            # workspace, workspace_bytes, scratch, scratch_bytes, stream
_PER_LEVEL, _LATENTS, _RAY_GRADS = [_p] * 2, [_p] * 3, [_p]   # parameter / gradient arrays c/f | three codes or their gradients | aon_ray_grads


def _path_sigs():
    sigs = {"aon_grender_fwd": _GENERAL + _PATH + _OPTS, "aon_grender_fwd_train": _GENERAL + _PATH + _OPTS}
    for net, prefix in (("aon_", _VANILLA), ("aon_art_", _ART)):
        head = prefix + _PATH
        sigs.update({net + "render_fwd": head, net + "render_fwd_ex": head + _OPTS, net + "render_fwd_occ": head + _OPTS + _OCC,
                     net + "render_fwd_stop": head + _OPTS + _OCC + _STOP, net + "render_fwd_bounds": head + _OPTS + _OCC + _STOP + _BOUNDS,
                     net + "render_fwd_train": head, net + "render_fwd_train_ex": head + _OPTS,
                     net + "render_fwd_train_bounds": head + _OPTS + _BOUNDS})
    return {name: (_i, args) for name, args in sigs.items()}


def _bwd_sigs():
    head, tail = _BWD
    vanilla = _VANILLA * 2 + head + _PER_LEVEL + tail                                 # transposed and forward stream c/f ... gradients
    art = _ART + head + _PER_LEVEL + _LATENTS + _PER_LEVEL + _LATENTS + tail           # ... parameters, codes, gradients, code gradients
    frozen = _ART + head + _PER_LEVEL + _LATENTS + tail + _OPTS                        # ... parameters, code gradients
    sigs = {"aon_render_bwd": vanilla, "aon_render_bwd_ex": vanilla + _OPTS, "aon_art_render_bwd": art, "aon_art_render_bwd_ex": art + _OPTS,
            "aon_art_render_bwd_latents": frozen, "aon_art_render_bwd_inputs": frozen + _RAY_GRADS,
            "aon_grender_bwd": _GENERAL + head + _PER_LEVEL + tail + _OPTS}
    return {name: (_i, args) for name, args in sigs.items()}


_SIGS = {
    **_path_sigs(),
    **_bwd_sigs(),
    "aon_abi_version": (_i, []),
    "aon_last_error": (C.c_char_p, []),
    "aon_raygen": (_i, [_p, _i, _i, _f, _l, _l, _p, _p, _p, _p]),
    "aon_train_loss_fwd": (_i, [_p, _p, _p, _l, _p, _p, _f, _p, _p, _p]),
    "aon_train_loss_bwd": (_i, [_p, _p, _p, _l, _p, _p, _f, _p, _p, _p, _p, _p]),
    "aon_ray_directions": (_i, [_i, _i, _f, _p, _p]),
    "aon_get_rays": (_i, [_p, _p, _l, _p, _p, _p, _p]),
    "aon_ray_radii": (_i, [_p, _p, _i, _i, _p, _p]),
    "aon_cast_rays": (_i, [_p, _p, _p, _l, _i, _p, _p]),
    "aon_sample_along_rays": (_i, [_p, _p, _l, _i, _f, _f, _p, _p, _p, _p]),
    "aon_pos_enc": (_i, [_p, _l, _i, _i, _p, _p]),
    "aon_mlp_packed_bytes": (_l, []),
    "aon_pack_vanilla_mlp": (_i, [_p, _p, _p]),
    "aon_mlp_fwd": (_i, [_p, _p, _p, _p, _p, _l, _i, _p, _p]),
    "aon_mlp_fwd_enc": (_i, [_p, _p, _p, _l, _i, _p, _p]),
    "aon_composite": (_i, [_p, _i, _p, _i, _p, _p, _l, _i, _i, _i, _p, _p, _p, _p, _p]),
    "aon_sample_pdf": (_i, [_p, _p, _l, _p, _p, _l, _l, _p, _p, _p]),
    "aon_art_packed_bytes": (_l, []),
    "aon_art_small_bytes": (_l, []),
    "aon_pack_art_mlp": (_i, [_p, _p, _p]),
    "aon_art_prepare": (_i, [_p, _p, _p, _p, _p, _p]),
    "aon_pack_art_mlp_deg": (_i, [_p, _i, _i, _i, _p, _p]),
    "aon_art_prepare_deg": (_i, [_p, _p, _p, _p, _i, _i, _i, _p, _p]),
    "aon_pack_art_mlp_bwd_deg": (_i, [_p, _i, _i, _i, _p, _p]),
    "aon_art_mlp_fwd": (_i, [_p, _p, _p, _p, _p, _p, _l, _i, _p, _p]),
    "aon_art_mlp_fwd_pos": (_i, [_p, _p, _p, _p, _l, _i, _p, _p]),
    "aon_train_plane_rows": (_l, []),
    "aon_bwd_packed_bytes": (_l, []),
    "aon_wgrad_workspace_bytes": (_l, []),
    "aon_pack_vanilla_mlp_bwd": (_i, [_p, _p, _p]),
    "aon_train_mask_bytes": (_l, [_l]),
    "aon_mlp_fwd_train": (_i, [_p, _p, _p, _p, _p, _l, _i, _p, _p, _p, _p]),
    "aon_composite_bwd": (_i, [_p, _p, _p, _p, _p, _p, _l, _i, _i, _i, _p, _p]),
    "aon_mlp_bwd_chain": (_i, [_p, _p, _p, _p, _p, _l, _p]),
    "aon_vanilla_wgrad": (_i, [_p, _p, _p, _l, _p, _p, _l, _p, _p]),
    "aon_wgrad_plan": (_i, [_i, _l, _i, _p, _i, _p]),
    "aon_wgrad_plan_segment": (_i, [_i, _l, _i, _i, _i, _p]),
    "aon_wgrad_kind_bench": (_i, [_i, _i, _p, _p, _i, _l, _p, _l, _p]),
    "aon_art_train_plane_rows": (_l, []),
    "aon_art_train_mask_bytes": (_l, [_l]),
    "aon_art_bwd_packed_bytes": (_l, []),
    "aon_pack_art_mlp_bwd": (_i, [_p, _p, _p]),
    "aon_art_mlp_fwd_train": (_i, [_p, _p, _p, _p, _p, _p, _l, _i, _p, _p, _p, _p]),
    "aon_art_bwd_chain": (_i, [_p, _p, _p, _p, _p, _p, _p, _l, _p]),
    "aon_art_wgrad": (_i, [_p, _p, _p, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p, _l, _p, _p]),
    "aon_art_wgrad_deg": (_i, [_p, _p, _p, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p, _l, _p, _i, _i, _i, _p]),
    "aon_set_bottleneck_fold": (_i, [_i]),
    "aon_get_bottleneck_fold": (_i, []),
    "aon_stream_is_folded": (_i, [_p]),
    "aon_stream_form": (_i, [_p]),
    "aon_declare_stream_form": (_i, [_p, _i]),
    "aon_adam_step": (_i, [_p, _p, _p, _p, _l, C.c_double, C.c_double, C.c_double, C.c_double, _l, _p]),
    "aon_code_library_fwd": (_i, [_p, _p, _p, _p, _p, _p]),
    "aon_code_library_bwd": (_i, [_p, _p, _p, _p, _p, _p]),
    "aon_ssim_workspace_bytes": (_l, [_i, _p, _p]),
    "aon_ssim": (_i, [_i, _p, _p, _p, _p, _p, _l, _p, _p]),
    "aon_density_grid": (_i, [_p, _p, _p, _p, _l, _l, _i, _p, _p]),
    "aon_art_density_grid": (_i, [_p, _p, _p, _p, _p, _l, _l, _i, _p, _p]),
    "aon_marching_cubes_workspace_bytes": (_l, [_p]),
    "aon_marching_cubes_count": (_i, [_p, _p, _f, _p, _l, _p, _p]),
    "aon_marching_cubes": (_i, [_p, _p, _f, _p, _p, _p, _l, _p, _l, _p, _l, _p]),
    "aon_occupancy_bytes": (_l, [_p]),
    "aon_occupancy_build": (_i, [_p, _p, _f, _i, _p, _p]),
    "aon_render_occ_workspace_bytes": (_l, [_l, _p]),
    "aon_render_stop_workspace_bytes": (_l, [_l, _p]),
    "aon_art_pack_step": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p]),
    "aon_vanilla_pack_step": (_i, [_p, _p, _i, _i, _i, _p, _p, _p, _p, _p]),
    "aon_set_bwd_early_heads": (_i, [_i]),
    "aon_set_view_bias": (_i, [_i]),
    "aon_get_view_bias": (_i, []),
    "aon_set_deferred_view": (_i, [_i]),
    "aon_get_deferred_view": (_i, []),
    "aon_render_deferred_workspace_bytes": (_l, [_l, _p]),
    "aon_test_set_deferred_slab": (_i, [_i]),
    "aon_view_bias": (_i, [_p, _p, _l, _p, _p]),
    "aon_set_bwd_overlap": (_i, [_i]),
    "aon_set_fwd_overlap": (_i, [_i]),
    "aon_set_fwd_merge": (_i, [_i]),
    "aon_set_bwd_merge": (_i, [_i]),
    "aon_set_wgrad_probe": (_i, [_p]),
    "aon_train_workspace_bytes": (_l, [_l, _i, _i]),
    "aon_train_scratch_bytes": (_l, [_l, _i, _i]),
    "aon_profile_begin": (_i, []),
    "aon_profile_end": (_i, [C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "aon_profile_class": (_i, [_i, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "aon_composite_pdf": (_i, [_p, _p, _p, _l, _i, _i, _p, _l, _p, _p, _p, _p, _p, _p]),
    "aon_set_coarse_fusion": (_i, [_i]),
    "aon_render_workspace_bytes": (_l, [_l]),
    # constructor arguments beyond the defaults (aon_render_opts; the *_ex forms take the struct pointer last)
    "aon_render_opts_init": (None, [_p]),
    "aon_pack_vanilla_mlp_deg": (_i, [_p, _i, _i, _i, _p, _p]),
    "aon_pack_vanilla_mlp_bwd_deg": (_i, [_p, _i, _i, _i, _p, _p]),
    "aon_sample_along_rays_ex": (_i, [_p, _p, _l, _i, _f, _f, _i, _f, _f, _p, _p, _p, _p]),
    "aon_composite_ex": (_i, [_p, _i, _p, _i, _p, _p, _l, _i, _i, _i, _p, _p, _p, _p, _p, _p]),
    "aon_sample_pdf_n": (_i, [_p, _p, _l, _p, _p, _l, _l, _i, _i, _i, _p, _p, _p]),
    "aon_render_workspace_bytes_ex": (_l, [_l, _p]),
    "aon_train_workspace_bytes_ex": (_l, [_l, _i, _i, _p]),
    "aon_train_scratch_bytes_ex": (_l, [_l, _i, _i, _p]),
    # scratch of the latent-only backward, and with the ray gradients' records (section 4.14)
    "aon_train_scratch_bytes_latents": (_l, [_l, _i, _p]),
    "aon_train_scratch_bytes_inputs": (_l, [_l, _i, _p]),
    # NeRFMLP of any constructor geometry (aon_mlp_geometry first)
    "aon_mlp_geometry_init": (None, [_p]),
    "aon_gmlp_param_count": (_i, [_p]),
    "aon_gmlp_workspace_bytes": (_l, [_p, _l]),
    "aon_gmlp_fwd": (_i, [_p, _p, _p, _p, _l, _i, _p, _p, _p, _l, _p]),
    "aon_grender_workspace_bytes": (_l, [_p, _l, _p]),
    "aon_grender_train_workspace_bytes": (_l, [_p, _l, _i, _p]),
    "aon_grender_train_scratch_bytes": (_l, [_p, _l, _i, _p]),
    # per-ray near / far from a ray-box intersection
    "aon_ray_limits_box": (_i, [_p, _p, _l, _p, _p, _p, _p, _p]),
    "aon_ray_limits_workspace_bytes": (_l, [_l]),
    "aon_ray_limits": (_i, [_p, _p, _l, _p, _p, _p, _p, _p, _p, _l, _p]),
    "aon_sample_along_rays_bounds": (_i, [_p, _p, _l, _i, _p, _p, _i, _p, _p, _p, _p]),
}


class MlpGeometryC(C.Structure):
    """aon_mlp_geometry (include/aon_hip.h): the arguments of NeRFMLP.__init__ (model.py:40-54)."""
    _fields_ = [(n, C.c_int32) for n in ("min_deg_point", "max_deg_point", "deg_view", "netdepth", "netwidth", "netdepth_condition",
                                         "netwidth_condition", "skip_layer", "input_ch", "input_ch_view", "num_rgb_channels",
                                         "num_density_channels")]


class RenderOptsC(C.Structure):
    """aon_render_opts (include/aon_hip.h)."""
    _fields_ = [("num_coarse_samples", C.c_int32), ("num_fine_samples", C.c_int32), ("lindisp", C.c_int32),
                ("inv_near", C.c_float), ("inv_far", C.c_float), ("noise_std", C.c_float),
                ("noise_c", C.c_void_p), ("noise_f", C.c_void_p),
                ("rgb_scale", C.c_float), ("rgb_shift", C.c_float), ("sigma_bias", C.c_float),
                ("min_deg_point", C.c_int32), ("max_deg_point", C.c_int32), ("deg_view", C.c_int32)]


class OccupancyC(C.Structure):
    """aon_occupancy (include/aon_hip.h)."""
    _fields_ = [("bits", C.c_void_p), ("cells", C.c_int64 * 3), ("lo", C.c_float * 3), ("step", C.c_float * 3)]


class RayGradsC(C.Structure):
    """aon_ray_grads (include/aon_hip.h)."""
    _fields_ = [("rays_o", C.c_void_p), ("viewdirs", C.c_void_p), ("g_rays_o", C.c_void_p), ("g_rays_d", C.c_void_p), ("g_viewdirs", C.c_void_p)]


class RayBoundsC(C.Structure):
    """aon_ray_bounds (include/aon_hip.h)."""
    _fields_ = [("near_ray", C.c_void_p), ("far_ray", C.c_void_p), ("live", C.c_void_p)]


class SceneObjectC(C.Structure):
    """aon_scene_object (include/aon_hip_scene.h)."""
    _fields_ = [("rot", C.c_float * 9), ("centre", C.c_float * 3), ("lo", C.c_float * 3), ("hi", C.c_float * 3)]


def _ext_sigs():
    """include/aon_hip_inputs.h: the extension header's entry points, composed like the others.  Bound like _SIGS, but kept out of
    `exported_symbols()`, which lists include/aon_hip.h's names."""
    head, tail = _BWD
    return {"aon_render_bwd_inputs": (_i, _VANILLA * 2 + head + _PER_LEVEL + tail + _OPTS + _RAY_GRADS),   # ... parameters
            "aon_train_scratch_bytes_inputs_vanilla": (_l, [_l, _i] + _OPTS)}


_EXT_SIGS = _ext_sigs()

# include/aon_hip_scene.h: a third table, kept out of `exported_symbols()` and `extension_symbols()`
_SCENE_SIGS = {
    "aon_scene_pairs_workspace_bytes": (_l, [_l, _i]),
    # rays_o, rays_d, viewdirs, n | objects_host, k | workspace, bytes | offsets, slot, pair_ray, pair_o, pair_d, pair_v, pair_near, pair_far | stream
    "aon_scene_pairs": (_i, [_p, _p, _p, _l] + [_p, _i] + [_p, _l] + [_p] * 8 + [_p]),
    # raw, t_vals, slot, rays_d | n, k, pairs, s, white_bkgd, act | opts | rgb, acc, depth, obj_acc, weights | stream
    "aon_scene_composite": (_i, [_p] * 4 + [_l, _i, _l, _i, _i, _i] + [_p] + [_p] * 5 + [_p]),
}

# include/aon_hip_scene_occ.h: a fourth table, kept out of the three lists above
_SCENE_OCC_SIGS = {
    "aon_scene_occ_workspace_bytes": (_l, [_l, _i, _i]),
    # packed, smalls_host, grids_host, starts_host | pair_o, pair_d, pair_v, t_vals | k, s | raw, occupied_dev | workspace, bytes | stream
    "aon_scene_art_mlp_fwd_occ": (_i, [_p] * 4 + [_p] * 4 + [_i, _i] + [_p, _p] + [_p, _l] + [_p]),
}


# include/aon_hip_scene_grad.h: a fifth table, kept out of the four lists above
_SCENE_GRAD_SIGS = {
    # raw, t_vals, slot, rays_d | g_rgb, g_acc, g_depth, g_obj_acc | n, k, pairs, s, white_bkgd, act | opts | d_raw | stream
    "aon_scene_composite_bwd": (_i, [_p] * 4 + [_p] * 4 + [_l, _i, _l, _i, _i, _i] + [_p] + [_p] + [_p]),
}


# include/aon_hip_scene_pose.h: a sixth table, kept out of the five lists above
_SCENE_POSE_SIGS = {
    "aon_art_ray_grads_record_bytes": (_l, [_l, _i]),
    # dplanes, dxp, params, t_vals, viewdirs | n_rays, s, np, deg_view | records, bytes | g_rays_o, g_rays_d, g_viewdirs | stream
    "aon_art_ray_grads": (_i, [_p] * 5 + [_l, _i, _l, _i] + [_p, _l] + [_p] * 3 + [_p]),
    # rays_o, rays_d, viewdirs, n | pair_ray, offsets | objects_host, k | pairs | g_o, g_d, g_v | g_pose | stream
    "aon_scene_pose_grads": (_i, [_p, _p, _p, _l] + [_p, _p] + [_p, _i] + [_l] + [_p] * 3 + [_p] + [_p]),
}


class SceneListC(C.Structure):
    """aon_scene_list (include/aon_hip_scene_lists.h)."""
    _fields_ = [("act", C.c_int), ("rgb_scale", C.c_float), ("rgb_shift", C.c_float), ("sigma_bias", C.c_float), ("open_end", C.c_int)]


# include/aon_hip_scene_lists.h: a seventh table, kept out of the six lists above
_SCENE_LISTS_SIGS = {
    # raw, t_vals, slot, rays_d | n, k, pairs, s, white_bkgd | lists_host | rgb, acc, depth, obj_acc, weights | stream
    "aon_scene_composite_lists": (_i, [_p] * 4 + [_l, _i, _l, _i, _i] + [_p] + [_p] * 5 + [_p]),
}


# include/aon_hip_scene_lists_grad.h: an eighth table, kept out of the seven lists above
_SCENE_LISTS_GRAD_SIGS = {
    # raw, t_vals, slot, rays_d | g_rgb, g_acc, g_depth, g_obj_acc | n, k, pairs, s, white_bkgd | lists_host | d_raw | stream
    "aon_scene_composite_lists_bwd": (_i, [_p] * 4 + [_p] * 4 + [_l, _i, _l, _i, _i] + [_p] + [_p] + [_p]),
}


for _name, (_res, _args) in {**_SIGS, **_EXT_SIGS, **_SCENE_SIGS, **_SCENE_OCC_SIGS, **_SCENE_GRAD_SIGS, **_SCENE_POSE_SIGS,
                             **_SCENE_LISTS_SIGS, **_SCENE_LISTS_GRAD_SIGS}.items():
    _fn = getattr(lib, _name)  # AttributeError here = the .so does not export what the header declares
    _fn.restype = _res
    _fn.argtypes = _args

ABI_VERSION = 5
if lib.aon_abi_version() != ABI_VERSION:
    raise ImportError(f"libaon_hip.so ABI {lib.aon_abi_version()} != binding ABI {ABI_VERSION}; rebuild")


class AonError(RuntimeError):
    pass


# measurements: AON_BOTTLENECK_FOLD=0 in the environment starts the process in the literal two-layer form (aon_set_bottleneck_fold(0)),
# so every tool / test can be A/B'd without a flag of its own
if os.environ.get("AON_BOTTLENECK_FOLD", "") == "0":
    lib.aon_set_bottleneck_fold(0)


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib.aon_last_error().decode("utf-8", "replace")
        raise AonError(f"{what or 'libaon_hip'} failed (code {rc}): {msg}")


def exported_symbols():
    return sorted(_SIGS)


def extension_symbols():
    """the names include/aon_hip_inputs.h declares"""
    return sorted(_EXT_SIGS)


def scene_symbols():
    """the names include/aon_hip_scene.h declares"""
    return sorted(_SCENE_SIGS)


def scene_occ_symbols():
    """the names include/aon_hip_scene_occ.h declares"""
    return sorted(_SCENE_OCC_SIGS)


def scene_grad_symbols():
    """the names include/aon_hip_scene_grad.h declares"""
    return sorted(_SCENE_GRAD_SIGS)


def scene_pose_symbols():
    """the names include/aon_hip_scene_pose.h declares"""
    return sorted(_SCENE_POSE_SIGS)


def scene_lists_symbols():
    """the names include/aon_hip_scene_lists.h declares"""
    return sorted(_SCENE_LISTS_SIGS)


def scene_lists_grad_symbols():
    """the names include/aon_hip_scene_lists_grad.h declares"""
    return sorted(_SCENE_LISTS_GRAD_SIGS)
