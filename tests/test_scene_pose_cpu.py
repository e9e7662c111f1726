"""Pose gradients of scenes, what can be checked without a GPU: the torch restatement tests/_scene_pose_ref.py against
central differences in fp64 at fixed t, the closed forms of g_R and g_c against autograd of the torch object rays, the extension header
include/aon_hip_scene_pose.h against the library and the binding, every refusal of the three entry points -- code, message, rank -- on fake
pointers, SceneObject's handling of a pose tensor and the argument rules of LitNeRF_AutoDecoder.fit_scene_poses."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scene_pose_ref as pref  # noqa: E402
import _scene_ref as sref  # noqa: E402
from test_scene_cpu import INVALID, WORKSPACE, _Entry, _fake, _latents, _pose  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "aon_hip_scene_pose.h"
DEG = (0, 3, 2)


# ---- the torch restatement ----
def _rotation(seed, angle):
    from aon_amd import ops
    w = np.random.default_rng(seed).normal(size=3)
    return ops.so3_exp(torch.tensor(w / np.linalg.norm(w) * angle, dtype=torch.float64)).float()


def small_scene(S=5):
    """4 x 6 rays of a camera at radius 4, two nested boxes turned their own ways, S evenly spaced t per pair (data), a low-frequency field
    (degrees (0, 3, 2), density bias lowered by 2: the smooth field of tests/test_hip_ray_grads.py's fit)"""
    import aon_amd.synthetic as syn

    rays = {k: v.numpy() for k, v in syn.make_rays(4, 6, syn.look_at_pose(4.0, 30.0, 30.0), syn.focal_from_fovy(4, 18.0)).items()}
    poses = [torch.cat([_rotation(1, 0.4), torch.tensor([[0.05], [-0.1], [0.0]])], 1), torch.cat([_rotation(2, 0.7), torch.tensor([[-0.1], [0.05], [0.1]])], 1)]
    boxes = [1.6, 1.1]
    pr = sref.pairs_ref(rays["rays_o"], rays["rays_d"], rays["viewdirs"], [(p.numpy(), b) for p, b in zip(poses, boxes)])
    P = len(pr["ray"])
    t = (pr["near"][:, None] + (pr["far"] - pr["near"])[:, None] * np.linspace(0.0, 1.0, S, dtype=np.float32)[None, :]).astype(np.float32)
    sd = syn.make_art_state_dict(seed=2, density_scale=30.0, min_deg_point=DEG[0], max_deg_point=DEG[1], deg_view=DEG[2])
    sd["coarse_mlp.density_layer.bias"] = sd["coarse_mlp.density_layer.bias"] - 2.0
    sd = {k: v.double() for k, v in sd.items() if k.startswith("coarse_mlp.")}
    gen = torch.Generator().manual_seed(4)
    lat = [{k: (0.2 * torch.rand(1, w, generator=gen, dtype=torch.float64) - 0.1) for k, w in (("density", 128), ("color", 128), ("articulation", 32))}
           for _ in range(2)]
    w = {"rgb": torch.rand(24, 3, generator=gen, dtype=torch.float64), "acc": torch.rand(24, generator=gen, dtype=torch.float64),
         "depth": torch.rand(24, generator=gen, dtype=torch.float64), "obj_acc": torch.rand(24, 2, generator=gen, dtype=torch.float64)}
    assert P > 0 and pr["offsets"][1] > 0 and pr["offsets"][2] > pr["offsets"][1]

    def loss(pose_list, round32):
        po, pd, pv = pref.pair_rays(pose_list, rays, pr["ray"], pr["offsets"], round32)
        out = pref.scene_level_oracle_t(sd, "coarse_mlp.", po, pd, pv, pr["offsets"], pr["slot"], t, lat, rays["rays_d"], True, torch.float64, DEG,
                                        round32=round32)
        return sum((out[k] * w[k]).sum() for k in w)
    return poses, loss, pr, rays


def test_the_restatements_pose_gradient_is_the_central_difference():
    """the bar of tests/test_scene_grad_cpu.py's own central differences: h = 1e-6, |autograd - difference| <= 1e-6 max|autograd|"""
    poses, loss, _, _ = small_scene()
    leaves = [p.double().clone().requires_grad_(True) for p in poses]
    got = torch.autograd.grad(loss(leaves, False), leaves)
    got = np.stack([g.numpy() for g in got])
    # the kernel's function (s = fl32(o - c), delta and raw + bias rounded in fp32) runs the same graph on inputs 1e-7 apart
    leaves = [p.double().clone().requires_grad_(True) for p in poses]
    k32 = np.stack([g.numpy() for g in torch.autograd.grad(loss(leaves, True), leaves)])
    assert np.abs(k32 - got).max() <= 1e-5 * np.abs(got).max()
    h, fd = 1e-6, np.zeros_like(got)
    base = [p.double() for p in poses]
    with torch.no_grad():
        for k, i, j in np.ndindex(2, 3, 4):
            up, dn = [p.clone() for p in base], [p.clone() for p in base]
            up[k][i, j] += h
            dn[k][i, j] -= h
            fd[k, i, j] = (float(loss(up, False)) - float(loss(dn, False))) / (2 * h)
    fig = np.abs(got - fd).max() / np.abs(got).max()
    print(f"max|g| = {np.abs(got).max():.3e}, |autograd - central difference| / max|g| = {fig:.2e}")
    assert np.abs(got).max() > 1e-2 and np.abs(got[0]).max() > 1e-3 and np.abs(got[1]).max() > 1e-3
    assert fig <= 1e-6, fig


def test_the_closed_forms_are_autograd_of_the_object_rays():
    """g_R[i][a] = sum_p (fl(o_i - c_i) g_o'[a] + d_i g_d'[a] + v_i g_v'[a]),  g_c[i] = - sum_a R[i][a] sum_p g_o'[a]: to fp64 rounding"""
    poses, _, pr, rays = small_scene()
    rng = np.random.default_rng(6)
    P = len(pr["ray"])
    g = [rng.normal(size=(P, 3)).astype(np.float32) for _ in range(3)]
    leaves = [p.double().clone().requires_grad_(True) for p in poses]
    po, pd, pv = pref.pair_rays(leaves, rays, pr["ray"], pr["offsets"], True)
    # the restated rays are the forward's own, to fp32 rounding
    assert np.abs(po.detach().numpy() - pr["o"]).max() <= 2e-6 and np.abs(pd.detach().numpy() - pr["d"]).max() <= 1e-6
    total = sum((x * torch.from_numpy(gx.astype(np.float64))).sum() for x, gx in zip((po, pd, pv), g))
    auto = torch.autograd.grad(total, leaves)
    for k in range(2):
        a, b = int(pr["offsets"][k]), int(pr["offsets"][k + 1])
        idx = pr["ray"][a:b]
        g_R, g_c, scale = pref.pose_grads_closed(poses[k].numpy(), rays["rays_o"][idx], rays["rays_d"][idx], rays["viewdirs"][idx], g[0][a:b], g[1][a:b], g[2][a:b])
        closed = np.concatenate([g_R, g_c[:, None]], 1)
        assert np.abs(closed).max() > 0.1
        assert np.abs(closed - auto[k].numpy()).max() <= 1e-13 * scale.max(), k


# ---- header, library, binding ----
POSE_ARGTYPES = {"aon_art_ray_grads_record_bytes": (C.c_int64, "l i"),
                 "aon_art_ray_grads": (C.c_int, "p p p p p l i l i p l p p p p"),
                 "aon_scene_pose_grads": (C.c_int, "p p p l p p p i l p p p p p")}


def _stripped(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def pose_declared_symbols():
    return sorted(set(re.findall(r"\b(aon_[a-z_0-9]+)\s*\(", _stripped(HEADER))))


def test_scene_pose_header_library_and_binding_agree():
    from aon_amd import _lib
    from test_abi_cpu import declared_symbols
    from test_scene_cpu import scene_declared_symbols
    from test_scene_grad_cpu import grad_declared_symbols
    from test_vanilla_ray_grads_cpu import ext_declared_symbols

    names = pose_declared_symbols()
    assert names == sorted(POSE_ARGTYPES) == _lib.scene_pose_symbols()
    kinds = {"p": C.c_void_p, "i": C.c_int, "l": C.c_int64}
    for n in names:
        assert hasattr(_lib.lib, n), f"{n} declared in {HEADER} but not exported"
        fn = getattr(_lib.lib, n)
        res, letters = POSE_ARGTYPES[n]
        assert fn.restype is res and list(fn.argtypes) == [kinds[k] for k in letters.split()], n
        assert list(_lib._SCENE_POSE_SIGS[n][1]) == list(fn.argtypes), n
    others = (set(declared_symbols()) | set(ext_declared_symbols()) | set(scene_declared_symbols()) | set(grad_declared_symbols())
              | set(_lib.exported_symbols()) | set(_lib.extension_symbols()) | set(_lib.scene_symbols()) | set(_lib.scene_occ_symbols())
              | set(_lib.scene_grad_symbols()))
    occ = set(re.findall(r"\b(aon_[a-z_0-9]+)\s*\(", _stripped("aon_hip_scene_occ.h")))
    assert not set(names) & (others | occ)
    assert '#include "aon_hip_scene_grad.h"' in open(os.path.join(ROOT, "include", HEADER)).read()
    assert _lib.lib.aon_abi_version() == 5 and _lib.ABI_VERSION == 5
    import importlib.util
    spec = importlib.util.spec_from_file_location("_aon_build_py", os.path.join(ROOT, "articulated-object-nerf_amd", "build.py"))
    aon_build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(aon_build)
    assert any(h.endswith(os.path.join("include", HEADER)) for h in aon_build.HEADERS)


def test_record_bytes():
    from aon_amd import _lib
    f = _lib.lib.aon_art_ray_grads_record_bytes
    assert f(0, 1) == 0 and f(9, 65) == 9 * 65 * 128 and f(1, 2 ** 31 - 1) == (2 ** 31 - 1) * 128
    assert f(-1, 3) == -1 and f(3, 0) == -1 and f(2, 2 ** 30) == -1


# ---- the refusal tables ----
class RayGradsEntry(_Entry):
    WHO = "aon_art_ray_grads"
    ORDER = ["dplanes", "dxp", "params", "t_vals", "viewdirs", "n", "s", "np", "deg_view", "records", "record_bytes", "g_o", "g_d", "g_v", "stream"]
    POINTERS = ["dplanes", "dxp", "params", "t_vals", "viewdirs", "records", "g_o", "g_d", "g_v"]

    def __init__(self):
        from aon_amd import _lib

        self.lib = _lib.lib
        a = {k: _fake(i + 60) for i, k in enumerate(self.POINTERS)}
        self.params = (C.c_void_p * 40)(*[_fake(80 + i) for i in range(40)])
        a.update(params=self.params, n=9, s=65, np=640, deg_view=4, record_bytes=9 * 65 * 128, stream=None)
        self.base = a

    def _params_without(self, j):
        arr = (C.c_void_p * 40)(*[None if i == j else _fake(80 + i) for i in range(40)])
        self.keep = getattr(self, "keep", []) + [arr]
        return arr

    def rows(self):
        bad, who = "bad size / view degree (s >= 1, 0 <= deg_view <= 4, n_rays * s <= 2^31 - 1)", self.WHO
        r = [("n = -1", {"n": -1}, 1, INVALID, bad), ("s = 0", {"s": 0}, 1, INVALID, bad), ("np = -1", {"np": -1}, 1, INVALID, bad),
             ("deg_view = 5", {"deg_view": 5}, 1, INVALID, bad), ("deg_view = -1", {"deg_view": -1}, 1, INVALID, bad),
             ("n * s = 2^31", {"n": 2 ** 16, "s": 2 ** 15}, 1, INVALID, bad)]
        r += [(k + " = NULL", {k: None}, 2, INVALID, "null pointer") for k in self.POINTERS]
        r += [("params[0] = NULL", {"params": self._params_without(0)}, 2, INVALID, "null pointer"),
              ("params[26] = NULL", {"params": self._params_without(26)}, 2, INVALID, "null pointer"),
              ("n * s > np", {"np": 9 * 65 - 1}, 3, INVALID, "n_rays * s exceeds the planes' np samples"),
              ("records one byte short", {"record_bytes": 9 * 65 * 128 - 1}, 4, WORKSPACE, "record scratch too small"),
              ("misaligned dplanes", {"dplanes": _fake(60) + 8}, 5, INVALID, "dplanes must be 16-byte aligned"),
              ("misaligned dxp", {"dxp": _fake(61) + 4}, 6, INVALID, "dxp must be 16-byte aligned"),
              ("misaligned records", {"records": _fake(65) + 8}, 7, INVALID, "records must be 16-byte aligned")]
        return [(label, o, rank, rc, f"{who}: {msg}") for label, o, rank, rc, msg in r]


class PoseGradsEntry(_Entry):
    WHO = "aon_scene_pose_grads"
    ORDER = ["rays_o", "rays_d", "viewdirs", "n", "pair_ray", "offsets", "objects", "k", "pairs", "g_o", "g_d", "g_v", "g_pose", "stream"]
    POINTERS = ["rays_o", "rays_d", "viewdirs", "pair_ray", "offsets", "objects", "g_o", "g_d", "g_v", "g_pose"]

    def __init__(self):
        from aon_amd import _lib

        self.lib = _lib.lib
        self.objects = (_lib.SceneObjectC * 3)()
        a = {k: _fake(i + 130) for i, k in enumerate(self.POINTERS)}
        a.update(objects=self.objects, n=37, k=3, pairs=50, stream=None)
        self.base = a

    def rows(self):
        bad, who = "bad size / object count (1 <= k <= 16)", self.WHO
        r = [("n = -1", {"n": -1}, 1, INVALID, bad), ("pairs = -1", {"pairs": -1}, 1, INVALID, bad), ("k = 0", {"k": 0}, 1, INVALID, bad),
             ("k = 17", {"k": 17}, 1, INVALID, bad)]
        r += [(k + " = NULL", {k: None}, 2, INVALID, "null pointer") for k in self.POINTERS]
        return [(label, o, rank, rc, f"{who}: {msg}") for label, o, rank, rc, msg in r]


@pytest.mark.parametrize("entry", [RayGradsEntry, PoseGradsEntry], ids=["art_ray_grads", "scene_pose_grads"])
def test_every_prelaunch_refusal(entry):
    e = entry()
    rows = e.rows()
    assert len(rows) >= 14
    for label, overrides, _rank, rc, msg in rows:
        assert e.call(overrides) == (rc, msg), label


@pytest.mark.parametrize("entry,least", [(RayGradsEntry, 100), (PoseGradsEntry, 30)], ids=["art_ray_grads", "scene_pose_grads"])
def test_the_refusals_keep_their_rank(entry, least):
    e = entry()
    pairs = 0
    for a, b in itertools.combinations(e.rows(), 2):
        if a[2] == b[2] or set(a[1]) & set(b[1]):
            continue
        first = a if a[2] < b[2] else b
        assert e.call({**a[1], **b[1]}) == (first[3], first[4]), (a[0], b[0])
        pairs += 1
    assert pairs > least


def test_an_empty_ray_grads_call_succeeds_without_a_launch():
    e = RayGradsEntry()
    assert e.call({"n": 0})[0] == 0
    assert e.call({"n": 0, **{k: None for k in e.POINTERS}})[0] == 0        # whatever the pointers
    assert e.call({"n": 0, "s": 0})[0] == INVALID                         # the sizes are still checked


# ---- SceneObject, fit_scene_poses ----
def test_scene_object_keeps_a_pose_that_carries_history():
    from aon_amd import ops, scene

    plain = scene.SceneObject(_latents(), _pose(), 2.0)
    assert plain.pose_tensor is None and tuple(plain.pose.shape) == (3, 4)
    leaf = _pose(c=(0.1, 0.2, 0.3)).requires_grad_(True)
    ob = scene.SceneObject(_latents(), leaf, 2.0)
    assert ob.pose_tensor is leaf
    # ob.pose is what it is today: the detached fp32 host copy check_pose returns
    assert not ob.pose.requires_grad and ob.pose.device.type == "cpu" and ob.pose.dtype == torch.float32 and torch.equal(ob.pose, leaf.detach())
    assert ob.pose.data_ptr() != leaf.data_ptr() or not ob.pose.requires_grad
    corr = torch.zeros(6, requires_grad=True)
    derived = ops.apply_pose_correction(_pose(), corr)
    ob2 = scene.SceneObject(_latents(), derived, 2.0)
    assert ob2.pose_tensor is derived and ob2.pose_tensor.grad_fn is not None and not ob2.pose.requires_grad
    assert scene.SceneObject(_latents(), _pose().double().requires_grad_(True), 2.0).pose.dtype == torch.float32
    assert scene.SceneObject(_latents(), _pose().tolist(), 2.0).pose_tensor is None
    with pytest.raises(ValueError, match="not orthonormal"):                # a grad-carrying pose is still validated
        scene.SceneObject(_latents(), _pose(1.01 * torch.eye(3)).requires_grad_(True), 2.0)


def test_fit_scene_poses_argument_errors():
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    lit = LitNeRF_AutoDecoder({"N_max_objs": 2}, randomized=False)
    batch = {k: torch.zeros(4, 3) for k in ("rays_o", "rays_d", "viewdirs", "target")}
    good = [(0, 4, _pose(), 1.4)]
    flags = [p.requires_grad for p in lit.model.parameters()]
    with pytest.raises(ValueError, match="fit_scene_poses: steps must be a positive int"):
        lit.fit_scene_poses([batch], good, 0, 1e-2)
    with pytest.raises(ValueError, match="fit_scene_poses: no batches"):
        lit.fit_scene_poses([], good, 3, 1e-2)
    with pytest.raises(ValueError, match="lr must be positive"):
        lit.fit_scene_poses([batch], good, 3, 0.0)
    with pytest.raises(ValueError, match="lr must be positive"):
        lit.fit_scene_poses([batch], good, 3, (1e-2, 1e-2, 1e-2))
    with pytest.raises(ValueError, match="1 to 16 objects, got 0"):
        lit.fit_scene_poses([batch], [], 3, 1e-2)
    with pytest.raises(ValueError, match="fit_scene_poses: placement 0: instance_id 5 outside the library"):
        lit.fit_scene_poses([batch], [(5, 0, _pose(), 1.0)], 3, 1e-2)
    with pytest.raises(ValueError, match="fit_scene_poses: placement 0: articulation row 19 outside"):
        lit.fit_scene_poses([batch], [(0, 19, _pose(), 1.0)], 3, 1e-2)
    with pytest.raises(ValueError, match="fit_scene_poses: placement 0 must be"):
        lit.fit_scene_poses([batch], [(0, 1, _pose())], 3, 1e-2)
    with pytest.raises(ValueError, match="not orthonormal"):
        lit.fit_scene_poses([batch], [(0, 1, _pose(1.01 * torch.eye(3)), 1.0)], 3, 1e-2)
    with pytest.raises(ValueError, match="every batch needs"):
        lit.fit_scene_poses([{k: v for k, v in batch.items() if k != "target"}], good, 3, 1e-2)
    assert [p.requires_grad for p in lit.model.parameters()] == flags
