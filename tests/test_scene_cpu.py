"""Scenes of several posed objects, what can be checked without a GPU: the reference composite of tests/_scene_ref.py
against the oracle's volumetric_rendering and against over-compositing, its tie rule, the extension header include/aon_hip_scene.h against
the library and the binding (the discipline tests/test_vanilla_ray_grads_cpu.py keeps for its header), every refusal of both entry points
-- code, message, rank -- on fake pointers, and the argument rules of scene.render_scene / scene.SceneObject."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scene_ref as sref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "aon_hip_scene.h"


# ---- the reference composite ----
def _lists(seed, P, S, lo=2.0, hi=6.0):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(lo, hi, (P, S)), -1).astype(np.float32)
    raw = rng.normal(0.0, 2.0, (P, S, 4)).astype(np.float32)
    return raw, t


def test_one_object_is_the_oracles_volumetric_rendering_without_the_far_plane():
    sys.path.insert(0, ROOT)
    from oracle import nerf_oracle as orc

    n, S = 9, 33
    raw, t = _lists(1, n, S)
    dirs = np.random.default_rng(2).normal(size=(n, 3)).astype(np.float32)
    slot = np.arange(n, dtype=np.int32)[:, None]
    rgb_s, sigma = sref.activate(raw, sref.DEFAULT_ACT, np.float64)
    for white in (True, False):
        got = sref.composite_ref(raw, t, slot, dirs, white, dtype=np.float64)
        ref = orc.volumetric_rendering(torch.from_numpy(rgb_s), torch.from_numpy(sigma)[..., None], torch.from_numpy(t).double(),
                                       torch.from_numpy(dirs).double(), white, far_alpha=0.0)
        for key, r in (("rgb", ref[0]), ("acc", ref[1]), ("weights", ref[2]), ("depth", ref[3])):
            assert np.abs(got[key] - r.numpy()).max() <= 1e-12, key
        assert np.abs(got["obj_acc"][:, 0] - got["acc"]).max() <= 1e-15


def test_disjoint_objects_are_over_composited():
    n, S, K = 11, 17, 3
    raws, ts = zip(*[_lists(10 + k, n, S, 2.0 + 1.5 * k, 3.0 + 1.5 * k) for k in range(K)])    # [2, 3], [3.5, 4.5], [5, 6]
    order = (2, 0, 1)                                                                          # object index != depth order
    raw, t = np.concatenate([raws[j] for j in order]), np.concatenate([ts[j] for j in order])
    slot = np.stack([np.arange(n) + n * k for k in range(K)], 1).astype(np.int32)
    slot[::4, 1] = -1                                                                          # some rays miss an object
    dirs = np.random.default_rng(3).normal(size=(n, 3)).astype(np.float32)
    for white in (True, False):
        got = sref.composite_ref(raw, t, slot, dirs, white, dtype=np.float64)
        layers = []
        for k in range(K):
            alone = sref.composite_ref(raw, t, slot[:, k:k + 1], dirs, False, dtype=np.float64)
            hit = slot[:, k] >= 0
            near = np.where(hit, t[np.maximum(slot[:, k], 0), 0], np.nan)
            layers.append((near, alone["rgb"], alone["acc"]))
            assert np.abs(alone["acc"][~hit]).max(initial=0) == 0
        rgb, acc = sref.over_composite(layers, white)
        assert np.abs(got["rgb"] - rgb).max() <= 1e-7 and np.abs(got["acc"] - acc).max() <= 1e-7


def test_identical_objects_alternate_and_the_first_wins():
    n, S = 6, 12
    raw, t = _lists(20, n, S)
    raw, t = np.concatenate([raw, raw]), np.concatenate([t, t])
    slot = np.stack([np.arange(n), np.arange(n) + n], 1).astype(np.int32)
    dirs = np.ones((n, 3), np.float32)
    for r in range(n):
        order = [(k, i) for _, k, i, _ in sref.merge_order(t, slot[r])]
        assert order == [(k, i) for i in range(S) for k in (0, 1)]
    got = sref.composite_ref(raw, t, slot, dirs, True, dtype=np.float64)
    seen = got["acc"] > 0
    assert seen.any() and (got["obj_acc"][seen, 0] > got["obj_acc"][seen, 1]).all()
    assert np.abs(got["obj_acc"].sum(1) - got["acc"]).max() <= 1e-12


def test_the_whole_reference_render_runs_on_the_oracle():
    """render_scene_ref: two overlapping objects, two levels, fp64 against fp32 -- the parts add up and the two precisions agree"""
    import aon_amd.synthetic as syn

    sd = syn.make_art_state_dict(seed=0, density_scale=2.0)
    rays = {k: v.numpy() for k, v in syn.make_rays(3, 4, syn.look_at_pose(4.0, 30.0, 30.0), syn.focal_from_fovy(3, 20.0)).items()}
    objects = [(_pose(c=(0.1, 0.0, 0.0)).numpy(), 1.6), (_pose(c=(-0.2, 0.3, 0.1)).numpy(), 1.2)]
    latents = [{k: 0.1 * syn.seeded_uniform(70 + 3 * j + i, 1, w) for i, (k, w) in enumerate((("density", 128), ("color", 128), ("articulation", 32)))}
               for j in range(2)]
    lv64 = sref.render_scene_ref(sd, objects, latents, rays, True, num_coarse=8, num_fine=8, dtype=np.float64)
    lv32 = sref.render_scene_ref(sd, objects, latents, rays, True, num_coarse=8, num_fine=8, dtype=np.float32)
    assert len(lv64) == 2 and lv64[0]["weights"].shape[1] == 9 and lv64[1]["weights"].shape[1] == 17
    for a, b in zip(lv64, lv32):
        assert a["rgb"].shape == (12, 3) and a["obj_acc"].shape == (12, 2) and (a["acc"] > 0).any()
        assert np.abs(a["obj_acc"].sum(1) - a["acc"]).max() <= 1e-12
        assert np.abs(a["rgb"] - b["rgb"]).max() <= 1e-3 and np.abs(a["acc"] - b["acc"]).max() <= 1e-3


# ---- header, library, binding ----
# hand-written: p = c_void_p, i = c_int, l = c_int64
SCENE_ARGTYPES = {
    "aon_scene_pairs_workspace_bytes": (C.c_int64, "l i"),
    "aon_scene_pairs": (C.c_int, "p p p l p i p l p p p p p p p p p"),
    "aon_scene_composite": (C.c_int, "p p p p l i l i i i p p p p p p p"),
}


def _stripped(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def scene_declared_symbols():
    return sorted(set(re.findall(r"\b(aon_[a-z_0-9]+)\s*\(", _stripped(HEADER))))


def scene_stream_entry_points():
    return sorted({m.group(1) for m in re.finditer(r"\b(aon_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", _stripped(HEADER), flags=re.S)
                   if re.search(r"\bstream\b", m.group(2))})


def test_scene_header_library_and_binding_agree():
    from aon_amd import _lib
    from test_abi_cpu import declared_symbols
    from test_vanilla_ray_grads_cpu import ext_declared_symbols

    names = scene_declared_symbols()
    assert names == sorted(SCENE_ARGTYPES) == _lib.scene_symbols()
    kinds = {"p": C.c_void_p, "i": C.c_int, "l": C.c_int64}
    for n in names:
        assert hasattr(_lib.lib, n), f"{n} declared in {HEADER} but not exported"
        fn = getattr(_lib.lib, n)
        res, letters = SCENE_ARGTYPES[n]
        assert fn.restype is res and list(fn.argtypes) == [kinds[k] for k in letters.split()], n
        assert list(_lib._SCENE_SIGS[n][1]) == list(fn.argtypes), n
    # neither of the other headers nor their tables know them
    others = set(declared_symbols()) | set(ext_declared_symbols()) | set(_lib.exported_symbols()) | set(_lib.extension_symbols())
    assert not set(names) & others
    assert '#include "aon_hip.h"' in open(os.path.join(ROOT, "include", HEADER)).read()
    assert _lib.lib.aon_abi_version() == 5 and _lib.ABI_VERSION == 5
    # the record's layout: 18 floats, rot first
    assert C.sizeof(_lib.SceneObjectC) == 72 and [f[0] for f in _lib.SceneObjectC._fields_] == ["rot", "centre", "lo", "hi"]


def test_every_stream_entry_point_of_the_scene_header_is_in_a_guard_case():
    import test_hip_scene as gpu

    names = scene_stream_entry_points()
    assert names == ["aon_scene_composite", "aon_scene_pairs"]
    reached = set().union(*(set(c.reaches) for c in gpu.GUARD_CASES))
    assert not set(names) - reached
    assert {c.name for c in gpu.GUARD_CASES} >= {f"scene_n{n}_k{k}" for n in (1, 5, 37) for k in (1, 3)} | {"scene_no_pair", "scene_k16_s256"}


# ---- the refusal tables ----
BASE = 0x7C000000           # fake device pointers: non-null, 256-byte aligned, never dereferenced
INVALID, WORKSPACE = -1, -2


def _fake(i):
    return BASE + 0x1000 * i


class _Entry:
    """ORDER: the argument names in the ABI's order; base: a call that would be valid; rows(): (label, overrides, rank, rc, message)"""

    def call(self, overrides):
        args = dict(self.base)
        args.update(overrides)
        rc = getattr(self.lib, self.WHO)(*[args[k] for k in self.ORDER])
        return rc, self.lib.aon_last_error().decode()


class PairsEntry(_Entry):
    WHO = "aon_scene_pairs"
    ORDER = ["rays_o", "rays_d", "viewdirs", "n", "objects", "k", "ws", "ws_bytes", "offsets", "slot", "pair_ray", "pair_o", "pair_d", "pair_v",
             "pair_near", "pair_far", "stream"]
    POINTERS = ["rays_o", "rays_d", "viewdirs", "objects", "ws", "offsets", "slot", "pair_ray", "pair_o", "pair_d", "pair_v", "pair_near", "pair_far"]

    def __init__(self):
        from aon_amd import _lib

        self.lib = _lib.lib
        self.objects = (_lib.SceneObjectC * 3)()
        a = {k: _fake(i + 1) for i, k in enumerate(self.POINTERS)}
        a.update(objects=self.objects, n=37, k=3, stream=None, ws_bytes=self.lib.aon_scene_pairs_workspace_bytes(37, 3))
        assert a["ws_bytes"] > 0
        self.base = a

    def rows(self):
        bad, who = "bad size / object count", self.WHO
        r = [("n = -1", {"n": -1}, 1, INVALID, bad), ("k = 0", {"k": 0}, 1, INVALID, bad), ("k = 17", {"k": 17}, 1, INVALID, bad),
             ("n * k = 2^31", {"n": 2 ** 31}, 1, INVALID, bad)]
        r += [(k + " = NULL", {k: None}, 2, INVALID, "null pointer") for k in self.POINTERS]
        r += [("misaligned workspace", {"ws": _fake(5) + 128}, 3, INVALID, "workspace must be 256-byte aligned"),
              ("workspace one byte short", {"ws_bytes": self.base["ws_bytes"] - 1}, 4, WORKSPACE, "workspace smaller than aon_scene_pairs_workspace_bytes()")]
        return [(label, o, rank, rc, f"{who}: {msg}") for label, o, rank, rc, msg in r]


class CompositeEntry(_Entry):
    WHO = "aon_scene_composite"
    ORDER = ["raw", "t_vals", "slot", "rays_d", "n", "k", "pairs", "s", "white", "act", "opts", "rgb", "acc", "depth", "obj_acc", "weights", "stream"]
    POINTERS = ["raw", "t_vals", "slot", "rays_d", "rgb", "acc", "depth"]

    def __init__(self):
        from aon_amd import _lib

        self.lib = _lib.lib
        a = {k: _fake(i + 20) for i, k in enumerate(self.POINTERS + ["obj_acc", "weights"])}
        a.update(n=37, k=3, pairs=50, s=65, white=1, act=2, opts=None, stream=None)
        self.base = a

    def rows(self):
        bad, who = "bad size / object count / act (1 <= k <= 16, s >= 2, k * s <= 4096)", self.WHO
        r = [("n = -1", {"n": -1}, 1, INVALID, bad), ("pairs = -1", {"pairs": -1}, 1, INVALID, bad), ("k = 0", {"k": 0}, 1, INVALID, bad),
             ("k = 17", {"k": 17}, 1, INVALID, bad), ("s = 1", {"s": 1}, 1, INVALID, bad), ("k * s = 4097", {"k": 1, "s": 4097}, 1, INVALID, bad),
             ("k * s = 4112", {"k": 16, "s": 257}, 1, INVALID, bad), ("act = 3", {"act": 3}, 1, INVALID, bad)]
        r += [(k + " = NULL", {k: None}, 2, INVALID, "null pointer") for k in self.POINTERS]
        r += [("misaligned raw", {"raw": _fake(20) + 8}, 3, INVALID, "raw must be 16-byte aligned")]
        return [(label, o, rank, rc, f"{who}: {msg}") for label, o, rank, rc, msg in r]


@pytest.mark.parametrize("entry", [PairsEntry, CompositeEntry], ids=["pairs", "composite"])
def test_every_prelaunch_refusal(entry):
    e = entry()
    rows = e.rows()
    assert len(rows) >= 16
    for label, overrides, _rank, rc, msg in rows:
        assert e.call(overrides) == (rc, msg), label


@pytest.mark.parametrize("entry", [PairsEntry, CompositeEntry], ids=["pairs", "composite"])
def test_refusals_keep_their_rank(entry):
    """Two faults at once: the refusal that ranks first is the one reported."""
    e = entry()
    pairs = 0
    for a, b in itertools.combinations(e.rows(), 2):
        if a[2] == b[2] or set(a[1]) & set(b[1]):
            continue
        first = a if a[2] < b[2] else b
        assert e.call({**a[1], **b[1]}) == (first[3], first[4]), (a[0], b[0])
        pairs += 1
    assert pairs > 50


def test_empty_calls_succeed_and_the_workspace_query():
    from aon_amd import _lib

    lib = _lib.lib
    # composite with n = 0: nothing to write; with pairs = 0 raw / t_vals may be NULL (the launch itself is the GPU test's)
    e = CompositeEntry()
    assert e.call({"n": 0}) == (0, e.lib.aon_last_error().decode())
    # mask (4 B per ray) + one count per (object, block of 256 rays), 256-byte aligned pieces
    assert lib.aon_scene_pairs_workspace_bytes(37, 3) == 256 + 256
    assert lib.aon_scene_pairs_workspace_bytes(65536, 16) == 65536 * 4 + 256 * 16 * 4
    assert lib.aon_scene_pairs_workspace_bytes(0, 1) == 512
    assert lib.aon_scene_pairs_workspace_bytes(5, 17) == 0 and lib.aon_scene_pairs_workspace_bytes(-1, 1) == 0


# ---- scene.SceneObject / scene.render_scene ----
def _latents():
    return {"density": torch.zeros(1, 128), "color": torch.zeros(1, 128), "articulation": torch.zeros(1, 32)}


def _pose(R=None, c=(0.0, 0.0, 0.0)):
    R = torch.eye(3) if R is None else torch.as_tensor(R, dtype=torch.float32)
    return torch.cat([R, torch.tensor(c, dtype=torch.float32)[:, None]], 1)


def test_scene_argument_errors():
    from aon_amd import scene
    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

    ok = scene.SceneObject(_latents(), _pose(), 2.0)
    assert tuple(ok.pose.shape) == (3, 4)
    with pytest.raises(ValueError, match="not orthonormal"):
        scene.SceneObject(_latents(), _pose(1.01 * torch.eye(3)), 2.0)                       # a scale
    with pytest.raises(ValueError, match="not orthonormal"):
        scene.SceneObject(_latents(), _pose([[1, 0.1, 0], [0, 1, 0], [0, 0, 1]]), 2.0)      # a shear
    with pytest.raises(ValueError, match="reflection"):
        scene.SceneObject(_latents(), _pose(torch.diag(torch.tensor([1.0, 1.0, -1.0]))), 2.0)
    with pytest.raises(ValueError, match=r"\(3, 4\)"):
        scene.SceneObject(_latents(), torch.eye(4), 2.0)
    with pytest.raises(ValueError, match="keys"):
        scene.SceneObject({"density": torch.zeros(1, 128)}, _pose(), 2.0)
    with pytest.raises(ValueError, match="32 values"):
        scene.SceneObject({**_latents(), "articulation": torch.zeros(1, 31)}, _pose(), 2.0)
    # a rotation about z by 30 degrees, rounded to fp32, passes
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    scene.SceneObject(_latents(), _pose([[c, -s, 0], [s, c, 0], [0, 0, 1]]), ((-1, -1, -0.5), (1, 1, 0.5)))

    model = NeRF_AE_Art()
    rays = {k: torch.zeros(4, 3) for k in ("rays_o", "rays_d", "viewdirs")}
    with pytest.raises(RuntimeError, match="inference only: call it under torch.no_grad"):
        scene.render_scene(model, [ok], rays, True)
    with torch.no_grad():
        with pytest.raises(ValueError, match="randomized=True is refused"):
            scene.render_scene(model, [ok], rays, True, randomized=True)
        with pytest.raises(ValueError, match="1 to 16 objects, got 0"):
            scene.render_scene(model, [], rays, True)
        with pytest.raises(ValueError, match="1 to 16 objects, got 17"):
            scene.render_scene(model, [ok] * 17, rays, True)
        with pytest.raises(TypeError, match="SceneObject"):
            scene.render_scene(model, [(_pose(), 2.0)], rays, True)
        with pytest.raises(NotImplementedError, match="no density noise"):
            scene.render_scene(NeRF_AE_Art(noise_std=0.5), [ok], rays, True)
