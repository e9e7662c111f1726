"""Scenes with a background field, what can be checked without a GPU: the restatement tests/_scene_lists_ref.py
against _scene_ref.composite_ref (homogeneous closed lists: exactly) and against the oracle's volumetric_rendering (one open vanilla list),
the extension header include/aon_hip_scene_lists.h against the library and the binding, every refusal of the entry point -- code, message,
rank -- on fake pointers (the pattern of tests/test_scene_cpu.py), ScenePairs.with_background's layout on CPU tensors, and every Python
refusal of scene.SceneBackground / scene.render_scene(background=...) / scene.render_scene_grad."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scene_lists_ref as lref  # noqa: E402
import _scene_ref as sref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "aon_hip_scene_lists.h"


# ---- the restatement against what exists ----
def _lists(seed, P, S, lo=2.0, hi=6.0):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(lo, hi, (P, S)), -1).astype(np.float32)
    raw = rng.normal(0.0, 2.0, (P, S, 4)).astype(np.float32)
    return raw, t


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_homogeneous_closed_lists_are_the_scene_restatement_exactly(dtype):
    n, S, K = 7, 13, 3
    raw, t = _lists(31, n * K, S)
    slot = np.stack([np.arange(n) + n * k for k in range(K)], 1).astype(np.int32)
    slot[::3, 1] = -1
    slot[1, :] = -1
    dirs = np.random.default_rng(32).normal(size=(n, 3)).astype(np.float32)
    for opts in (None, {"rgb_padding": 0.01, "density_bias": 0.5}):
        for white in (True, False):
            ref = sref.composite_ref(raw, t, slot, dirs, white, opts, dtype)
            got = lref.composite_ref(raw, t, slot, dirs, white, [(lref.ACT_ARTICULATED, opts, False)] * K, dtype)
            for key in ("rgb", "acc", "depth", "obj_acc", "weights"):
                assert got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key]), (key, white)


def test_one_open_vanilla_list_is_the_oracles_volumetric_rendering():
    sys.path.insert(0, ROOT)
    from oracle import nerf_oracle as orc

    n, S = 9, 33
    raw, t = _lists(33, n, S)
    raw[0, -1, 3], raw[1, -1, 3], raw[2, -1, 3] = 0.0, 40.0, -3.0      # the far sample: exactly 0, large, negative
    dirs = np.random.default_rng(34).normal(size=(n, 3)).astype(np.float32)
    slot = np.arange(n, dtype=np.int32)[:, None]
    rgb_s, sigma = lref.activate_list(raw, lref.ACT_VANILLA, None, np.float64)
    assert np.array_equal(sigma, np.maximum(raw[..., 3].astype(np.float64), 0)) and sigma[0, -1] == 0 and sigma[2, -1] == 0
    for white in (True, False):
        got = lref.composite_ref(raw, t, slot, dirs, white, [(lref.ACT_VANILLA, None, True)], np.float64)
        ref = orc.volumetric_rendering(torch.from_numpy(rgb_s), torch.from_numpy(sigma)[..., None], torch.from_numpy(t).double(),
                                       torch.from_numpy(dirs).double(), white)
        for key, r in (("rgb", ref[0]), ("acc", ref[1]), ("weights", ref[2]), ("depth", ref[3])):
            assert np.abs(got[key] - r.numpy()).max() <= 1e-12, key
        assert np.abs(got["obj_acc"][:, 0] - got["acc"]).max() <= 1e-15
        # the open interval: a far sample with density takes everything that is left (each of the S factors 1 - alpha + 1e-10 may add 1e-10)
        assert abs(got["acc"][1] - 1.0) <= S * 1e-10


def test_an_open_list_in_front_leaves_the_formulas_transmittance_behind_it():
    """list 1 (open, dense last sample) ends at t = 4; list 0 (closed) reaches to t = 6: its samples behind get T = 1e-10 times what was left"""
    S = 5
    t = np.stack([np.linspace(2.0, 6.0, S), np.linspace(2.0, 4.0, S)]).astype(np.float32)
    raw = np.zeros((2, S, 4), np.float32)
    raw[0, :, 3] = 1.0
    raw[1, :, 3] = -5.0
    raw[1, -1, 3] = 3.0
    slot = np.array([[0, 1]], np.int32)
    dirs = np.array([[0.0, 0.0, 1.0]], np.float32)
    got = lref.composite_ref(raw, t, slot, dirs, True, [(lref.ACT_ARTICULATED, None, False), (lref.ACT_VANILLA, None, True)], np.float64)
    w = got["weights"]
    assert np.isfinite(w).all() and w[1, -1] > 0.05 and (w[0, t[0] > 4.0] <= 1e-10).all() and (w[0, t[0] > 4.0] > 0).any()
    assert abs(got["acc"][0] - 1.0) <= 2 * S * 1e-10


def test_the_whole_reference_render_with_a_backdrop_runs_on_the_oracle():
    import aon_amd.synthetic as syn

    sd = syn.make_art_state_dict(seed=0, density_scale=2.0)
    bg = syn.make_smooth_nerf_state_dict(seed=5)
    rays = {k: v.numpy() for k, v in syn.make_rays(3, 4, syn.look_at_pose(4.0, 30.0, 30.0), syn.focal_from_fovy(3, 20.0)).items()}
    objects = [(_pose(c=(0.1, 0.0, 0.0)).numpy(), 1.6)]
    latents = [{k: 0.1 * syn.seeded_uniform(70 + i, 1, w) for i, (k, w) in enumerate((("density", 128), ("color", 128), ("articulation", 32)))}]
    lv = lref.render_scene_ref(sd, objects, latents, rays, True, bg, 2.0, 6.0, num_coarse=8, num_fine=8)
    lv0 = lref.render_scene_ref(sd, [], [], rays, True, bg, 2.0, 6.0, num_coarse=8, num_fine=8)
    assert len(lv) == 2 and lv[1]["weights"].shape[1] == 17 and lv[0]["obj_acc"].shape == (12, 2) and lv0[0]["obj_acc"].shape == (12, 1)
    for a in lv + lv0:
        assert np.abs(a["obj_acc"].sum(1) - a["acc"]).max() <= 1e-12 and (a["obj_acc"][:, -1] > 0).any()
    assert np.array_equal(lv0[1]["obj_acc"][:, 0], lv0[1]["acc"])


# ---- header, library, binding ----
# hand-written: p = c_void_p, i = c_int, l = c_int64
LISTS_ARGTYPES = {
    "aon_scene_composite_lists": (C.c_int, "p p p p l i l i i p p p p p p p"),
}


def _stripped(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def lists_declared_symbols():
    return sorted(set(re.findall(r"\b(aon_[a-z_0-9]+)\s*\(", _stripped(HEADER))))


def test_lists_header_library_and_binding_agree():
    from aon_amd import _lib

    names = lists_declared_symbols()
    assert names == sorted(LISTS_ARGTYPES) == _lib.scene_lists_symbols()
    kinds = {"p": C.c_void_p, "i": C.c_int, "l": C.c_int64}
    for n in names:
        assert hasattr(_lib.lib, n), f"{n} declared in {HEADER} but not exported"
        fn = getattr(_lib.lib, n)
        res, letters = LISTS_ARGTYPES[n]
        assert fn.restype is res and list(fn.argtypes) == [kinds[k] for k in letters.split()], n
        assert list(_lib._SCENE_LISTS_SIGS[n][1]) == list(fn.argtypes), n
    # none of the other tables knows it
    others = (set(_lib.exported_symbols()) | set(_lib.extension_symbols()) | set(_lib.scene_symbols()) | set(_lib.scene_occ_symbols())
              | set(_lib.scene_grad_symbols()) | set(_lib.scene_pose_symbols()))
    assert not set(names) & others
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "aon_hip_scene.h"' in text
    assert _lib.lib.aon_abi_version() == 5 and _lib.ABI_VERSION == 5
    # the record's layout: five 4-byte fields in the header's order
    assert C.sizeof(_lib.SceneListC) == 20
    assert [f[0] for f in _lib.SceneListC._fields_] == ["act", "rgb_scale", "rgb_shift", "sigma_bias", "open_end"]
    body = re.search(r"typedef struct aon_scene_list \{(.*?)\} aon_scene_list;", _stripped(HEADER), flags=re.S).group(1)
    assert re.findall(r"\b(act|rgb_scale|rgb_shift|sigma_bias|open_end)\b", body) == ["act", "rgb_scale", "rgb_shift", "sigma_bias", "open_end"]
    # the new source and header are part of the build
    build = open(os.path.join(ROOT, "articulated-object-nerf_amd", "build.py")).read()
    assert '"aon_scene_lists.hip"' in build and '"aon_hip_scene_lists.h"' in build


# ---- the refusal table ----
BASE = 0x7C000000           # fake device pointers: non-null, 256-byte aligned, never dereferenced
INVALID = -1


def _fake(i):
    return BASE + 0x1000 * i


class ListsEntry:
    """ORDER: the argument names in the ABI's order; base: a call that would be valid; rows(): (label, overrides, rank, rc, message)"""
    WHO = "aon_scene_composite_lists"
    ORDER = ["raw", "t_vals", "slot", "rays_d", "n", "k", "pairs", "s", "white", "lists", "rgb", "acc", "depth", "obj_acc", "weights", "stream"]
    POINTERS = ["raw", "t_vals", "slot", "rays_d", "rgb", "acc", "depth"]

    def __init__(self):
        from aon_amd import _lib

        self._lib = _lib
        self.lib = _lib.lib
        a = {k: _fake(i + 20) for i, k in enumerate(self.POINTERS + ["obj_acc", "weights"])}
        a.update(n=37, k=3, pairs=50, s=65, white=1, lists=self.records(), stream=None)
        self.base = a

    def records(self, k=16, **bad):
        """16 valid records (articulated closed ..., the last vanilla open); bad: {"act": (index, value)} / {"open_end": (index, value)}"""
        arr = (self._lib.SceneListC * k)()
        for j in range(k):
            arr[j].act, arr[j].rgb_scale, arr[j].rgb_shift, arr[j].sigma_bias, arr[j].open_end = 2, 1.002, 0.001, -1.0, 0
        arr[k - 1].act, arr[k - 1].open_end = 1, 1
        for field, (j, value) in bad.items():
            setattr(arr[j], field, value)
        return arr

    def call(self, overrides):
        args = dict(self.base)
        args.update(overrides)
        rc = getattr(self.lib, self.WHO)(*[args[k] for k in self.ORDER])
        return rc, self.lib.aon_last_error().decode()

    def rows(self):
        bad, who = "bad size / list count (1 <= k <= 16, s >= 2, k * s <= 4096)", self.WHO
        rec = "bad list record (act in [0, 2], open_end 0 or 1)"
        r = [("n = -1", {"n": -1}, 1, INVALID, bad), ("pairs = -1", {"pairs": -1}, 1, INVALID, bad), ("k = 0", {"k": 0}, 1, INVALID, bad),
             ("k = 17", {"k": 17}, 1, INVALID, bad), ("s = 1", {"s": 1}, 1, INVALID, bad), ("k * s = 4097", {"k": 1, "s": 4097}, 1, INVALID, bad),
             ("k * s = 4112", {"k": 16, "s": 257}, 1, INVALID, bad)]
        r += [(k + " = NULL", {k: None}, 2, INVALID, "null pointer") for k in self.POINTERS + ["lists"]]
        r += [("act = 3 in record 0", {"lists": self.records(act=(0, 3))}, 3, INVALID, rec),
              ("act = -1 in record 2", {"lists": self.records(act=(2, -1))}, 3, INVALID, rec),
              ("open_end = 2 in record 1", {"lists": self.records(open_end=(1, 2))}, 3, INVALID, rec),
              ("open_end = -1 in record 2", {"lists": self.records(open_end=(2, -1))}, 3, INVALID, rec)]
        r += [("misaligned raw", {"raw": _fake(20) + 8}, 4, INVALID, "raw must be 16-byte aligned")]
        return [(label, o, rank, rc, f"{who}: {msg}") for label, o, rank, rc, msg in r]


def test_every_prelaunch_refusal():
    e = ListsEntry()
    rows = e.rows()
    assert len(rows) >= 20
    for label, overrides, _rank, rc, msg in rows:
        assert e.call(overrides) == (rc, msg), label
    # only the k records of the call are read: a bad record past k is nobody's
    assert e.call({"n": 0, "lists": e.records(act=(3, 7))})[0] == 0


def test_refusals_keep_their_rank():
    """Two faults at once: the refusal that ranks first is the one reported."""
    e = ListsEntry()
    pairs = 0
    for a, b in itertools.combinations(e.rows(), 2):
        if a[2] == b[2] or set(a[1]) & set(b[1]):
            continue
        first = a if a[2] < b[2] else b
        assert e.call({**a[1], **b[1]}) == (first[3], first[4]), (a[0], b[0])
        pairs += 1
    assert pairs > 50


def test_the_empty_call_succeeds():
    e = ListsEntry()
    assert e.call({"n": 0})[0] == 0
    assert e.call({"n": 0, "pairs": 0, "raw": None, "t_vals": None})[0] == 0


# ---- ScenePairs.with_background on CPU tensors ----
def _cpu_pairs(n, K, live):
    """ops.ScenePairs as aon_scene_pairs lays it out, from a (n, K) boolean table, at the capacity n * K"""
    from aon_amd import ops

    live = np.asarray(live, bool).reshape(n, K)
    slot = np.full((n, K), -1, np.int32)
    counts, ray, P = [], [], 0
    for k in range(K):
        idx = np.nonzero(live[:, k])[0]
        slot[idx, k] = P + np.arange(len(idx))
        ray += idx.tolist()
        counts.append(len(idx))
        P += len(idx)
    cap = n * K
    g = torch.Generator().manual_seed(n * 31 + K)
    pad = lambda x, *tail: torch.cat([x, torch.full((cap - P, *tail), 7.0, dtype=x.dtype)])   # noqa: E731
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64)
    arrs = [torch.rand((P, 3), generator=g) for _ in range(3)] + [torch.rand((P,), generator=g) for _ in range(2)]
    return ops.ScenePairs(n, K, offsets, counts, torch.from_numpy(slot), pad(torch.tensor(ray, dtype=torch.int32)), pad(arrs[0], 3), pad(arrs[1], 3),
                          pad(arrs[2], 3), pad(arrs[3]), pad(arrs[4]))


@pytest.mark.parametrize("per_ray", [False, True], ids=["scalar", "per_ray"])
def test_with_background_layout(per_ray):
    n, K = 5, 2
    live = [[1, 0], [0, 0], [1, 1], [0, 1], [1, 1]]
    pairs = _cpu_pairs(n, K, live)
    P = pairs.P
    assert P == 6
    o, d, v = (torch.rand(n, 3) for _ in range(3))
    near, far = (torch.linspace(0.5, 1.0, n), torch.linspace(5.0, 6.0, n)[:, None]) if per_ray else (0.5, 6)
    bg = pairs.with_background(o, d, v, near, far)
    assert (bg.n, bg.K, bg.P) == (n, K + 1, P + n)
    assert bg.counts == [3, 3, n] and bg.starts == [0, 3, 6, 11]
    assert bg.offsets.dtype == torch.int64 and bg.offsets.tolist() == [0, 3, 6, 11]
    assert bg.slot.dtype == torch.int32 and tuple(bg.slot.shape) == (n, K + 1) and bg.slot.is_contiguous()
    assert torch.equal(bg.slot[:, :K], pairs.slot) and bg.slot[:, K].tolist() == [P + r for r in range(n)]
    for k in range(K):
        assert bg.segment(k) == pairs.segment(k)
    seg = bg.segment(K)
    assert (seg.start, seg.stop) == (P, P + n)
    assert bg.ray.dtype == torch.int32 and bg.ray[seg].tolist() == list(range(n)) and torch.equal(bg.ray[:P], pairs.ray)
    for name, world in (("rays_o", o), ("rays_d", d), ("viewdirs", v)):
        got = getattr(bg, name)
        assert tuple(got.shape) == (P + n, 3) and torch.equal(got[seg], world) and torch.equal(got[:P], getattr(pairs, name))
    want_near = near if per_ray else torch.full((n,), 0.5)
    want_far = far.reshape(-1) if per_ray else torch.full((n,), 6.0)
    assert bg.near.dtype == torch.float32 and torch.equal(bg.near[seg], want_near) and torch.equal(bg.far[seg], want_far)
    assert torch.equal(bg.near[:P], pairs.near) and torch.equal(bg.far[:P], pairs.far)
    # nothing of the capacity padding (rows past P, value 7) leaks in, and the source pairs are unchanged
    assert all(tuple(x.shape)[0] == P + n for x in bg.capacity.values())
    assert pairs.K == K and tuple(pairs.slot.shape) == (n, K)


def test_with_background_without_rays_and_without_objects():
    from aon_amd import ops

    e3 = torch.empty(0, 3)
    bg = _cpu_pairs(0, 2, np.zeros((0, 2))).with_background(e3, e3, e3, 1.0, 2.0)
    assert (bg.n, bg.K, bg.P) == (0, 3, 0) and tuple(bg.slot.shape) == (0, 3) and bg.offsets.tolist() == [0, 0, 0, 0] and bg.counts == [0, 0, 0]
    # no objects: K = 0 pairs, then the backdrop is list 0
    n = 4
    none = ops.ScenePairs.without_objects(n, torch.device("cpu"))
    assert (none.n, none.K, none.P) == (n, 0, 0) and tuple(none.slot.shape) == (n, 0) and none.offsets.tolist() == [0] and none.starts == [0]
    o, d, v = (torch.rand(n, 3) for _ in range(3))
    bg = none.with_background(o, d, v, torch.full((n,), 2.0), 6.0)
    assert (bg.n, bg.K, bg.P) == (n, 1, n) and bg.slot.reshape(-1).tolist() == [0, 1, 2, 3] and bg.offsets.tolist() == [0, n]
    assert bg.segment(0) == slice(0, n) and torch.equal(bg.rays_o, o) and bg.near.tolist() == [2.0] * n and bg.far.tolist() == [6.0] * n
    # refusals of the layout itself
    with pytest.raises(ValueError, match="rays_d must be float32"):
        none.with_background(o, d[:3], v, 2.0, 6.0)
    with pytest.raises(ValueError, match="per-ray near"):
        none.with_background(o, d, v, torch.zeros(n + 1), 6.0)


def test_scene_list_record():
    from aon_amd import _lib, ops

    rec = (_lib.SceneListC * 1)()
    ops.SceneList(ops.ACT_ARTICULATED, False, ops.RenderOpts(rgb_padding=0.01, density_bias=0.5)).fill(rec[0])
    assert (rec[0].act, rec[0].open_end) == (2, 0)
    assert (rec[0].rgb_scale, rec[0].rgb_shift, rec[0].sigma_bias) == (np.float32(1.02), np.float32(0.01), np.float32(0.5))
    ops.SceneList(ops.ACT_VANILLA, True).fill(rec[0])
    assert (rec[0].act, rec[0].open_end) == (1, 1)
    with pytest.raises(ValueError, match="act must be"):
        ops.SceneList(3)


# ---- scene.SceneBackground / render_scene(background=...) / render_scene_grad ----
def _latents():
    return {"density": torch.zeros(1, 128), "color": torch.zeros(1, 128), "articulation": torch.zeros(1, 32)}


def _pose(R=None, c=(0.0, 0.0, 0.0)):
    R = torch.eye(3) if R is None else torch.as_tensor(R, dtype=torch.float32)
    return torch.cat([R, torch.tensor(c, dtype=torch.float32)[:, None]], 1)


def test_scene_background_refusals():
    from aon_amd import scene
    from aon_amd.models.vanilla_nerf.model import NeRF
    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

    ok = scene.SceneBackground(NeRF(), 2.0, 6.0)
    assert (ok.near, ok.far) == (2.0, 6.0)
    per_ray = scene.SceneBackground(NeRF(), torch.full((4, 1), 0.0), torch.full((4,), 3.0))
    assert tuple(per_ray.near.shape) == (4,) and per_ray.bounds(1, 3, 4)[1].tolist() == [3.0, 3.0]
    with pytest.raises(TypeError, match="vanilla NeRF"):
        scene.SceneBackground(NeRF_AE_Art(), 2.0, 6.0)
    with pytest.raises(NotImplementedError, match="layer-wise"):                 # engine-only geometry
        scene.SceneBackground(NeRF(max_deg_point=12), 2.0, 6.0)
    with pytest.raises(NotImplementedError, match=r"degrees \(0, 10, 4\)"):      # padded slots: the stage call encodes at the default degrees
        scene.SceneBackground(NeRF(max_deg_point=8), 2.0, 6.0)
    with pytest.raises(NotImplementedError, match="use_viewdirs"):
        scene.SceneBackground(NeRF(use_viewdirs=False), 2.0, 6.0)
    with pytest.raises(NotImplementedError, match="no density noise"):
        scene.SceneBackground(NeRF(noise_std=0.5), 2.0, 6.0)
    for near, far in ((-0.1, 6.0), (6.0, 6.0), (7.0, 6.0), (2.0, float("inf")), (float("nan"), 6.0),
                      (torch.tensor([1.0, 2.0]), torch.tensor([3.0, 2.0])), (torch.tensor([-1.0, 2.0]), 3.0)):
        with pytest.raises(ValueError, match="0 <= near < far"):
            scene.SceneBackground(NeRF(), near, far)
    with pytest.raises(ValueError, match="same number of rays"):
        scene.SceneBackground(NeRF(), torch.zeros(3), torch.ones(4))
    with pytest.raises(TypeError, match="float32"):
        scene.SceneBackground(NeRF(), torch.zeros(3, dtype=torch.float64), 4.0)


def test_render_scene_background_refusals():
    from aon_amd import scene
    from aon_amd.models.vanilla_nerf.model import NeRF
    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

    ob = scene.SceneObject(_latents(), _pose(), 2.0)
    model = NeRF_AE_Art()
    bg = scene.SceneBackground(NeRF(), 2.0, 6.0)
    rays = {k: torch.zeros(4, 3) for k in ("rays_o", "rays_d", "viewdirs")}
    with pytest.raises(RuntimeError, match="inference only: call it under torch.no_grad"):
        scene.render_scene(model, [ob], rays, True, background=bg)
    with torch.no_grad():
        with pytest.raises(TypeError, match="SceneBackground"):
            scene.render_scene(model, [ob], rays, True, background=NeRF())
        with pytest.raises(ValueError, match="0 to 15 objects.*got 16"):                     # 16 objects plus a backdrop
            scene.render_scene(model, [ob] * 16, rays, True, background=bg)
        with pytest.raises(ValueError, match="1 to 16 objects, got 0"):                      # no backdrop: as ever
            scene.render_scene(model, [], rays, True)
        with pytest.raises(ValueError, match=r"backdrop runs 1 level\(s\), the scene model 2"):
            scene.render_scene(model, [ob], rays, True, background=scene.SceneBackground(NeRF(num_levels=1), 2.0, 6.0))
        # (K + 1) * S > 4096: 15 objects and a backdrop at 64 + 1 + 256 = 321 fine samples; one object and a backdrop at 1023 + 1 + 1100
        with pytest.raises(ValueError, match=r"5136 merged samples per ray; the merged composite holds at most 4096"):
            scene.render_scene(NeRF_AE_Art(num_fine_samples=256), [ob] * 15, rays, True, background=bg)
        with pytest.raises(ValueError, match=r"level 1 are 4248 merged samples"):
            scene.render_scene(NeRF_AE_Art(num_coarse_samples=1023, num_fine_samples=1100), [ob], rays, True, background=bg)
        with pytest.raises(ValueError, match="randomized=True is refused"):
            scene.render_scene(model, [], rays, True, randomized=True, background=bg)
    # gradients through a backdrop are not built
    with pytest.raises(NotImplementedError, match="inference only"):
        scene.render_scene_grad(model, [ob], rays, True, background=bg)


def test_the_harness_method_takes_a_background():
    import inspect

    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    sig = inspect.signature(LitNeRF_AutoDecoder.render_scene)
    assert list(sig.parameters)[1:] == ["batch", "placements", "occupancy", "background"] and sig.parameters["background"].default is None
