"""GPU: occupancy grids for scenes (csrc/aon_scene_occ.hip, include/aon_hip_scene_occ.h).

Behaviour is fully defined by the sentinel yardstick of tests/_scene_occ_ref.py: the dense records of ops.scene_art_mlp_fwd with the rows
that tests/_occ_ref.py's lookup calls empty overwritten by (0, 0, 0, -inf).  Everything here is bit for bit against that, or against
scene.render_scene without grids, except where an empty object is compared with a scene that lacks it (the composite's bar on every level:
the order of the transmittance products changes with K, section 4.16).  No test measures quality: what a grid drops is section 4.9's property."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _guard  # noqa: E402
import _scene_occ_ref as oref  # noqa: E402
from test_hip_extents import Case, run_case  # noqa: E402

pytestmark = pytest.mark.gpu

FLOORS = {"rgb": 2e-6, "acc": 2e-6, "obj_acc": 2e-6, "depth": 1e-5}     # the compositing bars of tests/test_hip_scene.py / test_hip_parity.py


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from aon_amd import ops as _ops

    was = _ops.bottleneck_fold()
    yield _ops
    _ops.set_bottleneck_fold(was)


def _syn():
    import aon_amd.synthetic as syn
    return syn


# ------------------------------------------------------------------ the networks, codes and placements of tests/test_hip_scene.py, restated
_MODELS: dict = {}


def art_model(dev, levels, nc, nf):
    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

    key = (levels, nc, nf)
    if key not in _MODELS:
        m = NeRF_AE_Art(num_levels=levels, num_coarse_samples=nc, num_fine_samples=nf).to(dev)
        m.load_state_dict(_syn().make_art_state_dict(seed=0, density_scale=2.0))
        _MODELS[key] = m
    return _MODELS[key]


def codes(dev, k):
    syn = _syn()
    return {key: (0.2 * syn.seeded_uniform(60 + 3 * k + i, 1, w) - 0.1).to(dev) for i, (key, w) in enumerate((("density", 128), ("color", 128), ("articulation", 32)))}


def rotation(seed):
    from aon_amd import ops as _ops
    w = np.random.default_rng(seed).normal(size=3)
    return _ops.so3_exp(torch.tensor(w / np.linalg.norm(w) * (0.3 + 0.2 * seed % 2.5), dtype=torch.float64)).float()


def pose(seed, centre):
    return torch.cat([rotation(seed), torch.tensor(centre, dtype=torch.float32)[:, None]], 1)


CAM = _syn().look_at_pose(4.0, 30.0, 30.0)


def placements(K):
    """(pose, box side) of K <= 3 objects: a box at the origin, one off the centre, a small one between them (lists interleave)"""
    c = np.random.default_rng(300).normal(size=3)
    return [(pose(20, (0.0, 0.0, 0.0)), 2.2), (pose(31, (0.6 * c / np.linalg.norm(c)).tolist()), 1.1), (pose(5, (0.3, 0.2, -0.1)), 0.9)][:K]


def frame(dev, H=8, W=12):
    syn = _syn()
    return {k: v.to(dev) for k, v in syn.make_rays(H, W, CAM, syn.focal_from_fovy(H, 30.0)).items()}


def box_cells(kind, seed):
    """cells over [-1.2, 1.2+]^3, uneven: contains every box of placements()"""
    return oref.make_cells(kind, seed, (6, 5, 7), (-1.2,) * 3, (0.4, 0.48, 0.35))


def placed(dev, K, grids):
    from aon_amd import scene
    return [scene.SceneObject(codes(dev, k), p, b, None if g is None else g.to_ops(dev)) for k, ((p, b), g) in enumerate(zip(placements(K), grids))]


def same(a, b, what=""):
    assert a.shape == b.shape and torch.equal(_guard.bits(a), _guard.bits(b)), what


def same_levels(got, want):
    assert len(got) == len(want)
    for lv, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip(("rgb", "acc", "depth", "obj_acc"), g, w):
            same(a, b, f"level {lv}: {name}")


# ------------------------------------------------------------------ 1. the stage call on fabricated segments
#              name            S    rows per object
STAGE_CASES = [("tile_edges",   64,  (0, 1, 16, 17, 33)),                 # empty, a partial tile, exactly 1,024 samples, one past it, a boundary inside
               ("k16_s9",       9,   (40, 0, 7, 0, 0, 61, 1, 30, 0, 25, 44, 0, 19, 50, 0, 23)),      # P = 300, K = 16, six empty segments
               ("s193",         193, (11, 20, 6)),                        # P = 37: tiles that end inside a row
               ("many_tiles",   193, (11000, 3))]                         # 2,074 tiles, more than one round of the scan; then offsets restart at 0
GUARD_REACHES = ["aon_scene_occ_workspace_bytes", "aon_scene_art_mlp_fwd_occ"]


def fabricated(ops, dev, seed, S, rows):
    """-> (ScenePairs over fabricated rows, t (P, S), host copies (o, d, t), starts)"""
    K, P = len(rows), sum(rows)
    o, d, v, t = oref.fabricated_pairs(seed, P, S)
    starts = [sum(rows[:k]) for k in range(K + 1)]
    td = lambda x: torch.from_numpy(x).to(dev)      # noqa: E731
    pairs = ops.ScenePairs(P, K, torch.tensor(starts, dtype=torch.int64, device=dev), list(rows), torch.zeros((P, K), dtype=torch.int32, device=dev),
                           torch.arange(P, dtype=torch.int32, device=dev), td(o), td(d), td(v), torch.zeros(P, device=dev), torch.ones(P, device=dev))
    assert pairs.starts == starts and pairs.P == P
    return pairs, td(t), (o, d, t), starts


def rotating_grids(K, shift):
    return [oref.make_cells(oref.KINDS[(k + shift) % len(oref.KINDS)], 50 + k) for k in range(K)]


def network(ops, dev, K):
    """the coarse network of the (1, 16, 16) model packed in the CURRENT form, and one per-call block per object"""
    mlp = art_model(dev, 1, 16, 16).coarse_mlp
    params = dict(mlp.named_parameters())
    with torch.no_grad():
        return ops.pack_art_mlp(params, degrees=mlp.degrees), [ops.art_prepare(params, codes(dev, k % 5), degrees=mlp.degrees) for k in range(K)]


@pytest.mark.parametrize("fold", [True, False], ids=["folded", "literal"])
@pytest.mark.parametrize("case", STAGE_CASES, ids=[c[0] for c in STAGE_CASES])
def test_stage_is_the_sentinel_yardstick(ops, dev, case, fold):
    name, S, rows = case
    ops.set_bottleneck_fold(fold)
    K = len(rows)
    packed, smalls = network(ops, dev, K)
    pairs, t, (o, d, t_host), starts = fabricated(ops, dev, 7 + S, S, rows)
    dense = ops.scene_art_mlp_fwd(packed, smalls, pairs, t)
    for shift in range(len(oref.KINDS) if name == "tile_edges" else 2):     # every kind meets every segment size of the first case
        cells = rotating_grids(K, shift)
        grids = [None if c is None else c.to_ops(dev) for c in cells]
        raw, occupied = ops.scene_art_mlp_fwd_occ(packed, smalls, grids, pairs, t)
        want, counts, _ = oref.yardstick(dense.cpu().numpy(), starts, cells, o, d, t_host)
        print(f"{name} fold={fold} shift={shift}: occupied {occupied.tolist()} of {[r * S for r in rows]}")
        assert occupied.tolist() == counts
        assert [c for c, g in zip(counts, cells) if g is None] == [r * S for r, g in zip(rows, cells) if g is None]
        same(raw, torch.from_numpy(want), f"{name} shift {shift}")
        assert 0 < sum(counts) < sum(rows) * S
    # every grid None: the dense call's bits
    raw, occupied = ops.scene_art_mlp_fwd_occ(packed, smalls, [None] * K, pairs, t)
    same(raw, dense)
    assert occupied.tolist() == [r * S for r in rows]


def test_stage_without_pairs(ops, dev):
    ops.set_bottleneck_fold(True)
    packed, smalls = network(ops, dev, 2)
    pairs, t, _, _ = fabricated(ops, dev, 1, 16, (0, 0))
    raw, occupied = ops.scene_art_mlp_fwd_occ(packed, smalls, [oref.make_cells("full", 0).to_ops(dev), None], pairs, t)
    assert tuple(raw.shape) == (0, 16, 4) and occupied.tolist() == [0, 0]


# ------------------------------------------------------------------ 2. full grids: the frame without grids, bit for bit
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("levels,nc,nf", [(1, 16, 16), (2, 16, 16), (2, 64, 128)], ids=["one_level_16", "two_levels_16_16", "two_levels_64_128"])
def test_full_grids_are_the_frame_without_grids(ops, dev, levels, nc, nf, K):
    from aon_amd import scene

    ops.set_bottleneck_fold(True)
    model = art_model(dev, levels, nc, nf)
    rays = frame(dev)
    with torch.no_grad():
        want, dense_count = scene.render_scene(model, placed(dev, K, [None] * K), rays, True, want_occupied=True)
        full = placed(dev, K, [oref.enclosing("full", k) for k in range(K)])
        got, occupied = scene.render_scene(model, full, rays, True, chunk=40, want_occupied=True)          # 96 rays: chunks of 40, 40, 16
        whole, _ = scene.render_scene(model, full, rays, True, want_occupied=True)
    same_levels(got, want)
    same_levels(whole, want)
    assert len(occupied) == levels and float(want[-1][1].max()) > 0.05
    for a, b in zip(occupied, dense_count):
        assert a.tolist() == b.tolist() and min(a.tolist()) > 0


# ------------------------------------------------------------------ 3. empty grids
def test_empty_grids_return_the_background(ops, dev):
    from aon_amd import scene

    ops.set_bottleneck_fold(True)
    model = art_model(dev, 2, 16, 16)
    rays = frame(dev)
    for white in (True, False):
        with torch.no_grad():
            got, occupied = scene.render_scene(model, placed(dev, 3, [oref.enclosing("empty", k) for k in range(3)]), rays, white, want_occupied=True)
        for rgb, acc, depth, obj_acc in got:
            assert torch.equal(rgb, torch.full_like(rgb, 1.0 if white else 0.0))
            assert not acc.any() and not depth.any() and not obj_acc.any()
        assert all(o.tolist() == [0, 0, 0] for o in occupied)


@pytest.mark.parametrize("levels,nc,nf", [(1, 16, 16), (2, 16, 16)], ids=["one_level", "two_levels"])
def test_one_empty_object_is_the_scene_without_it(ops, dev, levels, nc, nf):
    """An object with an empty grid, the others dense, against the scene rendered without that object, on EVERY level: each of its samples
    has weight exactly 0 and factor fl(1 - 0 + 1e-10) = 1 in the transmittance product, so the first level differs only by the grouping of
    that product's multiplications, and the second by what those last-bit differences of the merged weights do to the inverse CDF's draws
    -- the composite's bar, not bits (section 4.16).  The all-sentinel segment also passes through the coarse -> fine hand-over: its rows
    have zero weights, get draws all the same, and are all sentinel again.
    Measured on an MI355X (max over the three choices of the empty object; bars 2e-6 / 2e-6 / 1e-5 / 2e-6 for rgb / acc / depth / obj_acc):
    one level 1.2e-7 / 6.0e-8 / 2.4e-7 / 3.0e-8; two levels, first level the same, second level 3.6e-7 / 7.2e-7 / 3.3e-6 / 7.2e-7."""
    from aon_amd import scene

    ops.set_bottleneck_fold(True)
    model = art_model(dev, levels, nc, nf)
    rays = frame(dev)
    for gone in (0, 1, 2):
        keep = [k for k in range(3) if k != gone]
        with_empty = placed(dev, 3, [oref.enclosing("empty", 0) if k == gone else None for k in range(3)])
        with torch.no_grad():
            got, occupied = scene.render_scene(model, with_empty, rays, True, want_occupied=True)
            want = scene.render_scene(model, [with_empty[k] for k in keep], rays, True)
        assert all(o.tolist()[gone] == 0 and min(o.tolist()[k] for k in keep) > 0 for o in occupied)
        for lv, (g, w) in enumerate(zip(got, want)):
            dist = {"rgb": float((g[0] - w[0]).abs().max()), "acc": float((g[1] - w[1]).abs().max()), "depth": float((g[2] - w[2]).abs().max()),
                    "obj_acc": float((g[3][:, keep] - w[3]).abs().max())}
            print(f"levels={levels} gone={gone} level {lv}: " + "  ".join(f"{k} {v:.2e} (bar {FLOORS[k]:.0e})" for k, v in dist.items()))
            assert not g[3][:, gone].any()
            for key, v in dist.items():
                assert v <= FLOORS[key], (gone, lv, key, v)
        assert float(want[0][1].max()) > 0.05


# ------------------------------------------------------------------ 4. the whole path with mixed grids
def written_out(ops, model, objects, rays, white):
    """scene.render_scene's flow with stage-level ops calls, every ray in one chunk"""
    pairs = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], objects)
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, model.num_coarse_samples, pairs.near, pairs.far, want_coords=False)
    levels, occupied = [], []
    for level, mlp in enumerate([model.coarse_mlp, model.fine_mlp][: model.num_levels]):
        smalls = [ops.art_prepare(dict(mlp.named_parameters()), ob.latents, degrees=mlp.degrees) for ob in objects]
        raw, occ = ops.scene_art_mlp_fwd_occ(mlp.packed(), smalls, [ob.grid for ob in objects], pairs, t)
        rgb, acc, depth, obj_acc, weights = ops.scene_composite(raw, t, pairs, rays["rays_d"], white, opts=model._opts)
        levels.append((rgb, acc, depth, obj_acc))
        occupied.append(occ)
        if level + 1 < model.num_levels:
            t = ops.sample_pdf_t_n(t, weights, model.num_fine_samples)
    return levels, occupied, pairs


@pytest.mark.parametrize("levels,nc,nf", [(1, 16, 16), (2, 16, 16), (2, 64, 128)], ids=["one_level_16", "two_levels_16_16", "two_levels_64_128"])
def test_render_scene_is_the_written_out_chain(ops, dev, levels, nc, nf):
    from aon_amd import scene

    ops.set_bottleneck_fold(True)
    model = art_model(dev, levels, nc, nf)
    objects = placed(dev, 3, [box_cells("random", 1), None, box_cells("halfspace", 2)])
    rays = frame(dev)
    with torch.no_grad():
        got, occupied = scene.render_scene(model, objects, rays, True, want_occupied=True)
        plain = scene.render_scene(model, objects, rays, True)
        want, want_occ, pairs = written_out(ops, model, objects, rays, True)
        dense = scene.render_scene(model, placed(dev, 3, [None] * 3), rays, True)
    same_levels(got, want)
    same_levels(plain, want)
    total = [c * (nc + 1) for c in pairs.counts]
    for lv, (a, b) in enumerate(zip(occupied, want_occ)):
        assert a.tolist() == b.tolist(), lv
    first = occupied[0].tolist()
    print(f"levels={levels}: occupied {[o.tolist() for o in occupied]}, first level's samples {total}")
    assert 0 < first[0] < total[0] and first[1] == total[1] and 0 < first[2] < total[2]
    assert not torch.equal(got[-1][0], dense[-1][0]) and float(got[-1][1].max()) > 0.05      # the grids removed something, and something is seen


# ------------------------------------------------------------------ 5. repeat, and a side stream
def test_repeat_and_a_frame_on_a_side_stream(ops, dev):
    from aon_amd import scene

    ops.set_bottleneck_fold(True)
    model = art_model(dev, 2, 16, 16)
    objects = placed(dev, 3, [box_cells("random", 1), None, box_cells("halfspace", 2)])
    rays = frame(dev)
    with torch.no_grad():
        serial, occ = scene.render_scene(model, objects, rays, True, want_occupied=True)
        again, occ2 = scene.render_scene(model, objects, rays, True, want_occupied=True)
        same_levels(again, serial)
        assert [o.tolist() for o in occ] == [o.tolist() for o in occ2]
        torch.cuda.synchronize()
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        busy = hasattr(torch.cuda, "_sleep")
        if busy:
            torch.cuda._sleep(int(2.4e6 * 60))          # about 60 ms of the default stream
        gate = torch.cuda.Event()
        gate.record()
        with torch.cuda.stream(side):
            got, occ3 = scene.render_scene(model, objects, rays, True, want_occupied=True)
        side.synchronize()
        pending = not gate.query()
        torch.cuda.synchronize()
    same_levels(got, serial)
    assert [o.tolist() for o in occ] == [o.tolist() for o in occ3]
    if busy:
        assert pending, "the side stream's frame waited for the default stream"


# ------------------------------------------------------------------ 6. the memory contract
GUARD_CASES: list = []


def _guard_case(name, S, rows, shift):
    K = len(rows)

    def make(dev):
        from aon_amd import ops as _ops
        _ops.set_bottleneck_fold(True)
        packed, smalls = network(_ops, dev, K)
        pairs, t, _, starts = fabricated(_ops, dev, 7 + S, S, rows)
        grids = [None if c is None else c.to_ops(dev) for c in rotating_grids(K, shift)]
        return {"packed": packed, "smalls": smalls, "grids": grids, "o": pairs.rays_o, "d": pairs.rays_d, "v": pairs.viewdirs, "t": t, "rows": list(rows)}

    def call(ops, i):
        P = sum(i["rows"])
        dev = i["t"].device
        pairs = ops.ScenePairs(P, K, None, i["rows"], None, torch.arange(P, dtype=torch.int32, device=dev), i["o"], i["d"], i["v"], i["t"][:, 0], i["t"][:, 0])
        raw, occupied = ops.scene_art_mlp_fwd_occ(i["packed"], i["smalls"], i["grids"], pairs, i["t"])
        return [raw, occupied + 1]          # (+ 1: a count of 0xFFFFFFFF... would read as "nobody wrote this")
    return Case("scene_occ", name, make, call, GUARD_REACHES)


for _name, _S, _rows in STAGE_CASES[:3]:          # (many_tiles: the same code at a size the stage test covers)
    for _shift in (0, 3):
        GUARD_CASES.append(_guard_case(f"scene_occ_{_name}_shift{_shift}", _S, _rows, _shift))


@pytest.mark.parametrize("c", GUARD_CASES, ids=[c.name for c in GUARD_CASES])
def test_memory_contract(dev, monkeypatch, c):
    """Three runs (plain, guarded with 0xFF prefill, guarded with zero prefill) of ops.scene_art_mlp_fwd_occ: raw, the workspace of exactly
    the queried size and `occupied` sit between guard bands; bit-equal outputs, no unwritten word, no band touched, inputs unchanged."""
    run_case(c, dev, monkeypatch)


@pytest.mark.parametrize("prefill", ["nan", "zero"])
def test_rows_past_the_pairs_and_list_tails_keep_their_prefill(ops, dev, prefill):
    """The C call itself, on guarded buffers of its own: rows of raw from P on, and of each object's list the entries from its count on, hold
    what they held before (they lie inside the buffers, where no band looks); the lists are the yardstick's; `occupied` is added to."""
    ops.set_bottleneck_fold(True)
    name, S, rows = STAGE_CASES[0]
    K, extra = len(rows), 3
    packed, smalls = network(ops, dev, K)
    pairs, t, (o, d, t_host), starts = fabricated(ops, dev, 7 + S, S, rows)
    P = pairs.P
    cells = rotating_grids(K, 1)
    grids = [None if c is None else c.to_ops(dev) for c in cells]
    alloc = _guard.GuardedAlloc(prefill)
    need = int(ops.lib.aon_scene_occ_workspace_bytes(P, K, S))
    raw = alloc.alloc((P + extra, S, 4), torch.float32, dev, None, "raw")
    ws = alloc.alloc((need,), torch.uint8, dev, None, "workspace")
    occupied = alloc.alloc((K,), torch.int64, dev, 5, "occupied")
    structs = [None if g is None else g.c_struct() for g in grids]
    grid_arr = (C.c_void_p * K)(*[None if st is None else C.addressof(st) for st in structs])
    small_arr = (C.c_void_p * K)(*[ops._pk(s).value for s in smalls])
    rc = ops.lib.aon_scene_art_mlp_fwd_occ(ops._pk(packed), small_arr, grid_arr, (C.c_int64 * (K + 1))(*starts), pairs.rays_o.data_ptr(),
                                           pairs.rays_d.data_ptr(), pairs.viewdirs.data_ptr(), t.data_ptr(), K, S, raw.data_ptr(), occupied.data_ptr(),
                                           ws.data_ptr(), need, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    ops.check(rc, "aon_scene_art_mlp_fwd_occ")
    alloc.check()
    fill = _guard.FILL if prefill == "nan" else 0
    assert bool((raw[P:].contiguous().view(torch.uint8) == fill).all()), "rows of raw past P were written"
    want, counts, masks = oref.yardstick(ops.scene_art_mlp_fwd(packed, smalls, pairs, t).cpu().numpy(), starts, cells, o, d, t_host)
    same(raw[:P], torch.from_numpy(want))
    assert occupied.tolist() == [5 + c for c in counts]
    lists = ws[: 4 * P * S].view(torch.int32).cpu().numpy()
    fill_word = np.int32(-1) if prefill == "nan" else np.int32(0)
    for k in range(K):
        seg = lists[starts[k] * S: starts[k + 1] * S]
        if cells[k] is None:                              # dense: the mark / emit kernels do not touch its rows
            assert (seg == fill_word).all(), k
            continue
        assert np.array_equal(seg[: counts[k]], oref.local_list(masks[k])), k
        assert (seg[counts[k]:] == fill_word).all(), k


# ------------------------------------------------------------------ 7. LitNeRF_AutoDecoder.render_scene(..., occupancy=...)
def test_lit_render_scene_with_occupancy(ops, dev, monkeypatch):
    from aon_amd import occupancy, scene
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    ops.set_bottleneck_fold(True)
    syn = _syn()
    lit = LitNeRF_AutoDecoder({"N_max_objs": 2, "chunk": 100}, randomized=False, model_kwargs=dict(num_coarse_samples=16, num_fine_samples=16)).to(dev)
    lit.model.load_state_dict(syn.make_art_state_dict(seed=0, density_scale=2.0))
    lit.code_library.load_state_dict(syn.make_code_library_state(seed=0))
    lit.eval()
    H, W = 12, 16
    batch = {k: v.to(dev) for k, v in syn.make_rays(H, W, CAM, syn.focal_from_fovy(H, 30.0)).items()}
    explicit = syn.seeded_uniform(90, 32) * 0.1
    specs = [(0, 4, pose(1, (0.0, 0.0, 0.0)), 1.4), (1, 11, pose(2, (0.4, 0.3, 0.2)), 1.0), (0, explicit, pose(3, (-0.9, 0.8, 0.0)), 0.8),
             (0, 4, pose(4, (0.5, -0.6, 0.3)), 0.9)]                      # the last one: the first one's instance and articulation again
    occ_args = dict(bounds=(-0.8, 0.8), resolution=12, threshold=0.5, dilate=0)
    built = []
    real = occupancy.build_occupancy

    def counting(*a, **kw):
        built.append(kw)
        return real(*a, **kw)
    monkeypatch.setattr(occupancy, "build_occupancy", counting)
    a = lit.render_scene(batch, specs, occupancy=occ_args)
    assert len(built) == 3 and all(kw["resolution"] == 12 and kw["bounds"] == (-0.8, 0.8) for kw in built)        # four placements, three grids
    assert tuple(a["obj_acc"].shape) == (H * W, 4) and tuple(a["occupied"].shape) == (4,)
    lit.render_scene(batch, specs, occupancy=occ_args)
    assert len(built) == 3                                                 # cached
    lit.render_scene(batch, specs, occupancy={**occ_args, "dilate": 1})
    assert len(built) == 6                                                 # other arguments: other grids
    # the explicit-grid call
    table = lit.code_library.get_interpolated_articulations(max_interpolations=2, device=dev)
    objects = []
    with torch.no_grad():
        for iid, art, p, box in specs:
            ids = torch.tensor([iid], dtype=torch.int64, device=dev)
            code = table[art: art + 1] if isinstance(art, int) else art.to(dev).reshape(1, -1)
            lat = {"density": lit.code_library.embedding_instance_shape(ids), "color": lit.code_library.embedding_instance_appearance(ids), "articulation": code}
            objects.append(scene.SceneObject(lat, p, box, real(lit.model, latents=lat, **occ_args)))
        want, occupied = scene.render_scene(lit.model, objects, {k: batch[k] for k in ("rays_o", "rays_d", "viewdirs")}, lit.white_bkgd, chunk=100,
                                            want_occupied=True)
    for key, w in zip(("rgb", "acc", "depth", "obj_acc"), want[-1]):
        same(a[key], w, key)
    assert a["occupied"].tolist() == occupied[-1].tolist()
    # a box that sticks out of the bounds is refused, not cut
    with pytest.raises(ValueError, match="does not contain the box"):
        lit.render_scene(batch, [(0, 4, pose(1, (0.0, 0.0, 0.0)), 1.7)], occupancy=occ_args)
    with pytest.raises(ValueError, match="occupancy must be None or a dict"):
        lit.render_scene(batch, specs, occupancy={"cells": 12})
    # train() / eval() and load_state_dict() drop the grids
    n = len(built)
    lit.train()
    lit.eval()
    lit.render_scene(batch, specs, occupancy=occ_args)
    assert len(built) == n + 3
    lit.load_state_dict(lit.state_dict())
    lit.render_scene(batch, specs, occupancy=occ_args)
    assert len(built) == n + 6
    # ... and so does a change of the weights through one of the sub-modules, which is how weights are usually loaded, or in place
    lit.render_scene(batch, specs, occupancy=occ_args)
    assert len(built) == n + 6
    lit.model.load_state_dict(lit.model.state_dict())
    lit.render_scene(batch, specs, occupancy=occ_args)
    assert len(built) == n + 9
    lit.code_library.load_state_dict(lit.code_library.state_dict())
    lit.render_scene(batch, specs, occupancy=occ_args)
    assert len(built) == n + 12
    with torch.no_grad():
        lit.model.fine_mlp.density_layer.bias.add_(0.0)
    lit.render_scene(batch, specs, occupancy=occ_args)
    assert len(built) == n + 15
    lit.render_scene(batch, specs, occupancy=occ_args)
    assert len(built) == n + 15
    lit.clear_scene_grids()
    lit.render_scene(batch, specs, occupancy=occ_args)
    assert len(built) == n + 18
    n += 12
    # without occupancy: no grid is built, and the dict is the one it was
    plain = lit.render_scene(batch, specs)
    assert len(built) == n + 6 and "occupied" not in plain
