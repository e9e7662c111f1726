"""GPU: scenes of several posed articulated objects in one frame (csrc/aon_scene.hip, include/aon_hip_scene.h).

Pairs: bit-equal to the composition of existing pieces -- the torch elementwise restatement of R^T (o - c), ops.ray_limits_box on those tensors
followed by the clamp-and-live rule, and tests/_scene_ref.py's numpy pairs -- on every ray.
Composite: the HIP kernel against tests/_scene_ref.composite_ref in fp64 on the same raw and t, every ray, per output within
max(floor, 3 x max|composite_ref fp32 - composite_ref fp64|); the floors are the compositing bars of tests/test_hip_parity.py.
Bits: repeat, permuted rays, sub-batch, an object no ray hits; a permuted object list moves obj_acc's columns and stays within the bar.
Whole path: scene.render_scene against the same chain written out with stage-level ops calls (bit for bit), against over-compositing for
disjoint objects, against the oracle's volumetric_rendering(far_alpha=0) for one object, and LitNeRF_AutoDecoder.render_scene.
Contracts: guard bands (tests/_guard.py through test_hip_extents.run_case) and a side stream."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _guard  # noqa: E402
import _scene_ref as sref  # noqa: E402
from test_hip_extents import Case, run_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

FLOORS = {"rgb": 2e-6, "acc": 2e-6, "obj_acc": 2e-6, "weights": 1e-6, "depth": 1e-5}     # tests/test_hip_parity.py's compositing bars


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _syn():
    import aon_amd.synthetic as syn
    return syn


# ------------------------------------------------------------------ scenes
def rotation(seed):
    """a seeded rotation, orthonormal to fp32 rounding"""
    from aon_amd import ops
    w = np.random.default_rng(seed).normal(size=3)
    return ops.so3_exp(torch.tensor(w / np.linalg.norm(w) * (0.3 + 0.2 * seed % 2.5), dtype=torch.float64)).float()


def pose(seed, centre):
    R = torch.eye(3) if seed is None else rotation(seed)
    return torch.cat([R, torch.tensor(centre, dtype=torch.float32)[:, None]], 1)


CAM = _syn().look_at_pose(4.0, 30.0, 30.0)
EYE = CAM[:, 3].tolist()


def frame_rays(n, H=15, W=20):
    """n rays spread over an H x W frame of a camera at radius 4 looking at the origin (past H * W: the frame, then rays from random origins)"""
    syn = _syn()
    fr = syn.make_rays(H, W, CAM, syn.focal_from_fovy(H, 18.0))
    if n > H * W:
        extra = syn.random_rays(n - H * W, seed=3)
        fr = {k: torch.cat([fr[k], extra[k]]) for k in fr}
    idx = torch.arange(n) * (H * W) // n if n <= H * W else torch.arange(n)       # spread over the frame
    return {k: v[idx].contiguous() for k, v in fr.items()}


def mixed_rays(n, seed=5, away=6):
    """half frame rays, half rays from random origins on the radius-4 sphere; every `away`-th ray looks away from the scene, so it meets no
    box it is not inside of"""
    a, b = frame_rays(n - n // 2), _syn().random_rays(n // 2, seed=seed)
    rays = {k: torch.cat([a[k], b[k]]) if n // 2 else a[k] for k in a}
    for k in ("rays_d", "viewdirs"):
        rays[k][away - 1::away] = -rays[k][away - 1::away]
    return rays


ORIGIN_BOX = (pose(1, (0.05, -0.1, 0.0)), 1.2)
CAMERA_INSIDE = (pose(2, EYE), 1.0)                                                    # the camera sits inside this box: near clamps to 0
BEHIND = (pose(3, [1.8 * x for x in EYE]), 1.0)                                        # wholly behind the frame's camera: near = far = 0, dead
NOT_HIT = (pose(4, (60.0, 0.0, 0.0)), ((-0.2, -0.3, -0.1), (0.3, 0.2, 0.4)))          # no ray meets it


def filler(k):
    """objects 4..15 of the largest scene: seeded placements near the origin with anisotropic boxes"""
    rng = np.random.default_rng(100 + k)
    c = rng.uniform(-0.8, 0.8, 3)
    half = rng.uniform(0.15, 0.6, 3)
    return pose(10 + k, c.tolist()), ((-half).tolist(), half.tolist())


def scene_objects(K):
    base = {1: [ORIGIN_BOX], 2: [ORIGIN_BOX, CAMERA_INSIDE], 3: [CAMERA_INSIDE, BEHIND, ORIGIN_BOX]}
    if K in base:
        return base[K]
    return [CAMERA_INSIDE, BEHIND, ORIGIN_BOX, NOT_HIT] + [filler(k) for k in range(4, K)]


def to_dev(rays, dev):
    return {k: v.to(dev) for k, v in rays.items()}


def np_pairs(rays, objects):
    return sref.pairs_ref(rays["rays_o"].numpy(), rays["rays_d"].numpy(), rays["viewdirs"].numpy(), [(p.numpy(), b) for p, b in objects])


# ------------------------------------------------------------------ pairs
def _restated(x, R, c=None):
    """R^T (x - c) by torch elementwise fp32 operations in the stated order"""
    if c is not None:
        x = torch.stack([x[:, a] - c[a] for a in range(3)], 1)
    return torch.stack([(R[0][a] * x[:, 0] + R[1][a] * x[:, 1]) + R[2][a] * x[:, 2] for a in range(3)], 1)


def check_pairs(dev, rays_cpu, objects):
    from aon_amd import ops

    rays = to_dev(rays_cpu, dev)
    n, K = rays["rays_o"].shape[0], len(objects)
    got = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], objects)
    ref = np_pairs(rays_cpu, objects)
    assert got.offsets.cpu().tolist() == ref["offsets"].tolist() and got.P == int(ref["offsets"][K]) and got.counts == np.diff(ref["offsets"]).tolist()
    assert np.array_equal(got.slot.cpu().numpy(), ref["slot"]) and np.array_equal(got.ray.cpu().numpy(), ref["ray"])
    for key, t in (("o", got.rays_o), ("d", got.rays_d), ("v", got.viewdirs), ("near", got.near), ("far", got.far)):
        assert torch.equal(_guard.bits(t), _guard.bits(torch.from_numpy(ref[key]))), key
    # ... and the composition of existing pieces, on every ray
    for k, (p, box) in enumerate(objects):
        R, c = p[:, :3].tolist(), p[:, 3].tolist()
        oo, od, ov = _restated(rays["rays_o"], R, c), _restated(rays["rays_d"], R), _restated(rays["viewdirs"], R)
        near, far = (x.reshape(-1) for x in ops.ray_limits_box(oo, od, box))
        valid = far > near
        near, far = torch.where(near < 0, torch.zeros_like(near), near), torch.where(far < 0, torch.zeros_like(far), far)
        live = valid & (far > near)
        seg = got.segment(k)
        assert torch.equal(got.ray[seg].long(), live.nonzero().reshape(-1))
        assert torch.equal((got.slot[:, k] >= 0), live)
        for mine, theirs in ((got.rays_o, oo), (got.rays_d, od), (got.viewdirs, ov), (got.near, near), (got.far, far)):
            assert torch.equal(_guard.bits(mine[seg]), _guard.bits(theirs[live]))
    return got, ref


@pytest.mark.parametrize("K", [1, 2, 3, 16])
@pytest.mark.parametrize("n", [1, 5, 37, 300])
def test_pairs_bit_equal(dev, n, K):
    rays = mixed_rays(n) if n > 1 else frame_rays(1)
    got, ref = check_pairs(dev, rays, scene_objects(K))
    print(f"n={n} K={K}: P={got.P}, counts={got.counts}")
    if K >= 2 and n >= 5:
        cam = scene_objects(K)[0 if K > 2 else 1]
        assert cam is CAMERA_INSIDE and (got.near[got.segment(0 if K > 2 else 1)] == 0).any()          # a camera inside a box
    if K >= 3:
        assert got.counts[1] < n - n // 2                                                              # the box behind the frame camera
    if K == 16:
        assert got.counts[3] == 0                                                                      # the object no ray hits


def test_pairs_more_than_one_block_and_no_pair(dev):
    # 700 rays: three blocks of 256, the last one partial
    got, _ = check_pairs(dev, mixed_rays(700), scene_objects(16))
    assert got.P > 700
    got, _ = check_pairs(dev, frame_rays(37), [BEHIND, NOT_HIT])
    assert got.P == 0 and got.counts == [0, 0] and bool((got.slot == -1).all())


# ------------------------------------------------------------------ composite
def nested(k, j):
    return pose(20 + k, (0.0, 0.0, 0.0)), 2.2 - 0.25 * j          # same centre, shrinking: lists interleave


def disjoint(k, j):
    c = np.random.default_rng(300 + j).normal(size=3)
    return pose(30 + k, (0.6 * c / np.linalg.norm(c)).tolist()), 1.1         # off the centre: a good share of the rays miss them


def layout_objects(K):
    """object k by k % 3: nested / disjoint / an identical duplicate of the object before it"""
    out = []
    for k in range(K):
        out.append(out[-1] if k % 3 == 2 else (nested if k % 3 == 0 else disjoint)(k, k // 3))
    return out


def seeded_raw(seed, n, K, S):
    """(n, K, S, 4) raw records named by (world ray, object, sample): what a pair reads does not depend on which rows exist"""
    rng = np.random.default_rng(seed)
    raw = rng.normal(0.0, 2.0, (n, K, S, 4)).astype(np.float32)
    raw[..., 3] = raw[..., 3] * 1.5 + 2.0
    return torch.from_numpy(raw)


def gather_raw(raw_full, pairs, objects_index=None):
    k_of = torch.repeat_interleave(torch.arange(pairs.K, device=raw_full.device), torch.tensor(pairs.counts, device=raw_full.device))
    if objects_index is not None:
        k_of = torch.tensor(objects_index, device=raw_full.device)[k_of]
    return raw_full[pairs.ray.long(), k_of].contiguous()


def run_chain(dev, rays_cpu, objects, raw_full, S, white, t_from_pdf=False, raw_index=None, want_weights=True):
    """pairs -> HIP sampler -> seeded raw -> HIP composite; -> (pairs, t, raw, outputs dict on the host)"""
    from aon_amd import ops

    rays = to_dev(rays_cpu, dev)
    pairs = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], objects)
    if t_from_pdf:       # S = Sc + (S - Sc) through the inverse CDF of seeded weights
        Sc = S // 2 + 1
        tc, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, Sc - 1, pairs.near, pairs.far, want_coords=False)
        w = _syn().seeded_uniform(77, rays_cpu["rays_o"].shape[0] * len(objects), Sc)[: pairs.P].to(dev)
        t = ops.sample_pdf_t_n(tc, w.contiguous(), S - Sc)
    else:
        t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, S - 1, pairs.near, pairs.far, want_coords=False)
    raw = gather_raw(raw_full.to(dev), pairs, raw_index)
    rgb, acc, depth, obj_acc, weights = ops.scene_composite(raw, t, pairs, rays["rays_d"], white, want_weights=want_weights)
    torch.cuda.synchronize()
    out = {"rgb": rgb.cpu(), "acc": acc.cpu(), "depth": depth.cpu(), "obj_acc": obj_acc.cpu()}
    if want_weights:
        out["weights"] = weights.cpu()
    return pairs, t, raw, out


def bars_and_distances(out, raw, t, pairs, rays_cpu, white):
    """-> {output: (distance of HIP from fp64, bar, distance of the serial fp32 restatement from fp64)}"""
    args = (raw.cpu().numpy(), t.cpu().numpy(), pairs.slot.cpu().numpy(), rays_cpu["rays_d"].numpy(), white)
    r64, r32 = sref.composite_ref(*args, dtype=np.float64), sref.composite_ref(*args, dtype=np.float32)
    res = {}
    for key in out:
        own = float(np.abs(r32[key].astype(np.float64) - r64[key]).max(initial=0.0))
        res[key] = (float(np.abs(out[key].numpy().astype(np.float64) - r64[key]).max(initial=0.0)), max(FLOORS[key], 3 * own), own)
    return res, r64


def full_weights(weights, pairs, n, K, S):
    """(P, S) in the pairs' layout -> (n, K, S) named by (ray, object), zero where there is no pair"""
    out = torch.zeros(n, K, S)
    slot = pairs.slot.cpu().long()
    r, k = (slot >= 0).nonzero(as_tuple=True)
    out[r, k] = weights[slot[r, k]]
    return out


# `away`: every away-th ray looks away from the scene, chosen per case (with tests/_scene_ref.pairs_ref, on the CPU) so that about a third of
# the n * K pairs are dead -- between the rays that look away and the rays that miss a box -- and some ray has no pair at all
#            name           n   K   S    away  objects
COMPOSITE = [("one",        37, 1,  65,  3,    lambda: [nested(0, 2)]),
             ("three",      37, 3,  65,  6,    lambda: layout_objects(3)),
             ("s3",         5,  2,  3,   3,    lambda: layout_objects(2)),
             ("s9_pdf",     5,  2,  9,   3,    lambda: layout_objects(2)),
             ("k16",        20, 16, 193, 5,    lambda: layout_objects(16)),
             ("k16_s256",   7,  16, 256, 4,    lambda: layout_objects(16)),
             ("merged_64",  9,  2,  32,  3,    lambda: [nested(0, 0), nested(3, 1)]),
             ("merged_65",  9,  5,  13,  4,    lambda: [nested(3 * j, j) for j in range(5)])]


@pytest.mark.parametrize("white", [True, False], ids=["white", "black"])
@pytest.mark.parametrize("case", COMPOSITE, ids=[c[0] for c in COMPOSITE])
def test_composite_against_fp64(dev, case, white):
    name, n, K, S, away, make = case
    objects = make()
    rays_cpu = mixed_rays(n, seed=7, away=away)
    pairs, t, raw, out = run_chain(dev, rays_cpu, objects, seeded_raw(40 + K + S, n, K, S), S, white, t_from_pdf=name == "s9_pdf")
    live_lists = (pairs.slot >= 0).sum(1).cpu()
    dead = 1 - pairs.P / (n * K)
    print(f"{name} white={white}: P={pairs.P} of {n * K} ({dead:.2f} dead), live lists per ray {sorted(set(live_lists.tolist()))}")
    if name == "merged_64":
        assert (live_lists * S == 64).any()
    if name == "merged_65":
        assert (live_lists * S == 65).any()
    if name == "k16_s256":
        assert K * S == 4096
    assert 0.25 <= dead <= 0.42 and (live_lists == 0).any(), (dead, live_lists)            # about a third of the pairs dead, rays with no pair
    res, r64 = bars_and_distances(out, raw, t, pairs, rays_cpu, white)
    for key, (dist, bar, own) in res.items():
        print(f"  {key:8s} HIP - fp64 {dist:.2e}   bar {bar:.2e}   (serial fp32 - fp64 {own:.2e})")
    for key, (dist, bar, _) in res.items():
        assert dist <= bar, (name, key, dist, bar)
    # rays without a pair return the background exactly, and the parts add up
    none = live_lists == 0
    assert torch.equal(out["rgb"][none], torch.full((int(none.sum()), 3), 1.0 if white else 0.0))
    assert not out["acc"][none].any() and not out["depth"][none].any() and not out["obj_acc"][none].any()
    assert float((out["obj_acc"].sum(1) - out["acc"]).abs().max()) <= 2e-6


def test_composite_ties_and_nullable_outputs(dev):
    """identical duplicates: every key ties with its twin, object 0's sample goes first and takes the larger share; weights / obj_acc NULL"""
    from aon_amd import ops

    n, S = 9, 17
    ob = nested(0, 1)
    rays_cpu = frame_rays(n)
    raw_full = seeded_raw(9, n, 1, S).expand(n, 2, S, 4).contiguous()
    pairs, t, raw, out = run_chain(dev, rays_cpu, [ob, ob], raw_full, S, True)
    assert pairs.counts == [n, n] and torch.equal(t[:n], t[n:])
    seen = out["acc"] > 0
    assert seen.any() and bool((out["obj_acc"][seen, 0] > out["obj_acc"][seen, 1]).all())
    res, _ = bars_and_distances(out, raw, t, pairs, rays_cpu, True)
    assert all(dist <= bar for dist, bar, _ in res.values()), res
    rays = to_dev(rays_cpu, dev)
    st, _keep = ops.DEFAULT_OPTS.c_struct(1.0, 1.0)
    import ctypes as C
    rgb, acc, depth = torch.empty(n, 3, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
    ops.check(ops.lib.aon_scene_composite(raw.data_ptr(), t.data_ptr(), pairs.slot.data_ptr(), rays["rays_d"].data_ptr(), n, 2, pairs.P, S, 1, 2, C.byref(st),
                                          rgb.data_ptr(), acc.data_ptr(), depth.data_ptr(), None, None, None), "aon_scene_composite")
    torch.cuda.synchronize()
    assert torch.equal(rgb.cpu(), out["rgb"]) and torch.equal(acc.cpu(), out["acc"]) and torch.equal(depth.cpu(), out["depth"])


# ------------------------------------------------------------------ bits
BITS = dict(n=37, K=3, S=65)


def _bits_run(dev, rays_cpu, objects, raw_full, raw_index=None):
    pairs, t, raw, out = run_chain(dev, rays_cpu, objects, raw_full, BITS["S"], True, raw_index=raw_index)
    n = rays_cpu["rays_o"].shape[0]
    out["weights"] = full_weights(out["weights"], pairs, n, len(objects), BITS["S"])
    return out, (pairs, t, raw)


def _same(a, b, keys=("rgb", "acc", "depth", "obj_acc", "weights"), index=None):
    for key in keys:
        x = a[key] if index is None else a[key][index]
        assert torch.equal(_guard.bits(x), _guard.bits(b[key])), key


def test_bits_do_not_depend_on_the_call(dev):
    n, K = BITS["n"], BITS["K"]
    objects, rays_cpu, raw_full = layout_objects(K), mixed_rays(n, seed=7), seeded_raw(5, n, K + 1, BITS["S"])
    base, (pairs, t, raw) = _bits_run(dev, rays_cpu, objects, raw_full)
    assert 0 < pairs.P < n * K
    again, _ = _bits_run(dev, rays_cpu, objects, raw_full)
    _same(base, again)                                                                          # repeat
    perm = torch.from_numpy(np.random.default_rng(1).permutation(n))
    permuted, _ = _bits_run(dev, {k: v[perm] for k, v in rays_cpu.items()}, objects, raw_full[perm])
    _same(base, permuted, index=perm)                                                           # permuted rays
    sub, _ = _bits_run(dev, {k: v[5:20].contiguous() for k, v in rays_cpu.items()}, objects, raw_full[5:20])
    _same(base, sub, index=slice(5, 20))                                                        # sub-batch
    for where in (K, 0, 1):                                                                     # an object no ray hits, at any position
        idx = list(range(K))
        idx.insert(where, K)
        more, (p2, _, _) = _bits_run(dev, rays_cpu, [NOT_HIT if i == K else objects[i] for i in idx], raw_full, raw_index=idx)
        assert p2.counts[where] == 0
        keep = [j for j, i in enumerate(idx) if i != K]
        _same(base, {**more, "obj_acc": more["obj_acc"][:, keep], "weights": more["weights"][:, keep]})
        assert not more["obj_acc"][:, where].any()
    # the object list permuted: obj_acc's columns move and everything stays within the bar -- each of the two results against the fp64
    # reference of ITS OWN problem, and the two against one another (the order of the sums changes, nothing else).  On a scene without exact
    # duplicates: where two samples tie in t, which goes first is decided by the object index, and with different raw values in the two
    # that is a different -- equally valid -- image, not rounding.
    objects = [nested(0, 0), disjoint(1, 0), nested(3, 1)]
    order = [2, 0, 1]
    runs = {}
    for tag, obs, index in (("base", objects, None), ("moved", [objects[i] for i in order], order)):
        pairs, t, raw, out = run_chain(dev, rays_cpu, obs, raw_full, BITS["S"], True, raw_index=index)
        res, _ = bars_and_distances(out, raw, t, pairs, rays_cpu, True)
        for key, (dist, bar, _) in res.items():
            assert dist <= bar, (tag, key, dist, bar)
        out["weights"] = full_weights(out["weights"], pairs, n, K, BITS["S"])
        runs[tag] = (out, {key: bar for key, (_, bar, _) in res.items()})
    (base, bars), (moved, _) = runs["base"], runs["moved"]
    for key in ("rgb", "acc", "depth"):
        assert float((moved[key] - base[key]).abs().max()) <= bars[key], key
    assert float((moved["obj_acc"] - base["obj_acc"][:, order]).abs().max()) <= bars["obj_acc"]
    assert float((moved["weights"] - base["weights"][:, order]).abs().max()) <= bars["weights"]
    assert float(base["obj_acc"].max()) > 0.05 and not torch.equal(base["obj_acc"], base["obj_acc"][:, order])      # the columns did move


# ------------------------------------------------------------------ whole path
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


def placed(dev, objects):
    from aon_amd import scene
    return [scene.SceneObject(codes(dev, k), p, b) for k, (p, b) in enumerate(objects)]


def written_out(model, objects, rays, white):
    """scene.render_scene's flow with stage-level ops calls, every ray in one chunk -> (levels, (pairs, t, raw) of the first level)"""
    from aon_amd import ops

    pairs = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], objects)
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, model.num_coarse_samples, pairs.near, pairs.far, want_coords=False)
    levels, first = [], None
    for level, mlp in enumerate([model.coarse_mlp, model.fine_mlp][: model.num_levels]):
        raw = torch.empty((pairs.P, t.shape[1], 4), device=t.device)
        for k, ob in enumerate(objects):
            seg = pairs.segment(k)
            if seg.stop > seg.start:
                small = ops.art_prepare(dict(mlp.named_parameters()), ob.latents, degrees=mlp.degrees)
                ops.art_mlp_fwd(mlp.packed(), small, pairs.rays_o[seg], pairs.rays_d[seg], pairs.viewdirs[seg], t[seg], out=raw[seg])
        rgb, acc, depth, obj_acc, weights = ops.scene_composite(raw, t, pairs, rays["rays_d"], white, opts=model._opts)
        levels.append((rgb, acc, depth, obj_acc))
        first = first or (pairs, t, raw)
        if level + 1 < model.num_levels:
            t = ops.sample_pdf_t_n(t, weights, model.num_fine_samples)
    return levels, first


@pytest.mark.parametrize("levels,nc,nf", [(1, 16, 16), (2, 16, 16), (2, 64, 128)], ids=["one_level_16", "two_levels_16_16", "two_levels_64_128"])
def test_render_scene_is_the_written_out_chain(dev, levels, nc, nf):
    from aon_amd import scene

    model = art_model(dev, levels, nc, nf)
    objects = placed(dev, [nested(0, 0), disjoint(1, 0), (pose(5, (0.3, 0.2, -0.1)), 0.9)])
    syn = _syn()
    rays = to_dev(syn.make_rays(8, 12, CAM, syn.focal_from_fovy(8, 30.0)), dev)
    with torch.no_grad():
        got = scene.render_scene(model, objects, rays, True, chunk=40)           # 96 rays: chunks of 40, 40, 16
        want, (pairs, _, _) = written_out(model, objects, rays, True)
    assert len(got) == len(want) == levels and 0 < pairs.P < 96 * 3
    for g, w in zip(got, want):
        assert [tuple(x.shape) for x in g] == [(96, 3), (96,), (96,), (96, 3)]
        for a, b in zip(g, w):
            assert torch.equal(_guard.bits(a), _guard.bits(b))
    assert float(got[-1][1].max()) > 0.05          # something is seen


def test_render_scene_against_the_oracle_whole_path(dev):
    """scene.render_scene, both levels, against tests/_scene_ref.render_scene_ref: the oracle's network, samplers and inverse CDF around the
    reference pairs and composite, in fp64.  The yardstick is the one the training tests use for quantities whose reference arithmetic is
    itself uncertain in fp32 (tests/_gradcheck.py): per output the relative L2 distance to the fp64 render is at most 5 x that of the SAME
    reference run in fp32 (floor 1e-4) -- the network's fp32 sums and, at the fine level, draws that land next to a knot move both alike."""
    from _gradcheck import assert_as_close_as_fp32
    from aon_amd import scene

    syn = _syn()
    model = art_model(dev, 2, 16, 16)
    specs = [nested(0, 0), disjoint(1, 0), (pose(5, (0.3, 0.2, -0.1)), 0.9)]
    objects = placed(dev, specs)
    rays_cpu = syn.make_rays(8, 12, CAM, syn.focal_from_fovy(8, 30.0))
    with torch.no_grad():
        got = scene.render_scene(model, objects, to_dev(rays_cpu, dev), True)
    args = (syn.make_art_state_dict(seed=0, density_scale=2.0), [(p.numpy(), b) for p, b in specs],
            [{k: v.cpu() for k, v in ob.latents.items()} for ob in objects], {k: v.numpy() for k, v in rays_cpu.items()}, True)
    r64 = sref.render_scene_ref(*args, num_coarse=16, num_fine=16, dtype=np.float64)
    r32 = sref.render_scene_ref(*args, num_coarse=16, num_fine=16, dtype=np.float32)
    names = ("rgb", "acc", "depth", "obj_acc")
    for level in range(2):
        assert float(r64[level]["acc"].max()) > 0.05
        assert_as_close_as_fp32({k: got[level][i].cpu() for i, k in enumerate(names)}, {k: torch.from_numpy(r64[level][k]) for k in names},
                                {k: torch.from_numpy(r32[level][k]) for k in names}, f"scene, level {level}")


def test_render_scene_without_rays(dev):
    from aon_amd import scene

    model = art_model(dev, 2, 16, 16)
    rays = {k: torch.empty(0, 3, device=dev) for k in ("rays_o", "rays_d", "viewdirs")}
    with torch.no_grad():
        out = scene.render_scene(model, placed(dev, [nested(0, 0), disjoint(1, 0)]), rays, True)
    assert len(out) == 2 and [tuple(x.shape) for x in out[1]] == [(0, 3), (0,), (0,), (0, 2)]


def test_disjoint_objects_are_the_over_composite_of_single_renders(dev):
    from aon_amd import scene

    model = art_model(dev, 1, 64, 128)
    specs = [(pose(7, (0.0, 0.0, 0.0)), 0.8), (pose(8, (1.2, 1.2, 1.0)), 0.7), (pose(9, (-1.3, -1.2, -1.1)), 0.7)]    # along the view axis
    objects = placed(dev, specs)
    syn = _syn()
    rays_cpu = syn.make_rays(8, 12, CAM, syn.focal_from_fovy(8, 30.0))
    rays = to_dev(rays_cpu, dev)
    layers = []
    with torch.no_grad():
        (rgb, acc, depth, obj_acc), = scene.render_scene(model, objects, rays, True)
        _, (pairs, t, raw) = written_out(model, objects, rays, True)
        for k, ob in enumerate(objects):
            (r1, a1, _, _), = scene.render_scene(model, [ob], rays, False)
            slot = pairs.slot[:, k].cpu()
            near = torch.where(slot >= 0, pairs.near.cpu()[slot.clamp(min=0).long()], torch.full((96,), float("nan")))
            layers.append((near.numpy().astype(np.float64), r1.cpu().numpy(), a1.cpu().numpy()))
    # disjoint along every ray: each later list starts behind the end of the one before
    order = np.argsort(np.where(np.isnan(np.stack([l[0] for l in layers], 1)), np.inf, np.stack([l[0] for l in layers], 1)), 1)
    far = np.stack([np.where(pairs.slot[:, k].cpu().numpy() >= 0, pairs.far.cpu().numpy()[np.maximum(pairs.slot[:, k].cpu().numpy(), 0)], np.nan) for k in range(3)], 1)
    nears = np.stack([l[0] for l in layers], 1)
    for r in range(96):
        hit = [k for k in order[r] if not np.isnan(nears[r, k])]
        assert all(far[r, a] < nears[r, b] for a, b in zip(hit, hit[1:])), r
    assert int((~np.isnan(nears)).sum(1).max()) >= 2
    want_rgb, want_acc = sref.over_composite(layers, True)
    out = {"rgb": rgb.cpu(), "acc": acc.cpu()}
    res, _ = bars_and_distances(out, raw, t, pairs, rays_cpu, True)
    d_rgb, d_acc = float(np.abs(out["rgb"].numpy() - want_rgb).max()), float(np.abs(out["acc"].numpy() - want_acc).max())
    print(f"scene - over-composite: rgb {d_rgb:.2e} (bar {res['rgb'][1]:.2e}), acc {d_acc:.2e} (bar {res['acc'][1]:.2e})")
    assert d_rgb <= res["rgb"][1] and d_acc <= res["acc"][1]


def test_one_object_is_the_oracles_rendering_of_the_same_raw(dev):
    from aon_amd import ops, scene
    sys.path.insert(0, ROOT)
    from oracle import nerf_oracle as orc

    model = art_model(dev, 1, 64, 128)
    ob, = placed(dev, [(pose(6, (0.0, 0.0, 0.0)), 3.0)])          # the whole frame crosses this box
    syn = _syn()
    rays_cpu = syn.make_rays(8, 12, CAM, syn.focal_from_fovy(8, 30.0))
    rays = to_dev(rays_cpu, dev)
    with torch.no_grad():
        (rgb, acc, depth, obj_acc), = scene.render_scene(model, [ob], rays, True)
        pairs = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], [ob])
        assert pairs.P == 96 and torch.equal(pairs.ray.cpu(), torch.arange(96, dtype=torch.int32))
        t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, 64, pairs.near, pairs.far, want_coords=False)
        mlp = model.coarse_mlp
        raw = ops.art_mlp_fwd(mlp.packed(), ops.art_prepare(dict(mlp.named_parameters()), ob.latents), pairs.rays_o, pairs.rays_d, pairs.viewdirs, t)
    r = raw.cpu().double()
    c = torch.sigmoid(r[..., :3]) * float(np.float32(1.002)) - float(np.float32(0.001))
    sigma = torch.nn.functional.softplus(r[..., 3:] + (-1.0))
    want = orc.volumetric_rendering(c, sigma, t.cpu().double(), rays_cpu["rays_d"].double(), True, far_alpha=0.0)
    out = {"rgb": rgb.cpu(), "acc": acc.cpu(), "depth": depth.cpu()}
    res, _ = bars_and_distances(out, raw, t, pairs, rays_cpu, True)
    for key, w in (("rgb", want[0]), ("acc", want[1]), ("depth", want[3])):
        dist = float((out[key].double() - w).abs().max())
        print(f"{key}: scene - oracle {dist:.2e} (bar {res[key][1]:.2e})")
        assert dist <= res[key][1], key
    assert torch.equal(obj_acc[:, 0], acc)


def test_lit_render_scene(dev):
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    syn = _syn()
    lit = LitNeRF_AutoDecoder({"N_max_objs": 2, "chunk": 100}, randomized=False, model_kwargs=dict(num_coarse_samples=16, num_fine_samples=16)).to(dev)
    lit.model.load_state_dict(syn.make_art_state_dict(seed=0, density_scale=2.0))
    lit.code_library.load_state_dict(syn.make_code_library_state(seed=0))
    H, W = 12, 16
    batch = to_dev(syn.make_rays(H, W, CAM, syn.focal_from_fovy(H, 30.0)), dev)
    explicit = syn.seeded_uniform(90, 32) * 0.1
    placements = [(0, 4, pose(1, (0.0, 0.0, 0.0)), 1.4), (1, 11, pose(2, (0.4, 0.3, 0.2)), 1.0), (0, explicit, pose(3, (-0.9, 0.8, 0.0)), 0.8)]
    a = lit.render_scene(batch, placements)
    assert tuple(a["rgb"].shape) == (H * W, 3) and tuple(a["acc"].shape) == (H * W,) and tuple(a["depth"].shape) == (H * W,)
    assert tuple(a["obj_acc"].shape) == (H * W, 3)
    assert float((a["obj_acc"].sum(1) - a["acc"]).abs().max()) <= 1e-6 and float(a["acc"].max()) > 0.05
    order = [2, 0, 1]
    b = lit.render_scene(batch, [placements[i] for i in order])
    # the bar of the compositing outputs at these sizes is its floor (the serial fp32 restatement sits below 6e-7 at 65 samples)
    for key in ("rgb", "acc", "depth"):
        assert float((a[key] - b[key]).abs().max()) <= FLOORS[key], key
    assert float((a["obj_acc"][:, order] - b["obj_acc"]).abs().max()) <= FLOORS["obj_acc"]
    with pytest.raises(ValueError, match="outside the library"):
        lit.render_scene(batch, [(5, 0, pose(1, (0.0, 0.0, 0.0)), 1.0)])
    with pytest.raises(ValueError, match="interpolated states"):
        lit.render_scene(batch, [(0, 19, pose(1, (0.0, 0.0, 0.0)), 1.0)])


# ------------------------------------------------------------------ the memory contract (tests/_guard.py through test_hip_extents.run_case)
GUARD_CASES: list = []


def _guard_case(name, n, K, S, objects_fn, rays_fn):
    def make(dev):
        return {"rays": to_dev(rays_fn(n), dev), "objects": objects_fn(), "raw_full": seeded_raw(3, n, K, S).to(dev)}

    def call(ops, i):
        r = i["rays"]
        pairs = ops.scene_pairs(r["rays_o"], r["rays_d"], r["viewdirs"], i["objects"])
        t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, S - 1, pairs.near, pairs.far, want_coords=False)
        outs = ops.scene_composite(gather_raw(i["raw_full"], pairs), t, pairs, r["rays_d"], True)
        # "rows from offsets[K] on are not written": they lie inside the buffers, where no band looks, so in the guarded runs the tail of
        # every per-pair array (pairs.capacity) must still hold its prefill, 0xFF bytes or zeros
        alloc = getattr(ops.torch, "_alloc", None)
        if alloc is not None:
            torch.cuda.synchronize()
            want = _guard.FILL if alloc.prefill == "nan" else 0
            for key, full in pairs.capacity.items():
                assert full.shape[0] == n * K, key
                tail = full[pairs.P:].contiguous().reshape(-1).view(torch.uint8)
                assert bool((tail == want).all()), f"{name}: {key} rows past P = {pairs.P} were written"
        # slot + 1: a slot of -1 is the 0xFFFFFFFF word the protocol reads as "nobody wrote this"; the per-pair arrays are cut to the P rows
        # the contract says are written
        return [pairs.offsets, pairs.slot + 1, pairs.ray, pairs.rays_o, pairs.rays_d, pairs.viewdirs, pairs.near, pairs.far, *outs]
    return Case("scene", name, make, call, ["aon_scene_pairs_workspace_bytes", "aon_scene_pairs", "aon_scene_composite"])


for _n in (1, 5, 37):
    for _K in (1, 3):
        GUARD_CASES.append(_guard_case(f"scene_n{_n}_k{_K}", _n, _K, 41, lambda K=_K: layout_objects(K), lambda n: mixed_rays(n, seed=7)))
GUARD_CASES.append(_guard_case("scene_no_pair", 37, 2, 41, lambda: [BEHIND, NOT_HIT], frame_rays))
GUARD_CASES.append(_guard_case("scene_k16_s256", 7, 16, 256, lambda: layout_objects(16), lambda n: mixed_rays(n, seed=7)))


@pytest.mark.parametrize("c", GUARD_CASES, ids=[c.name for c in GUARD_CASES])
def test_memory_contract(dev, monkeypatch, c):
    """Three runs (plain, guarded with 0xFF prefill, guarded with zero prefill): bit-equal outputs, no 0xFFFFFFFF word left, no band touched,
    inputs unchanged, a workspace of exactly the queried size."""
    run_case(c, dev, monkeypatch)


# ------------------------------------------------------------------ streams
def test_a_frame_on_a_side_stream(dev):
    """The frame enqueued on a side stream while the default stream is busy equals the serial bits, and finishes before the default stream's
    delay does: every launch and the one read-back went to the side stream."""
    from aon_amd import scene

    model = art_model(dev, 2, 16, 16)
    objects = placed(dev, [nested(0, 0), disjoint(1, 0), (pose(5, (0.3, 0.2, -0.1)), 0.9)])
    syn = _syn()
    rays = to_dev(syn.make_rays(8, 12, CAM, syn.focal_from_fovy(8, 30.0)), dev)
    with torch.no_grad():
        serial = scene.render_scene(model, objects, rays, True)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        busy = hasattr(torch.cuda, "_sleep")
        if busy:
            torch.cuda._sleep(int(2.4e6 * 60))          # about 60 ms of the default stream
        gate = torch.cuda.Event()
        gate.record()
        with torch.cuda.stream(side):
            got = scene.render_scene(model, objects, rays, True)
        side.synchronize()
        pending = not gate.query()
        torch.cuda.synchronize()
    for g, w in zip(got, serial):
        for a, b in zip(g, w):
            assert torch.equal(_guard.bits(a), _guard.bits(b))
    if busy:
        assert pending, "the side stream's frame waited for the default stream"
