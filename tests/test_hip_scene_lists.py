"""GPU: scenes with a background field (csrc/aon_scene_lists.hip, include/aon_hip_scene_lists.h).

Composite: the HIP kernel against tests/_scene_lists_ref.composite_ref in fp64 on the same raw and t, every ray, per output within
max(floor, 3 x max|restatement fp32 - restatement fp64|) -- the convention and the floors of tests/test_hip_scene.py, restated here.
Bits: homogeneous closed lists are aon_scene_composite's bits; repeat, permuted rays, sub-batch, side stream.
Whole path: scene.render_scene(background=...) against the chain written out with stage calls (bit for bit), against ops.composite_raw where
no object is in the way, against the oracle (tests/_scene_lists_ref.render_scene_ref), with grids, and through the harness method.
Contracts: guard bands (tests/_guard.py), nullable outputs, rows past `pairs`."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _guard  # noqa: E402
import _scene_lists_ref as lref  # noqa: E402
import _scene_ref as sref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

FLOORS = {"rgb": 2e-6, "acc": 2e-6, "obj_acc": 2e-6, "weights": 1e-6, "depth": 1e-5}     # the compositing bars of tests/test_hip_scene.py
KEYS = ("rgb", "acc", "depth", "obj_acc", "weights")


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
NOT_HIT = (pose(4, (60.0, 0.0, 0.0)), ((-0.2, -0.3, -0.1), (0.3, 0.2, 0.4)))          # no ray meets it
BG_NEAR, BG_FAR = 2.0, 6.0


def frame_rays(n, H=15, W=20):
    """n rays spread over an H x W frame of a camera at radius 4 looking at the origin"""
    syn = _syn()
    fr = syn.make_rays(H, W, CAM, syn.focal_from_fovy(H, 18.0))
    idx = torch.arange(n) * (H * W) // n
    return {k: v[idx].contiguous() for k, v in fr.items()}


def mixed_rays(n, seed=5):
    """half frame rays, half rays from random origins on the radius-4 sphere looking roughly at the origin"""
    a, b = frame_rays(n - n // 2), _syn().random_rays(n // 2, seed=seed)
    return {k: torch.cat([a[k], b[k]]) if n // 2 else a[k] for k in a}


def small_frame():
    syn = _syn()
    return syn.make_rays(8, 12, CAM, syn.focal_from_fovy(8, 30.0))           # 96 rays


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


def to_dev(rays, dev):
    return {k: v.to(dev) for k, v in rays.items()}


def seeded_raw(seed, n, K1, S):
    """(n, K + 1, S, 4) raw records named by (world ray, list, sample); the backdrop (the last list) has mixed signs of sigma and, in its
    LAST sample, a raw sigma of exactly 0 on every third ray and a large positive one on the next"""
    rng = np.random.default_rng(seed)
    raw = rng.normal(0.0, 2.0, (n, K1, S, 4)).astype(np.float32)
    raw[:, :-1, :, 3] = raw[:, :-1, :, 3] * 1.5 + 2.0
    raw[:, -1, :, 3] = raw[:, -1, :, 3] * 0.5 - 0.3
    raw[0::3, -1, -1, 3] = 0.0
    raw[1::3, -1, -1, 3] = 40.0
    return torch.from_numpy(raw)


def gather_raw(raw_full, pairs):
    k_of = torch.repeat_interleave(torch.arange(pairs.K, device=raw_full.device), torch.tensor(pairs.counts, device=raw_full.device))
    return raw_full[pairs.ray.long(), k_of].contiguous()


def scene_lists(ops, K, open_end=True):
    return [ops.SceneList(ops.ACT_ARTICULATED, False)] * K + [ops.SceneList(ops.ACT_VANILLA, open_end)]


REF_LISTS = lambda K: [(lref.ACT_ARTICULATED, None, False)] * K + [(lref.ACT_VANILLA, None, True)]   # noqa: E731


def bg_pairs(ops, rays, objects, near=BG_NEAR, far=BG_FAR):
    n, dev = rays["rays_o"].shape[0], rays["rays_o"].device
    obj = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], objects) if objects else ops.ScenePairs.without_objects(n, dev)
    return obj, obj.with_background(rays["rays_o"], rays["rays_d"], rays["viewdirs"], near, far)


def host(outs, want_weights=True):
    rgb, acc, depth, obj_acc, weights = outs
    torch.cuda.synchronize()
    out = {"rgb": rgb.cpu(), "acc": acc.cpu(), "depth": depth.cpu(), "obj_acc": obj_acc.cpu()}
    if want_weights:
        out["weights"] = weights.cpu()
    return out


def run_chain(dev, rays_cpu, objects, raw_full, S, white, near=BG_NEAR, far=BG_FAR, edit_t=None):
    """pairs + backdrop -> HIP sampler -> seeded raw -> HIP composite; -> (pairs, t, raw, outputs dict on the host)"""
    from aon_amd import ops

    rays = to_dev(rays_cpu, dev)
    _, pairs = bg_pairs(ops, rays, objects, near, far)
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, S - 1, pairs.near, pairs.far, want_coords=False)
    if edit_t is not None:
        t = edit_t(pairs, t)
    raw = gather_raw(raw_full.to(dev), pairs)
    out = host(ops.scene_composite_lists(raw, t, pairs, rays["rays_d"], white, scene_lists(ops, len(objects))))
    return pairs, t, raw, out


def bars_and_distances(out, raw, t, slot, dirs_cpu, white, lists):
    """-> {output: (distance of HIP from fp64, bar, distance of the serial fp32 restatement from fp64)}, the fp64 restatement"""
    args = (raw.cpu().numpy(), t.cpu().numpy(), slot.cpu().numpy(), dirs_cpu.numpy(), white, lists)
    r64, r32 = lref.composite_ref(*args, dtype=np.float64), lref.composite_ref(*args, dtype=np.float32)
    res = {}
    for key in out:
        own = float(np.abs(r32[key].astype(np.float64) - r64[key]).max(initial=0.0))
        res[key] = (float(np.abs(out[key].numpy().astype(np.float64) - r64[key]).max(initial=0.0)), max(FLOORS[key], 3 * own), own)
    return res, r64


def check_bars(name, res):
    for key, (dist, bar, own) in res.items():
        print(f"  {name} {key:8s} HIP - fp64 {dist:.2e}   bar {bar:.2e}   (serial fp32 - fp64 {own:.2e})")
    for key, (dist, bar, _) in res.items():
        assert np.isfinite(dist) and dist <= bar, (name, key, dist, bar)


# ------------------------------------------------------------------ 1. against fp64
#            name          n   S    objects
COMPOSITE = [("bg_s2",     11, 2,   lambda: []),
             ("bg_s64",    11, 64,  lambda: []),
             ("bg_s65",    11, 65,  lambda: []),
             ("one_s3",    9,  3,   lambda: [nested(0, 0)]),
             ("three_s65", 37, 65,  lambda: layout_objects(3)),
             ("k15_s256",  7,  256, lambda: layout_objects(15))]


@pytest.mark.parametrize("white", [True, False], ids=["white", "black"])
@pytest.mark.parametrize("case", COMPOSITE, ids=[c[0] for c in COMPOSITE])
def test_composite_lists_against_fp64(dev, case, white):
    name, n, S, make = case
    objects = make()
    K = len(objects)
    rays_cpu = mixed_rays(n, seed=7)
    raw_full = seeded_raw(40 + K + S, n, K + 1, S)
    pairs, t, raw, out = run_chain(dev, rays_cpu, objects, raw_full, S, white)
    live_lists = (pairs.slot >= 0).sum(1).cpu()
    print(f"{name} white={white}: P={pairs.P} of {n * (K + 1)}, live lists per ray {sorted(set(live_lists.tolist()))}")
    assert pairs.K == K + 1 and pairs.counts[K] == n and (live_lists >= 1).all()
    if K:
        assert (live_lists >= 2).any()                     # mixed activations on one ray
    if name == "k15_s256":
        assert (K + 1) * S == 4096
    # the backdrop's last sample: a raw sigma of exactly 0 and a large one are both there
    last = raw[pairs.segment(K)][:, -1, 3].cpu()
    assert (last == 0).any() and (last == 40).any()
    res, r64 = bars_and_distances(out, raw, t, pairs.slot, rays_cpu["rays_d"], white, REF_LISTS(K))
    check_bars(name, res)
    # a dense last sample takes all that is left (every factor may add 1e-10), and the parts add up
    dense = (last == 40).numpy()
    assert np.abs(r64["acc"][dense] - 1).max() <= (K + 1) * S * 1e-10
    assert float((out["obj_acc"].sum(1) - out["acc"]).abs().max()) <= 2e-6


# ------------------------------------------------------------------ 2. ties
def test_ties_the_backdrop_goes_after_the_object(dev):
    n, S = 9, 17
    rays_cpu = frame_rays(n)

    def copy_t(pairs, t):
        slot0 = pairs.slot[:, 0].long()
        hit = slot0 >= 0
        assert bool(hit.any())
        t = t.clone()
        t[pairs.segment(1)][hit] = t[slot0[hit]]
        return t
    pairs, t, raw, out = run_chain(dev, rays_cpu, [nested(0, 1)], seeded_raw(9, n, 2, S), S, True, edit_t=copy_t)
    hit = (pairs.slot[:, 0] >= 0).cpu()
    rows0, rows1 = pairs.slot[:, 0].long().cpu()[hit], pairs.slot[:, 1].long().cpu()[hit]
    assert torch.equal(t.cpu()[rows0], t.cpu()[rows1])
    for r in np.nonzero(hit.numpy())[0][:2]:             # the restatement's order: at equal t the object (list 0), then the backdrop (list 1)
        order = [(k, i) for _, k, i, _ in sref.merge_order(t.cpu().numpy(), pairs.slot[r].cpu().numpy())]
        assert order == [(k, i) for i in range(S) for k in (0, 1)]
    res, r64 = bars_and_distances(out, raw, t, pairs.slot, rays_cpu["rays_d"], True, REF_LISTS(1))
    check_bars("ties", res)
    # the other order is another picture: far outside the bar
    swapped = lref.composite_ref(raw.cpu().numpy()[np.r_[rows1.numpy(), rows0.numpy()]], t.cpu().numpy()[np.r_[rows1.numpy(), rows0.numpy()]],
                                 np.stack([np.arange(len(rows0)), np.arange(len(rows0)) + len(rows0)], 1).astype(np.int32),
                                 rays_cpu["rays_d"].numpy()[hit.numpy()], True, [(lref.ACT_VANILLA, None, True), (lref.ACT_ARTICULATED, None, False)])
    assert np.abs(swapped["weights"][: len(rows0)] - r64["weights"][rows1.numpy()]).max() > 100 * res["weights"][1]


# ------------------------------------------------------------------ 3. the open interval in the middle
def test_the_open_interval_in_the_middle(dev):
    """the object's box reaches beyond the backdrop's far and the backdrop's last sample has density: what lies behind it gets the formula's
    1e-10 transmittance -- finite, within the bar"""
    n, S, far = 9, 17, 3.6
    rays_cpu = frame_rays(n)
    raw_full = seeded_raw(11, n, 2, S)
    raw_full[:, 1, -1, 3] = 5.0
    pairs, t, raw, out = run_chain(dev, rays_cpu, [nested(0, 0)], raw_full, S, True, far=far)
    hit = (pairs.slot[:, 0] >= 0).cpu()
    rows0 = pairs.slot[:, 0].long().cpu()[hit]
    behind = t.cpu()[rows0] > far
    assert bool(hit.any()) and bool(behind.any(1).all())             # every object list has samples behind the backdrop's end
    for key in KEYS:
        assert bool(torch.isfinite(out[key]).all()), key
    w_behind = out["weights"][rows0][behind]
    assert float(w_behind.max()) <= 1.0001e-10 and float(w_behind.max()) > 0
    res, _ = bars_and_distances(out, raw, t, pairs.slot, rays_cpu["rays_d"], True, REF_LISTS(1))
    check_bars("open_in_the_middle", res)
    assert float((out["acc"] - 1).abs().max()) <= FLOORS["acc"]


# ------------------------------------------------------------------ 4. the bits of the existing entry
@pytest.mark.parametrize("K", [1, 3, 16])
def test_homogeneous_closed_lists_are_scene_composite_bit_for_bit(dev, K):
    from aon_amd import ops

    n, S = 37, 65
    rays_cpu = mixed_rays(n, seed=7)
    rays = to_dev(rays_cpu, dev)
    pairs = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], layout_objects(K))
    assert 0 < pairs.P < n * K or K == 1
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, S - 1, pairs.near, pairs.far, want_coords=False)
    raw = gather_raw(seeded_raw(5, n, K + 1, S)[:, :K].contiguous().to(dev), pairs)
    custom = ops.RenderOpts(rgb_padding=0.01, density_bias=0.5)
    for act, opts in ((ops.ACT_ARTICULATED, None), (ops.ACT_ARTICULATED, custom), (ops.ACT_VANILLA, None), (ops.ACT_NONE, None)):
        for white in (True, False):
            for want_weights in (True, False):
                want = ops.scene_composite(raw, t, pairs, rays["rays_d"], white, opts=opts, want_weights=want_weights, act=act)
                got = ops.scene_composite_lists(raw, t, pairs, rays["rays_d"], white, [ops.SceneList(act, False, opts)] * K, want_weights=want_weights)
                for key, a, b in zip(KEYS, got, want):
                    if a is None:
                        assert b is None and not want_weights
                        continue
                    assert torch.equal(_guard.bits(a), _guard.bits(b)), (K, act, white, key)


# ------------------------------------------------------------------ 5. bits do not depend on the call
def full_weights(weights, pairs, n, S):
    """(P, S) in the pairs' layout -> (n, K, S) named by (ray, list), zero where there is no row"""
    out = torch.zeros(n, pairs.K, S)
    slot = pairs.slot.cpu().long()
    r, k = (slot >= 0).nonzero(as_tuple=True)
    out[r, k] = weights[slot[r, k]]
    return out


def test_bits_do_not_depend_on_the_call(dev):
    from aon_amd import ops

    n, K, S = 37, 3, 65
    objects, rays_cpu, raw_full = layout_objects(K), mixed_rays(n, seed=7), seeded_raw(5, n, K + 1, S)

    def run(rays_cpu, raw_full):
        pairs, t, raw, out = run_chain(dev, rays_cpu, objects, raw_full, S, True)
        out["weights"] = full_weights(out["weights"], pairs, rays_cpu["rays_o"].shape[0], S)
        return out, (pairs, t, raw)

    def same(a, b, index=None):
        for key in KEYS:
            x = a[key] if index is None else a[key][index]
            assert torch.equal(_guard.bits(x), _guard.bits(b[key])), key
    base, (pairs, t, raw) = run(rays_cpu, raw_full)
    assert n < pairs.P < n * (K + 1)
    same(base, run(rays_cpu, raw_full)[0])                                                      # repeat
    perm = torch.from_numpy(np.random.default_rng(1).permutation(n))
    same(base, run({k: v[perm] for k, v in rays_cpu.items()}, raw_full[perm])[0], index=perm)   # permuted rays
    same(base, run({k: v[5:20].contiguous() for k, v in rays_cpu.items()}, raw_full[5:20])[0], index=slice(5, 20))   # sub-batch
    # a side stream.  A HIGH-priority one: torch hands out normal-priority streams round robin from one pool per process and the runtime
    # spreads the streams in use over a few hardware queues, so which queue a later test's side stream shares -- the default stream's, in
    # the tests that time a frame against a busy default stream -- depends on how many normal streams were used before it.  High-priority
    # streams have their own pool and their own queues: this test leaves the other one as it found it.
    rays = to_dev(rays_cpu, dev)
    side = torch.cuda.Stream(dev, priority=-1)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        outs = ops.scene_composite_lists(raw, t, pairs, rays["rays_d"], True, scene_lists(ops, K))
    side.synchronize()
    got = host(outs)
    got["weights"] = full_weights(got["weights"], pairs, n, S)
    same(base, got)


# ------------------------------------------------------------------ 6. the memory contract
GUARD = [("n1_bg", 1, 41, lambda: []), ("n5_k1", 5, 41, lambda: layout_objects(1)), ("n37_k3", 37, 41, lambda: layout_objects(3)),
         ("n7_k15_s256", 7, 256, lambda: layout_objects(15))]


@pytest.mark.parametrize("case", GUARD, ids=[c[0] for c in GUARD])
def test_memory_contract(dev, monkeypatch, case):
    """Three runs (plain, guarded with 0xFF prefill, guarded with zero prefill): bit-equal outputs, no 0xFFFFFFFF word left, no band touched,
    inputs unchanged."""
    from aon_amd import ops

    name, n, S, make = case
    objects = make()
    K = len(objects)
    rays = to_dev(mixed_rays(n, seed=7), dev)
    _, pairs = bg_pairs(ops, rays, objects)
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, S - 1, pairs.near, pairs.far, want_coords=False)
    raw = gather_raw(seeded_raw(3, n, K + 1, S).to(dev), pairs)
    torch.cuda.synchronize()

    def one(prefill):
        if prefill is None:
            ins = [raw, t, pairs.slot, rays["rays_d"]]
            before = [_guard.bits(x) for x in ins]
            outs = [_guard.bits(x) for x in ops.scene_composite_lists(ins[0], ins[1], pairs, ins[3], True, scene_lists(ops, K))]
            assert all(torch.equal(_guard.bits(x), b) for x, b in zip(ins, before))
            return outs
        with _guard.guarded(monkeypatch, prefill) as (alloc, rec):
            ins = [_guard.place(alloc, x) for x in (raw, t, pairs.slot, rays["rays_d"])]
            guarded_pairs = ops.ScenePairs(pairs.n, pairs.K, pairs.offsets, pairs.counts, ins[2], pairs.ray, pairs.rays_o, pairs.rays_d, pairs.viewdirs,
                                           pairs.near, pairs.far)
            before = [_guard.bits(x) for x in ins]
            placed = len(alloc)
            outs = ops.scene_composite_lists(ins[0], ins[1], guarded_pairs, ins[3], True, scene_lists(ops, K))
            assert len(alloc) == placed + 5, "the call's outputs did not come from the guarded allocator"
            alloc.check()
            assert all(torch.equal(_guard.bits(x), b) for x, b in zip(ins, before)), "an input was written"
            if prefill == "nan":
                assert not [i for i, x in enumerate(outs) if _guard.has_unwritten_word(x)], "an output element nobody wrote"
            assert "aon_scene_composite_lists" in rec.names
            return [_guard.bits(x) for x in outs]
    plain, nan, zero = one(None), one("nan"), one("zero")
    for a, b, z in zip(plain, nan, zero):
        assert a.shape == b.shape == z.shape and torch.equal(b, z) and torch.equal(a, b)


def test_nullable_outputs_and_rows_past_pairs(dev):
    from aon_amd import _lib, ops

    n, S, K = 9, 17, 2
    rays = to_dev(mixed_rays(n, seed=7), dev)
    _, pairs = bg_pairs(ops, rays, layout_objects(K))
    P = pairs.P
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, S - 1, pairs.near, pairs.far, want_coords=False)
    raw = gather_raw(seeded_raw(3, n, K + 1, S).to(dev), pairs)
    want = ops.scene_composite_lists(raw, t, pairs, rays["rays_d"], True, scene_lists(ops, K))
    arr = (_lib.SceneListC * (K + 1))()
    for k, x in enumerate(scene_lists(ops, K)):
        x.fill(arr[k])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(pairs_arg, obj_acc, weights):
        rgb, acc, depth = torch.empty(n, 3, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
        ops.check(ops.lib.aon_scene_composite_lists(raw.data_ptr(), t.data_ptr(), pairs.slot.data_ptr(), rays["rays_d"].data_ptr(), n, K + 1, pairs_arg, S, 1, arr,
                                                    rgb.data_ptr(), acc.data_ptr(), depth.data_ptr(), None if obj_acc is None else obj_acc.data_ptr(),
                                                    None if weights is None else weights.data_ptr(), stream), "aon_scene_composite_lists")
        torch.cuda.synchronize()
        return rgb, acc, depth
    # obj_acc and weights NULL: the other three are the same bits
    for a, b in zip(call(P, None, None), want[:3]):
        assert torch.equal(_guard.bits(a), _guard.bits(b))
    # weights with rows past P: untouched
    weights = torch.full((P + 5, S), -7.0, device=dev)
    call(P, None, weights)
    assert torch.equal(_guard.bits(weights[:P]), _guard.bits(want[4])) and bool((weights[P:] == -7.0).all())
    # pairs cut in front of the backdrop's rows: those rows are nobody's -- never read, never written, the backdrop's list dead on every ray
    P0 = pairs.starts[K]
    weights = torch.full((P, S), -7.0, device=dev)
    obj_acc = torch.full((n, K + 1), -7.0, device=dev)
    rgb, acc, depth = call(P0, obj_acc, weights)
    assert bool((weights[P0:] == -7.0).all()) and bool((obj_acc[:, K] == 0).all()) and not bool((obj_acc == -7.0).any())
    obj_only = ops.scene_composite_lists(raw[:P0].contiguous(), t[:P0].contiguous(), ops.ScenePairs(n, K, pairs.offsets[:K + 1], pairs.counts[:K],
                                         pairs.slot[:, :K].contiguous(), pairs.ray, pairs.rays_o, pairs.rays_d, pairs.viewdirs, pairs.near, pairs.far),
                                         rays["rays_d"], True, scene_lists(ops, K)[:K])
    for a, b in zip((rgb, acc, depth, obj_acc[:, :K], weights[:P0]), obj_only):
        assert torch.equal(_guard.bits(a), _guard.bits(b))
    # pairs == 0 with NULL raw / t: every ray gets the background colour
    rgb, acc, depth = torch.empty(n, 3, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
    ops.check(ops.lib.aon_scene_composite_lists(None, None, pairs.slot.data_ptr(), rays["rays_d"].data_ptr(), n, K + 1, 0, S, 0, arr, rgb.data_ptr(), acc.data_ptr(),
                                                depth.data_ptr(), None, None, stream), "aon_scene_composite_lists")
    torch.cuda.synchronize()
    assert not rgb.any() and not acc.any() and not depth.any()


# ------------------------------------------------------------------ whole path
_MODELS: dict = {}
BG_SEED = 7


def art_model(dev, levels, nc, nf):
    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

    key = ("art", levels, nc, nf)
    if key not in _MODELS:
        m = NeRF_AE_Art(num_levels=levels, num_coarse_samples=nc, num_fine_samples=nf).to(dev)
        m.load_state_dict(_syn().make_art_state_dict(seed=0, density_scale=2.0))
        _MODELS[key] = m
    return _MODELS[key]


def bg_state_dict():
    """the backdrop's field: a seeded smooth state dict with a density bias (see test 9 for how it was chosen)"""
    return _syn().make_smooth_nerf_state_dict(seed=BG_SEED)


def backdrop(dev, levels, near=BG_NEAR, far=BG_FAR):
    from aon_amd import scene
    from aon_amd.models.vanilla_nerf.model import NeRF

    key = ("bg", levels)
    if key not in _MODELS:
        m = NeRF(num_levels=levels).to(dev)
        m.load_state_dict(bg_state_dict())
        _MODELS[key] = m
    return scene.SceneBackground(_MODELS[key], near, far)


def codes(dev, k):
    syn = _syn()
    return {key: (0.2 * syn.seeded_uniform(60 + 3 * k + i, 1, w) - 0.1).to(dev) for i, (key, w) in enumerate((("density", 128), ("color", 128), ("articulation", 32)))}


def placed(dev, objects, grids=None):
    from aon_amd import scene
    return [scene.SceneObject(codes(dev, k), p, b, None if grids is None else grids[k]) for k, (p, b) in enumerate(objects)]


THREE = lambda: [nested(0, 0), disjoint(1, 0), (pose(5, (0.3, 0.2, -0.1)), 0.9)]   # noqa: E731


def written_out(model, objects, rays, white, bg=None):
    """scene.render_scene's flow with stage-level ops calls, every ray in one chunk -> (levels, [(pairs, t, raw) per level]).  bg None: the
    flow of a scene without a backdrop (ops.scene_composite), as tests/test_hip_scene.py writes it out."""
    from aon_amd import ops

    if bg is None:
        pairs = obj_pairs = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], objects)
    else:
        obj_pairs, pairs = bg_pairs(ops, rays, objects, bg.near, bg.far)
    K = len(objects)
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, model.num_coarse_samples, pairs.near, pairs.far, want_coords=False)
    levels, stages = [], []
    bg_mlps = None if bg is None else [bg.model.coarse_mlp, bg.model.fine_mlp]
    for level, mlp in enumerate([model.coarse_mlp, model.fine_mlp][: model.num_levels]):
        raw = torch.empty((pairs.P, t.shape[1], 4), device=t.device)
        for k, ob in enumerate(objects):
            seg = obj_pairs.segment(k)
            if seg.stop > seg.start:
                small = ops.art_prepare(dict(mlp.named_parameters()), ob.latents, degrees=mlp.degrees)
                ops.art_mlp_fwd(mlp.packed(), small, pairs.rays_o[seg], pairs.rays_d[seg], pairs.viewdirs[seg], t[seg], out=raw[seg])
        if bg is None:
            rgb, acc, depth, obj_acc, weights = ops.scene_composite(raw, t, pairs, rays["rays_d"], white, opts=model._opts)
        else:
            seg = pairs.segment(K)
            raw[seg] = ops.mlp_fwd(bg_mlps[level].packed(), rays["rays_o"], rays["rays_d"], rays["viewdirs"], t[seg])
            lists = [ops.SceneList(ops.ACT_ARTICULATED, False, model._opts)] * K + [ops.SceneList(ops.ACT_VANILLA, True)]
            rgb, acc, depth, obj_acc, weights = ops.scene_composite_lists(raw, t, pairs, rays["rays_d"], white, lists)
        levels.append((rgb, acc, depth, obj_acc))
        stages.append((pairs, t, raw))
        if level + 1 < model.num_levels:
            t = ops.sample_pdf_t_n(t, weights, model.num_fine_samples)
    return levels, stages


def same_levels(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert a.shape == b.shape and torch.equal(_guard.bits(a), _guard.bits(b))


# ------------------------------------------------------------------ 7. the written-out chain
@pytest.mark.parametrize("levels", [1, 2], ids=["one_level", "two_levels"])
def test_render_scene_with_a_background_is_the_written_out_chain(dev, levels):
    from aon_amd import scene

    model, bg = art_model(dev, levels, 16, 16), backdrop(dev, levels)
    objects = placed(dev, THREE())
    rays = to_dev(small_frame(), dev)
    with torch.no_grad():
        got = scene.render_scene(model, objects, rays, True, chunk=40, background=bg)           # 96 rays: chunks of 40, 40, 16
        want, stages = written_out(model, objects, rays, True, bg)
        plain = scene.render_scene(model, objects, rays, True, chunk=40)                        # background=None: the parent's calls and bits
        want_plain, _ = written_out(model, objects, rays, True)
    assert len(got) == levels and 96 < stages[0][0].P < 96 * 4
    for g in got:
        assert [tuple(x.shape) for x in g] == [(96, 3), (96,), (96,), (96, 4)]
    same_levels(got, want)
    for g in plain:
        assert [tuple(x.shape) for x in g] == [(96, 3), (96,), (96,), (96, 3)]
    same_levels(plain, want_plain)
    assert float(got[-1][3][:, 3].max()) > 0.05 and float(got[-1][3][:, :3].max()) > 0.05          # the backdrop and an object are seen
    # per-ray near / far tensors of the same values: the same bits, chunk by chunk
    per_ray = backdrop(dev, levels, torch.full((96, 1), BG_NEAR, device=dev), torch.full((96,), BG_FAR, device=dev))
    with torch.no_grad():
        same_levels(scene.render_scene(model, objects, rays, True, chunk=40, background=per_ray), want)


# ------------------------------------------------------------------ 8. no object in the way
@pytest.mark.parametrize("white", [True, False], ids=["white", "black"])
def test_without_an_object_in_the_way_the_frame_is_the_backdrops_own_composite(dev, white):
    from aon_amd import ops, scene

    model, bg = art_model(dev, 2, 16, 16), backdrop(dev, 2)
    rays_cpu = small_frame()
    rays = to_dev(rays_cpu, dev)
    with torch.no_grad():
        empty, stages = written_out(model, [], rays, white, bg)
        same_levels(scene.render_scene(model, [], rays, white, background=bg), empty)
        missed = scene.render_scene(model, placed(dev, [NOT_HIT, NOT_HIT]), rays, white, background=bg)
        hit = scene.render_scene(model, placed(dev, THREE()), rays, white, background=bg)
    for level, (pairs, t, raw) in enumerate(stages):
        assert pairs.K == 1 and pairs.P == 96
        comp, acc, weights, depth = ops.composite_raw(raw, t, rays["rays_d"], white, act=ops.ACT_VANILLA)
        torch.cuda.synchronize()
        args = (raw.cpu().numpy(), t.cpu().numpy(), pairs.slot.cpu().numpy(), rays_cpu["rays_d"].numpy(), white, REF_LISTS(0))
        r64, r32 = lref.composite_ref(*args, dtype=np.float64), lref.composite_ref(*args, dtype=np.float32)
        for key, mine, theirs in (("rgb", empty[level][0], comp), ("acc", empty[level][1], acc), ("depth", empty[level][2], depth)):
            bar = max(FLOORS[key], 3 * float(np.abs(r32[key].astype(np.float64) - r64[key]).max()))
            dist = float((mine - theirs).abs().max())
            print(f"  level {level} {key:6s} scene - composite_raw {dist:.2e}   bar {bar:.2e}")
            assert dist <= bar, (level, key, dist, bar)
        assert torch.equal(_guard.bits(empty[level][3][:, 0]), _guard.bits(empty[level][1]))          # obj_acc[:, K] is acc, bit for bit
        # objects that no ray hits: the same frame (the same lists per ray, so the same bits), two empty columns in front
        m = missed[level]
        assert tuple(m[3].shape) == (96, 3) and not m[3][:, :2].any() and torch.equal(_guard.bits(m[3][:, 2]), _guard.bits(m[1]))
        for a, b in zip(m[:3], empty[level][:3]):
            assert torch.equal(_guard.bits(a), _guard.bits(b))
        # rays that do hit an object differ from the backdrop-only frame
        seen = hit[level][3][:, :3].sum(1) > 0.05
        moved = ((hit[level][0] - empty[level][0]).abs().max(1).values > 1e-4) | ((hit[level][2] - empty[level][2]).abs() > 1e-4)
        assert bool(seen.any()) and bool(moved[seen].all())


# ------------------------------------------------------------------ 9. the whole path against the oracle
SIGMA_LAST_MARGIN = 2e-2


def oracle_fixture():
    """two objects + backdrop, 8 x 12 rays, 16 + 16 samples -> the arguments of _scene_lists_ref.render_scene_ref"""
    syn = _syn()
    specs = [nested(0, 0), (pose(5, (0.3, 0.2, -0.1)), 0.9)]
    rays_cpu = small_frame()
    lat = [{k: v.cpu() for k, v in codes("cpu", k).items()} for k in range(2)]
    args = (syn.make_art_state_dict(seed=0, density_scale=2.0), [(p.numpy(), b) for p, b in specs], lat, {k: v.numpy() for k, v in rays_cpu.items()}, True,
            bg_state_dict(), BG_NEAR, BG_FAR)
    return specs, rays_cpu, args


def test_render_scene_with_a_background_against_the_oracle_whole_path(dev):
    """scene.render_scene(background=...), both levels, against tests/_scene_lists_ref.render_scene_ref in fp64, by the yardstick of
    test_hip_scene.test_render_scene_against_the_oracle_whole_path (tests/_gradcheck.assert_as_close_as_fp32: factor 5, floor 1e-4).
    The open last interval makes a ray flip when the raw sigma of the backdrop's last sample changes sign, so the backdrop's field
    (make_smooth_nerf_state_dict(seed=7): density gain 2, density bias 0.75; seeds 1, 5, 8, 9, 11 fail this, 3, 4, 6, 7 pass) was chosen so that in the fp64 oracle NO ray of the fixture has
    |raw sigma_last| < 2e-2 at either level (the smallest are 0.61 coarse, 0.39 fine); that is asserted here, and no ray is left out."""
    from _gradcheck import assert_as_close_as_fp32
    from aon_amd import scene

    specs, rays_cpu, args = oracle_fixture()
    model, bg = art_model(dev, 2, 16, 16), backdrop(dev, 2)
    with torch.no_grad():
        got = scene.render_scene(model, placed(dev, specs), to_dev(rays_cpu, dev), True, background=bg)
    r64 = lref.render_scene_ref(*args, num_coarse=16, num_fine=16, dtype=np.float64, return_raw=True)
    r32 = lref.render_scene_ref(*args, num_coarse=16, num_fine=16, dtype=np.float32)
    names = ("rgb", "acc", "depth", "obj_acc")
    for level in range(2):
        last = np.abs(r64[level]["raw"][r64[level]["bg_rows"]][:, -1, 3])
        print(f"level {level}: min |raw sigma_last| of the backdrop in fp64 {last.min():.3e} (margin {SIGMA_LAST_MARGIN}), rays left out: 0")
        assert last.shape == (96,) and last.min() >= SIGMA_LAST_MARGIN
        assert float(r64[level]["obj_acc"][:, :2].max()) > 0.05 and float(r64[level]["obj_acc"][:, 2].max()) > 0.05
        assert_as_close_as_fp32({k: got[level][i].cpu() for i, k in enumerate(names)}, {k: torch.from_numpy(r64[level][k]) for k in names},
                                {k: torch.from_numpy(r32[level][k]) for k in names}, f"scene with a backdrop, level {level}")


# ------------------------------------------------------------------ 10. grids and a backdrop together
def test_full_grids_and_a_backdrop_are_the_dense_frame(dev):
    import _scene_occ_ref as oref
    from aon_amd import scene

    model, bg = art_model(dev, 2, 16, 16), backdrop(dev, 2)
    rays = to_dev(small_frame(), dev)
    with torch.no_grad():
        want, dense_count = scene.render_scene(model, placed(dev, THREE()), rays, True, chunk=40, background=bg, want_occupied=True)
        full = placed(dev, THREE(), [oref.enclosing("full", k).to_ops(dev) for k in range(3)])
        got, occupied = scene.render_scene(model, full, rays, True, chunk=40, background=bg, want_occupied=True)
    same_levels(got, want)
    for a, b in zip(occupied, dense_count):                      # the K objects only
        assert tuple(a.shape) == (3,) and torch.equal(a.cpu(), b.cpu()) and int(a.sum()) > 0


# ------------------------------------------------------------------ 11. the harness method
def test_lit_render_scene_with_a_background(dev):
    from aon_amd import scene
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    syn = _syn()
    lit = LitNeRF_AutoDecoder({"N_max_objs": 2, "chunk": 100}, randomized=False, model_kwargs=dict(num_coarse_samples=16, num_fine_samples=16)).to(dev)
    lit.model.load_state_dict(syn.make_art_state_dict(seed=0, density_scale=2.0))
    lit.code_library.load_state_dict(syn.make_code_library_state(seed=0))
    H, W = 12, 16
    batch = to_dev(syn.make_rays(H, W, CAM, syn.focal_from_fovy(H, 30.0)), dev)
    placements = [(0, 4, pose(1, (0.0, 0.0, 0.0)), 1.4), (1, 11, pose(2, (0.4, 0.3, 0.2)), 1.0)]
    bg = backdrop(dev, 2)
    a = lit.render_scene(batch, placements, background=bg)
    assert tuple(a["rgb"].shape) == (H * W, 3) and tuple(a["obj_acc"].shape) == (H * W, 3)
    objects = [scene.SceneObject(latents, p, b) for _, _, latents, p, b in lit._placement_codes("render_scene", placements)]
    with torch.no_grad():
        want = scene.render_scene(lit.model, objects, batch, lit.white_bkgd, chunk=100, background=bg)[-1]
    for key, w in zip(("rgb", "acc", "depth", "obj_acc"), want):
        assert torch.equal(_guard.bits(a[key]), _guard.bits(w)), key
    assert float(a["obj_acc"][:, 2].max()) > 0.05 and float(a["obj_acc"][:, :2].max()) > 0.05
    # no placement at all: the backdrop alone
    b = lit.render_scene(batch, [], background=bg)
    assert tuple(b["obj_acc"].shape) == (H * W, 1) and torch.equal(_guard.bits(b["obj_acc"][:, 0]), _guard.bits(b["acc"]))
