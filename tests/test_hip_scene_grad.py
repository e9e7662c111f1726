"""GPU: gradients through scenes (csrc/aon_scene_grad.hip, include/aon_hip_scene_grad.h).

Kernel: aon_scene_composite_bwd against tests/_scene_grad_ref.composite_grads (torch autograd in fp64 on the same raw and the HIP samplers' t),
bar max|got - ref| / max_ray|ref| < 2e-5 -- the project's own for aon_composite_bwd (tests/test_hip_training.py) -- on the scenes of
tests/test_hip_scene.py; ties, sentinel records, the last sample of every list.
Bits: repeat, permuted rays, a sub-batch, an object no ray hits.  Memory: guard bands, the capacity tail, both stream forms, a side stream.
One level through the network: autograd.RenderLevelScene against the oracle's autograd (tests/_gradcheck.py).  Whole path:
scene.render_scene_grad against scene.render_scene (forward bits) and against the chain written out with stage calls (gradient bits).
LitNeRF_AutoDecoder.fit_scene_codes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _guard  # noqa: E402
import _scene_grad_ref as gref  # noqa: E402
import test_hip_scene as hs  # noqa: E402
from test_hip_extents import Case, run_case  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("density", "color", "articulation")
BAR = 2e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------ the kernel against the fp64 restatement
def all16():
    """sixteen boxes around one centre, each turned its own way: the rays through the middle cross all of them"""
    return [(hs.pose(40 + j, (0.0, 0.0, 0.0)), 2.3 - 0.1 * j) for j in range(16)]


# `away` as in tests/test_hip_scene.py: chosen per case (tests/_scene_ref.pairs_ref, on the CPU) so that about a third of the n * K pairs are dead
#         name        n   K   S    away  objects
CASES = [("s2",       5,  2,  2,   3,    lambda: hs.layout_objects(2)),            # the minimum S: only i = 0 has an interval
         ("s3",       5,  2,  3,   3,    lambda: hs.layout_objects(2)),
         ("one",      37, 1,  65,  3,    lambda: [hs.nested(0, 2)]),
         ("three",    37, 3,  65,  6,    lambda: hs.layout_objects(3)),
         ("merged_64", 9, 2,  32,  3,    lambda: [hs.nested(0, 0), hs.nested(3, 1)]),
         ("merged_65", 9, 5,  13,  4,    lambda: [hs.nested(3 * j, j) for j in range(5)]),      # the scan carry
         ("k16",      20, 16, 193, 5,    lambda: hs.layout_objects(16)),
         ("k16_s256", 7,  16, 256, 3,    all16)]                                   # K * S = 4096, rays crossing all 16 boxes: 90,368 B of LDS


def upstream(seed, n, K):
    rng = np.random.default_rng(seed)
    g = {"g_rgb": rng.normal(size=(n, 3)), "g_acc": rng.normal(size=n), "g_depth": rng.normal(size=n), "g_obj_acc": rng.normal(size=(n, K))}
    return {k: torch.from_numpy(v.astype(np.float32)) for k, v in g.items()}


def chain(dev, rays_cpu, objects, raw_full, S, raw_index=None):
    """pairs -> HIP sampler -> seeded raw (named by (ray, object)) -> (pairs, t, raw)"""
    from aon_amd import ops

    rays = hs.to_dev(rays_cpu, dev)
    pairs = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], objects)
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, S - 1, pairs.near, pairs.far, want_coords=False)
    return pairs, t, hs.gather_raw(raw_full.to(dev), pairs, raw_index)


def backward(dev, pairs, t, raw, rays_cpu, g, white, nulls=False, act=2):
    from aon_amd import ops

    gd = {k: v.to(dev) for k, v in g.items()}
    extra = {} if nulls else {k: gd[k] for k in ("g_acc", "g_depth", "g_obj_acc")}
    return ops.scene_composite_bwd(raw, t, pairs, rays_cpu["rays_d"].to(dev), gd["g_rgb"], white_bkgd=white, act=act, **extra)


def reference(pairs, t, raw, rays_cpu, g, white, nulls=False, act=2):
    extra = {} if nulls else {k: g[k].numpy() for k in ("g_acc", "g_depth", "g_obj_acc")}
    return gref.composite_grads(raw.cpu().numpy(), t.cpu().numpy(), pairs.slot.cpu().numpy(), rays_cpu["rays_d"].numpy(), white, g["g_rgb"].numpy(),
                                act=act, **extra)


def figure(got, ref, pairs):
    """max over the samples of |got - ref| / (the largest |ref| on the sample's RAY, over all of its lists)"""
    P = pairs.P
    if P == 0:
        return 0.0
    ray = pairs.ray.cpu().long()
    per_row = ref.abs().amax(dim=(1, 2))
    scale = torch.zeros(pairs.n, dtype=torch.float64).scatter_reduce(0, ray, per_row, "amax", include_self=True).clamp_min(1e-12)
    return float(((got.cpu().double() - ref).abs().amax(dim=(1, 2)) / scale[ray]).max())


@pytest.mark.parametrize("nulls", [False, True], ids=["all_four", "rgb_only"])
@pytest.mark.parametrize("white", [True, False], ids=["white", "black"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_backward_against_fp64(dev, case, white, nulls):
    name, n, K, S, away, make = case
    rays_cpu = hs.mixed_rays(n, seed=7, away=away)
    pairs, t, raw = chain(dev, rays_cpu, make(), hs.seeded_raw(40 + K + S, n, K, S), S)
    live_lists = (pairs.slot >= 0).sum(1).cpu()
    dead = 1 - pairs.P / (n * K)
    assert 0.25 <= dead <= 0.42 and (live_lists == 0).any(), (dead, live_lists)            # about a third of the pairs dead, rays with no pair
    if name == "merged_64":
        assert (live_lists * S == 64).any()
    if name == "merged_65":
        assert (live_lists * S == 65).any()
    if name == "k16_s256":
        assert K * S == 4096 and (live_lists == 16).any()
    g = upstream(3 + n, n, K)
    got = backward(dev, pairs, t, raw, rays_cpu, g, white, nulls)
    ref = reference(pairs, t, raw, rays_cpu, g, white, nulls)
    torch.cuda.synchronize()
    fig = figure(got, ref, pairs)
    print(f"{name} white={white} nulls={nulls}: P={pairs.P} of {n * K}, worst |got - ref| / max_ray|ref| = {fig:.2e} (bar {BAR:.0e})")
    assert tuple(got.shape) == (pairs.P, S, 4) and bool(torch.isfinite(got).all())
    assert float(ref.abs().max()) > 1e-3
    assert fig < BAR
    assert not got[:, S - 1].any()                                                         # delta = 0: the whole record is exact zeros


@pytest.mark.parametrize("act", [0, 1, 2])
def test_backward_activations(dev, act):
    name, n, K, S, away, make = CASES[1]
    rays_cpu = hs.mixed_rays(n, seed=7, away=away)
    pairs, t, raw = chain(dev, rays_cpu, make(), hs.seeded_raw(11, n, K, S), S)
    g = upstream(4, n, K)
    for white in (True, False):
        fig = figure(backward(dev, pairs, t, raw, rays_cpu, g, white, act=act), reference(pairs, t, raw, rays_cpu, g, white, act=act), pairs)
        print(f"act {act} white={white}: {fig:.2e}")
        assert fig < BAR


def test_ties_are_decided_by_the_object_index(dev):
    """two identical objects with DIFFERENT records: every t ties with its twin's, and which of the two goes first changes the gradient"""
    n, S = 9, 17
    ob = hs.nested(0, 1)
    rays_cpu = hs.frame_rays(n)
    pairs, t, raw = chain(dev, rays_cpu, [ob, ob], hs.seeded_raw(9, n, 2, S), S)
    assert pairs.counts == [n, n] and torch.equal(t[:n], t[n:]) and not torch.equal(raw[:n], raw[n:])
    g = upstream(5, n, 2)
    got, ref = backward(dev, pairs, t, raw, rays_cpu, g, True), reference(pairs, t, raw, rays_cpu, g, True)
    assert figure(got, ref, pairs) < BAR
    # the other order is a different function: the reference with the twins' rows exchanged is far away
    swapped = pairs.slot.cpu().numpy()[:, ::-1].copy()
    other = gref.composite_grads(raw.cpu().numpy(), t.cpu().numpy(), swapped, rays_cpu["rays_d"].numpy(), True, g["g_rgb"].numpy(), g["g_acc"].numpy(),
                                 g["g_depth"].numpy(), g["g_obj_acc"].numpy()[:, ::-1].copy())
    assert figure(got, other, pairs) > 1e-3


def test_sentinel_records_get_exact_zeros(dev):
    name, n, K, S, away, make = CASES[3]
    rays_cpu = hs.mixed_rays(n, seed=7, away=away)
    pairs, t, raw = chain(dev, rays_cpu, make(), hs.seeded_raw(12, n, K, S), S)
    sentinel = torch.tensor([0.0, 0.0, 0.0, float("-inf")], device=dev)
    mask = torch.from_numpy(np.random.default_rng(2).random((pairs.P, S)) < 0.3).to(dev)
    mask[1] = True                                                                          # a whole list
    raw = raw.clone()
    raw[mask] = sentinel
    g = upstream(6, n, K)
    for white in (True, False):
        got = backward(dev, pairs, t, raw, rays_cpu, g, white)
        assert bool(torch.isfinite(got).all()) and not got[mask].any() and got[~mask].any()
        assert figure(got, reference(pairs, t, raw, rays_cpu, g, white), pairs) < BAR


# ------------------------------------------------------------------ bits
BITS = dict(n=37, K=3, S=65)


def full_rows(d_raw, pairs, n, K, S):
    """(P, S, 4) in the pairs' layout -> (n, K, S, 4) named by (ray, object), zero where there is no pair"""
    out = torch.zeros(n, K, S, 4)
    slot = pairs.slot.cpu().long()
    r, k = (slot >= 0).nonzero(as_tuple=True)
    out[r, k] = d_raw.cpu()[slot[r, k]]
    return out


def _bits_run(dev, rays_cpu, objects, raw_full, g, raw_index=None):
    pairs, t, raw = chain(dev, rays_cpu, objects, raw_full, BITS["S"], raw_index)
    got = backward(dev, pairs, t, raw, rays_cpu, g, True)
    return full_rows(got, pairs, rays_cpu["rays_o"].shape[0], len(objects), BITS["S"]), pairs


def test_bits_do_not_depend_on_the_call(dev):
    n, K = BITS["n"], BITS["K"]
    objects, rays_cpu, raw_full = hs.layout_objects(K), hs.mixed_rays(n, seed=7), hs.seeded_raw(5, n, K + 1, BITS["S"])
    g = upstream(7, n, K)
    base, pairs = _bits_run(dev, rays_cpu, objects, raw_full, g)
    assert 0 < pairs.P < n * K and base.any()
    same = lambda a, b: torch.equal(_guard.bits(a), _guard.bits(b))      # noqa: E731
    assert same(base, _bits_run(dev, rays_cpu, objects, raw_full, g)[0])                                     # repeat
    perm = torch.from_numpy(np.random.default_rng(1).permutation(n))
    permuted, _ = _bits_run(dev, {k: v[perm] for k, v in rays_cpu.items()}, objects, raw_full[perm], {k: v[perm] for k, v in g.items()})
    assert same(base[perm], permuted)                                                                        # permuted rays
    sub, _ = _bits_run(dev, {k: v[5:20].contiguous() for k, v in rays_cpu.items()}, objects, raw_full[5:20], {k: v[5:20].contiguous() for k, v in g.items()})
    assert same(base[5:20], sub)                                                                             # a sub-batch
    for where in (K, 0, 1):                                                                                  # an object no ray hits, at any position
        idx = list(range(K))
        idx.insert(where, K)
        g_more = dict(g)
        g_more["g_obj_acc"] = torch.cat([g["g_obj_acc"], torch.ones(n, 1)], 1)[:, idx].contiguous()
        more, p2 = _bits_run(dev, rays_cpu, [hs.NOT_HIT if i == K else objects[i] for i in idx], raw_full, g_more, raw_index=idx)
        assert p2.counts[where] == 0
        keep = [j for j, i in enumerate(idx) if i != K]
        assert same(base, more[:, keep]) and not more[:, where].any()


# ------------------------------------------------------------------ memory and streams
def _guard_case(name, n, K, S, objects_fn, away):
    def make(dev):
        return {"rays": hs.to_dev(hs.mixed_rays(n, seed=7, away=away), dev), "objects": objects_fn(), "raw_full": hs.seeded_raw(3, n, K, S).to(dev),
                "g": {k: v.to(dev) for k, v in upstream(8, n, K).items()}}

    def call(ops, i):
        r, g = i["rays"], i["g"]
        pairs = ops.scene_pairs(r["rays_o"], r["rays_d"], r["viewdirs"], i["objects"])
        t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, S - 1, pairs.near, pairs.far, want_coords=False)
        return [ops.scene_composite_bwd(hs.gather_raw(i["raw_full"], pairs), t, pairs, r["rays_d"], g["g_rgb"], g["g_acc"], g["g_depth"], g["g_obj_acc"], True)]
    return Case("scene_grad", name, make, call, ["aon_scene_composite_bwd"])


GUARD_CASES = [_guard_case("scene_grad_n5_k2_s3", 5, 2, 3, lambda: hs.layout_objects(2), 3),
               _guard_case("scene_grad_n37_k3_s41", 37, 3, 41, lambda: hs.layout_objects(3), 6),
               _guard_case("scene_grad_k16_s256", 7, 16, 256, all16, 3)]


@pytest.mark.parametrize("c", GUARD_CASES, ids=[c.name for c in GUARD_CASES])
def test_memory_contract(dev, monkeypatch, c):
    run_case(c, dev, monkeypatch)


def test_capacity_tail_and_both_stream_forms(dev):
    """a d_raw of the pairs' capacity n * K rows: rows from P on keep their prefill; the NULL stream and the current stream give the same bits"""
    from aon_amd import ops

    name, n, K, S, away, make = CASES[3]
    rays_cpu = hs.mixed_rays(n, seed=7, away=away)
    pairs, t, raw = chain(dev, rays_cpu, make(), hs.seeded_raw(13, n, K, S), S)
    g = {k: v.to(dev) for k, v in upstream(9, n, K).items()}
    d = rays_cpu["rays_d"].to(dev)
    want = ops.scene_composite_bwd(raw, t, pairs, d, g["g_rgb"], g["g_acc"], g["g_depth"], g["g_obj_acc"], True)
    torch.cuda.synchronize()
    st, _keep = ops.DEFAULT_OPTS.c_struct(1.0, 1.0)
    for stream in (None, C.c_void_p(torch.cuda.current_stream().cuda_stream)):
        full = torch.full((n * K, S, 4), -7.25, device=dev)
        ops.check(ops.lib.aon_scene_composite_bwd(raw.data_ptr(), t.data_ptr(), pairs.slot.data_ptr(), d.data_ptr(), g["g_rgb"].data_ptr(), g["g_acc"].data_ptr(),
                                                  g["g_depth"].data_ptr(), g["g_obj_acc"].data_ptr(), n, K, pairs.P, S, 1, 2, C.byref(st), full.data_ptr(), stream),
                  "aon_scene_composite_bwd")
        torch.cuda.synchronize()
        assert 0 < pairs.P < n * K and bool((full[pairs.P:] == -7.25).all())
        assert torch.equal(_guard.bits(full[: pairs.P]), _guard.bits(want))


def test_a_backward_on_a_side_stream(dev):
    name, n, K, S, away, make = CASES[6]
    rays_cpu = hs.mixed_rays(n, seed=7, away=away)
    pairs, t, raw = chain(dev, rays_cpu, make(), hs.seeded_raw(14, n, K, S), S)
    g = upstream(10, n, K)
    serial = backward(dev, pairs, t, raw, rays_cpu, g, True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    busy = hasattr(torch.cuda, "_sleep")
    if busy:
        torch.cuda._sleep(int(2.4e6 * 60))          # about 60 ms of the default stream
    gate = torch.cuda.Event()
    gate.record()
    with torch.cuda.stream(side):
        got = backward(dev, pairs, t, raw, rays_cpu, g, True)
    side.synchronize()
    pending = not gate.query()
    torch.cuda.synchronize()
    assert torch.equal(_guard.bits(got), _guard.bits(serial))
    if busy:
        assert pending, "the side stream's backward waited for the default stream"


# ------------------------------------------------------------------ one level through the network
def _level_setup(dev):
    import aon_amd.synthetic as syn
    from aon_amd import ops

    sd = syn.make_art_state_dict(seed=2, density_scale=10.0)
    prefix = "fine_mlp."
    params = {k[len(prefix):]: v.to(dev) for k, v in sd.items() if k.startswith(prefix)}
    specs = [hs.nested(0, 0), hs.nested(3, 1)]
    rays_cpu = hs.frame_rays(24)
    rays = hs.to_dev(rays_cpu, dev)
    pairs = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], specs)
    codes = [{k: v.cpu() for k, v in hs.codes(dev, k).items()} for k in range(2)]
    return sd, prefix, params, rays_cpu, rays, pairs, codes


def _level_loss(out, target, w):
    rgb, acc, depth, obj_acc = out
    return torch.mean((rgb - target) ** 2) + (0.3 * acc * w[:, 0]).mean() + (0.1 * depth * w[:, 1]).mean() + (0.2 * obj_acc * w[:, 2:4]).mean()


def _level_check(dev, setup, t, what):
    from _gradcheck import assert_as_close_as_fp32
    from aon_amd import ops
    from aon_amd.autograd import RenderLevelScene

    sd, prefix, params, rays_cpu, rays, pairs, codes = setup
    n = 24
    gen = torch.Generator().manual_seed(31)
    target, w = torch.rand(n, 3, generator=gen), torch.rand(n, 4, generator=gen)
    pr = {"o": pairs.rays_o.cpu().numpy(), "d": pairs.rays_d.cpu().numpy(), "v": pairs.viewdirs.cpu().numpy(), "offsets": np.asarray(pairs.starts),
          "slot": pairs.slot.cpu().numpy()}

    def oracle(dtype):
        sd_o = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items() if k.startswith(prefix)}
        lat_o = [{k: v.to(dtype).clone().requires_grad_(True) for k, v in c.items()} for c in codes]
        out = gref.scene_level_oracle(sd_o, prefix, pr, t.cpu().numpy(), lat_o, rays_cpu["rays_d"].numpy(), True, dtype)
        _level_loss((out["rgb"], out["acc"], out["depth"], out["obj_acc"]), target.to(dtype), w.to(dtype)).backward()
        g = {k[len(prefix):]: v.grad for k, v in sd_o.items()}
        for j, c in enumerate(lat_o):
            g.update({f"object{j}.{k}": v.grad.reshape(-1) for k, v in c.items()})
        return g

    g64, g32 = oracle(torch.float64), oracle(torch.float32)
    leaves = [p.clone().requires_grad_(True) for p in (params[name] for name in ops.ART_PARAM_ORDER)]
    lat = [{k: c[k].to(dev).requires_grad_(True) for k in KEYS} for c in codes]
    pd = dict(zip(ops.ART_PARAM_ORDER, leaves))
    out = RenderLevelScene.apply(pairs, t, rays["rays_d"], True, None, ops.pack_art_mlp(pd), ops.pack_art_mlp_bwd(pd), (0, 10, 4),
                                 *[c[k] for c in lat for k in KEYS], *leaves)
    assert not out[4].requires_grad and tuple(out[4].shape) == tuple(t.shape)
    _level_loss(out[:4], target.to(dev), w.to(dev)).backward()
    got = {name: p.grad.cpu() for name, p in pd.items()}
    for j, c in enumerate(lat):
        got.update({f"object{j}.{k}": c[k].grad.reshape(-1).cpu() for k in KEYS})
    assert len(got) == 40 + 6 and all(bool(torch.isfinite(v).all()) and bool(v.any()) for v in got.values())
    assert_as_close_as_fp32(got, g64, g32, what)
    return out[4].detach()


@pytest.mark.parametrize("S", [65, 9])
def test_one_level_against_the_oracles_autograd(dev, S):
    from aon_amd import ops

    setup = _level_setup(dev)
    pairs = setup[5]
    assert pairs.counts[0] > 0 and pairs.counts[1] > 0 and ((pairs.slot >= 0).sum(1) == 2).any()
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, S - 1, pairs.near, pairs.far, want_coords=False)
    weights = _level_check(dev, setup, t, f"scene level, S = {S}, sampler's t")
    # ... and on HIP's own fine draws from the merged weights: each level's t is data
    t2 = ops.sample_pdf_t_n(t, weights, 16)
    assert tuple(t2.shape) == (pairs.P, S + 16)
    _level_check(dev, setup, t2, f"scene level, S = {S} + 16, inverse-CDF t")


# ------------------------------------------------------------------ the whole path
def _leaf_objects(dev, specs):
    from aon_amd import scene
    return [scene.SceneObject({k: v.clone().requires_grad_(True) for k, v in hs.codes(dev, j).items()}, p, b) for j, (p, b) in enumerate(specs)]


def _frame(dev):
    syn = hs._syn()
    return hs.to_dev(syn.make_rays(8, 12, hs.CAM, syn.focal_from_fovy(8, 30.0)), dev)


SPECS = {1: lambda: [hs.nested(0, 0)], 3: lambda: [hs.nested(0, 0), hs.disjoint(1, 0), (hs.pose(5, (0.3, 0.2, -0.1)), 0.9)]}


def _scene_loss(levels, target):
    return sum(torch.mean((lv[0] - target) ** 2) + 0.1 * lv[1].mean() + 0.05 * lv[2].mean() + 0.2 * (lv[3] ** 2).mean() for lv in levels)


def _whole_grads(model, objects, rays, target):
    from aon_amd import scene

    levels = scene.render_scene_grad(model, objects, rays, True)
    wrt = [ob.latents[k] for ob in objects for k in KEYS] + [p for m in (model.coarse_mlp, model.fine_mlp)[: model.num_levels] for p in m.ordered_params()]
    return levels, torch.autograd.grad(_scene_loss(levels, target), wrt)


def _written_out_grads(model, objects, rays, target):
    """render_scene_grad's forward and backward with stage-level ops calls; the loss's own derivative from torch on detached leaves"""
    from aon_amd import ops

    pairs = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], objects)
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, model.num_coarse_samples, pairs.near, pairs.far, want_coords=False)
    S0 = t.shape[1]
    kept, outs = [], []
    for level, mlp in enumerate([model.coarse_mlp, model.fine_mlp][: model.num_levels]):
        params = {k: v.detach() for k, v in mlp.named_parameters()}
        raw = torch.empty((pairs.P, t.shape[1], 4), device=t.device)
        per = []
        for k, ob in enumerate(objects):
            seg = pairs.segment(k)
            if seg.stop > seg.start:
                small = ops.art_prepare(params, ob.latents, degrees=mlp.degrees)
                _, planes, masks = ops.art_mlp_fwd_train(mlp.packed(True), small, pairs.rays_o[seg], pairs.rays_d[seg], pairs.viewdirs[seg], t[seg], out=raw[seg])
                per.append((small, planes, masks))
            else:
                per.append(None)
        rgb, acc, depth, obj_acc, weights = ops.scene_composite(raw, t, pairs, rays["rays_d"], True, opts=model._opts)
        leaves = [x.detach().requires_grad_(True) for x in (rgb, acc, depth, obj_acc)]
        outs.append(leaves)
        kept.append((mlp, params, raw, t, per))
        if level + 1 < model.num_levels:
            t = ops.sample_pdf_t_n(t, weights, model.num_fine_samples)
    up = torch.autograd.grad(_scene_loss(outs, target), [x for lv in outs for x in lv])
    g_codes = [[torch.zeros_like(ob.latents[k]) for k in KEYS] for ob in objects]
    g_params = []
    for level, (mlp, params, raw, t, per) in enumerate(kept):
        g_rgb, g_acc, g_depth, g_obj = up[4 * level: 4 * level + 4]
        d_raw = ops.scene_composite_bwd(raw, t, pairs, rays["rays_d"], g_rgb, g_acc, g_depth, g_obj, True, opts=model._opts)
        bwd, total = mlp.packed_bwd(True), None
        for k, ob in enumerate(objects):
            if per[k] is None:
                continue
            small, planes, masks = per[k]
            seg = pairs.segment(k)
            rows = (seg.stop - seg.start) * t.shape[1]
            buf = torch.zeros((ops.padded_samples(rows), 4), device=t.device)
            buf[:rows] = d_raw[seg].reshape(rows, 4)
            dplanes, dxp = ops.art_bwd_chain(bwd, small, buf, masks, planes)
            grads, g_lat = ops.art_wgrad(planes, dplanes, buf, dxp, params, ob.latents, mlp.degrees, packed_bwd=bwd)
            total = grads if total is None else {name: total[name] + grads[name] for name in ops.ART_PARAM_ORDER}
            for j, key in enumerate(KEYS):
                g_codes[k][j] = g_codes[k][j] + g_lat[key].reshape(g_codes[k][j].shape)
        g_params += [total[name] for name in ops.ART_PARAM_ORDER]
    assert S0 == model.num_coarse_samples + 1
    return [g for oc in g_codes for g in oc] + g_params


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("levels", [1, 2])
def test_render_scene_grad_is_render_scene_and_the_written_out_chain(dev, levels, K):
    from aon_amd import scene

    model = hs.art_model(dev, levels, 16, 16)
    rays = _frame(dev)
    objects = _leaf_objects(dev, SPECS[K]())
    target = hs._syn().seeded_uniform(21, 96, 3).to(dev)
    with torch.no_grad():
        want = scene.render_scene(model, objects, rays, True)
    got, grads = _whole_grads(model, objects, rays, target)
    assert len(got) == len(want) == levels
    for g, w in zip(got, want):
        assert all(x.requires_grad for x in g)
        for a, b in zip(g, w):
            assert torch.equal(_guard.bits(a.detach()), _guard.bits(b))                     # the forward, bit for bit
    assert float(want[-1][1].max()) > 0.05
    ref = _written_out_grads(model, objects, rays, target)
    assert len(grads) == len(ref) == 3 * K + 40 * levels
    for i, (a, b) in enumerate(zip(grads, ref)):
        assert torch.equal(_guard.bits(a), _guard.bits(b)), i                               # the gradients, bit for bit
        assert bool(torch.isfinite(a).all())
    assert all(bool(g.any()) for g in grads[: 3 * K]) and all(p.grad is None for p in model.parameters())
    # a fresh forward gives equal, independent tensors
    _, again = _whole_grads(model, objects, rays, target)
    for a, b in zip(grads, again):
        assert torch.equal(_guard.bits(a), _guard.bits(b)) and a.data_ptr() != b.data_ptr()


def test_a_second_backward_raises_and_in_place_edits_are_seen(dev):
    from aon_amd import scene

    model = hs.art_model(dev, 2, 16, 16)
    rays = _frame(dev)
    objects = _leaf_objects(dev, SPECS[3]())
    loss = scene.render_scene_grad(model, objects, rays, True)[1][0].sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="released by its first backward"):
        loss.backward()
    out = scene.render_scene_grad(model, objects, rays, True)
    with torch.no_grad():
        objects[1].latents["articulation"].add_(1e-3)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out[1][0].sum().backward()
    model.zero_grad(set_to_none=True)


# ------------------------------------------------------------------ fit_scene_codes
FIT = dict(H=8, W=12, steps=20, lr=5e-3, amp=0.3, degrees=dict(min_deg_point=0, max_deg_point=3, deg_view=2), seed=2, density_scale=30.0, bias_shift=2.0)


def test_fit_scene_codes(dev):
    """K = 2, one 8 x 12 view, one level of 33 samples, degrees (0, 3, 2) with the density bias lowered by 2 (the smooth field of
    tests/test_hip_ray_grads.py's fit).  The target is rendered with known codes; the start has both articulation codes moved by
    0.3 x N(0, 1); 20 Adam steps at lr 5e-3 on all six codes.  The fp64 loop of the reference restatement alone (tests/_scene_grad_ref.py
    around the oracle's network, on the CPU, the pairs from tests/_scene_ref.py and t from the oracle's fp32 sampler) falls to 0.587 of its
    starting loss with this setting (2.331e-4 -> 1.368e-4), so `losses[-1] < losses[0]` is not marginal; at lr 2e-2 the same loop overshoots
    on nearby codes (ratio above 1)."""
    import aon_amd.synthetic as syn
    from aon_amd import ops
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    deg = (0, 3, 2)
    lit = LitNeRF_AutoDecoder(hparams={"N_max_objs": 2}, randomized=False, white_bkgd=True,
                              model_kwargs=dict(num_levels=1, num_coarse_samples=32, **FIT["degrees"])).to(dev)
    sd = syn.make_art_state_dict(seed=FIT["seed"], density_scale=FIT["density_scale"], **FIT["degrees"])
    sd["coarse_mlp.density_layer.bias"] = sd["coarse_mlp.density_layer.bias"] - FIT["bias_shift"]
    lit.model.load_state_dict(sd)
    lit.code_library.load_state_dict(syn.make_code_library_state(seed=0, n_max_objs=2))
    table = lit.code_library.get_interpolated_articulations(max_interpolations=2, device=dev)
    poses = [(hs.pose(1, (0.35, 0.0, 0.0)), 1.6), (hs.pose(2, (-0.45, 0.1, 0.1)), 1.4)]
    true_art = [table[4].detach().clone(), table[11].detach().clone()]
    rays = hs.to_dev(syn.make_rays(FIT["H"], FIT["W"], hs.CAM, syn.focal_from_fovy(FIT["H"], 30.0)), dev)
    known = [(j, true_art[j], *poses[j]) for j in range(2)]
    target = lit.render_scene(rays, known)["rgb"].clone()
    gen = torch.Generator().manual_seed(5)
    start = [(j, true_art[j] + FIT["amp"] * torch.randn(32, generator=gen).to(dev), *poses[j]) for j in range(2)]
    next(lit.model.coarse_mlp.parameters()).requires_grad_(False)   # a flag the fit must hand back as it found it
    flags = [p.requires_grad for p in lit.model.parameters()]
    before = [p.detach().clone() for p in lit.model.parameters()]
    codes, losses = lit.fit_scene_codes([{**rays, "target": target}], start, FIT["steps"], lr=FIT["lr"])
    assert [p.requires_grad for p in lit.model.parameters()] == flags                        # the flags are restored
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, lit.model.parameters()))   # the network is bit-identical
    assert all(p.grad is None for p in lit.model.parameters())                               # no .grad is left on it
    assert losses.shape == (FIT["steps"],) and losses.device.type == "cuda" and bool(torch.isfinite(losses).all())
    print("fit_scene_codes losses", [f"{x:.4e}" for x in losses.tolist()])
    assert losses[-1].item() < losses[0].item()
    assert len(codes) == 2 and all(tuple(c[k].shape) == (1, w) for c in codes for k, w in (("density", 128), ("color", 128), ("articulation", 32)))
    d0 = [float((start[j][1] - true_art[j]).norm()) for j in range(2)]
    d1 = [float((codes[j]["articulation"].reshape(-1) - true_art[j]).norm()) for j in range(2)]
    print(f"articulation code distance to the truth: {d0} -> {d1}")
    assert all(not torch.equal(codes[j]["articulation"].reshape(-1), start[j][1]) for j in range(2))
    # the first step's loss against the fp64 restatement around the oracle (pairs and t are data: the HIP stages')
    pairs = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], poses)
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, 32, pairs.near, pairs.far, want_coords=False)
    pr = {"o": pairs.rays_o.cpu().numpy(), "d": pairs.rays_d.cpu().numpy(), "v": pairs.viewdirs.cpu().numpy(), "offsets": np.asarray(pairs.starts),
          "slot": pairs.slot.cpu().numpy()}
    lib = lit.code_library

    def first_loss(dtype):
        lat = [{"density": lib.embedding_instance_shape.weight[j: j + 1].detach().cpu().to(dtype),
                "color": lib.embedding_instance_appearance.weight[j: j + 1].detach().cpu().to(dtype), "articulation": start[j][1].cpu().reshape(1, 32).to(dtype)}
               for j in range(2)]
        out = gref.scene_level_oracle({k: v.to(dtype) for k, v in sd.items()}, "coarse_mlp.", pr, t.cpu().numpy(), lat, rays["rays_d"].cpu().numpy(), True,
                                      dtype, deg)
        reg = 1e-4 * sum(torch.mean(torch.norm(v, dim=0)) for c in lat for v in c.values())
        return float(torch.mean((out["rgb"] - target.cpu().to(dtype)) ** 2) + reg)

    loss64, loss32 = first_loss(torch.float64), first_loss(torch.float32)
    bar = max(5.0 * abs(loss32 - loss64), 2e-6 * abs(loss64))
    print(f"first loss: hip {losses[0].item():.7e} fp64 {loss64:.7e} fp32 {loss32:.7e} bar {bar:.1e}")
    assert abs(losses[0].item() - loss64) <= bar
