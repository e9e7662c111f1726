"""GPU: pose gradients of scenes (csrc/aon_scene_pose.hip, csrc/aon_ray_grad.hip, include/aon_hip_scene_pose.h).

aon_art_ray_grads against an fp64 evaluation of the same formulas from the read-back chain outputs (tests/_scene_pose_ref.ray_grads_fp64), bar
(130 + S) 2^-24 sum|products| per output (a 128-term fp32 fmaf chain, one add, then fp64 sums rounded once); the reduce alone against fp64
sums of the kernel's own records, one fp32 ulp.  aon_scene_pose_grads on random per-pair gradients against numpy fp64, bar
2^-24 |ref| + 1e-12 sum|terms|.  Bits: repeats, a side stream, another object's pairs, permuted and sub-batched blocks.  Memory: guard bands,
the capacity tail.  One level against the oracle's autograd (tests/_gradcheck.py); the whole path against scene.render_scene and the chain
written out with stage calls; LitNeRF_AutoDecoder.fit_scene_poses."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _guard  # noqa: E402
import _scene_pose_ref as pref  # noqa: E402
import test_hip_scene as hs  # noqa: E402
import test_hip_scene_grad as hsg  # noqa: E402
from test_hip_extents import Case, run_case  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("density", "color", "articulation")
F = np.float32
ROW_D0, ROW_V0 = 32, 2944      # aplane_d(0), aplane_v(0) (csrc/aon_common.h)
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------ aon_art_ray_grads
_NETS: dict = {}


def network(dev, dv):
    import aon_amd.synthetic as syn
    from aon_amd import ops

    if dv not in _NETS:
        sd = syn.make_art_state_dict(seed=2, density_scale=10.0, deg_view=dv)
        params = {k[len("fine_mlp."):]: v.to(dev) for k, v in sd.items() if k.startswith("fine_mlp.")}
        degrees = (0, 10, dv)
        _NETS[dv] = (params, degrees, ops.pack_art_mlp(params, degrees=degrees), ops.pack_art_mlp_bwd(params, degrees=degrees))
    return _NETS[dv]


def block_inputs(n, S, seed=0):
    """rays, sorted t in [2, 6] and upstream d_raw rows, all named by the ray"""
    import aon_amd.synthetic as syn

    r = syn.random_rays(n, seed=11 + seed)
    t = torch.sort(2.0 + 4.0 * syn.seeded_uniform(70 + seed, n, S), dim=1).values.contiguous()
    d_raw = (syn.seeded_uniform(90 + seed, n, S, 4) - 0.5).contiguous()
    return {"rays_o": r["rays_o"], "rays_d": r["rays_d"], "viewdirs": r["viewdirs"], "t": t, "d_raw": d_raw}


def run_block(dev, dv, inp):
    """forward -> chain -> aon_art_ray_grads on one block -> (outputs, dplanes, dxp, records)"""
    from aon_amd import ops

    params, degrees, packed, packed_bwd = network(dev, dv)
    o, d, v, t = (inp[k].to(dev) for k in ("rays_o", "rays_d", "viewdirs", "t"))
    n, S = t.shape
    small = ops.art_prepare(params, hs.codes(dev, 1), degrees=degrees)
    _, planes, masks = ops.art_mlp_fwd_train(packed, small, o, d, v, t)
    d_seg = torch.zeros((ops.plane_samples(planes), 4), device=dev)
    d_seg[: n * S] = inp["d_raw"].to(dev).reshape(n * S, 4)
    dplanes, dxp = ops.art_bwd_chain(packed_bwd, small, d_seg, masks, planes)
    got = ops.art_ray_grads(dplanes, dxp, params, t, v, degrees)
    rec = ops._scratch(ops._RAY_REC, dev, n * S * 128)[: n * S * 128].view(torch.float32).reshape(n * S, 32).clone()
    torch.cuda.synchronize()
    return got, dplanes, dxp, rec


SHAPES = [(1, 2), (5, 3), (3, 7), (4, 8), (9, 65), (2, 193)]      # (9, 65): 585 samples, a partial 32-sample step and a partial 256-thread block


@pytest.mark.parametrize("dv", [4, 2, 0])
@pytest.mark.parametrize("n,S", SHAPES)
def test_ray_grads_against_fp64(dev, n, S, dv):
    from aon_amd import ops

    inp = block_inputs(n, S)
    got, dplanes, dxp, _ = run_block(dev, dv, inp)
    params = network(dev, dv)[0]
    rows = ops.plane_rows_view(dplanes)
    ref = pref.ray_grads_fp64(rows[ROW_D0: ROW_D0 + 128].cpu().numpy(), rows[ROW_V0: ROW_V0 + 128].cpu().numpy(), dxp.cpu().numpy(),
                              params["deformations_linear.0.weight"].cpu().numpy(), params["views_linear.0.weight"].cpu().numpy(),
                              inp["t"].numpy(), inp["viewdirs"].numpy(), dv)
    for x, key in zip(got, ("o", "d", "v")):
        x = x.cpu().double().numpy()
        assert x.shape == (n, 3) and np.isfinite(x).all()
        bar = (130 + S) * U * ref["abs_" + key]
        err = np.abs(x - ref["g_" + key])
        print(f"n={n} S={S} deg_view={dv} g_{key}: max|g| {np.abs(ref['g_' + key]).max():.3e}, worst err / bar {float((err / np.maximum(bar, 1e-300)).max()):.3f}")
        assert np.abs(ref["g_" + key]).max() > 1e-6
        assert (err <= bar).all(), key


def _fma(a, b, c):
    return F(np.float64(a) * np.float64(b) + np.float64(c))


def cos_f32(x):
    """csrc/aon_common.h's cos_f32, operation by operation, for |x| < 2^19 (beyond, the kernels' function takes the exact quadrant reduction;
    the view encodings this copy is used on stay below 2^3 + pi/2)"""
    h = float.fromhex
    ax = F(abs(F(x)))
    assert ax < F(2.0 ** 19)
    k = F(np.rint(F(ax * F(0.636619747))))
    q = int(k)
    r = _fma(k, F(-h("0x1.921fb4p+0")), ax)
    r = _fma(k, F(-h("0x1.4442d0p-24")), r)
    r = _fma(k, F(-h("0x1.846988p-48")), r)
    z = F(r * r)
    ps = _fma(z, F(-1.9515295891e-4), F(8.3321608736e-3))
    ps = _fma(z, ps, F(-1.6666654611e-1))
    s = _fma(F(r * z), ps, r)
    pc = _fma(z, F(2.443315711809948e-5), F(-1.388731625493765e-3))
    pc = _fma(z, pc, F(4.166664568298827e-2))
    c = _fma(F(z * z), pc, _fma(z, F(-0.5), F(1.0)))
    res = s if q & 1 else c
    return F(-res) if (q + 1) & 2 else res


@pytest.mark.parametrize("n,S,dv", [(9, 65, 4), (3, 7, 2), (2, 193, 0)])
def test_the_reduce_alone_is_the_fp64_sum_of_its_records(dev, n, S, dv):
    inp = block_inputs(n, S, seed=1)
    got, _, _, rec = run_block(dev, dv, inp)
    rec = rec.cpu().double().numpy().reshape(n, S, 32)
    assert not rec[..., 30:].any() and rec[..., :3].any()
    t = inp["t"].double().numpy()
    want = {"o": rec[..., :3].sum(1), "d": (t[..., None] * rec[..., :3]).sum(1)}
    part = rec[..., 3: 3 + 3 + 6 * dv].sum(1)
    want["v"] = np.stack([pref.view_backward(part[r], inp["viewdirs"][r].numpy(), dv, cos=cos_f32)[0] for r in range(n)])
    for x, key in zip(got, ("o", "d", "v")):
        x = x.cpu().numpy()
        ulp = np.spacing(np.abs(want[key]).astype(F)).astype(np.float64)
        assert (np.abs(x.astype(np.float64) - want[key]) <= ulp).all(), key


def test_ray_grad_rows_do_not_depend_on_the_block(dev):
    """a ray's three rows under a permutation of the block and in a sub-batch of it: the same bits; and on every run"""
    n, S, dv = 9, 65, 4
    inp = block_inputs(n, S, seed=2)
    base = [x.cpu() for x in run_block(dev, dv, inp)[0]]
    again = [x.cpu() for x in run_block(dev, dv, inp)[0]]
    perm = torch.from_numpy(np.random.default_rng(1).permutation(n))
    permuted = [x.cpu() for x in run_block(dev, dv, {k: v[perm].contiguous() for k, v in inp.items()})[0]]
    sub = [x.cpu() for x in run_block(dev, dv, {k: v[2:7].contiguous() for k, v in inp.items()})[0]]
    for a, b, p, s in zip(base, again, permuted, sub):
        assert a.any()
        assert torch.equal(_guard.bits(a), _guard.bits(b))
        assert torch.equal(_guard.bits(a[perm]), _guard.bits(p))
        assert torch.equal(_guard.bits(a[2:7]), _guard.bits(s))


# ------------------------------------------------------------------ aon_scene_pose_grads
def fake_pairs(dev, n, counts, seed):
    """a ScenePairs with the given segment lengths: ascending world rays inside each object (as aon_scene_pairs lays them out)"""
    from aon_amd import ops

    rng = np.random.default_rng(seed)
    K, P = len(counts), int(sum(counts))
    ray = np.concatenate([np.sort(rng.choice(n, c, replace=False)) for c in counts] + [np.zeros(0, np.int64)]).astype(np.int32)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64, device=dev)
    e = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)   # noqa: E731
    return ops.ScenePairs(n, K, offsets, [int(c) for c in counts], e(n, K, dtype=torch.int32), torch.from_numpy(ray).to(dev), e(P, 3), e(P, 3), e(P, 3), e(P), e(P))


def pose_case(dev, counts, seed):
    import aon_amd.synthetic as syn

    n = 300
    rays = syn.random_rays(n, seed=seed)
    objects = [(hs.pose(50 + k, (0.3 * np.cos(k), 0.2 * np.sin(k), 0.1 * k - 0.4)), 1.0) for k in range(len(counts))]
    pairs = fake_pairs(dev, n, counts, seed)
    g = [torch.from_numpy(np.random.default_rng(seed + 1 + i).normal(size=(pairs.P, 3)).astype(F)) for i in range(3)]
    return rays, objects, pairs, g


def pose_reference(rays, objects, pairs, g):
    ray = pairs.ray.cpu().numpy()
    out, scale = np.zeros((pairs.K, 12)), np.zeros((pairs.K, 12))
    for k, (pose, _) in enumerate(objects):
        seg = pairs.segment(k)
        idx = ray[seg]
        g_R, g_c, a = pref.pose_grads_closed(pose.numpy(), rays["rays_o"].numpy()[idx], rays["rays_d"].numpy()[idx], rays["viewdirs"].numpy()[idx],
                                             g[0].numpy()[seg], g[1].numpy()[seg], g[2].numpy()[seg])
        out[k], scale[k] = np.concatenate([g_R.reshape(-1), g_c]), a
    return out, scale


def pose_call(dev, rays, objects, pairs, g):
    from aon_amd import ops
    return ops.scene_pose_grads(rays["rays_o"].to(dev), rays["rays_d"].to(dev), rays["viewdirs"].to(dev), pairs, objects, *[x.to(dev) for x in g])


@pytest.mark.parametrize("counts", [(0, 1, 5), (255, 256, 257), (2,) * 16, (0,)], ids=["0_1_5", "255_256_257", "k16", "no_pairs"])
def test_pose_grads_against_fp64(dev, counts):
    rays, objects, pairs, g = pose_case(dev, counts, seed=7)
    got = pose_call(dev, rays, objects, pairs, g).cpu().double().numpy()
    ref, scale = pose_reference(rays, objects, pairs, g)
    assert got.shape == (len(counts), 12)
    bar = U * np.abs(ref) + 1e-12 * scale
    print(f"counts {counts}: worst err / bar {float((np.abs(got - ref) / np.maximum(bar, 1e-300)).max()):.3f}")
    assert (np.abs(got - ref) <= bar).all()
    for k, c in enumerate(counts):
        if c == 0:
            assert not got[k].any() and not np.signbit(got[k][:9]).any()           # twelve exact zeros
        else:
            assert got[k].all()


def test_pose_grad_bits(dev):
    """every run, a side stream while the default stream is busy, and another object's pairs"""
    counts = (255, 256, 257)
    rays, objects, pairs, g = pose_case(dev, counts, seed=8)
    base = pose_call(dev, rays, objects, pairs, g)
    torch.cuda.synchronize()
    assert torch.equal(_guard.bits(base), _guard.bits(pose_call(dev, rays, objects, pairs, g)))
    from aon_amd import ops
    on_dev = [rays[k].to(dev) for k in ("rays_o", "rays_d", "viewdirs")] + [x.to(dev) for x in g]
    call = lambda: ops.scene_pose_grads(*on_dev[:3], pairs, objects, *on_dev[3:])      # noqa: E731
    # a stream may share its hardware queue with the default stream (4 queues per process): of four streams at least one does not
    busy = hasattr(torch.cuda, "_sleep")
    overlapped = []
    for _ in range(4):
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            call()                                  # the side stream's own blocks exist before the gate: no allocation of the device's inside it
        torch.cuda.synchronize()
        if busy:
            torch.cuda._sleep(int(2.4e6 * 60))      # about 60 ms of the default stream
        gate = torch.cuda.Event()
        gate.record()
        with torch.cuda.stream(side):
            got = call()
        side.synchronize()
        overlapped.append(not gate.query())
        torch.cuda.synchronize()
        assert torch.equal(_guard.bits(got), _guard.bits(base))
    if busy:
        assert any(overlapped), "every side stream's call waited for the default stream"
    # object 1 loses 100 of its pairs and the rest get other gradients: rows 0 and 2 keep their bits
    keep = np.concatenate([np.arange(255), 255 + np.arange(156), 511 + np.arange(257)])
    p2 = fake_pairs(dev, 300, (255, 156, 257), 8)
    p2.ray.copy_(pairs.ray[torch.from_numpy(keep).to(dev)])
    g2 = [x[keep].clone() for x in g]
    for x in g2:
        x[255: 255 + 156] *= -1.5
    other = pose_call(dev, rays, objects, p2, g2)
    assert torch.equal(_guard.bits(other[0]), _guard.bits(base[0])) and torch.equal(_guard.bits(other[2]), _guard.bits(base[2]))
    assert not torch.equal(other[1], base[1])


def test_pose_grads_capacity_tail(dev):
    """per-pair arrays at their capacity n * K rows (rows from P on hold NaN / -1) and a g_pose with a row to spare: the same bits, the spare
    row untouched; the NULL stream and the current stream agree"""
    from aon_amd import ops

    counts = (0, 1, 5)
    rays, objects, pairs, g = pose_case(dev, counts, seed=9)
    want = pose_call(dev, rays, objects, pairs, g)
    torch.cuda.synchronize()
    arr, K = ops._scene_objects(objects)
    cap = 900
    ray = torch.full((cap,), -1, dtype=torch.int32, device=dev)
    ray[: pairs.P] = pairs.ray
    gs = [torch.full((cap, 3), float("nan"), device=dev) for _ in range(3)]
    for dst, src in zip(gs, g):
        dst[: pairs.P] = src.to(dev)
    o, d, v = (rays[k].to(dev) for k in ("rays_o", "rays_d", "viewdirs"))
    for stream in (None, C.c_void_p(torch.cuda.current_stream().cuda_stream)):
        out = torch.full((K + 1, 12), -7.25, device=dev)
        ops.check(ops.lib.aon_scene_pose_grads(o.data_ptr(), d.data_ptr(), v.data_ptr(), 300, ray.data_ptr(), pairs.offsets.data_ptr(), arr, K, pairs.P,
                                               gs[0].data_ptr(), gs[1].data_ptr(), gs[2].data_ptr(), out.data_ptr(), stream), "aon_scene_pose_grads")
        torch.cuda.synchronize()
        assert bool((out[K] == -7.25).all()) and torch.equal(_guard.bits(out[:K]), _guard.bits(want))


# ------------------------------------------------------------------ memory
def _guard_case(name, n, S, dv, counts):
    def make(dev):
        inp = {k: v.to(dev) for k, v in block_inputs(n, S, seed=3).items()}
        rays, objects, pairs, g = pose_case(dev, counts, seed=10)
        return {"block": inp, "rays": hs.to_dev(rays, dev), "objects": objects, "pair_ray": pairs.ray, "offsets": pairs.offsets, "g": [x.to(dev) for x in g]}

    def call(ops, i):
        params, degrees, packed, packed_bwd = network(i["block"]["t"].device, dv)
        b = i["block"]
        small = ops.art_prepare(params, hs.codes(b["t"].device, 1), degrees=degrees)
        _, planes, masks = ops.art_mlp_fwd_train(packed, small, b["rays_o"], b["rays_d"], b["viewdirs"], b["t"])
        d_seg = torch.zeros((ops.plane_samples(planes), 4), device=b["t"].device)
        d_seg[: n * S] = b["d_raw"].reshape(n * S, 4)
        dplanes, dxp = ops.art_bwd_chain(packed_bwd, small, d_seg, masks, planes)
        ops._RAY_REC.clear()                                   # the records come from the guarded allocator, at their exact size
        outs = list(ops.art_ray_grads(dplanes, dxp, params, b["t"], b["viewdirs"], degrees))
        ops._RAY_REC.clear()
        dev = b["t"].device
        e = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)   # noqa: E731
        P = int(sum(counts))
        pairs = ops.ScenePairs(300, len(counts), i["offsets"], [int(c) for c in counts], e(1, len(counts), dtype=torch.int32), i["pair_ray"], e(P, 3), e(P, 3),
                               e(P, 3), e(P), e(P))
        r = i["rays"]
        return outs + [ops.scene_pose_grads(r["rays_o"], r["rays_d"], r["viewdirs"], pairs, i["objects"], *i["g"])]
    return Case("scene_pose", name, make, call, ["aon_art_ray_grads", "aon_scene_pose_grads"])


GUARD_CASES = [_guard_case("scene_pose_n5_s3", 5, 3, 2, (0, 1, 5)), _guard_case("scene_pose_n9_s65", 9, 65, 4, (255, 256, 257))]


@pytest.mark.parametrize("c", GUARD_CASES, ids=[c.name for c in GUARD_CASES])
def test_memory_contract(dev, monkeypatch, c):
    run_case(c, dev, monkeypatch)


# ------------------------------------------------------------------ one level through the network
def _level_check(dev, setup, t, what):
    from _gradcheck import assert_as_close_as_fp32
    from aon_amd import ops
    from aon_amd.autograd import RenderLevelScene, RenderLevelScenePoses

    sd, prefix, params, rays_cpu, rays, pairs, codes = setup
    specs = [hs.nested(0, 0), hs.nested(3, 1)]
    n = 24
    gen = torch.Generator().manual_seed(31)
    target, w = torch.rand(n, 3, generator=gen), torch.rand(n, 4, generator=gen)
    pair_ray, starts, slot = pairs.ray.cpu().numpy(), np.asarray(pairs.starts), pairs.slot.cpu().numpy()
    rays_np = {k: v.numpy() for k, v in rays_cpu.items()}

    def oracle(dtype):
        sd_o = {k: v.detach().to(dtype) for k, v in sd.items() if k.startswith(prefix)}
        lat_o = [{k: v.to(dtype) for k, v in c.items()} for c in codes]
        leaves = [p.to(dtype).clone().requires_grad_(True) for p, _ in specs]
        po, pd, pv = pref.pair_rays(leaves, rays_np, pair_ray, starts, round32=dtype == torch.float64)
        out = pref.scene_level_oracle_t(sd_o, prefix, po, pd, pv, starts, slot, t.cpu().numpy(), lat_o, rays_np["rays_d"], True, dtype)
        hsg._level_loss((out["rgb"], out["acc"], out["depth"], out["obj_acc"]), target.to(dtype), w.to(dtype)).backward()
        return {f"pose{j}": p.grad for j, p in enumerate(leaves)}

    g64, g32 = oracle(torch.float64), oracle(torch.float32)

    def run(fn, with_poses):
        leaves = [p.clone().requires_grad_(True) for p in (params[name] for name in ops.ART_PARAM_ORDER)]
        lat = [{k: c[k].to(dev).requires_grad_(True) for k in KEYS} for c in codes]
        pd_ = dict(zip(ops.ART_PARAM_ORDER, leaves))
        poses = [p.clone().requires_grad_(True) for p, _ in specs]
        head = (pairs, t, rays["rays_o"], rays["rays_d"], rays["viewdirs"], specs) if with_poses else (pairs, t, rays["rays_d"])
        out = fn.apply(*head, True, None, ops.pack_art_mlp(pd_), ops.pack_art_mlp_bwd(pd_), (0, 10, 4), *(poses if with_poses else []),
                       *[c[k] for c in lat for k in KEYS], *leaves)
        hsg._level_loss(out[:4], target.to(dev), w.to(dev)).backward()
        return out, poses, [c[k].grad for c in lat for k in KEYS] + [p.grad for p in leaves]

    out, poses, rest = run(RenderLevelScenePoses, True)
    out0, _, rest0 = run(RenderLevelScene, False)
    for a, b in zip(out, out0):
        assert torch.equal(_guard.bits(a.detach()), _guard.bits(b.detach()))              # RenderLevelScene's forward, bit for bit
    assert len(rest) == 46
    for i, (a, b) in enumerate(zip(rest, rest0)):
        assert torch.equal(_guard.bits(a), _guard.bits(b)), i                               # and its code and parameter gradients
    got = {f"pose{j}": p.grad for j, p in enumerate(poses)}
    assert all(g is not None and tuple(g.shape) == (3, 4) and g.device.type == "cpu" and bool(torch.isfinite(g).all()) and bool(g.any()) for g in got.values())
    assert_as_close_as_fp32(got, g64, g32, what)
    return out[4].detach()


@pytest.mark.parametrize("S", [65, 9])
def test_one_level_against_the_oracles_autograd(dev, S):
    from aon_amd import ops

    setup = hsg._level_setup(dev)
    pairs = setup[5]
    assert pairs.counts[0] > 0 and pairs.counts[1] > 0
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, S - 1, pairs.near, pairs.far, want_coords=False)
    weights = _level_check(dev, setup, t, f"scene level poses, S = {S}, sampler's t")
    t2 = ops.sample_pdf_t_n(t, weights, 16)
    _level_check(dev, setup, t2, f"scene level poses, S = {S} + 16, inverse-CDF t")


# ------------------------------------------------------------------ the whole path
def _pose_objects(dev, specs, code_grads=False):
    from aon_amd import scene
    return [scene.SceneObject({k: v.clone().requires_grad_(code_grads) for k, v in hs.codes(dev, j).items()}, p.clone().requires_grad_(True), b)
            for j, (p, b) in enumerate(specs)]


def _written_out_pose_grads(model, objects, rays, target):
    """render_scene_grad's forward and pose backward with stage-level ops calls; the loss's own derivative from torch on detached leaves"""
    from aon_amd import ops

    pairs = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], objects)
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, model.num_coarse_samples, pairs.near, pairs.far, want_coords=False)
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
        outs.append([x.detach().requires_grad_(True) for x in (rgb, acc, depth, obj_acc)])
        kept.append((mlp, params, raw, t, per))
        if level + 1 < model.num_levels:
            t = ops.sample_pdf_t_n(t, weights, model.num_fine_samples)
    up = torch.autograd.grad(hsg._scene_loss(outs, target), [x for lv in outs for x in lv])
    total = None
    for level, (mlp, params, raw, t, per) in enumerate(kept):
        g_rgb, g_acc, g_depth, g_obj = up[4 * level: 4 * level + 4]
        d_raw = ops.scene_composite_bwd(raw, t, pairs, rays["rays_d"], g_rgb, g_acc, g_depth, g_obj, True, opts=model._opts)
        bwd = mlp.packed_bwd(True)
        g = torch.zeros((3, pairs.P, 3), device=t.device)
        for k in range(len(objects)):
            if per[k] is None:
                continue
            small, planes, masks = per[k]
            seg = pairs.segment(k)
            rows = (seg.stop - seg.start) * t.shape[1]
            buf = torch.zeros((ops.padded_samples(rows), 4), device=t.device)
            buf[:rows] = d_raw[seg].reshape(rows, 4)
            dplanes, dxp = ops.art_bwd_chain(bwd, small, buf, masks, planes)
            for dst, x in zip(g, ops.art_ray_grads(dplanes, dxp, params, t[seg], pairs.viewdirs[seg], mlp.degrees)):
                dst[seg] = x
        g_pose = ops.scene_pose_grads(rays["rays_o"], rays["rays_d"], rays["viewdirs"], pairs, objects, g[0], g[1], g[2]).cpu()
        total = g_pose if total is None else total + g_pose
    return [torch.cat([total[k, :9].view(3, 3), total[k, 9:].view(3, 1)], 1) for k in range(len(objects))]


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("levels", [1, 2])
def test_render_scene_grad_with_pose_leaves(dev, levels, K, monkeypatch):
    from aon_amd import ops, scene

    model = hs.art_model(dev, levels, 16, 16)
    rays = hsg._frame(dev)
    target = hs._syn().seeded_uniform(21, 96, 3).to(dev)
    objects = _pose_objects(dev, hsg.SPECS[K]())
    with torch.no_grad():
        want = scene.render_scene(model, objects, rays, True)
    calls = []
    real = ops.art_wgrad
    monkeypatch.setattr(ops, "art_wgrad", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    flags = [p.requires_grad for p in model.parameters()]
    try:
        for p in model.parameters():
            p.requires_grad_(False)
        got = scene.render_scene_grad(model, objects, rays, True)
        for g, w in zip(got, want):
            for a, b in zip(g, w):
                assert torch.equal(_guard.bits(a.detach()), _guard.bits(b))                 # render_scene's forward, bit for bit
        grads = torch.autograd.grad(hsg._scene_loss(got, target), [ob.pose_tensor for ob in objects])
        assert not calls                                                                    # poses only: no weight-gradient stage
        ref = _written_out_pose_grads(model, objects, rays, target)
        for k, (a, b) in enumerate(zip(grads, ref)):
            assert tuple(a.shape) == (3, 4) and bool(torch.isfinite(a).all()) and bool(a.any()), k
            assert torch.equal(_guard.bits(a), _guard.bits(b)), k                           # the written-out chain, bit for bit
        # with a code that needs its gradient the weight-gradient stage runs, and the pose gradients keep their bits
        more = _pose_objects(dev, hsg.SPECS[K](), code_grads=True)
        lv = scene.render_scene_grad(model, more, rays, True)
        both = torch.autograd.grad(hsg._scene_loss(lv, target), [ob.pose_tensor for ob in more] + [more[0].latents["articulation"]])
        assert calls and bool(both[-1].any())
        for a, b in zip(both[:K], grads):
            assert torch.equal(_guard.bits(a), _guard.bits(b))
    finally:
        for p, f in zip(model.parameters(), flags):
            p.requires_grad_(f)
    # without a pose tensor: the path of section 4.18
    plain = hsg._leaf_objects(dev, hsg.SPECS[K]())
    assert all(ob.pose_tensor is None for ob in plain)
    lv = scene.render_scene_grad(model, plain, rays, True)
    assert type(lv[0][0].grad_fn).__name__.startswith("RenderLevelSceneBackward")


# ------------------------------------------------------------------ fit_scene_poses
FIT = dict(H=8, W=12, steps=200, lr=2e-3, degrees=dict(min_deg_point=0, max_deg_point=3, deg_view=2), seed=2, density_scale=30.0, bias_shift=3.0,
           boxes=(2.4, 2.1), corrections=([0.020, -0.025, 0.015, 0.03, -0.03, 0.025], [-0.022, 0.018, 0.02, -0.025, 0.035, 0.025]))


def pose_errors(p, q):
    """(rotation angle in degrees, translation distance) between two (3, 4) poses"""
    p, q = p.detach().cpu().double(), q.detach().cpu().double()
    c = torch.clamp((torch.trace(p[:, :3] @ q[:, :3].T) - 1.0) / 2.0, -1.0, 1.0)
    return float(torch.rad2deg(torch.acos(c))), float((p[:, 3] - q[:, 3]).norm())


def test_fit_scene_poses_recovers_perturbed_poses(dev):
    """K = 2, one 8 x 12 frame, one level of 33 samples, from poses perturbed by 2.03 / 1.99 degrees and 0.0492 / 0.0497.  The field: the seeded
    weights at encoding degrees (0, 3, 2) with the density bias lowered by 3, boxes of side 2.4 and 2.1.  The boxes matter: a box's faces cut
    the field, and near / far are data, so a box tight around dense space (sides 1.6 / 1.4, bias lowered by 2 -- the first choice) shows faces
    whose motion the gradient does not see; there the oracle's own fp64 loop ends at 1.30 / 2.59 and 0.84 / 0.61 of the starting rotation /
    translation errors after 60 steps at lr 5e-3 (and at 0.53 / 0.83, 0.39 / 0.24 with the bias lowered by 4 and 120 steps at 2e-3).  With this
    field the fp64 oracle loop on the CPU (tests/_scene_pose_ref.fit_poses_oracle, same Adam, lr 2e-3, 200 steps) ends at 0.0100 / 0.0744 and
    0.0093 / 0.0056 of the starting errors: below a quarter.
    Here: the first 8 losses against that loop in fp64 and fp32, bar max(2 |oracle32 - oracle64|, 5e-5) per step; both errors of both objects
    end below half their start; parameters and flags come back untouched."""
    import aon_amd.synthetic as syn
    from aon_amd import ops
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    lit = LitNeRF_AutoDecoder(hparams={"N_max_objs": 2}, randomized=False, white_bkgd=True,
                              model_kwargs=dict(num_levels=1, num_coarse_samples=32, **FIT["degrees"])).to(dev)
    sd = syn.make_art_state_dict(seed=FIT["seed"], density_scale=FIT["density_scale"], **FIT["degrees"])
    sd["coarse_mlp.density_layer.bias"] = sd["coarse_mlp.density_layer.bias"] - FIT["bias_shift"]
    lit.model.load_state_dict(sd)
    lit.code_library.load_state_dict(syn.make_code_library_state(seed=0, n_max_objs=2))
    true = [hs.pose(1, (0.35, 0.0, 0.0)), hs.pose(2, (-0.45, 0.1, 0.1))]
    start = [ops.apply_pose_correction(p.double(), torch.tensor(c, dtype=torch.float64)).float() for p, c in zip(true, FIT["corrections"])]
    arts = (4, 11)
    rays_cpu = syn.make_rays(FIT["H"], FIT["W"], hs.CAM, syn.focal_from_fovy(FIT["H"], 30.0))
    rays = hs.to_dev(rays_cpu, dev)
    target = lit.render_scene(rays, [(j, arts[j], true[j], FIT["boxes"][j]) for j in range(2)])["rgb"].clone()
    placements = [(j, arts[j], start[j], FIT["boxes"][j]) for j in range(2)]
    next(lit.model.coarse_mlp.parameters()).requires_grad_(False)   # a flag the fit must hand back as it found it
    flags = [p.requires_grad for p in lit.model.parameters()]
    before = [p.detach().clone() for p in lit.model.parameters()]
    poses, codes, losses = lit.fit_scene_poses([{**rays, "target": target}], placements, FIT["steps"], FIT["lr"])
    assert [p.requires_grad for p in lit.model.parameters()] == flags
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, lit.model.parameters())) and all(p.grad is None for p in lit.model.parameters())
    assert losses.shape == (FIT["steps"],) and losses.device.type == "cuda" and bool(torch.isfinite(losses).all())
    placed = lit._placement_codes("test", placements)
    assert all(torch.equal(codes[j][k], placed[j][2][k].detach().reshape(1, -1)) for j in range(2) for k in KEYS)      # fit_codes off: as given
    e0 = [pose_errors(s, t) for s, t in zip(start, true)]
    e1 = [pose_errors(p, t) for p, t in zip(poses, true)]
    print(f"fit_scene_poses: (degrees, distance) {e0} -> {e1}; losses {[f'{x:.4e}' for x in losses[:8].tolist()]} ... {losses[-1].item():.4e}")
    assert all(1.9 < a < 2.2 and 0.045 < b < 0.055 for a, b in e0)
    lat = [{k: v.detach().cpu() for k, v in p[2].items()} for p in placed]
    rays_np = {k: v.numpy() for k, v in rays_cpu.items()}
    l64, _ = pref.fit_poses_oracle(sd, "coarse_mlp.", rays_np, target.cpu().numpy(), start, FIT["boxes"], lat, 8, FIT["lr"], torch.float64, (0, 3, 2), 32)
    l32, _ = pref.fit_poses_oracle(sd, "coarse_mlp.", rays_np, target.cpu().numpy(), start, FIT["boxes"], lat, 8, FIT["lr"], torch.float32, (0, 3, 2), 32)
    hip8 = losses[:8].tolist()
    for i in range(8):
        bar = max(2.0 * abs(l32[i] - l64[i]), 5e-5)
        print(f"step {i}: hip {hip8[i]:.6e} oracle64 {l64[i]:.6e} oracle32 {l32[i]:.6e} bar {bar:.1e}")
        assert abs(hip8[i] - l64[i]) <= bar, (i, hip8[i], l64[i], bar)
    for a, b in zip(e0, e1):
        assert b[0] < 0.5 * a[0] and b[1] < 0.5 * a[1], (e0, e1)
    # with the codes fitted too: both buffers move, the loss falls
    poses2, codes2, losses2 = lit.fit_scene_poses([{**rays, "target": target}], placements, 12, (2e-3, 5e-3), fit_codes=True)
    assert all(not torch.equal(codes2[j][k], codes[j][k]) for j in range(2) for k in KEYS) and not torch.equal(poses2[0].cpu(), start[0])
    assert bool(torch.isfinite(losses2).all()) and losses2[-1].item() < losses2[0].item()
