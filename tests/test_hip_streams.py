"""GPU: the stream contract.  Every other GPU test enqueues on torch's default (null) stream from one host thread; the library promises
that every call "enqueues on the caller's current stream", owns side streams it forks from / joins to that stream, keeps its scratch
per (device, stream) (ops.StreamCache) and its error text per thread.  Here the same calls run on non-default streams, on two streams at
once and from two host threads.

Every comparison is torch.equal against the same call made serially on the default stream: the kernels give the same bits on the same
inputs (test_gradient_bits_are_pinned, the chunking / fusion equalities), so the tolerance is zero.

(a) ordering probe: on a stream S a device-side delay is enqueued, then -- still on S -- inputs and parameters are overwritten in place
    from a batch B0 to a batch B1, then the op runs on S.  A launch that is not ordered behind S (left on the null stream, forked from the
    wrong place) reads B0; a side stream that is not joined back lets the output copy run early.  Non-vacuity is asserted: an event recorded
    on S right after the call returns must still be pending (the delay is still running), and B0 / B1 must give different outputs.
(b) two streams, two different jobs released together; each equals its own serial result and their intervals overlapped (asserted).
(c) two host threads, each with its own stream and model, three training steps; the error text is thread-local.
(d) the pool and the caches on the device.

The two-stream cases are only meaningful with the per-stream caches: the evidence that they discriminate is the CPU mutation check
(tests/test_stream_cache_cpu.py::test_parent_rule_aliases) plus the data_ptr() assertions of (d); a shared workspace is never raced here."""
import threading
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

NEAR, FAR = 2.0, 6.0
# Length of the device-side delay in front of every probe.  The delay primitive is calibrated per session (`delay` fixture).  Measured on
# one MI355X: torch.cuda._sleep runs 2,398,939 cycles per ms (the 2.4 GHz shader clock); asked for 60.0 ms it took 60.0 ms.  With it,
# every probe found its event still pending when the call returned, and in (b) the host had enqueued both jobs (the longest: a 768-ray
# articulated forward + backward beside a 6000-ray render) while the gate was still closed: the jobs started 59.7 ms after the delay did.
DELAY_MS = 60.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from aon_amd import ops as _ops

    return _ops


def _timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _make_delay(dev):
    """-> (enqueue(ms): a device-side delay of about `ms` on the current stream, description)."""
    if hasattr(torch.cuda, "_sleep"):
        probe = 20_000_000
        torch.cuda._sleep(1000)
        ms = min(_timed(lambda: torch.cuda._sleep(probe), dev) for _ in range(2))
        per_ms = probe / max(ms, 1e-3)
        return (lambda want: torch.cuda._sleep(int(per_ms * want))), f"torch.cuda._sleep, {per_ms:.0f} cycles per ms"
    x = torch.rand(4096, 4096, device=dev)
    x @ x
    ms = min(_timed(lambda: x @ x, dev) for _ in range(2))

    def chain(want):
        for _ in range(max(1, int(want / ms + 1))):
            x @ x

    return chain, f"4096^3 matmul chain, {ms:.3f} ms each"


@pytest.fixture(scope="module")
def delay(dev):
    enqueue, what = _make_delay(dev)
    got = _timed(lambda: enqueue(DELAY_MS), dev)
    print(f"\n[streams] delay primitive: {what}; asked {DELAY_MS} ms, measured {got:.1f} ms")
    assert 0.6 * DELAY_MS <= got <= 3.0 * DELAY_MS, f"delay primitive: asked {DELAY_MS} ms, got {got:.1f} ms ({what})"
    return enqueue


# ------------------------------------------------------------------ inputs
def _syn():
    import aon_amd.synthetic as syn

    return syn


def _u(seed, *shape, lo=0.0, hi=1.0):
    return _syn().seeded_uniform(seed, *shape) * (hi - lo) + lo


class State:
    """Live device tensors with two valid contents each: batch 0 and batch 1, all contiguous fp32 / int64 on the device up front."""

    def __init__(self, dev):
        self.dev, self.items = dev, []

    def add(self, b0, b1, live=None):
        b0, b1 = b0.to(self.dev).contiguous(), b1.to(self.dev).contiguous()
        assert b0.shape == b1.shape and b0.dtype == b1.dtype
        live = b0.clone() if live is None else live
        self.items.append((live, b0, b1))
        return live

    def add_module(self, module, sd0, sd1):
        for name, p in module.state_dict().items():
            self.add(sd0[name], sd1[name], live=p)

    def set(self, which):
        with torch.no_grad():
            for live, b0, b1 in self.items:
                live.copy_(b1 if which else b0)


def _rays(st, n, s0, s1):
    r0, r1 = _syn().random_rays(n, seed=s0), _syn().random_rays(n, seed=s1)
    return tuple(st.add(r0[k], r1[k]) for k in ("rays_o", "rays_d", "viewdirs"))


def _flat(x):
    if isinstance(x, torch.Tensor):
        return [x]
    out = []
    for y in x:
        if y is not None:
            out += _flat(y)
    return out


def _vanilla_params(st, seeds=(0, 1), level="coarse_mlp."):
    sds = [_syn().make_nerf_state_dict(seed=s, density_scale=30.0) for s in seeds]
    return {k[len(level):]: st.add(sds[0][k], sds[1][k]) for k in sds[0] if k.startswith(level)}


def _art_params(st, seeds=(0, 1), level="coarse_mlp."):
    sds = [_syn().make_art_state_dict(seed=s, density_scale=30.0) for s in seeds]
    return {k[len(level):]: st.add(sds[0][k], sds[1][k]) for k in sds[0] if k.startswith(level)}


def _latent_state(st):
    return {"density": st.add(_u(40, 1, 128, lo=-0.2, hi=0.2), _u(41, 1, 128, lo=-0.2, hi=0.2)),
            "color": st.add(_u(42, 1, 128, lo=-0.2, hi=0.2), _u(43, 1, 128, lo=-0.2, hi=0.2)),
            "articulation": st.add(_u(44, 1, 32, lo=-0.2, hi=0.2), _u(45, 1, 32, lo=-0.2, hi=0.2))}


def _sorted_t(seed, n, S):
    return torch.sort(_u(seed, n, S, lo=NEAR, hi=FAR), dim=-1)[0]


# ------------------------------------------------------------------ (a) the table: name -> builder(ops, dev) -> (State, call)
def _case_sample_along_rays(ops, dev):
    st = State(dev)
    o, d, _ = _rays(st, 333, 1, 2)
    tr = st.add(_u(3, 333, 65), _u(4, 333, 65))
    return st, lambda: (ops.sample_along_rays(o, d, 64, NEAR, FAR, tr), ops.sample_along_rays(o, d, 64, NEAR, FAR, None, lindisp=True))


def _case_pos_enc(ops, dev):
    st = State(dev)
    x = st.add(_u(5, 777, 3, lo=-4, hi=4), _u(6, 777, 3, lo=-4, hi=4))
    return st, lambda: (ops.pos_enc(x, 0, 10), ops.pos_enc(x, 0, 4))


def _case_mlp_fwd(ops, dev):
    st = State(dev)
    params = _vanilla_params(st)
    o, d, v = _rays(st, 257, 1, 2)
    t = st.add(_sorted_t(7, 257, 65), _sorted_t(8, 257, 65))
    return st, lambda: ops.mlp_fwd(ops.pack_vanilla_mlp(params), o, d, v, t)


def _case_mlp_fwd_enc(ops, dev):
    st = State(dev)
    params = _vanilla_params(st)
    x = st.add(_u(9, 129, 33, 63, lo=-1, hi=1), _u(10, 129, 33, 63, lo=-1, hi=1))
    c = st.add(_u(11, 129, 27, lo=-1, hi=1), _u(12, 129, 27, lo=-1, hi=1))
    return st, lambda: ops.mlp_fwd_enc(ops.pack_vanilla_mlp(params), x, c)


def _case_composite_raw(ops, dev):
    st = State(dev)
    raw = st.add(_u(13, 401, 193, 4, lo=-2, hi=3), _u(14, 401, 193, 4, lo=-2, hi=3))
    t = st.add(_sorted_t(15, 401, 193), _sorted_t(16, 401, 193))
    _, d, _ = _rays(st, 401, 1, 2)
    return st, lambda: (ops.composite_raw(raw, t, d, True), ops.composite_raw(raw, t, d, False, ops.ACT_ARTICULATED, False))


def _case_composite_pdf(ops, dev):
    st = State(dev)
    raw = st.add(_u(17, 401, 65, 4, lo=-2, hi=3), _u(18, 401, 65, 4, lo=-2, hi=3))
    t = st.add(_sorted_t(19, 401, 65), _sorted_t(20, 401, 65))
    _, d, _ = _rays(st, 401, 1, 2)
    u = st.add(_u(21, 401, 128), _u(22, 401, 128))
    return st, lambda: (ops.composite_pdf(raw, t, d, True, want_weights=True), ops.composite_pdf(raw, t, d, True, u=u))


def _case_sample_pdf_t(ops, dev):
    st = State(dev)
    t = st.add(_sorted_t(23, 300, 65), _sorted_t(24, 300, 65))
    w = st.add(_u(25, 300, 65), _u(26, 300, 65))
    t2 = st.add(_sorted_t(27, 300, 33), _sorted_t(28, 300, 33))
    w2 = st.add(_u(29, 300, 33), _u(30, 300, 33))
    u2 = st.add(_u(31, 300, 40), _u(32, 300, 40))
    return st, lambda: (ops.sample_pdf_t(t, w), ops.sample_pdf_t_n(t2, w2, 40, u2), ops.sample_pdf_t_n(t2, w2, 40))


def _case_train_loss(ops, dev):
    from aon_amd.models.vanilla_nerf.helper import train_loss

    st = State(dev)
    rc = st.add(_u(33, 1000, 3), _u(34, 1000, 3)).requires_grad_(True)
    rf = st.add(_u(35, 1000, 3), _u(36, 1000, 3)).requires_grad_(True)
    tgt = st.add(_u(37, 1000, 3), _u(38, 1000, 3))
    lat = _latent_state(st)
    lats = [lat[k].requires_grad_(True) for k in ("density", "color", "articulation")]

    def call():
        for x in [rc, rf] + lats:
            x.grad = None
        loss, stats = train_loss([(rc, None, None), (rf, None, None)], tgt, lats, 1e-4)
        loss.backward()
        return [loss.detach(), stats, rc.grad, rf.grad] + [x.grad for x in lats]

    return st, call


def _case_render_fwd(ops, dev):
    st = State(dev)
    pc, pf = _vanilla_params(st), _vanilla_params(st, level="fine_mlp.")
    o, d, v = _rays(st, 700, 1, 2)
    tr, u = st.add(_u(50, 700, 65), _u(51, 700, 65)), st.add(_u(52, 700, 128), _u(53, 700, 128))
    return st, lambda: (ops.render_fwd(ops.pack_vanilla_mlp(pc), ops.pack_vanilla_mlp(pf), o, d, v, NEAR, FAR, True),
                        ops.render_fwd(ops.pack_vanilla_mlp(pc), ops.pack_vanilla_mlp(pf), o, d, v, NEAR, FAR, False, 2, tr, u))


def _art_packs(ops, pc, pf, lat):
    return ops.pack_art_mlp(pc), ops.art_prepare(pc, lat), ops.pack_art_mlp(pf), ops.art_prepare(pf, lat)


def _case_art_render_fwd(ops, dev):
    st = State(dev)
    pc, pf, lat = _art_params(st), _art_params(st, level="fine_mlp."), _latent_state(st)
    o, d, v = _rays(st, 500, 1, 2)
    return st, lambda: ops.art_render_fwd(*_art_packs(ops, pc, pf, lat), o, d, v, NEAR, FAR, True)


def _grid_state(st, dims=(9, 10, 11)):
    return st.add(_u(60, *dims), _u(61, *dims))


def _case_render_fwd_occ(ops, dev):
    st = State(dev)
    pc, pf = _vanilla_params(st), _vanilla_params(st, level="fine_mlp.")
    o, d, v = _rays(st, 700, 1, 2)
    dens = _grid_state(st)

    def call():
        grid = ops.occupancy_grid(dens, -1.5, 1.5, 0.6, 0)
        return ops.render_fwd_occ(ops.pack_vanilla_mlp(pc), ops.pack_vanilla_mlp(pf), o, d, v, NEAR, FAR, True, grid)

    return st, call


def _case_art_render_fwd_occ(ops, dev):
    st = State(dev)
    pc, pf, lat = _art_params(st), _art_params(st, level="fine_mlp."), _latent_state(st)
    o, d, v = _rays(st, 500, 1, 2)
    dens = _grid_state(st)

    def call():
        grid = ops.occupancy_grid(dens, -1.5, 1.5, 0.6, 0)
        return ops.art_render_fwd_occ(*_art_packs(ops, pc, pf, lat), o, d, v, NEAR, FAR, True, grid)

    return st, call


def _case_render_fwd_stop(ops, dev):
    st = State(dev)
    pc, pf = _vanilla_params(st), _vanilla_params(st, level="fine_mlp.")
    o, d, v = _rays(st, 700, 1, 2)
    dens = _grid_state(st)

    def call():
        grid = ops.occupancy_grid(dens, -1.5, 1.5, 0.3, 1)
        pk = ops.pack_vanilla_mlp(pc), ops.pack_vanilla_mlp(pf)
        return (ops.render_fwd_stop(*pk, o, d, v, NEAR, FAR, True, grid, 1e-2, 16),      # eps > 0: the round loop runs (13 rounds at the fine level)
                ops.render_fwd_stop(*pk, o, d, v, NEAR, FAR, True, None, 1e-3))

    return st, call


GENERAL = dict(min_deg_point=0, max_deg_point=10, deg_view=4, netdepth=4, netwidth=256, netwidth_condition=128, skip_layer=2, netdepth_condition=1)


def _general_params(st, ops):
    geom = ops.MlpGeometry(**GENERAL)
    sds = [_syn().make_general_nerf_state_dict(70 + i, **GENERAL) for i in range(2)]
    out = []
    for level in ("coarse_mlp.", "fine_mlp."):
        out.append({k[len(level):]: st.add(sds[0][k], sds[1][k]) for k in sds[0] if k.startswith(level)})
    return geom, out[0], out[1]


def _case_grender_fwd(ops, dev):
    st = State(dev)
    geom, pc, pf = _general_params(st, ops)
    o, d, v = _rays(st, 300, 1, 2)
    return st, lambda: ops.grender_fwd(geom, pc, pf, o, d, v, NEAR, FAR, True)


def _train_call(model, rays, target, draws, extra=(), latents_of=None):
    """zero the gradients, forward, loss, backward -> [loss, stats, the levels' colours, every gradient]; `call.params`: what it trains"""
    from aon_amd.models.vanilla_nerf.helper import train_loss

    params = [p for m in (model,) + tuple(extra) for p in m.parameters()]

    def call():
        for p in params:
            p.grad = None
        if latents_of is None:
            out = model(rays, True, True, NEAR, FAR, t_rand=draws[0], u=draws[1])
            loss, stats = train_loss(out, target)
        else:
            lat = latents_of()
            out = model(rays, True, True, NEAR, FAR, lat, t_rand=draws[0], u=draws[1])
            loss, stats = train_loss(out, target, (lat["density"], lat["color"], lat["articulation"]), 1e-4)
        loss.backward()
        assert all(p.grad is not None for p in params)
        return [loss.detach(), stats] + [o[0].detach() for o in out] + [p.grad for p in params]

    call.params = params
    return call


def _train_data(st, n, seed):
    o, d, v = _rays(st, n, seed, seed + 1)
    rays = {"rays_o": o, "rays_d": d, "viewdirs": v}
    target = st.add(_u(seed + 2, n, 3), _u(seed + 3, n, 3))
    draws = (st.add(_u(seed + 4, n, 65), _u(seed + 5, n, 65)), st.add(_u(seed + 6, n, 128), _u(seed + 7, n, 128)))
    return rays, target, draws


def _case_general_train(ops, dev):
    from aon_amd.models.vanilla_nerf.model import NeRF

    st = State(dev)
    kw = dict(min_deg_point=0, max_deg_point=6, deg_view=2)
    model = NeRF(**kw).to(dev)
    model._fused_inference = False        # (0, 6, 2) fits the fused kernels' slots: this case is about the layer-wise engine
    st.add_module(model, *[_syn().make_general_nerf_state_dict(80 + i, **kw) for i in range(2)])
    rays, target, draws = _train_data(st, 256, 100)
    return st, _train_call(model, rays, target, draws)


def _case_vanilla_train(ops, dev, n=640):
    from aon_amd.models.vanilla_nerf.model import NeRF

    st = State(dev)
    model = NeRF().to(dev)
    st.add_module(model, *[_syn().make_nerf_state_dict(seed=s, density_scale=3.0) for s in (0, 1)])
    rays, target, draws = _train_data(st, n, 110)
    return st, _train_call(model, rays, target, draws)


def _case_art_train(ops, dev, n=512):
    from aon_amd.models.code_library import CodeLibraryArticulated
    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

    st = State(dev)
    model = NeRF_AE_Art().to(dev)
    st.add_module(model, *[_syn().make_art_state_dict(seed=s, density_scale=2.0) for s in (5, 6)])
    lib = CodeLibraryArticulated(types.SimpleNamespace(N_max_objs=2, N_obj_code_length=128)).to(dev)
    st.add_module(lib, *[_syn().make_code_library_state(seed=s, n_max_objs=2) for s in (3, 4)])
    ids = {"instance_id": st.add(torch.tensor([1]), torch.tensor([0])), "articulation_id": st.add(torch.tensor([6]), torch.tensor([2]))}
    rays, target, draws = _train_data(st, n, 120)
    return st, _train_call(model, rays, target, draws, extra=(lib,), latents_of=lambda: lib(ids))


def _case_occupancy_grid(ops, dev):
    st = State(dev)
    dens = _grid_state(st, (17, 12, 33))
    return st, lambda: (ops.occupancy_grid(dens, -1.5, 1.5, 0.6, 0).bits, ops.occupancy_grid(dens, -1.5, 1.5, 0.9, 2).bits)


def _case_density_grid(ops, dev):
    st = State(dev)
    pc = _vanilla_params(st)
    pa, lat = _art_params(st), _latent_state(st)
    return st, lambda: (ops.density_grid(ops.pack_vanilla_mlp(pc), (9, 10, 11), -1.5, 1.5, ops.ACT_VANILLA),
                        ops.density_grid(ops.pack_art_mlp(pa), (7, 8, 9), -1.5, 1.5, ops.ACT_ARTICULATED, small=ops.art_prepare(pa, lat)))


def _case_marching_cubes(ops, dev):
    st = State(dev)
    g = st.add(_u(62, 12, 13, 14), _u(63, 12, 13, 14))
    return st, lambda: ops.marching_cubes(g, 0.5, -1.0, 1.0)


def _case_ssim(ops, dev):
    st = State(dev)
    p = [st.add(_u(64 + i, h, w, 3), _u(74 + i, h, w, 3)) for i, (h, w) in enumerate(((24, 31), (40, 17)))]
    g = [st.add(_u(84 + i, h, w, 3), _u(94 + i, h, w, 3)) for i, (h, w) in enumerate(((24, 31), (40, 17)))]
    return st, lambda: ops.ssim(p, g)


def _case_adam_step(ops, dev):
    st = State(dev)
    n = 100_003
    flat = st.add(_u(200, n, lo=-1, hi=1), _u(201, n, lo=-1, hi=1))
    grad = st.add(_u(202, n, lo=-1e-2, hi=1e-2), _u(203, n, lo=-1e-2, hi=1e-2))
    m = st.add(_u(204, n, lo=-1e-3, hi=1e-3), _u(205, n, lo=-1e-3, hi=1e-3))
    v = st.add(_u(206, n, lo=0, hi=1e-5), _u(207, n, lo=0, hi=1e-5))

    def call():   # (in place: the probe re-sets the state before every call)
        ops.adam_step(flat, grad, m, v, 16, n - 19, 5e-4, 0.9, 0.999, 1e-8, 3)
        return flat, m, v

    return st, call


def _case_code_library(ops, dev):
    from aon_amd.models.code_library import CodeLibraryArticulated

    st = State(dev)
    lib = CodeLibraryArticulated(types.SimpleNamespace(N_max_objs=3, N_obj_code_length=128)).to(dev)
    st.add_module(lib, *[_syn().make_code_library_state(seed=s, n_max_objs=3) for s in (3, 4)])
    ids = {"instance_id": st.add(torch.tensor([2]), torch.tensor([1])), "articulation_id": st.add(torch.tensor([6]), torch.tensor([9]))}
    coef = {k: st.add(_u(210 + i, 1, w), _u(220 + i, 1, w)) for i, (k, w) in enumerate((("density", 128), ("color", 128), ("articulation", 32)))}

    def call():
        for p in lib.parameters():
            p.grad = None
        lat = lib(ids)
        sum((lat[k] * coef[k]).sum() for k in coef).backward()
        return [lat[k].detach() for k in coef] + [p.grad for p in lib.parameters()]

    return st, call


TABLE = {
    "sample_along_rays": _case_sample_along_rays, "pos_enc": _case_pos_enc, "mlp_fwd": _case_mlp_fwd, "mlp_fwd_enc": _case_mlp_fwd_enc,
    "composite_raw": _case_composite_raw, "composite_pdf": _case_composite_pdf, "sample_pdf_t_and_n": _case_sample_pdf_t,
    "train_loss_fwd_bwd": _case_train_loss, "render_fwd": _case_render_fwd, "art_render_fwd": _case_art_render_fwd,
    "render_fwd_occ": _case_render_fwd_occ, "art_render_fwd_occ": _case_art_render_fwd_occ, "render_fwd_stop": _case_render_fwd_stop,
    "grender_fwd": _case_grender_fwd, "general_engine_train_step": _case_general_train, "occupancy_grid": _case_occupancy_grid,
    "density_grid": _case_density_grid, "marching_cubes": _case_marching_cubes, "ssim": _case_ssim, "adam_step": _case_adam_step,
    "code_library_fwd_bwd": _case_code_library, "nerf_loss_backward": _case_vanilla_train, "nerf_ae_art_loss_backward": _case_art_train,
}
SYNCS_ITS_STREAM = {"marching_cubes"}     # aon_marching_cubes_count is documented to synchronise its stream: the only entry exempt from `pending`


def _probe(dev, delay, st, call, name, must_be_pending=True):
    # 1. the serial default-stream result for batch 1
    st.set(1)
    want = [x.clone() for x in _flat(call())]
    torch.cuda.synchronize(dev)
    # 2. batch 0 on the stream (also: first-use work -- allocator blocks of this stream, lazily made side streams -- happens here)
    S = torch.cuda.Stream(device=dev)
    st.set(0)
    S.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(S):
        warm = [x.clone() for x in _flat(call())]
    S.synchronize()
    assert len(warm) == len(want)
    assert any(not torch.equal(a, b) for a, b in zip(warm, want)), f"{name}: batches 0 and 1 give the same outputs, the probe would be vacuous"
    # 3. delay, overwrite 0 -> 1 in place, the call, the copies: all on S, nothing synchronised until the end
    ev = torch.cuda.Event()
    with torch.cuda.stream(S):
        delay(DELAY_MS)
        st.set(1)
        outs = _flat(call())
        ev.record(S)
        pending = not ev.query()
        got = [x.clone() for x in outs]
    S.synchronize()
    torch.cuda.synchronize(dev)
    print(f"[streams] probe {name}: pending={pending}, {len(got)} outputs")
    if must_be_pending:
        assert pending, f"{name}: the stream had already drained when the call returned (a host synchronisation inside it, or the delay is too short)"
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), f"{name}: output {i} differs from the serial default-stream result"


@pytest.mark.parametrize("name", list(TABLE))
def test_ordering_probe(ops, dev, delay, name):
    st, call = TABLE[name](ops, dev)
    _probe(dev, delay, st, call, name, must_be_pending=name not in SYNCS_ITS_STREAM)


# schedule switches that change the stream topology of a training step (ops.set_*): name -> (setter, value); all default to "on" (1)
SCHEDULES = {
    "bwd_overlap=0": ("set_bwd_overlap", 0), "bwd_overlap=1": ("set_bwd_overlap", 1), "bwd_overlap=2": ("set_bwd_overlap", 2),
    "bwd_merge=0": ("set_bwd_merge", 0), "bwd_merge=1": ("set_bwd_merge", 1),
    "fwd_merge=0": ("set_fwd_merge", 0), "fwd_merge=2": ("set_fwd_merge", 2),     # 2: merged even where no round is saved (these batch sizes)
    "fwd_overlap=0": ("set_fwd_overlap", 0), "fwd_overlap=1": ("set_fwd_overlap", 1),
    "fwd_merge=0,fwd_overlap=1": ("set_fwd_merge", 0, "set_fwd_overlap", 1), "fwd_merge=0,fwd_overlap=0": ("set_fwd_merge", 0, "set_fwd_overlap", 0),
    "bwd_early_heads=0": ("set_bwd_early_heads", 0), "bwd_early_heads=1": ("set_bwd_early_heads", 1),
    "bwd_merge=0,bwd_overlap=0": ("set_bwd_merge", 0, "set_bwd_overlap", 0), "bwd_merge=0,bwd_overlap=1": ("set_bwd_merge", 0, "set_bwd_overlap", 1),
}


def _restore_schedule(ops):
    ops.set_bwd_overlap(1)
    ops.set_bwd_merge(1)
    ops.set_fwd_merge(1)
    ops.set_fwd_overlap(1)
    ops.set_bwd_early_heads(1)


@pytest.mark.parametrize("net", ["vanilla", "articulated"])
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_ordering_probe_training_schedules(ops, dev, delay, net, schedule):
    sw = SCHEDULES[schedule]
    try:
        for i in range(0, len(sw), 2):
            getattr(ops, sw[i])(sw[i + 1])
        st, call = (_case_vanilla_train(ops, dev, 1024) if net == "vanilla" else _case_art_train(ops, dev, 768))
        _probe(dev, delay, st, call, f"{net} training step, {schedule}")
    finally:
        _restore_schedule(ops)


# ------------------------------------------------------------------ (b) two streams, two different jobs
def _concurrent_pair(dev, delay):
    """Two torch streams whose work demonstrably runs side by side (streams may share a hardware queue, which serialises them: the overlap
    assertion of (b) is about the library, so it is made on a pair that can overlap at all)."""
    cands = [torch.cuda.Stream(device=dev) for _ in range(6)]
    for i in range(len(cands)):
        for j in range(i + 1, len(cands)):
            A, B = cands[i], cands[j]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            torch.cuda.synchronize(dev)
            base = torch.cuda.Event(enable_timing=True)
            base.record()
            for s, (e0, e1) in ((A, ev[:2]), (B, ev[2:])):
                s.wait_event(base)
                with torch.cuda.stream(s):
                    e0.record(s)
                    delay(5.0)
                    e1.record(s)
            torch.cuda.synchronize(dev)
            a0, a1, b0, b1 = (base.elapsed_time(e) for e in ev)
            if a0 < b1 and b0 < a1:
                return A, B
    pytest.fail("no two of six torch streams ran a 5 ms delay side by side on this device")


def _serial(st, call, dev):
    st.set(1)
    want = [x.clone() for x in _flat(call())]
    torch.cuda.synchronize(dev)
    return want


def _two_jobs(dev, delay, jobs, name):
    """jobs: two (State, call).  Serial results first; then both streams are blocked behind one event recorded after a delay, both jobs are
    enqueued while they are blocked, released together."""
    wants = [_serial(st, call, dev) for st, call in jobs]
    A, B = _concurrent_pair(dev, delay)
    for (st, call), s in zip(jobs, (A, B)):      # first use of each stream (allocator blocks, side streams), then the state of the job
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            call()
            st.set(1)
        s.synchronize()
    base, gate = torch.cuda.Event(enable_timing=True), torch.cuda.Event()
    base.record()
    delay(DELAY_MS)
    gate.record()
    marks, gots, pend = [], [], []
    for (st, call), s in zip(jobs, (A, B)):
        s.wait_event(gate)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record(s)
            outs = _flat(call())
            e1.record(s)
            gots.append([x.clone() for x in outs])
        marks.append((e0, e1))
    pend = not gate.query()      # the host finished enqueuing both jobs while both were still blocked
    A.synchronize()
    B.synchronize()
    torch.cuda.synchronize(dev)
    (a0, a1), (b0, b1) = [(base.elapsed_time(e0), base.elapsed_time(e1)) for e0, e1 in marks]
    print(f"[streams] pair {name}: job 1 [{a0:.2f}, {a1:.2f}] ms, job 2 [{b0:.2f}, {b1:.2f}] ms, enqueued while blocked={pend}")
    assert pend, f"{name}: the gate had opened before both jobs were enqueued"
    assert a0 < b1 and b0 < a1, f"{name}: the two jobs did not overlap ([{a0:.2f}, {a1:.2f}] and [{b0:.2f}, {b1:.2f}] ms): nothing was proved"
    for k, (got, want) in enumerate(zip(gots, wants)):
        assert len(got) == len(want)
        for i, (x, y) in enumerate(zip(got, want)):
            assert torch.equal(x, y), f"{name}: job {k + 1} output {i} differs from its serial result"


def _render_job(ops, dev, n, seeds, art=False):
    st = State(dev)
    if art:
        pc, pf, lat = _art_params(st, seeds), _art_params(st, seeds, "fine_mlp."), _latent_state(st)
        o, d, v = _rays(st, n, seeds[0] + 30, seeds[1] + 30)
        return st, lambda: ops.art_render_fwd(*_art_packs(ops, pc, pf, lat), o, d, v, NEAR, FAR, True)
    pc, pf = _vanilla_params(st, seeds), _vanilla_params(st, seeds, "fine_mlp.")
    o, d, v = _rays(st, n, seeds[0] + 30, seeds[1] + 30)
    return st, lambda: ops.render_fwd(ops.pack_vanilla_mlp(pc), ops.pack_vanilla_mlp(pf), o, d, v, NEAR, FAR, True)


def _occ_job(ops, dev, n, seeds, stop):
    st = State(dev)
    pc, pf = _vanilla_params(st, seeds), _vanilla_params(st, seeds, "fine_mlp.")
    o, d, v = _rays(st, n, seeds[0] + 40, seeds[1] + 40)
    dens = st.add(_u(60 + seeds[0], 9, 10, 11), _u(61 + seeds[1], 9, 10, 11))

    def call():
        grid = ops.occupancy_grid(dens, -1.5, 1.5, 0.5, 0)
        pk = ops.pack_vanilla_mlp(pc), ops.pack_vanilla_mlp(pf)
        if stop:
            return ops.render_fwd_stop(*pk, o, d, v, NEAR, FAR, True, grid, 1e-2, 16)
        return ops.render_fwd_occ(*pk, o, d, v, NEAR, FAR, True, grid)

    return st, call


def test_two_streams_exact_renders_of_different_sizes(ops, dev, delay):
    ops.release_workspaces()
    _two_jobs(dev, delay, [_render_job(ops, dev, 3000, (0, 1)), _render_job(ops, dev, 9000, (2, 3))], "exact render 3000 + exact render 9000 rays")
    _two_jobs(dev, delay, [_render_job(ops, dev, 2500, (0, 1), art=True), _render_job(ops, dev, 4000, (4, 5))], "articulated render + exact render")


def test_two_streams_render_and_training_step(ops, dev, delay):
    _two_jobs(dev, delay, [_render_job(ops, dev, 6000, (0, 1)), _case_vanilla_train(ops, dev, 1024)], "exact render + training step")
    _two_jobs(dev, delay, [_case_art_train(ops, dev, 768), _render_job(ops, dev, 6000, (2, 3))], "articulated training step + exact render")


def test_two_streams_occupancy_renders(ops, dev, delay):
    ops.release_workspaces()
    _two_jobs(dev, delay, [_occ_job(ops, dev, 3000, (0, 1), False), _occ_job(ops, dev, 7000, (2, 3), False)], "occupancy render + occupancy render")
    _two_jobs(dev, delay, [_occ_job(ops, dev, 3000, (0, 1), True), _occ_job(ops, dev, 7000, (2, 3), False)], "early-stop render + occupancy render")


def test_two_streams_general_engine_and_fused_render(ops, dev, delay):
    st = State(dev)
    geom, pc, pf = _general_params(st, ops)
    o, d, v = _rays(st, 2000, 7, 8)
    general = (st, lambda: ops.grender_fwd(geom, pc, pf, o, d, v, NEAR, FAR, True))
    _two_jobs(dev, delay, [general, _render_job(ops, dev, 6000, (0, 1))], "general-engine render + fused render")


# ------------------------------------------------------------------ (c) two host threads
def _steps(dev, net, seed, stream, barrier=None):
    """Three training steps (forward, backward, arena Adam) of an own model on `stream` -> [every parameter after step 3] + [every gradient
    of every step]."""
    from aon_amd import ops
    from aon_amd.arena import ArenaAdam, ParamArena

    with torch.cuda.stream(stream):
        st, call = (_case_vanilla_train(ops, dev, 640) if net == "vanilla" else _case_art_train(ops, dev, 512))
        st.set(seed)
        plist = call.params
        arena = ParamArena(_ParamBag(plist))
        opt = ArenaAdam(arena, lr=5e-4)
        out = []
        for step in range(3):
            if barrier is not None:
                barrier.wait(timeout=120)
            res = call()
            out += [g.clone() for g in res[2:]]
            opt.step()
        out = [p.detach().clone() for p in plist] + out
    stream.synchronize()
    return out


class _ParamBag(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        self.ps = torch.nn.ParameterList(params)


@pytest.mark.parametrize("net", ["vanilla", "articulated"])
def test_two_host_threads(dev, net):
    from aon_amd import ops
    from aon_amd._lib import lib

    null = torch.cuda.current_stream(dev)
    wants = [_steps(dev, net, k, null) for k in (0, 1)]           # single-threaded, default stream
    assert any(not torch.equal(a, b) for a, b in zip(*wants))     # two different jobs
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    barrier = threading.Barrier(2)
    results, failures, messages = [None, None], [], [None, None]

    def work(k):
        try:
            torch.cuda.set_device(dev)
            results[k] = _steps(dev, net, k, streams[k], barrier=barrier)
            # the error text is thread-local: thread 0 provokes a refusal (host-side checks: AON_E_INVALID from null pointers / a bad
            # size, nothing reaches the GPU), then thread 1 another one; thread 0's text must be what it was
            if k == 0:
                assert lib.aon_ray_radii(None, None, 8, 8, None, None) != 0
                messages[0] = bytes(lib.aon_last_error())
            barrier.wait(timeout=120)
            if k == 1:
                assert lib.aon_composite_pdf(None, None, None, 4, 1, 3, None, 0, None, None, None, None, None, None) != 0
                messages[1] = bytes(lib.aon_last_error())
            barrier.wait(timeout=120)
            if k == 0:
                assert bytes(lib.aon_last_error()) == messages[0], "thread 0's error text was changed by thread 1's refusal"
        except BaseException as e:   # noqa: BLE001  (reported by the main thread)
            failures.append((k, repr(e)))
            barrier.abort()

    threads = [threading.Thread(target=work, args=(k,)) for k in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    torch.cuda.synchronize(dev)
    assert not failures, failures
    assert all(not t.is_alive() for t in threads)
    assert b"null" in messages[0] and b"bad size" in messages[1] and messages[0] != messages[1]
    for k in (0, 1):
        assert len(results[k]) == len(wants[k])
        for i, (a, b) in enumerate(zip(results[k], wants[k])):
            assert torch.equal(a, b), f"{net}: thread {k}, tensor {i} differs from the single-threaded run"
    ops.release_workspaces()


# ------------------------------------------------------------------ (d) pool and caches on the device
def test_pool_buffer_given_back_on_one_stream_is_not_handed_out_on_another(ops, dev):
    ops.release_workspaces()
    A, B = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    nbytes = 1 << 20
    with torch.cuda.stream(A):
        t = ops._pool_take(nbytes, "test", dev)
        ptr = t.data_ptr()
        ops.pool_give(t)
        del t
    with torch.cuda.stream(B):
        b = ops._pool_take(nbytes, "test", dev)
        assert b.data_ptr() != ptr
    with torch.cuda.stream(A):
        a = ops._pool_take(nbytes, "test", dev)
        assert a.data_ptr() == ptr                     # ... and is handed out again on its own stream
    torch.cuda.synchronize(dev)
    ops.release_workspaces()
    assert not ops._TRAIN_POOL


def test_workspaces_are_per_stream_and_released(ops, dev):
    from aon_amd.models.vanilla_nerf.model import NeRF

    ops.release_workspaces()
    caches = {"_WS_CACHE": ops._WS_CACHE, "_GWS_CACHE": ops._GWS_CACHE, "_OCC_WS_CACHE": ops._OCC_WS_CACHE, "_WG_WS": ops._WG_WS}
    assert all(len(c) == 0 for c in caches.values())
    A, B = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    jobs = {"_WS_CACHE": _render_job(ops, dev, 500, (0, 1)), "_OCC_WS_CACHE": _occ_job(ops, dev, 500, (0, 1), True)}
    st = State(dev)
    geom, pc, pf = _general_params(st, ops)
    o, d, v = _rays(st, 200, 7, 8)
    jobs["_GWS_CACHE"] = (st, lambda: ops.grender_fwd(geom, pc, pf, o, d, v, NEAR, FAR, True))
    model = NeRF(num_levels=3).to(dev)      # three levels train through the stage-level calls: ops.vanilla_wgrad's workspace
    model.load_state_dict(_syn().make_nerf_state_dict(seed=0, density_scale=3.0))
    r = {k: x.to(dev) for k, x in _syn().random_rays(128, seed=3).items()}

    def wg():
        model.zero_grad(set_to_none=True)
        out = model(r, False, True, NEAR, FAR)
        sum((x[0] ** 2).mean() for x in out).backward()

    jobs["_WG_WS"] = (None, wg)
    for name, (_, call) in jobs.items():
        for s in (A, B):        # one after the other: this test is about who owns which buffer, not about a race
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                call()
            s.synchronize()
        bufs = caches[name].values()
        assert len(bufs) == 2 and bufs[0].data_ptr() != bufs[1].data_ptr(), name
        keys = list(caches[name]._entries)
        assert {k[1] for k in keys} == {A.cuda_stream, B.cuda_stream} and {k[0] for k in keys} == {dev.index}, (name, keys)
        with torch.cuda.stream(A):      # the same stream gets its own buffer again
            before = {k: b.data_ptr() for k, b in caches[name]._entries.items()}
            call()
            assert {k: b.data_ptr() for k, b in caches[name]._entries.items()} == before, name
        A.synchronize()
    # the model's own packed inference buffers are per stream as well (one model instance may render from several streams)
    m2 = NeRF().to(dev)
    m2.load_state_dict(_syn().make_nerf_state_dict(seed=0, density_scale=30.0))
    torch.cuda.synchronize(dev)
    ptrs, outs = [], []
    with torch.no_grad():
        for s in (A, B, A):
            with torch.cuda.stream(s):
                outs.append(m2(r, False, True, NEAR, FAR)[1][0].clone())
                ptrs.append(tuple(m._streams["fwd"]._entries[ops.stream_key(dev)].data_ptr() for m in (m2.coarse_mlp, m2.fine_mlp)))
            s.synchronize()
    assert ptrs[0] == ptrs[2] and ptrs[0][0] != ptrs[1][0] and ptrs[0][1] != ptrs[1][1]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    torch.cuda.synchronize(dev)
    ops.release_workspaces()
    assert all(len(c) == 0 for c in caches.values()) and not ops._TRAIN_POOL

