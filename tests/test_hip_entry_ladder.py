"""GPU: the ladder of exported whole-path forwards (plain, _ex, _occ, _stop, _bounds; _train, _train_ex, _train_bounds) called through
ctypes directly, both networks.  Every rung with its extras switched off must give the bits of the rung below it: all of them hand one
call record to the same driver, and an argument transposed on the way compiles and type-checks.  ops.py never
calls the plain forms nor the _bounds forms with a null `bounds`, so only this file reaches them.  The training ladder ends in the
backwards: plain and _ex, and for the articulated network the latent-only one and aon_art_render_bwd_inputs with and without ray gradients."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

NEAR, FAR = 2.0, 6.0
N_RAYS = 257           # with a workspace sized for about 150 rays: two chunks, the second one shorter
WS_RAYS = 150
# tau_stop = -ln 0.9 = 0.105.  The articulated network's density is softplus(raw - 1), about 0.3 per unit length where raw is near zero, so a
# ray that enters the occupied half-space within its first round reaches tau_stop after a third of a unit: some of the 257 stop at each
# level whatever the random weights do (asserted); the vanilla field (relu, density_scale 30) is far denser.
EPS = 0.9
ROUND = 48
N_TRAIN = 3            # the smallest ray count tests/test_hip_training.py uses


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


class Net:
    """Random weights of both levels packed through the pack ops, as the C calls take them."""

    def __init__(self, dev, art):
        import aon_amd.synthetic as syn
        from aon_amd import ops

        self.art = art
        sd = (syn.make_art_state_dict if art else syn.make_nerf_state_dict)(seed=0, density_scale=30.0)
        self.params = [{k[len(p):]: v.to(dev) for k, v in sd.items() if k.startswith(p)} for p in ("coarse_mlp.", "fine_mlp.")]
        if art:
            gen = torch.Generator().manual_seed(7)
            self.latents = {k: (0.1 * torch.randn(1, w, generator=gen)).to(dev) for k, w in (("density", 128), ("color", 128), ("articulation", 32))}
            self.fwd = [ops.pack_art_mlp(p) for p in self.params]
            self.small = [ops.art_prepare(p, self.latents) for p in self.params]
            self.bwd = [ops.pack_art_mlp_bwd(p) for p in self.params]
            self.packs = (self.fwd[0], self.small[0], self.fwd[1], self.small[1])
            self.order, self.shapes = ops.ART_PARAM_ORDER, ops.ART_PARAM_SHAPES
        else:
            self.fwd = [ops.pack_vanilla_mlp(p) for p in self.params]
            self.bwd = [ops.pack_vanilla_mlp_bwd(p) for p in self.params]
            self.packs = (self.fwd[0], self.fwd[1])
            self.order, self.shapes = ops.VANILLA_PARAM_ORDER, ops.vanilla_param_shapes()
        self.stem = "aon_art_render_fwd" if art else "aon_render_fwd"


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _rays(dev, n, seed):
    import aon_amd.synthetic as syn

    r = syn.random_rays(n, seed=seed)
    return tuple(r[k].to(dev) for k in ("rays_o", "rays_d", "viewdirs"))


def _forward(name, net, rays, ws, *extra):
    """One exported forward -> its six outputs (NaN where the call wrote nothing).  `extra`: what follows `stream` in the C signature."""
    from aon_amd import _lib, ops

    o, d, v = rays
    n, dev = o.shape[0], o.device
    outs = [torch.full(s, float("nan"), device=dev) for s in ((n, 3), (n,), (n,)) * 2]
    u = ops.deterministic_u(dev)
    with torch.cuda.device(dev):
        rc = getattr(_lib.lib, name)(*(_p(t) for t in net.packs), _p(o), _p(d), _p(v), n, NEAR, FAR, 1, 2, None, _p(u), 0, *(_p(t) for t in outs),
                                     _p(ws), ws.numel(), None, *extra)
    _lib.check(rc, name)
    torch.cuda.synchronize(dev)
    assert all(torch.isfinite(t).all() for t in outs), name
    return outs


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: output {i} differs, max |diff| = {(x - y).abs().max().item():.3e}"


def _half_space_grid(dev):
    """x > 0 occupied, x < 0 empty (but for the one layer of cells the dilation adds), over the box the rays cross."""
    from aon_amd import ops

    x = torch.linspace(-2.0, 2.0, 17, device=dev)
    density = (x > 0.2).float()[:, None, None].expand(17, 17, 17).contiguous()
    grid = ops.occupancy_grid(density, -2.0, 2.0, threshold=0.01, dilate=1)
    assert 0.3 < grid.occupied_fraction() < 0.7
    return grid


@pytest.mark.parametrize("art", [False, True], ids=["vanilla", "articulated"])
def test_inference_ladder(dev, art):
    from aon_amd import _lib, ops

    lib = _lib.lib
    net = Net(dev, art)
    rays = _rays(dev, N_RAYS, seed=21)
    grid = _half_space_grid(dev)
    occ = grid.c_struct()
    opts = ops.RenderOpts().c_struct(NEAR, FAR)[0]
    S = (ops.DEFAULT_OPTS.Sc, ops.DEFAULT_OPTS.Sf)

    def ws(query):
        need = int(getattr(lib, query)(WS_RAYS, None))
        assert 0 < need < int(getattr(lib, query)(N_RAYS, None))
        return torch.empty(need, dtype=torch.uint8, device=dev)

    def stats():
        return torch.full((2,), -1, dtype=torch.int64, device=dev), torch.full((N_RAYS, 2), -1, dtype=torch.int32, device=dev)

    # 1. no extras: the plain form, _ex without options, _ex with the default options
    plain_ws = ws("aon_render_workspace_bytes_ex")
    plain = _forward(net.stem, net, rays, plain_ws)
    _same(_forward(net.stem + "_ex", net, rays, plain_ws, None), plain, "fwd_ex(opts=NULL) vs fwd")
    _same(_forward(net.stem + "_ex", net, rays, plain_ws, C.byref(opts)), plain, "fwd_ex(default opts) vs fwd")

    # 2. a grid, no termination: _occ, _stop with eps = 0, _bounds with eps = 0 and no bounds
    stop_ws = ws("aon_render_stop_workspace_bytes")
    tally_occ = stats()[0]
    occd = _forward(net.stem + "_occ", net, rays, ws("aon_render_occ_workspace_bytes"), None, C.byref(occ), _p(tally_occ))
    tally_s, stop_s = stats()
    stopped = _forward(net.stem + "_stop", net, rays, stop_ws, None, C.byref(occ), _p(tally_s), 0.0, ROUND, _p(stop_s))
    tally_b, stop_b = stats()
    bounded = _forward(net.stem + "_bounds", net, rays, stop_ws, None, C.byref(occ), _p(tally_b), 0.0, ROUND, _p(stop_b), None)
    _same(stopped, occd, "fwd_stop(grid, eps=0) vs fwd_occ(grid)")
    _same(bounded, occd, "fwd_bounds(grid, eps=0, bounds=NULL) vs fwd_occ(grid)")
    assert torch.equal(tally_s, tally_occ) and torch.equal(tally_b, tally_s) and torch.equal(stop_b, stop_s)
    # not vacuous: some samples ran (a ray hit an occupied cell), some were skipped, and the grid changed the picture
    assert 0 < int(tally_s[0]) < N_RAYS * S[0] and 0 < int(tally_s[1]) < N_RAYS * S[1]
    assert (stop_s == torch.tensor(S, dtype=torch.int32, device=dev)).all()      # eps = 0: no ray stopped
    assert not torch.equal(occd[3], plain[3])

    # 3. a grid and termination: _stop, _bounds without bounds
    tally_s, stop_s = stats()
    stopped = _forward(net.stem + "_stop", net, rays, stop_ws, None, C.byref(occ), _p(tally_s), EPS, ROUND, _p(stop_s))
    tally_b, stop_b = stats()
    bounded = _forward(net.stem + "_bounds", net, rays, stop_ws, None, C.byref(occ), _p(tally_b), EPS, ROUND, _p(stop_b), None)
    _same(bounded, stopped, "fwd_bounds(grid, eps, bounds=NULL) vs fwd_stop(grid, eps)")
    assert torch.equal(tally_b, tally_s) and torch.equal(stop_b, stop_s)
    assert int(tally_s[0]) > 0 and int(tally_s[1]) > 0
    for lvl in (0, 1):      # not vacuous: at least one ray stopped at each level
        assert 0 < int((stop_s[:, lvl] < S[lvl]).sum()) and (stop_s[:, lvl] >= 0).all()

    # 4. per-ray planes that are the scalars: _bounds without grid and termination against _ex
    near_ray, far_ray = torch.full((N_RAYS,), NEAR, device=dev), torch.full((N_RAYS,), FAR, device=dev)
    rb = _lib.RayBoundsC(near_ray.data_ptr(), far_ray.data_ptr(), None)
    _same(_forward(net.stem + "_bounds", net, rays, plain_ws, None, None, None, 0.0, ROUND, None, C.byref(rb)), plain,
          "fwd_bounds(no grid, eps=0, constant planes) vs fwd_ex")


@pytest.mark.parametrize("art", [False, True], ids=["vanilla", "articulated"])
def test_training_ladder(dev, art):
    from aon_amd import _lib, ops

    lib = _lib.lib
    net = Net(dev, art)
    n = N_TRAIN
    rays = _rays(dev, n, seed=22)
    stem = net.stem + "_train"
    ws_bytes, scratch_bytes = int(lib.aon_train_workspace_bytes(n, int(art), 2)), int(lib.aon_train_scratch_bytes(n, int(art), 2))
    assert ws_bytes > 0 and scratch_bytes > 0
    wss = [torch.zeros(ws_bytes, dtype=torch.uint8, device=dev) for _ in range(3)]
    plain = _forward(stem, net, rays, wss[0])
    _same(_forward(stem + "_ex", net, rays, wss[1], None), plain, "fwd_train_ex(NULL) vs fwd_train")
    _same(_forward(stem + "_bounds", net, rays, wss[2], None, None), plain, "fwd_train_bounds(NULL, NULL) vs fwd_train")

    # backward: plain form and _ex without options, on the same workspace contents
    gen = torch.Generator().manual_seed(23)
    g_rgb = [torch.randn(n, 3, generator=gen).to(dev) for _ in range(2)]
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])   # noqa: E731

    def backward(name, ws, *opts):
        grads = [[torch.full(net.shapes[k], float("nan"), device=dev) for k in net.order] for _ in range(2)]
        scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        head = (_p(rays[1]), n, 1, 2, arr(g_rgb), None, None)
        tail = (arr(grads[0]), arr(grads[1]))
        out = list(grads[0]) + list(grads[1])
        with torch.cuda.device(dev):
            if art:
                lat = [net.latents[k].reshape(-1).contiguous() for k in ("density", "color", "articulation")]
                g_lat = [torch.full_like(t, float("nan")) for t in lat]
                params = [arr([p[k] for k in net.order]) for p in net.params]
                rc = getattr(lib, name)(_p(net.bwd[0]), _p(net.small[0]), _p(net.bwd[1]), _p(net.small[1]), *head, *params, *(_p(t) for t in lat), *tail,
                                        *(_p(t) for t in g_lat), _p(ws), ws.numel(), _p(scratch), scratch.numel(), None, *opts)
                out += g_lat
            else:
                rc = getattr(lib, name)(_p(net.bwd[0]), _p(net.fwd[0]), _p(net.bwd[1]), _p(net.fwd[1]), *head, *tail, _p(ws), ws.numel(), _p(scratch),
                                        scratch.numel(), None, *opts)
        _lib.check(rc, name)
        torch.cuda.synchronize(dev)
        assert all(torch.isfinite(t).all() for t in out), name
        return out

    bwd = ("aon_art_render_bwd" if art else "aon_render_bwd")
    want = backward(bwd, wss[0].clone())
    _same(backward(bwd + "_ex", wss[0].clone(), None), want, "render_bwd_ex(NULL) vs render_bwd")
    assert sum(bool((t != 0).any()) for t in want) > len(want) // 2      # not vacuous: gradients arrived
    if not art:
        return

    # the frozen network's backwards on the same workspace contents: the latent gradients are aon_art_render_bwd_ex's bits
    def frozen(name, query, ws, rg=()):
        need = int(getattr(lib, query)(n, 2, None))
        assert 0 < need < scratch_bytes
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        g_lat = [torch.full((w,), float("nan"), device=dev) for w in (128, 128, 32)]
        params = [arr([p[k] for k in net.order]) for p in net.params]
        with torch.cuda.device(dev):
            rc = getattr(lib, name)(_p(net.bwd[0]), _p(net.small[0]), _p(net.bwd[1]), _p(net.small[1]), _p(rays[1]), n, 1, 2, arr(g_rgb), None, None, *params,
                                    *(_p(t) for t in g_lat), _p(ws), ws.numel(), _p(scratch), scratch.numel(), None, None, *rg)
        _lib.check(rc, name)
        torch.cuda.synchronize(dev)
        return g_lat

    _same(frozen("aon_art_render_bwd_latents", "aon_train_scratch_bytes_latents", wss[0].clone()), want[-3:], "render_bwd_latents vs render_bwd_ex")
    _same(frozen("aon_art_render_bwd_inputs", "aon_train_scratch_bytes_latents", wss[0].clone(), (None,)), want[-3:],
          "render_bwd_inputs(rg=NULL) vs render_bwd_ex")
    g_rays = [torch.full((n, 3), float("nan"), device=dev) for _ in range(3)]
    rg = _lib.RayGradsC(rays[0].data_ptr(), rays[2].data_ptr(), *(t.data_ptr() for t in g_rays))
    _same(frozen("aon_art_render_bwd_inputs", "aon_train_scratch_bytes_inputs", wss[0].clone(), (C.byref(rg),)), want[-3:],
          "render_bwd_inputs(rg) vs render_bwd_ex")
    assert all(torch.isfinite(t).all() for t in g_rays) and any(bool((t != 0).any()) for t in g_rays)
