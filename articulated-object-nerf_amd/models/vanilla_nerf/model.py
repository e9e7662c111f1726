"""Drop-in ``NeRFMLP`` / ``NeRF`` modules: same constructor defaults, attribute and parameter names (so the
reference's Lightning checkpoints load unchanged) and the same ``forward`` signatures and return structure as
``models/vanilla_nerf/model.py:39-199`` -- with ``forward`` running on the fused HIP kernels.

Two engines, chosen by the constructor arguments.  The reference's default NeRFMLP (8x256 trunk with a skip at layer 4,
1x128 view branch, 10/4 encoding degrees) -- the only one its CLI can build (``LitNeRF`` builds ``NeRF()``, model.py:218) --
runs on the fused register-resident kernels.  Every other ``NeRFMLP(...)`` geometry and every ``NeRF(min_deg_point,
max_deg_point, deg_view)`` runs on the layer-wise MFMA GEMM engine (``csrc/aon_gmlp.hip``): same C boundary, same module
interface, forward and backward.  Sample counts, ``lindisp`` and ``noise_std`` are runtime arguments of both.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.init as init

from ... import ops
from ...autograd import RenderGeneral, RenderLevelVanilla, RenderVanilla, RenderVanillaInputs


class WeightStreams:
    """The kernel-side weight streams of a NeRFMLP, vanilla or articulated (a mixin: it owns no parameter and no buffer).  The class names
    its ops packers (_PACKERS) and the C byte queries (_BYTES) per stream kind and says in _pack_degrees() what the packers take beside
    the parameters; its __init__ sets ``self._streams = {}``.

    The streams are rebuilt from the LIVE parameters on every call (one ~6 us HIP pack kernel, 2.4 MB): no version/pointer key can go
    stale, so `p.data.copy_()`, `dist.broadcast(p.data)`, EMA or clipping code that mutates parameters without bumping `p._version` is
    seen exactly as nn.Linear would see it.  `fresh=True` (training) writes into a new buffer, because autograd saves the stream for
    backward and a later forward must not overwrite what an earlier graph still needs; inference reuses one buffer per stream kind and
    per (device, torch stream) the call is made on (stream-ordered; `_stream_buffer`)."""

    def _pack(self, kind: str, fresh: bool, out: torch.Tensor | None = None) -> torch.Tensor:
        params = dict(self.named_parameters())
        dev = next(iter(params.values())).device
        if out is None and not fresh:
            out = self._stream_buffer(kind, dev)
        return getattr(ops, self._PACKERS[kind])(params, out=out, **self._pack_degrees())

    def _stream_buffer(self, kind: str, dev) -> torch.Tensor:
        """The module's inference buffer of `kind` for `dev`'s current stream (ops.StreamCache: one per (device, stream), so renders of one
        model on two streams never re-pack into a buffer the other stream's kernels still read)."""
        cache = self._streams.get(kind)
        if cache is None:
            cache = self._streams[kind] = ops.StreamCache(register=False)
        return ops._scratch(cache, dev, int(getattr(ops.lib, self._BYTES[kind])()))

    def packed(self, fresh: bool = False) -> torch.Tensor:
        """Forward weight stream of the fp32 kernels."""
        return self._pack("fwd", fresh)

    def packed_bwd(self, fresh: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
        """Transposed weight stream for the backward data chain (training only)."""
        return self._pack("bwd", fresh, out)

    def new_bwd_buffer(self) -> torch.Tensor:
        return torch.empty(int(getattr(ops.lib, self._BYTES["bwd"])()), dtype=torch.uint8, device=next(self.parameters()).device)


def _draw_samples(model, rays, randomized, t_rand, u):
    """The stratified / inverse-CDF draws of a forward -> (t_rand, u).  They may ride in the batch dict (keys "aon_t_rand", "aon_u": an
    extension, namespaced so that a user batch carrying its own "u" / "t_rand" is never misread -- the reference's forward ignores extra
    keys, model.py:299-306 -- that makes a harness run reproducible: tests/test_hip_long_training.py); what is still missing is drawn,
    t_rand first, u with two levels only.  Not randomized: (None, None)."""
    if not randomized:
        return None, None
    n, dev = rays["rays_o"].shape[0], rays["rays_o"].device
    if t_rand is None:
        t_rand = rays.get("aon_t_rand")
    if u is None:
        u = rays.get("aon_u")
    if t_rand is None:
        t_rand = torch.rand((n, model.num_coarse_samples + 1), device=dev)
    if u is None and model.num_levels == 2:
        u = torch.rand((n, model.num_fine_samples), device=dev)
    return t_rand, u


def _draw_noise(model, noise, randomized, n, device):
    """The density noise of a forward (model.py:183-184), one (n, S) tensor per level: the caller's, else drawn level by level; or None."""
    if not (model.noise_std > 0 and randomized):
        return None
    noise = list(noise) if noise is not None else []
    noise += [None] * (model.num_levels - len(noise))
    return [noise[lvl] if noise[lvl] is not None else torch.rand((n, model._opts.S(lvl)), device=device)
            for lvl in range(model.num_levels)]


class NeRFMLP(WeightStreams, nn.Module):
    """model.py:39-120.  ``forward(x, condition)``: x (N,S,63) encoded samples, condition (N,27) encoded view
    directions -> (raw_rgb (N,S,3), raw_density (N,S,1))."""

    def __init__(self, min_deg_point, max_deg_point, deg_view, netdepth: int = 8, netwidth: int = 256,
                 netdepth_condition: int = 1, netwidth_condition: int = 128, skip_layer: int = 4, input_ch: int = 3,
                 input_ch_view: int = 3, num_rgb_channels: int = 3, num_density_channels: int = 1):
        super().__init__()
        # validated by the C side (aon_gmlp_param_count): e.g. a skip concatenation after the LAST trunk layer is rejected, the
        # reference's own forward fails on it (density_layer is built for netwidth inputs)
        self.geometry = ops.MlpGeometry(min_deg_point, max_deg_point, deg_view, netdepth, netwidth, netdepth_condition, netwidth_condition,
                                        skip_layer, input_ch, input_ch_view, num_rgb_channels, num_density_channels)
        self.min_deg_point, self.max_deg_point, self.deg_view = min_deg_point, max_deg_point, deg_view
        self.netdepth, self.netwidth, self.skip_layer = netdepth, netwidth, skip_layer
        self.netdepth_condition, self.netwidth_condition = netdepth_condition, netwidth_condition
        self.num_rgb_channels, self.num_density_channels = num_rgb_channels, num_density_channels
        self.net_activation = nn.ReLU()
        pos_size = ((max_deg_point - min_deg_point) * 2 + 1) * input_ch
        view_pos_size = (deg_view * 2 + 1) * input_ch_view
        layers = [nn.Linear(pos_size, netwidth)]
        for idx in range(netdepth - 1):
            layers.append(nn.Linear(netwidth + pos_size if (idx % skip_layer == 0 and idx > 0) else netwidth, netwidth))
        for layer in layers:
            init.xavier_uniform_(layer.weight)
        self.pts_linears = nn.ModuleList(layers)
        views = [nn.Linear(netwidth + view_pos_size, netwidth_condition)]
        for _ in range(netdepth_condition - 1):
            layer = nn.Linear(netwidth_condition, netwidth_condition)
            init.xavier_uniform_(layer.weight)
            views.append(layer)
        self.views_linear = nn.ModuleList(views)
        self.bottleneck_layer = nn.Linear(netwidth, netwidth)
        self.density_layer = nn.Linear(netwidth, num_density_channels)
        self.rgb_layer = nn.Linear(netwidth_condition, num_rgb_channels)
        init.xavier_uniform_(self.bottleneck_layer.weight)
        init.xavier_uniform_(self.density_layer.weight)
        init.xavier_uniform_(self.rgb_layer.weight)
        self._streams = {}

    # the weight streams: WeightStreams
    _PACKERS = {"fwd": "pack_vanilla_mlp", "bwd": "pack_vanilla_mlp_bwd"}
    _BYTES = {"fwd": "aon_mlp_packed_bytes", "bwd": "aon_bwd_packed_bytes"}

    def _pack_degrees(self):
        # other degrees on the fused kernels (fits_fused_inference): zero-weight slots
        return {} if self.geometry.is_default else {"degrees": (self.min_deg_point, self.max_deg_point, self.deg_view)}

    def ordered_params(self):
        params = dict(self.named_parameters())
        return [params[name] for name in self.geometry.param_order]   # == ops.VANILLA_PARAM_ORDER for the default geometry

    def forward(self, x, condition):
        if not self.geometry.is_default:   # layer-wise engine, any geometry (inference; training goes through NeRF.forward)
            return ops.gmlp_fwd(self.geometry, dict(self.named_parameters()), x, condition)
        raw = ops.mlp_fwd_enc(self.packed(), x, condition)
        return raw[..., :3], raw[..., 3:4]


class NeRF(nn.Module):
    """model.py:123-199.  ``forward(rays, randomized, white_bkgd, near, far)`` with ``rays`` a dict holding
    ``rays_o``, ``rays_d``, ``viewdirs`` (extra keys are ignored, as in the reference) returns
    ``[(comp_rgb, acc, depth)_coarse, (comp_rgb, acc, depth)_fine]``.

    ``t_rand`` (N,num_coarse+1) / ``u`` (N,num_fine) / ``noise`` (per level (N,S), read when ``noise_std > 0 and randomized``,
    model.py:183-184) optionally replace the reference's in-function ``torch.rand`` / ``torch.rand_like`` draws."""

    def __init__(self, num_levels: int = 2, min_deg_point: int = 0, max_deg_point: int = 10, deg_view: int = 4,
                 num_coarse_samples: int = 64, num_fine_samples: int = 128, use_viewdirs: bool = True,
                 noise_std: float = 0.0, lindisp: bool = False):
        super().__init__()
        if num_levels < 1:
            raise ValueError("num_levels must be >= 1")
        if num_levels > 2 and (min_deg_point, max_deg_point, deg_view) != (0, 10, 4):
            raise NotImplementedError("more than two levels are served for the default network only (stage-level calls, inference)")
        # sample counts, lindisp and noise_std are runtime arguments of the C calls (aon_render_opts); use_viewdirs is stored and
        # never read by the reference's forward (model.py:147-199 always encodes rays["viewdirs"])
        self._opts = ops.RenderOpts(num_coarse_samples, num_fine_samples, lindisp, noise_std)
        self.num_levels, self.min_deg_point, self.max_deg_point, self.deg_view = num_levels, min_deg_point, max_deg_point, deg_view
        self.num_coarse_samples, self.num_fine_samples = num_coarse_samples, num_fine_samples
        self.use_viewdirs, self.noise_std, self.lindisp = use_viewdirs, noise_std, lindisp
        self.rgb_activation = nn.Sigmoid()
        self.sigma_activation = nn.ReLU()
        self.coarse_mlp = NeRFMLP(min_deg_point, max_deg_point, deg_view)
        self.fine_mlp = NeRFMLP(min_deg_point, max_deg_point, deg_view)
        geom = self.coarse_mlp.geometry
        # other encoding degrees: on the fused kernels (inference AND training) when the levels fit their 63 / 27 input slots -- zero-weight
        # slots in the packed streams, encodings in the padded layout -- else on the layer-wise engine
        self._fused_inference = geom.fits_fused_inference
        self._general = not geom.is_default and not self._fused_inference
        self._fused_training = True      # (tests / measurements: False sends the training step of a padded-slot network to the layer-wise engine)
        if not geom.is_default and self._fused_inference:
            self._opts.degrees = (min_deg_point, max_deg_point, deg_view)

    def _forward_many_levels(self, rays, randomized, white_bkgd, near, far, t_rand, u, noise, training=False):
        """model.py:147-199 for num_levels > 2 (every level after the first resamples from the previous level's t and weights
        with fine_mlp, :162-173), driven level by level through the stage-level C calls: fused cast + encode + MLP, compositing with
        the weights written, general-size inverse CDF.  ``u``: the first resampling's draws, or a list with one entry per
        resampling level.  ``training`` (round 4): every level is an autograd node built from the stage-level training calls
        (autograd.RenderLevelVanilla); fine_mlp's gradients add up over the levels that use it, as under the reference's autograd."""
        o, d, v = rays["rays_o"], rays["rays_d"], rays["viewdirs"]
        n = o.shape[0]
        us = list(u) if isinstance(u, (list, tuple)) else [u]
        t, _ = ops.sample_along_rays(o, d, self.num_coarse_samples, near, far, t_rand, want_coords=False, lindisp=self.lindisp)
        mlps = [self.coarse_mlp, self.fine_mlp]
        if training:
            # (limits of this unmerged path -- one launch set per level, no merged three-launch forward, no one-launch chain -- named up
            # front, not as AON_E_INVALID from inside loss.backward() after a full forward: ADVICE r4)
            s_last = self.num_coarse_samples + 1 + (self.num_levels - 1) * self.num_fine_samples
            if s_last > 512:
                raise NotImplementedError(f"training with num_levels={self.num_levels}: level {self.num_levels - 1} evaluates {s_last} samples per ray, "
                                          "the compositing backward (aon_composite_bwd) holds at most 512; inference has no such limit")
            if self.noise_std > 0 and randomized:
                raise NotImplementedError("training with num_levels > 2 AND density noise (noise_std > 0, randomized=True): the stage-level "
                                          "compositing backward takes no noise; inference with noise, and training with noise at num_levels <= 2, work")
            if n == 0:
                raise ValueError("empty ray batch in training mode")
            packs = [(m.packed(True), m.packed_bwd(True)) for m in mlps]
        else:
            packed = [m.packed() for m in mlps]
        ret, weights = [], None
        for lvl in range(self.num_levels):
            if lvl > 0:
                ul = us[lvl - 1] if lvl - 1 < len(us) else None
                if randomized and ul is None:
                    ul = torch.rand((n, self.num_fine_samples), device=o.device)
                t = ops.sample_pdf_t_n(t, weights, self.num_fine_samples, ul if randomized else None)
            k = min(lvl, 1)
            if training:
                comp, acc, depth, weights = RenderLevelVanilla.apply(o, d, v, t, bool(white_bkgd), packs[k][0], packs[k][1], *mlps[k].ordered_params())
            else:
                raw = ops.mlp_fwd(packed[k], o, d, v, t)
                nz = None
                if self.noise_std > 0 and randomized:
                    nz = noise[lvl] if (noise is not None and lvl < len(noise) and noise[lvl] is not None) else torch.rand(t.shape, device=o.device)
                comp, acc, weights, depth = ops.composite_raw(raw, t, d, white_bkgd, ops.ACT_VANILLA, True, opts=self._opts if nz is not None else None, noise=nz)
            ret.append((comp, acc, depth))
        return ret

    def forward(self, rays, randomized, white_bkgd, near, far, t_rand=None, u=None, noise=None, occupancy=None, early_stop=None, ray_live=None):
        """``occupancy`` (ops.OccupancyGrid, occupancy.build_occupancy): inference that skips every sample in an empty cell of the grid
        (DESIGN.md section 4.9); refused with randomized sampling or grad mode.  None: the exact path.
        ``early_stop`` (eps in [0, 1), with or without a grid): a ray stops once its transmittance has fallen to eps (DESIGN.md section
        4.10); the same refusals.  None: no termination.
        ``near`` / ``far``: numbers, or the (N, 1) tensors of helper.get_ray_limits, as the reference's forward takes them (DESIGN.md section
        4.11).  ``ray_live`` ((N,) uint8, ops.ray_limits): inference only; a dead ray runs no MLP and returns the background."""
        rays_o = rays["rays_o"]
        n = rays_o.shape[0]
        per_ray = isinstance(near, torch.Tensor) or isinstance(far, torch.Tensor)
        if ray_live is not None and (randomized or torch.is_grad_enabled() or self.num_levels > 2):
            raise ValueError("ray_live is inference only: randomized=False, under torch.no_grad(), one or two levels")
        if occupancy is not None or early_stop is not None:
            return self._forward_occupancy(rays, randomized, white_bkgd, near, far, u, occupancy, early_stop, ray_live)
        t_rand, u = _draw_samples(self, rays, randomized, t_rand, u)
        noise = _draw_noise(self, noise, randomized, n, rays_o.device) if self.num_levels <= 2 else noise
        training = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        # a FROZEN network whose rays require grad (refining a camera pose, LitNeRF.fit_pose): the training forward and a backward that ends at
        # rays_o, rays_d and viewdirs.  A parameter that trains, anywhere, keeps the path it took: its rays get none.
        if torch.is_grad_enabled() and not training and any(getattr(rays[k], "requires_grad", False) for k in ("rays_o", "rays_d", "viewdirs")):
            if self.num_levels > 2:
                raise ValueError("ray gradients (a ray tensor requires grad on a frozen network) are served for one or two levels, not for "
                                 f"num_levels={self.num_levels}")
            if self._general or not self._fused_inference:
                raise ValueError("ray gradients (a ray tensor requires grad on a frozen network) are served by the fused kernels only: this "
                                 "network's geometry runs on the layer-wise engine")
            return self._forward_ray_grads(rays, white_bkgd, near, far, t_rand, u, noise)
        if self.num_levels > 2:
            if self._general or not self.coarse_mlp.geometry.is_default:
                raise NotImplementedError("num_levels > 2 is served for the default network geometry / encoding degrees only")
            return self._forward_many_levels(rays, randomized, white_bkgd, near, far, t_rand, u, noise, training=training)
        layerwise = self._general or not self._fused_inference or (training and not self._fused_training and not self.coarse_mlp.geometry.is_default)
        if layerwise:
            if per_ray or ray_live is not None:
                raise ValueError("per-ray near / far tensors and ray_live are served by the fused kernels only: this network's geometry runs on the "
                                 "layer-wise engine, which takes scalar near / far")
            geom = self.coarse_mlp.geometry
            mlps = [self.coarse_mlp, self.fine_mlp][: self.num_levels]
            if training:
                if n == 0:
                    raise ValueError("empty ray batch in training mode")
                params = [p for m in mlps for p in m.ordered_params()]
                flat = RenderGeneral.apply(rays_o, rays["rays_d"], rays["viewdirs"], float(near), float(far), bool(white_bkgd),
                                           self.num_levels, t_rand, u, geom, self._opts, noise, *params)
                return [tuple(flat[3 * i: 3 * i + 3]) for i in range(self.num_levels)]
            pd = [dict(m.named_parameters()) for m in mlps]
            outs = ops.grender_fwd(geom, pd[0], pd[1] if self.num_levels == 2 else None, rays_o, rays["rays_d"], rays["viewdirs"], near, far,
                                   white_bkgd, self.num_levels, t_rand, u, opts=self._opts, noise=noise)
            return [tuple(o) for o in outs]
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            # training: fused forward that keeps the activation planes + HIP backward (autograd.RenderVanilla)
            if n == 0:
                raise ValueError("empty ray batch in training mode")
            mlps = [self.coarse_mlp, self.fine_mlp][: self.num_levels]
            packs = self._vanilla_packs(mlps)
            params = [p for m in mlps for p in m.ordered_params()]
            flat = RenderVanilla.apply(rays_o, rays["rays_d"], rays["viewdirs"], *[x.detach() if isinstance(x, torch.Tensor) else float(x) for x in (near, far)], bool(white_bkgd),
                                       self.num_levels, t_rand, u, packs, self._opts, noise, *params)
            return [tuple(flat[3 * i: 3 * i + 3]) for i in range(self.num_levels)]
        coarse = self.coarse_mlp.packed()
        fine = self.fine_mlp.packed() if self.num_levels == 2 else None
        outs = ops.render_fwd(coarse, fine, rays_o, rays["rays_d"], rays["viewdirs"], near, far,
                              white_bkgd, self.num_levels, t_rand, u, opts=self._opts, noise=noise, ray_live=ray_live)
        return [tuple(o) for o in outs]

    def _vanilla_packs(self, mlps):
        """Per level (forward stream, transposed stream), freshly packed from the live parameters for one autograd graph."""
        degs = [(m.min_deg_point, m.max_deg_point, m.deg_view) for m in mlps]
        if len(mlps) == 2 and degs[0] == degs[1]:
            # both networks' forward and transposed streams in ONE C call -- the eight fp64 fold products as one launch in front
            # instead of four in a row with their pack kernels (aon_vanilla_pack_step; the same bytes in every buffer)
            return ops.vanilla_pack_step(dict(mlps[0].named_parameters()), dict(mlps[1].named_parameters()), degrees=degs[0])
        bwd = [m.packed_bwd(True) for m in mlps]
        return [(m.packed(True), b) for m, b in zip(mlps, bwd)]

    def _forward_ray_grads(self, rays, white_bkgd, near, far, t_rand, u, noise):
        if rays["rays_o"].shape[0] == 0:
            raise ValueError("empty ray batch under grad mode")
        mlps = [self.coarse_mlp, self.fine_mlp][: self.num_levels]
        params = [p for m in mlps for p in m.ordered_params()]
        flat = RenderVanillaInputs.apply(rays["rays_o"], rays["rays_d"], rays["viewdirs"],
                                         *[x.detach() if isinstance(x, torch.Tensor) else float(x) for x in (near, far)], bool(white_bkgd),
                                         self.num_levels, t_rand, u, self._vanilla_packs(mlps), self._opts, noise, *params)
        return [tuple(flat[3 * i: 3 * i + 3]) for i in range(self.num_levels)]

    def _forward_occupancy(self, rays, randomized, white_bkgd, near, far, u, occupancy, early_stop=None, ray_live=None):
        if randomized:
            raise ValueError("occupancy rendering is inference only: randomized=True is refused")
        if torch.is_grad_enabled():
            raise RuntimeError("occupancy rendering is inference only: call it under torch.no_grad()")
        if self.num_levels > 2 or self._general or not self.coarse_mlp.geometry.is_default:
            raise NotImplementedError("occupancy rendering serves the default network geometry and encoding degrees with 1 or 2 levels")
        if self.noise_std > 0:
            raise NotImplementedError("occupancy rendering takes no density noise (noise_std > 0)")
        if early_stop is not None:
            outs, _, _ = ops.render_fwd_stop(self.coarse_mlp.packed(), self.fine_mlp.packed() if self.num_levels == 2 else None, rays["rays_o"],
                                             rays["rays_d"], rays["viewdirs"], near, far, white_bkgd, occupancy, early_stop,
                                             num_levels=self.num_levels, u=u, opts=self._opts, ray_live=ray_live)
            return [tuple(o) for o in outs]
        outs, _ = ops.render_fwd_occ(self.coarse_mlp.packed(), self.fine_mlp.packed() if self.num_levels == 2 else None, rays["rays_o"],
                                     rays["rays_d"], rays["viewdirs"], near, far, white_bkgd, occupancy, self.num_levels, u, opts=self._opts,
                                     ray_live=ray_live)
        return [tuple(o) for o in outs]

    def _level_mlp(self, level: str):
        if level not in ("coarse", "fine"):
            raise ValueError(f"level must be 'coarse' or 'fine', got {level!r}")
        if level == "fine" and self.num_levels < 2:
            raise ValueError("a one-level NeRF has no fine network")
        return self.fine_mlp if level == "fine" else self.coarse_mlp

    @torch.no_grad()
    def density_grid(self, bounds, resolution, level: str = "fine", chunk: int = 1 << 18) -> torch.Tensor:
        """relu density (model.py:187) of the `level` network at the points of a grid spanning bounds = (lo, hi) (a number or 3 numbers each)
        with `resolution` points per axis (an int or 3 ints) -> (nx, ny, nz) fp32, C order (ops.grid_points: x_a = lo_a + idx_a * step_a).
        The default geometry (degrees 0, 10, 4) runs the fused grid kernel (ops.density_grid); any other geometry evaluates the points
        through the per-point route, `chunk` points at a time: ops.pos_enc + the network's own forward (the layer-wise engine)."""
        mlp = self._level_mlp(level)
        lo, hi = bounds
        dims = ops._dims3(resolution)
        if mlp.geometry.is_default:
            return ops.density_grid(mlp.packed(), dims, lo, hi, ops.ACT_VANILLA)
        dev = next(mlp.parameters()).device
        P = dims[0] * dims[1] * dims[2]
        out = torch.empty(P, dtype=torch.float32, device=dev)
        for b in range(0, P, chunk):
            e = min(P, b + chunk)
            pts = ops.grid_points(dims, lo, hi, b, e, device=dev)
            enc = ops.pos_enc(pts[:, None, :], self.min_deg_point, self.max_deg_point)
            cond = ops.pos_enc(torch.zeros_like(pts), 0, self.deg_view)   # the density does not depend on the view direction
            _, raw_sigma = mlp(enc, cond)
            out[b:e] = torch.relu(raw_sigma.reshape(-1))
        return out.view(*dims)


# --------------------------------------------------------------------------------------------------------------------
# Harness-level equivalents of the reference's LightningModule methods, without pytorch-lightning.
# --------------------------------------------------------------------------------------------------------------------
import math
from types import SimpleNamespace

from . import helper
from ..interface import Harness


def _ray_box_limits(ray_box, batch):
    """LitNeRF / LitNeRF_AutoDecoder(ray_box=...): (near, far, live) of ALL rays of `batch` -- the reference's min / max fallback for the
    rays that miss the box is a property of the ray set, so an image's limits are computed once, before its chunk loop."""
    return ops.ray_limits(batch["rays_o"], batch["rays_d"], ray_box)


def _fused_adam(params) -> bool:
    """torch.optim.Adam's fused form when every parameter lives on a GPU (AON_FUSED_ADAM=0 in the environment: the foreach form, A/B)."""
    import os

    return os.environ.get("AON_FUSED_ADAM", "1") != "0" and all(p.is_cuda for p in params)


def build_adam(modules, lr: float):
    """``torch.optim.Adam(params, lr, betas=(0.9, 0.999))`` of the reference's ``configure_optimizers`` (model.py:386-389,
    model_autodecoder.py:604-606).  On a GPU (round 6): the parameters move into ONE flat arena and the optimizer is ``ArenaAdam`` -- the
    same update as ONE HIP launch, the HIP backward writes the gradients into the arena, the data-parallel mean reduces it in place
    (``aon_amd/arena.py``).  ``state_dict`` keeps torch.optim.Adam's layout.  AON_ARENA=0 in the environment (A/B) or CPU parameters:
    torch's own Adam (fused form on a GPU)."""
    import os

    params = [p for m in modules for p in m.parameters()]
    if os.environ.get("AON_ARENA", "1") != "0" and params and all(p.is_cuda and p.dtype == torch.float32 for p in params):
        from ...arena import ArenaAdam, ParamArena

        return ArenaAdam(ParamArena.for_modules(list(modules)), lr=lr, betas=(0.9, 0.999))   # (a second call reuses the arena the parameters live in)
    return torch.optim.Adam(params=params, lr=lr, betas=(0.9, 0.999), fused=_fused_adam(params))


class LitNeRF(Harness):
    """``models/vanilla_nerf/model.py:202-419`` minus Lightning: same method names, batch contracts and return
    structures for ``training_step`` (:256-282), ``render_rays`` (:295-321, fine level only, chunked by ``hparams.chunk``,
    logs val/psnr), ``render_rays_test`` (:323-348), ``validation_step`` (:353-375), ``test_step`` (:377-384),
    ``configure_optimizers`` (:386-389) and the learning-rate rule of ``optimizer_step`` (:391-419).
    Values the reference hands to ``self.log`` are collected in ``self.logged``.  near / far / white_bkgd, which the
    reference copies from its dataset in ``setup`` (:245-254), are constructor arguments here (dataset IO is out of scope)."""

    def __init__(self, hparams=None, lr_init: float = 5.0e-4, lr_final: float = 5.0e-6, lr_delay_steps: int = 2500,
                 lr_delay_mult: float = 0.01, randomized: bool = True, near: float = 2.0, far: float = 6.0, white_bkgd: bool = True,
                 model_kwargs: dict | None = None, ray_box=None):
        super().__init__()
        self._init_harness(hparams, dict(chunk=3840, run_max_steps=100000, img_wh=(640, 480)),  # opt.py:103,112,17
                           lr_init, lr_final, lr_delay_steps, lr_delay_mult, randomized, near, far, white_bkgd, ray_box)
        # the reference builds NeRF() (model.py:218); `model_kwargs` hands its constructor arguments through (sample counts, degrees, ...)
        self.model = NeRF(**(model_kwargs or {}))

    def training_step(self, batch, batch_idx):
        batch = {k: (v if k == "obj_idx" else v.squeeze(0)) for k, v in batch.items()}
        near, far = self.near, self.far
        if self.ray_box is not None:
            near, far, _ = _ray_box_limits(self.ray_box, batch)
        rendered = self.model(batch, self.randomized, self.white_bkgd, near, far)
        # model.py:271-279: loss0 + loss1 and the three logged values -- one launch forward, one backward (helper.train_loss)
        loss, stats = helper.train_loss(rendered, batch["target"])
        self.log("train/psnr1", stats[5])
        self.log("train/psnr0", stats[4])
        self.log("train/loss", stats[3])
        return loss

    def fit_pose(self, batches, steps: int, lr: float = 5.0e-3, poses=None, seed: int = 0):
        """Refine the camera pose of observed views of the scene with the network FROZEN (iNeRF): `steps` Adam steps
        against training_step's loss (helper.train_loss), view `i % len(batches)` at step i.  LitNeRF_AutoDecoder.fit_pose without codes.

        batches: one dict per VIEW with "directions" (camera-space ray directions, (N, 3) or (H, W, 3): ops.ray_directions, or a subset of
        its pixels) and "target" (N, 3).  poses: the initial (3, 4) camera-to-world matrix of every view.  One 6-vector (omega, tau) is
        kept per view and applied as R = exp([omega]x) R0, t = t0 + tau (ops.rays_from_pose).  seed: of the stratified / inverse-CDF draws
        when the harness samples randomly.  -> (list of corrected (3, 4) poses, per-step losses as one (steps,) device tensor); no host
        synchronisation per step.

        The network's requires_grad flags are cleared for the duration and restored; with them cleared and the rays requiring grad,
        NeRF.forward takes autograd.RenderVanillaInputs.  The views' 6-vectors, their gradients and Adam moments are one flat
        (4, 6 * views) buffer stepped by aon_adam_step; a view's 6-vector keeps its own step count.  Scalar near / far only (a ray box's
        per-ray limits would move with the pose and carry no gradient)."""
        batches, poses = self._fit_args("fit_pose", steps, batches, poses)
        if isinstance(lr, bool) or not isinstance(lr, (int, float)) or not lr > 0:
            raise ValueError(f"fit_pose: lr must be positive, got {lr!r}")
        self._fit_pose_batches(batches)
        fitted, _, losses = self._fit_frozen(batches, steps, seed, poses=poses, lr_pose=lr)
        return fitted, losses

    def _frozen_loss(self, rays, target, near, far, codes, t_rand, u):
        rendered = self.model(rays, self.randomized, self.white_bkgd, near, far, t_rand=t_rand, u=u)
        return helper.train_loss(rendered, target)[0]

    @torch.no_grad()
    def render_rays(self, batch, batch_idx):
        ret = self._render_chunks(batch, whole=("obj_idx",))
        self.log("val/psnr", self.psnr_legacy(ret["comp_rgb"], batch["target"]).mean().item())
        return ret

    @torch.no_grad()
    def render_rays_test(self, batch, batch_idx):
        return {"target": batch["target"], "instance_mask": batch["instance_mask"], "rgb": self._render_chunks(batch)["comp_rgb"]}

    def validation_step(self, batch, batch_idx):
        batch = {k: (v if k == "obj_idx" else v.squeeze(0)) for k, v in batch.items()}
        return self.render_rays(batch, batch_idx)  # the reference renders twice (:367,:375); once is the same result

    def test_step(self, batch, batch_idx):
        batch = {k: v.squeeze(0) if v.dim() > 0 and v.shape[0] == 1 else v for k, v in batch.items()}
        return self.render_rays_test(batch, batch_idx)

    def configure_optimizers(self):
        # model.py:386-389.  On a GPU the optimizer runs in its fused form -- one kernel for all 48 parameter tensors instead of the
        # foreach form's dozen multi-tensor launches: the same update rule, 1 ms of a 32 ms training step (round 5, tools/train_bench.py)
        return build_adam([self], self.lr_init)     # (round 6: ONE launch on a parameter arena; torch.optim.Adam's state layout)
