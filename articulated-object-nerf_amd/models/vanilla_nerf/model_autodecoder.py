"""Drop-in articulated ``NeRFMLP`` / ``NeRF_AE_Art`` (reference ``models/vanilla_nerf/model_autodecoder.py:60-337``):
same constructor defaults, parameter names (``deformations_linear.*``, ``deformation_layer``, ``pts_linears.*``,
``views_linear.*``, ``bottleneck_layer``, ``density_layer``, ``rgb_layer`` under ``coarse_mlp`` / ``fine_mlp``) and
``forward`` signatures, running on the fused HIP kernels.  Only the reference's default geometry
(deformation_mlp=True, enc_after=True, embed_deg=False, 4x128 deformation and view branches) has kernels."""
from __future__ import annotations

import contextlib

import torch
import torch.nn as nn
import torch.nn.init as init

from ... import fit, ops
from ...autograd import RenderArticulated, RenderArticulatedInputs, RenderArticulatedLatents
from .model import WeightStreams, _draw_noise, _draw_samples


class NeRFMLP(WeightStreams, nn.Module):
    """model_autodecoder.py:60-239.  ``forward(pos, condition, latents)``: pos (N,S,3) un-encoded sample positions,
    condition (N,27) encoded view dirs, latents {"density": (1,128), "color": (1,128), "articulation": (1,32)}
    -> (raw_rgb (N,S,3), raw_density (N,S,1))."""

    def __init__(self, min_deg_point, max_deg_point, deg_view, netdepth: int = 8, netwidth: int = 256,
                 netdepth_deformation=4, netwidth_deformation: int = 128, netdepth_condition: int = 4,
                 netwidth_condition: int = 128, shape_latent_dim=128, appearance_latent_dim=128,
                 articulation_latent_dim=32, skip_layer: int = 4, input_ch: int = 3, input_ch_view: int = 3,
                 num_rgb_channels: int = 3, num_density_channels: int = 1, deformation_mlp: bool = True,
                 enc_after: bool = True, embed_deg: bool = False):
        super().__init__()
        geometry = (min_deg_point, max_deg_point, deg_view, netdepth, netwidth, netdepth_deformation, netwidth_deformation,
                    netdepth_condition, netwidth_condition, shape_latent_dim, appearance_latent_dim, articulation_latent_dim,
                    skip_layer, input_ch, input_ch_view, num_rgb_channels, num_density_channels, deformation_mlp, enc_after,
                    embed_deg)
        if geometry[3:] != (8, 256, 4, 128, 4, 128, 128, 128, 32, 4, 3, 3, 3, 1, True, True, False):
            raise NotImplementedError(f"articulated NeRFMLP geometry {geometry} has no HIP kernel (the reference's default widths / latent sizes "
                                      "do, at any encoding degrees of up to 10 position and 4 view levels; enc_after=False and embed_deg=True "
                                      "change the network, model_autodecoder.py:95-103,181-184)")
        # round 4: other encoding degrees on the same kernels (zero-weight slots + run-time encoding scales, aon_pack_art_mlp_deg)
        self.degrees = (int(min_deg_point), int(max_deg_point), int(deg_view))
        ops.art_param_shapes(self.degrees)      # raises for more than 10 / 4 levels
        self.net_activation = nn.ReLU()
        self.enc_after, self.embed_deg, self.deformation_mlp = enc_after, embed_deg, deformation_mlp
        self.netdepth, self.netdepth_deformation, self.netdepth_condition, self.skip_layer = netdepth, 4, 4, skip_layer
        self.min_deg_point, self.max_deg_point, self.deg_view = min_deg_point, max_deg_point, deg_view
        self.num_rgb_channels, self.num_density_channels = num_rgb_channels, num_density_channels
        deform = [nn.Linear(3 + 128 + 32, 128)] + [nn.Linear(128, 128) for _ in range(3)]
        self.deformations_linear = nn.ModuleList(deform)
        self.deformation_layer = nn.Linear(128, 3)
        pos_size = ((max_deg_point - min_deg_point) * 2 + 1) * 3 + 128        # model_autodecoder.py:127-129
        view_pos_size = (deg_view * 2 + 1) * 3                                # :91
        pts = [nn.Linear(pos_size, 256)]
        for idx in range(7):
            pts.append(nn.Linear(256 + pos_size if (idx % skip_layer == 0 and idx > 0) else 256, 256))
        self.pts_linears = nn.ModuleList(pts)
        self.views_linear = nn.ModuleList([nn.Linear(256 + view_pos_size + 128, 128)] + [nn.Linear(128, 128) for _ in range(3)])
        self.bottleneck_layer = nn.Linear(256, 256)
        self.density_layer = nn.Linear(256, 1)
        self.rgb_layer = nn.Linear(128, 3)
        for m in list(self.deformations_linear) + [self.deformation_layer] + list(self.pts_linears) + \
                list(self.views_linear)[1:] + [self.bottleneck_layer, self.density_layer, self.rgb_layer]:
            init.xavier_uniform_(m.weight)  # views_linear[0] keeps the default init, like the reference (:147-151)
        self._streams = {}

    # the weight streams: model.WeightStreams
    _PACKERS = {"fwd": "pack_art_mlp", "bwd": "pack_art_mlp_bwd"}
    _BYTES = {"fwd": "aon_art_packed_bytes", "bwd": "aon_art_bwd_packed_bytes", "small": "aon_art_small_bytes"}

    def _pack_degrees(self):
        return {"degrees": self.degrees}

    def ordered_params(self):
        params = dict(self.named_parameters())
        return [params[name] for name in ops.ART_PARAM_ORDER]

    def prepared(self, latents: dict) -> torch.Tensor:
        """Per-call latent-folded block (cheap: ~0.1 MFLOP); always rebuilt because latents are call arguments."""
        params = dict(self.named_parameters())
        dev = next(iter(params.values())).device
        return ops.art_prepare(params, latents, out=self._stream_buffer("small", dev), degrees=self.degrees)

    def forward(self, pos, condition, latents):
        if self.embed_deg:
            raise NotImplementedError
        dv = self.degrees[2]
        if dv != 4:   # the kernel reads the view encoding in its 27-wide slot layout [v ; sin block of 12 ; shifted block of 12]
            padded = condition.new_zeros((condition.shape[0], 27))
            padded[:, : 3 + 3 * dv] = condition[:, : 3 + 3 * dv]
            padded[:, 15: 15 + 3 * dv] = condition[:, 3 + 3 * dv:]
            condition = padded
        raw = ops.art_mlp_fwd_pos(self.packed(), self.prepared(latents), pos, condition)
        return raw[..., :3], raw[..., 3:4]


class NeRF_AE_Art(nn.Module):
    """model_autodecoder.py:242-337.  ``forward(rays, randomized, white_bkgd, near, far, latents, train=True)`` ->
    ``[(comp_rgb, acc, depth)_coarse, (comp_rgb, acc, depth)_fine]`` with rgb = sigmoid(raw)*(1+2*0.001)-0.001 and
    sigma = softplus(raw - 1)."""

    def __init__(self, num_levels: int = 2, min_deg_point: int = 0, max_deg_point: int = 10, deg_view: int = 4,
                 num_coarse_samples: int = 64, num_fine_samples: int = 128, use_viewdirs: bool = True,
                 noise_std: float = 0.0, lindisp: bool = False, rgb_padding: float = 0.001, density_bias: float = -1.0,
                 enc_after=True, embed_deg=False):
        super().__init__()
        if (enc_after, embed_deg) != (True, False) or num_levels not in (1, 2):
            raise NotImplementedError("enc_after=False / embed_deg=True change the network (model_autodecoder.py:95-103,181-184): only the "
                                      "reference's default articulated NeRFMLP has HIP kernels; num_levels must be 1 or 2")
        # sample counts, lindisp, noise_std, rgb_padding and density_bias are runtime arguments of the C calls (aon_render_opts)
        self._opts = ops.RenderOpts(num_coarse_samples, num_fine_samples, lindisp, noise_std, rgb_padding, density_bias,
                                    degrees=(min_deg_point, max_deg_point, deg_view))   # (read by the backward for the gradients' layout)
        self.use_viewdirs, self.noise_std, self.lindisp = use_viewdirs, noise_std, lindisp
        self.num_levels, self.min_deg_point, self.max_deg_point, self.deg_view = num_levels, min_deg_point, max_deg_point, deg_view
        self.num_coarse_samples, self.num_fine_samples = num_coarse_samples, num_fine_samples
        self.rgb_padding, self.density_bias, self.enc_after, self.embed_deg = rgb_padding, density_bias, enc_after, embed_deg
        self.rgb_activation = nn.Sigmoid()
        self.sigma_activation = nn.Softplus()
        self.coarse_mlp = NeRFMLP(min_deg_point, max_deg_point, deg_view)
        self.fine_mlp = NeRFMLP(min_deg_point, max_deg_point, deg_view)

    def forward(self, rays, randomized, white_bkgd, near, far, latents, train=True, t_rand=None, u=None, noise=None, occupancy=None,
                early_stop=None, ray_live=None):
        """``occupancy`` (ops.OccupancyGrid built under the same latents, occupancy.build_occupancy): inference that skips every sample in an
        empty cell of the grid; refused with randomized sampling or grad mode.  None: the exact path.
        ``early_stop`` (eps in [0, 1), with or without a grid): a ray stops once its transmittance has fallen to eps (DESIGN.md section
        4.10); the same refusals.  None: no termination.
        ``near`` / ``far``: numbers, or the (N, 1) tensors of helper.get_ray_limits, as the reference's forward takes them (DESIGN.md section
        4.11).  ``ray_live`` ((N,) uint8, ops.ray_limits): inference only; a dead ray runs no MLP and returns the background."""
        rays_o = rays["rays_o"]
        n = rays_o.shape[0]
        if ray_live is not None and (randomized or torch.is_grad_enabled()):
            raise ValueError("ray_live is inference only: randomized=False, under torch.no_grad()")
        if occupancy is not None or early_stop is not None:
            if randomized:
                raise ValueError("occupancy rendering is inference only: randomized=True is refused")
            if torch.is_grad_enabled():
                raise RuntimeError("occupancy rendering is inference only: call it under torch.no_grad()")
            if self.noise_std > 0:
                raise NotImplementedError("occupancy rendering takes no density noise (noise_std > 0)")
            two = self.num_levels == 2
            if early_stop is not None:
                outs, _, _ = ops.art_render_fwd_stop(self.coarse_mlp.packed(), self.coarse_mlp.prepared(latents), self.fine_mlp.packed() if two else None,
                                                     self.fine_mlp.prepared(latents) if two else None, rays_o, rays["rays_d"], rays["viewdirs"], near,
                                                     far, white_bkgd, occupancy, early_stop, num_levels=self.num_levels, u=u, opts=self._opts,
                                                     ray_live=ray_live)
                return [tuple(o) for o in outs]
            outs, _ = ops.art_render_fwd_occ(self.coarse_mlp.packed(), self.coarse_mlp.prepared(latents), self.fine_mlp.packed() if two else None,
                                             self.fine_mlp.prepared(latents) if two else None, rays_o, rays["rays_d"], rays["viewdirs"], near, far,
                                             white_bkgd, occupancy, self.num_levels, u, opts=self._opts, ray_live=ray_live)
            return [tuple(o) for o in outs]
        t_rand, u = _draw_samples(self, rays, randomized, t_rand, u)
        noise = _draw_noise(self, noise, randomized, n, rays_o.device)   # model_autodecoder.py:318-319
        ray_grad = any(getattr(rays[k], "requires_grad", False) for k in ("rays_o", "rays_d", "viewdirs"))
        if torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters())
                                        or any(getattr(v, "requires_grad", False) for v in latents.values()) or ray_grad):
            # training: HIP forward that keeps the activation planes + HIP backward (autograd.RenderArticulated);
            # the per-call block must not alias the cached inference buffer (it is saved for backward)
            mlps = [self.coarse_mlp, self.fine_mlp][: self.num_levels]
            if len(mlps) == 2 and mlps[0].degrees == mlps[1].degrees:
                # both networks' streams, per-call blocks and transposed streams in ONE C call -- the four fp64 fold products as one
                # launch in front instead of four in a row with their pack kernels (aon_art_pack_step; the same bytes in every buffer)
                packs = ops.art_pack_step(dict(mlps[0].named_parameters()), dict(mlps[1].named_parameters()), latents, degrees=mlps[0].degrees)
            else:
                bwd = [m.packed_bwd(True) for m in mlps]
                # per level: the per-call latent-folded block + the forward weight stream (prepare | fold -> pack)
                small = [ops.art_prepare(dict(m.named_parameters()), latents, degrees=m.degrees) for m in mlps]
                packs = [(m.packed(True), sm, b) for m, sm, b in zip(mlps, small, bwd)]
            params = [p for mlp in mlps for p in mlp.ordered_params()]
            # a frozen network (only latents require grad: fitting codes, LitNeRF_AutoDecoder.fit_latents): the same forward and the same latent
            # gradients, bit for bit, from a backward without the weight-gradient stage
            # ... and when, on a frozen network, a ray tensor requires grad (refining a camera pose, LitNeRF_AutoDecoder.fit_pose): that backward
            # plus the gradients of rays_o, rays_d and viewdirs.  A network that trains gives the rays none, as ever.
            render = RenderArticulated if any(p.requires_grad for p in params) else (RenderArticulatedInputs if ray_grad else RenderArticulatedLatents)
            flat = render.apply(rays_o, rays["rays_d"], rays["viewdirs"], *[x.detach() if isinstance(x, torch.Tensor) else float(x) for x in (near, far)], bool(white_bkgd),
                                self.num_levels, t_rand, u, packs, self._opts, noise, latents["density"], latents["color"],
                                latents["articulation"], *params)
            return [tuple(flat[3 * i: 3 * i + 3]) for i in range(self.num_levels)]
        two = self.num_levels == 2
        pc = self.coarse_mlp.packed()
        pf = self.fine_mlp.packed() if two else None
        outs = ops.art_render_fwd(pc, self.coarse_mlp.prepared(latents), pf, self.fine_mlp.prepared(latents) if two else None,
                                  rays_o, rays["rays_d"], rays["viewdirs"], near, far, white_bkgd, self.num_levels, t_rand, u,
                                  opts=self._opts, noise=noise, ray_live=ray_live)
        return [tuple(o) for o in outs]

    def _level_mlp(self, level: str):
        if level not in ("coarse", "fine"):
            raise ValueError(f"level must be 'coarse' or 'fine', got {level!r}")
        if level == "fine" and self.num_levels < 2:
            raise ValueError("a one-level NeRF_AE_Art has no fine network")
        return self.fine_mlp if level == "fine" else self.coarse_mlp

    @torch.no_grad()
    def density_grid(self, bounds, resolution, latents: dict, level: str = "fine") -> torch.Tensor:
        """softplus(raw - 1) density (model_autodecoder.py:318-323) of the `level` network under `latents` (the code library's "density",
        "color", "articulation" rows) at the points of a grid spanning bounds = (lo, hi) with `resolution` points per axis -> (nx, ny, nz)
        fp32, C order (ops.grid_points).  One fused launch at every encoding degree set (ops.density_grid)."""
        if float(self.density_bias) != -1.0:
            raise NotImplementedError("the grid kernel's articulated activation is softplus(raw - 1): density_bias must be -1.0")
        mlp = self._level_mlp(level)
        lo, hi = bounds
        return ops.density_grid(mlp.packed(), ops._dims3(resolution), lo, hi, ops.ACT_ARTICULATED, small=mlp.prepared(latents))


# --------------------------------------------------------------------------------------------------------------------
from . import helper  # noqa: E402
from ..code_library import CodeLibraryArticulated  # noqa: E402
from ..interface import Harness  # noqa: E402
from .model import _ray_box_limits, build_adam  # noqa: E402

_SCALAR_KEYS = ("deg", "instance_id", "articulation_id")


class LitNeRF_AutoDecoder(Harness):
    """``model_autodecoder.py:340-701`` minus Lightning: ``NeRF_AE_Art`` + ``CodeLibraryArticulated`` with the
    reference's ``training_step`` (:393-477: mse(coarse)+mse(fine) + 1e-4 * latent-norm regulariser), ``render_rays``
    (:479-513, fine level, chunked, logs val/psnr and the object-pixel PSNR), ``render_rays_test`` (:515-543),
    ``validation_step`` (:548-586, wandb image grid dropped), ``test_step`` (:588-605, test-time interpolated
    articulation codes), ``configure_optimizers`` (:607-609: one Adam over model + code library) and the
    learning-rate rule (:611-640).  near / far / white_bkgd come from the dataset in the reference's ``setup``
    (:359-391); ``setup(dataset)`` copies them the same way."""

    def __init__(self, hparams=None, lr_init: float = 5.0e-4, lr_final: float = 5.0e-6, lr_delay_steps: int = 2500,
                 lr_delay_mult: float = 0.01, randomized: bool = True, near: float = 2.0, far: float = 6.0, white_bkgd: bool = True,
                 model_kwargs: dict | None = None, ray_box=None):
        super().__init__()
        self._init_harness(hparams, dict(chunk=3840, run_max_steps=100000, img_wh=(320, 240), N_max_objs=1, N_obj_code_length=128),
                           lr_init, lr_final, lr_delay_steps, lr_delay_mult, randomized, near, far, white_bkgd, ray_box)
        self.model = NeRF_AE_Art(**(model_kwargs or {}))   # the reference builds NeRF_AE_Art() (model_autodecoder.py:352)
        self.code_library = CodeLibraryArticulated(self.hparams)

    @property
    def _scene_grids(self) -> dict:
        """render_scene(occupancy=...)'s grids, keyed by (instance_id, articulation, arguments); not a module attribute torch would see.
        The dict is emptied whenever a parameter of the network or of the code library has been replaced or written through autograd's
        version counter since the grids were built: an optimiser step, `load_state_dict` on this module or on `model` / `code_library`,
        `p.copy_()`, `p.mul_()` ...  A write that bypasses the counter (`p.data.copy_()`) is not seen: call clear_scene_grids()."""
        stamp = tuple((p.data_ptr(), p._version) for m in (self.model, self.code_library) for p in m.parameters())
        if self.__dict__.get("_scene_grid_stamp") != stamp:
            self.__dict__["_scene_grid_stamp"] = stamp
            self.__dict__["_scene_grid_cache"] = {}
        return self.__dict__.setdefault("_scene_grid_cache", {})

    def clear_scene_grids(self) -> None:
        """Drop the occupancy grids render_scene(occupancy=...) keeps (after a change of the weights that torch's version counters miss)."""
        self.__dict__["_scene_grid_cache"] = {}

    def setup(self, dataset):
        self.near, self.far, self.white_bkgd = dataset.near, dataset.far, dataset.white_back

    @staticmethod
    def _unbatch(batch):
        return {k: (v if k in _SCALAR_KEYS else v.squeeze(0)) for k, v in batch.items()}

    def training_step(self, batch, batch_idx):
        batch = self._unbatch(batch)
        latents = self.code_library(batch)
        near, far = self.near, self.far
        if self.ray_box is not None:
            near, far, _ = _ray_box_limits(self.ray_box, batch)
        rendered = self.model(batch, self.randomized, self.white_bkgd, near, far, latents)
        # model_autodecoder.py:455-477: loss1 + loss0 + 1e-4 * (mean ||shape|| + mean ||appearance|| + mean ||articulation||) and the four
        # logged values -- one launch forward, one backward (helper.train_loss) where torch runs ~47
        loss, stats = helper.train_loss(rendered, batch["target"], (latents["density"], latents["color"], latents["articulation"]), 1e-4)
        self.log("train/psnr1", stats[5])
        self.log("train/psnr0", stats[4])
        self.log("train/loss", stats[3])
        self.log("train/loss/reg", stats[2])
        return loss

    def _initial_latents(self, init, dev) -> dict:
        """`init` of fit_latents -> {"density": (1,128), "color": (1,128), "articulation": (1,32)} fp32 copies on `dev`."""
        lib3 = self.code_library
        tables = {"density": lib3.embedding_instance_shape.weight, "color": lib3.embedding_instance_appearance.weight,
                  "articulation": lib3.embedding_instance_articulation.weight}
        if isinstance(init, str):
            if init != "mean":
                raise ValueError(f"fit_latents: init must be a dict of three tensors, 'mean' or (instance_id, articulation_id), got {init!r}")
            out = {k: w.detach().mean(dim=0, keepdim=True) for k, w in tables.items()}   # column means of the library's tables
        elif isinstance(init, dict):
            if set(init) != set(tables):
                raise ValueError(f"fit_latents: init dict needs exactly the keys {sorted(tables)}, got {sorted(init)}")
            out = {}
            for k, w in tables.items():
                t = torch.as_tensor(init[k])
                if t.numel() != w.shape[1]:
                    raise ValueError(f"fit_latents: init[{k!r}] must hold {w.shape[1]} values, got {tuple(t.shape)}")
                out[k] = t.detach().reshape(1, -1)
        elif isinstance(init, (tuple, list)) and len(init) == 2 and all(isinstance(i, int) and not isinstance(i, bool) for i in init):
            iid, aid = init
            if not (0 <= iid < tables["density"].shape[0] and 0 <= aid < tables["articulation"].shape[0]):
                raise ValueError(f"fit_latents: init ids {tuple(init)} outside the library ({tables['density'].shape[0]} instances, "
                                 f"{tables['articulation'].shape[0]} articulation states)")
            out = {"density": tables["density"].detach()[iid: iid + 1], "color": tables["color"].detach()[iid: iid + 1],
                   "articulation": tables["articulation"].detach()[aid: aid + 1]}
        else:
            raise ValueError(f"fit_latents: init must be a dict of three tensors, 'mean' or (instance_id, articulation_id), got {init!r}")
        return {k: v.to(device=dev, dtype=torch.float32).clone() for k, v in out.items()}

    def fit_latents(self, batches, steps: int, lr: float = 5.0e-3, init="mean", seed: int = 0, full_backward: bool = False):
        """Fit the three codes of ONE object / joint state to observed rays with the network FROZEN (what an auto-decoder does with an
        instance that is not in its library): `steps` Adam steps on the 288 latent floats against the reference's training_step loss
        (helper.train_loss: mse(fine) + mse(coarse) + 1e-4 * latent norms, model_autodecoder.py:428-466), batch `i % len(batches)` at step i.

        batches: training batches of that one object (the dicts training_step takes; instance / articulation ids are ignored).
        init: a dict {"density", "color", "articulation"} of tensors, "mean" (column means of the library's tables), or
        (instance_id, articulation_id) (those rows of the library).  seed: of the stratified / inverse-CDF draws when the harness samples
        randomly.  -> (latents dict of (1, dim) tensors, per-step losses as one (steps,) device tensor); no host synchronisation per step.

        The network's requires_grad flags are cleared for the duration and restored; with them cleared NeRF_AE_Art.forward runs the
        latent-only backward.  The codes, their gradients and the Adam moments are one flat (4, 288) buffer
        stepped by ONE launch (aon_adam_step).  full_backward=True (the A/B partner, tools/latent_fit_bench.py): the network keeps its flags,
        so every step pays the full training backward -- same losses and codes, bit for bit."""
        batches, _ = self._fit_args("fit_latents", steps, batches)
        if not (isinstance(lr, (int, float)) and lr > 0):
            raise ValueError(f"fit_latents: lr must be positive, got {lr!r}")
        lat0 = self._initial_latents(init, next(self.model.parameters()).device)
        _, codes, losses = self._fit_frozen([self._unbatch(b) for b in batches], steps, seed, codes=lat0, lr_codes=lr, fit_codes=True,
                                            freeze=not full_backward)
        return codes, losses

    def _frozen_loss(self, rays, target, near, far, codes, t_rand, u):
        rendered = self.model(rays, self.randomized, self.white_bkgd, near, far, codes, t_rand=t_rand, u=u)
        return helper.train_loss(rendered, target, tuple(codes[k] for k, _ in ops._LATENT_KEYS), 1e-4)[0]

    def fit_pose(self, batches, steps: int, lr=5.0e-3, codes="mean", poses=None, fit_codes: bool = False, seed: int = 0):
        """Refine the camera pose of observed views of ONE object with the network FROZEN (iNeRF-style), alone or
        together with its three codes: `steps` Adam steps against the reference's training_step loss (helper.train_loss), view
        `i % len(batches)` at step i.

        batches: one dict per VIEW with "directions" (camera-space ray directions, (N, 3) or (H, W, 3): ops.ray_directions, or a subset of
        its pixels) and "target" (N, 3).  poses: the initial (3, 4) camera-to-world matrix of every view.  One 6-vector (omega, tau) is
        kept per view and applied as R = exp([omega]x) R0, t = t0 + tau (ops.rays_from_pose).  codes: as fit_latents' `init`.  fit_codes:
        step the (4, 288) code buffer too.  lr: one rate, or (pose rate, code rate).  seed: as fit_latents.
        -> (list of corrected (3, 4) poses, codes dict of (1, dim) tensors, per-step losses as one (steps,) device tensor); no host
        synchronisation per step.

        The network's requires_grad flags are cleared for the duration and restored; with them cleared and the rays requiring grad,
        NeRF_AE_Art.forward takes autograd.RenderArticulatedInputs.  Every buffer is stepped by aon_adam_step; a view's 6-vector keeps its
        own step count.  Scalar near / far only (a ray box's per-ray limits would move with the pose and carry no gradient)."""
        batches, poses = self._fit_args("fit_pose", steps, batches, poses)
        lrs = fit.lr_pair("fit_pose", lr)
        self._fit_pose_batches(batches)
        lat0 = self._initial_latents(codes, next(self.model.parameters()).device)
        return self._fit_frozen(batches, steps, seed, poses=poses, lr_pose=lrs[0], codes=lat0, lr_codes=lrs[1], fit_codes=fit_codes)

    _CHUNK_SKIP = _SCALAR_KEYS

    @torch.no_grad()
    def render_rays(self, batch, latents):
        ret = self._render_chunks(batch, latents, skip=("img_wh", "src_imgs"))
        self.log("val/psnr", self.psnr_legacy(ret["comp_rgb"], batch["target"]).mean().item())
        mask = batch["instance_mask"].view(-1, 1).expand(-1, 3)
        self.log("val/psnr_obj", self.psnr_legacy(ret["comp_rgb"][mask], batch["target"][mask]).mean().item())
        return ret

    @torch.no_grad()
    def render_rays_test(self, batch, latents):
        ret = self._render_chunks(batch, latents, skip=("img_wh", "src_imgs"))
        return {"target": batch["target"], "instance_mask": batch["instance_mask"], "rgb": ret["comp_rgb"]}

    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        batch = self._unbatch(batch)
        return self.render_rays(batch, self.code_library(batch))

    @torch.no_grad()
    def test_step(self, batch, batch_idx):
        batch = self._unbatch(batch)
        return self.render_rays_test(batch, self.code_library(batch, is_test=True))

    def _placement_codes(self, who, placements):
        """``(instance_id, articulation, pose, box)`` placements -> [(instance_id, articulation, latents, pose, box)], the latents looked up in the
        library: ``articulation`` a row index into get_interpolated_articulations or an explicit (32,) code."""
        dev = next(self.model.parameters()).device
        table = self.code_library.get_interpolated_articulations(max_interpolations=2, device=dev)
        n_inst = self.code_library.embedding_instance_shape.weight.shape[0]
        out = []
        for j, placement in enumerate(placements):
            if len(placement) != 4:
                raise ValueError(f"{who}: placement {j} must be (instance_id, articulation, pose, box)")
            iid, art, pose, box = placement
            if isinstance(iid, bool) or not isinstance(iid, int) or not 0 <= iid < n_inst:
                raise ValueError(f"{who}: placement {j}: instance_id {iid!r} outside the library ({n_inst} instances)")
            if isinstance(art, int) and not isinstance(art, bool):
                if not 0 <= art < table.shape[0]:
                    raise ValueError(f"{who}: placement {j}: articulation row {art} outside the {table.shape[0]} interpolated states")
                code = table[art: art + 1]
            else:
                code = torch.as_tensor(art, dtype=torch.float32, device=dev).reshape(1, -1)
            ids = torch.tensor([iid], dtype=torch.int64, device=dev)
            latents = {"density": self.code_library.embedding_instance_shape(ids), "color": self.code_library.embedding_instance_appearance(ids),
                       "articulation": code}
            out.append((iid, art, latents, pose, box))
        return out

    def _scene_fit_placed(self, who, placements, batches):
        """What fit_scene_codes and fit_scene_poses check alike, in this order: the placements and their number, the batches' keys, every
        object's code, pose and box (SceneObject raises) -> _placement_codes' list."""
        from ...scene import SceneObject

        placed = self._placement_codes(who, placements)
        if not 1 <= len(placed) <= ops.SCENE_MAX_OBJECTS:
            raise ValueError(f"{who}: a scene holds 1 to {ops.SCENE_MAX_OBJECTS} objects, got {len(placed)}")
        for b in batches:
            if not all(k in b for k in ("rays_o", "rays_d", "viewdirs", "target")):
                raise ValueError(f"{who}: every batch needs 'rays_o', 'rays_d', 'viewdirs' (world) and 'target'")
        for _, _, latents, pose, box in placed:
            SceneObject(latents, pose, box)
        return placed

    @staticmethod
    def _scene_fit_background(who, background):
        """background=None, or a scene.SceneBackground -> the module to freeze beside the scene network (None without a backdrop)"""
        from ...scene import SceneBackground

        if background is None:
            return None
        if not isinstance(background, SceneBackground):
            raise TypeError(f"{who}: background must be a scene.SceneBackground or None, got {type(background)}")
        return background.model

    def _scene_fit_loss(self, objects, batch, dev, reg_codes=None, background=None):
        """mse over the levels of `objects` rendered on the batch's rays against its target, plus the code-norm penalty of reg_codes.
        background: a scene.SceneBackground standing behind the objects, or None."""
        from ...scene import render_scene_background_grad, render_scene_grad

        rays = {k: batch[k].to(device=dev, dtype=torch.float32).reshape(-1, 3) for k in ("rays_o", "rays_d", "viewdirs")}
        target = batch["target"].to(device=dev, dtype=torch.float32).reshape(-1, 3)
        if background is None:
            levels = render_scene_grad(self.model, objects, rays, self.white_bkgd)
        else:
            levels = render_scene_background_grad(self.model, objects, rays, self.white_bkgd, background)
        loss = helper.train_loss([lvl[:3] for lvl in levels], target, (), 1e-4)[0]
        return loss if reg_codes is None else loss + fit.code_norm_penalty(reg_codes)

    def fit_scene_codes(self, batches, placements, steps: int, lr: float = 5.0e-3, fit_keys=("density", "color", "articulation"), seed: int = 0,
                        background=None):
        """Fit the codes of the K objects of ONE frame layout to observed frames with the network FROZEN: `steps` Adam
        steps against mse over the levels (helper.train_loss) + 1e-4 * sum over objects and codes of mean ||code||, batch `i % len(batches)`
        at step i.

        batches: dicts of WORLD rays ("rays_o", "rays_d", "viewdirs") plus "target".  placements: as render_scene takes them, at known poses;
        each object's codes start from the library rows (or the explicit articulation code) of its placement.  fit_keys: the codes that
        move; the others keep their starting values.  seed: accepted for symmetry with fit_latents; scenes sample without randomness.
        -> (list of K code dicts of (1, dim) tensors, per-step losses as one (steps,) device tensor); the only host synchronisation of a
        step is the read-back of the pair counts (ops.scene_pairs).

        The network's requires_grad flags are cleared for the duration and restored.  The codes of all K objects, their gradients and the
        Adam moments are one flat (4, 288 K) buffer stepped by ONE launch (aon_adam_step).  Every step pays the full weight-gradient stage
        (scene.render_scene_grad has no latent-only shortcut).

        background: None, or a scene.SceneBackground -- the observed frames show the objects in front of that
        backdrop, and the loss is rendered by scene.render_scene_background_grad with the backdrop network frozen for the duration too (it
        keeps no activation planes and launches no backward of its own).  None: the calls and the bits of a fit without one."""
        from ...scene import SceneObject

        bg_model = self._scene_fit_background("fit_scene_codes", background)
        batches, _ = self._fit_args("fit_scene_codes", steps, batches)
        if not (isinstance(lr, (int, float)) and lr > 0):
            raise ValueError(f"fit_scene_codes: lr must be positive, got {lr!r}")
        keys = [k for k, _ in ops._LATENT_KEYS]
        fit_keys = tuple(fit_keys)
        if not fit_keys or not set(fit_keys) <= set(keys):
            raise ValueError(f"fit_scene_codes: fit_keys must name some of {keys}, got {fit_keys!r}")
        placed = self._scene_fit_placed("fit_scene_codes", placements, batches)
        dev = next(self.model.parameters()).device
        codes = fit.CodeBuffer([latents for _, _, latents, _, _ in placed], dev, fit_keys)
        objects = [SceneObject(leaves, pose, box) for leaves, (_, _, _, pose, box) in zip(codes.leaves, placed)]

        def forward(i):
            return self._scene_fit_loss(objects, batches[i % len(batches)], dev, codes.leaves, background), codes.wrt

        def apply(i, grads):
            codes.take(grads)
            codes.step(lr, i + 1)

        with fit.frozen(self.model), (fit.frozen(bg_model) if bg_model is not None else contextlib.nullcontext()):
            losses = fit.run(steps, dev, forward, apply)
        return codes.clones(), losses

    def fit_scene_poses(self, batches, placements, steps: int, lr, fit_codes: bool = False, seed: int = 0, background=None):
        """Recover where the K objects of ONE frame layout ARE from observed frames with the network FROZEN, alone or
        together with their codes: `steps` Adam steps against mse over the levels (helper.train_loss), batch `i % len(batches)` at step i;
        with fit_codes the loss also carries fit_scene_codes' 1e-4 * sum over objects and codes of mean ||code||.

        batches, placements, seed: as fit_scene_codes; a placement's pose is the starting guess.  One 6-vector (omega, tau) is kept per
        object and applied as R = exp([omega]x) R0, c = c0 + tau (ops.apply_pose_correction); the poses are rebuilt from it every step.
        lr: one rate, or (pose rate, code rate).
        -> (list of K fitted (3, 4) poses, list of K code dicts of (1, dim) tensors, per-step losses as one (steps,) device tensor); the host
        synchronisations of a step are the read-backs of the poses (the pair kernel takes them from the host) and of the pair counts.

        The network's requires_grad flags are cleared for the duration and restored.  The 6-vectors, their gradients and the Adam moments
        are one flat (4, 6 K) buffer, the codes one flat (4, 288 K) buffer when fit_codes; each is stepped by ONE launch (aon_adam_step).
        With fit_codes off no code and no weight requires grad, and a step launches no weight-gradient kernel
        (autograd.RenderLevelScenePoses).  The pairs' existence, near / far and the sample positions are data: a pose moves only through the
        samples a ray already has inside the object's box, so start close enough for the boxes to overlap the object.

        background: as fit_scene_codes'  -- the objects stand in front of that frozen backdrop."""
        from ...scene import SceneObject

        bg_model = self._scene_fit_background("fit_scene_poses", background)
        batches, _ = self._fit_args("fit_scene_poses", steps, batches)
        lrs = fit.lr_pair("fit_scene_poses", lr)
        placed = self._scene_fit_placed("fit_scene_poses", placements, batches)
        dev = next(self.model.parameters()).device
        K = len(placed)
        codes = fit.CodeBuffer([latents for _, _, latents, _, _ in placed], dev, [k for k, _ in ops._LATENT_KEYS] if fit_codes else ())
        pose_buf = fit.AdamBuffer(6 * K, dev)
        corrections = pose_buf.leaf(0, 6 * K)
        poses0 = [ops.check_pose(pose).to(dev) for _, _, _, pose, _ in placed]

        def current_poses():
            return [ops.apply_pose_correction(poses0[j], corrections[6 * j: 6 * j + 6]) for j in range(K)]

        def forward(i):
            objects = [SceneObject(leaves, pose, p[4]) for leaves, pose, p in zip(codes.leaves, current_poses(), placed)]
            return self._scene_fit_loss(objects, batches[i % len(batches)], dev, codes.leaves if fit_codes else None, background), [corrections] + codes.wrt

        def apply(i, grads):
            pose_buf.take(grads[:1])
            pose_buf.step(lrs[0], i + 1)
            if fit_codes:
                codes.take(grads[1:])
                codes.step(lrs[1], i + 1)

        with fit.frozen(self.model), (fit.frozen(bg_model) if bg_model is not None else contextlib.nullcontext()):
            losses = fit.run(steps, dev, forward, apply)
        with torch.no_grad():
            fitted_poses = [p.clone() for p in current_poses()]
        return fitted_poses, codes.clones(), losses

    @torch.no_grad()
    def render_scene(self, batch, placements, occupancy=None, background=None):
        """Several instances of the library in ONE frame (scene.render_scene): ``placements`` is a list of up to 16
        ``(instance_id, articulation, pose, box)`` -- ``articulation`` a row index into get_interpolated_articulations (the 19 rows of the
        test epoch) or an explicit (32,) code, ``pose`` the (3, 4) rigid object-to-world matrix, ``box`` the object's box in its own
        frame -- and ``batch`` holds the WORLD rays ("rays_o", "rays_d", "viewdirs"; "target" / "instance_mask" are passed through when
        present).  -> {"rgb" (N, 3), "acc" (N,), "depth" (N,), "obj_acc" (N, K)} of the last level, rendered hparams.chunk rays at a time.
        ``occupancy``: None, or a dict of occupancy.build_occupancy's keyword arguments (``bounds``, ``resolution``,
        ``threshold``, ``dilate``, ``level``; the bounds must enclose every box): one grid is built per distinct (instance_id, articulation)
        among the placements and the objects' empty space is skipped.  In eval mode the grids are kept on the module, keyed by those and the
        arguments, until train() / eval() or load_state_dict() is called or a parameter of the network or the code library changes (their
        version counters are compared on every call; clear_scene_grids() drops them by hand): a stale grid is a wrong picture.  The dict gains "occupied", the
        (K,) samples of the last level that ran through the MLP.
        ``background``: None, or a scene.SceneBackground -- a vanilla NeRF standing behind the objects.  Then
        ``placements`` may be empty (at most 15), and "obj_acc" is (N, K + 1) with the backdrop's opacity last."""
        from ... import occupancy as _occupancy
        from ...scene import SceneObject, render_scene

        if occupancy is not None:
            if not isinstance(occupancy, dict) or not set(occupancy) <= set(self._OCC_KEYS):
                raise ValueError(f"render_scene: occupancy must be None or a dict with keys among {list(self._OCC_KEYS)}, got {occupancy!r}")
            occ_args = {"bounds": (-1.2, 1.2), **occupancy}
            occ_key = tuple(repr(occ_args.get(k)) for k in self._OCC_KEYS)

        objects = []
        for iid, art, latents, pose, box in self._placement_codes("render_scene", placements):
            grid = None
            if occupancy is not None:
                key = (iid, art if isinstance(art, int) else tuple(latents["articulation"].reshape(-1).tolist()), occ_key)
                grid = self._scene_grids.get(key)
                if grid is None:
                    grid = _occupancy.build_occupancy(self.model, latents=latents, **occ_args)
                    self._scene_grids[key] = grid
            objects.append(SceneObject(latents, pose, box, grid))
        rays = {k: batch[k].reshape(-1, 3) for k in ("rays_o", "rays_d", "viewdirs")}
        levels = render_scene(self.model, objects, rays, self.white_bkgd, chunk=self.hparams.chunk, want_occupied=occupancy is not None,
                              background=background)
        if occupancy is not None:
            levels, occupied = levels
        if self.training:      # the weights may move before the next frame
            self._scene_grids.clear()
        rgb, acc, depth, obj_acc = levels[-1]
        ret = {"rgb": rgb, "acc": acc, "depth": depth, "obj_acc": obj_acc}
        if occupancy is not None:
            ret["occupied"] = occupied[-1]
        ret.update({k: batch[k] for k in ("target", "instance_mask") if k in batch})
        return ret

    _OCC_KEYS = ("bounds", "resolution", "threshold", "dilate", "level")

    def train(self, mode: bool = True):
        if "model" in self._modules:      # (nn.Module.__init__ does not call this, but a subclass may before the network exists)
            self.clear_scene_grids()      # render_scene(occupancy=...)'s grids belong to the weights they were built from
        return super().train(mode)

    def load_state_dict(self, *args, **kwargs):
        self.clear_scene_grids()
        return super().load_state_dict(*args, **kwargs)

    def configure_optimizers(self):
        return build_adam([self.model, self.code_library], self.lr_init)   # (model_autodecoder.py:604-606; one arena, one launch: LitNeRF)

    @torch.no_grad()
    def build_occupancies(self, instance_id: int = 0, bounds=(-1.2, 1.2), resolution=128, threshold: float = 0.01, dilate: int = 1,
                          level: str = "fine") -> list:
        """One occupancy grid per articulation state of the test epoch (the rows of get_interpolated_articulations, as extract_meshes) with the
        shape / appearance codes of `instance_id`: the density depends on the latents (occupancy.build_occupancy for the arguments).  Grid a
        goes with latents {"density": shape, "color": app, "articulation": table[a: a + 1]}."""
        from ...occupancy import build_occupancy

        dev = next(self.model.parameters()).device
        iid = torch.tensor([int(instance_id)], dtype=torch.int64, device=dev)
        shape = self.code_library.embedding_instance_shape(iid)
        app = self.code_library.embedding_instance_appearance(iid)
        table = self.code_library.get_interpolated_articulations(max_interpolations=2, device=dev)
        return [build_occupancy(self.model, bounds, resolution, threshold, dilate, level=level,
                                latents={"density": shape, "color": app, "articulation": table[a: a + 1]}) for a in range(table.shape[0])]

    @torch.no_grad()
    def extract_meshes(self, instance_id: int = 0, resolution: int = 256, bounds=(-1.0, 1.0), threshold: float | None = None, level: str = "fine",
                       color: bool = False) -> list:
        """One mesh per articulation state of the test epoch: the 19 rows of get_interpolated_articulations (the 10 learned codes and the
        mid-points of neighbours) with the shape / appearance codes of `instance_id` (mesh.extract_mesh for the arguments)."""
        from ...mesh import extract_mesh

        dev = next(self.model.parameters()).device
        iid = torch.tensor([int(instance_id)], dtype=torch.int64, device=dev)
        shape = self.code_library.embedding_instance_shape(iid)
        app = self.code_library.embedding_instance_appearance(iid)
        table = self.code_library.get_interpolated_articulations(max_interpolations=2, device=dev)
        return [extract_mesh(self.model, bounds, resolution, threshold=threshold, level=level, color=color,
                             latents={"density": shape, "color": app, "articulation": table[a: a + 1]}) for a in range(table.shape[0])]
