"""Mirror of ``models/interface.py:LitModel``'s metric / gather helpers (interface.py:31-74) without the
pytorch-lightning base class (Lightning is the reference's harness, not part of the rendered path)."""
from __future__ import annotations

import math
import os

import torch
import torch.distributed as dist

from .. import fit, ops


class LitModel(torch.nn.Module):
    def mse(self, image_pred, image_gt, valid_mask=None, reduction="mean"):
        """interface.py:64-70"""
        value = (image_pred - image_gt) ** 2
        if valid_mask is not None:
            value = value[valid_mask]
        return torch.mean(value) if reduction == "mean" else value

    @torch.no_grad()
    def psnr_legacy(self, image_pred, image_gt, valid_mask=None, reduction="mean"):
        """interface.py:72-74"""
        return -10 * torch.log10(self.mse(image_pred, image_gt, valid_mask, reduction))

    @torch.no_grad()
    def psnr_each(self, preds, gts):
        """interface.py:54-62"""
        out = []
        for pred, gt in zip(preds, gts):
            mse = torch.mean((torch.clip(pred, 0, 1) - torch.clip(gt, 0, 1)) ** 2)
            out.append(-10.0 * torch.log(mse) / math.log(10.0))
        return torch.stack(out)

    def all_gather(self, t: torch.Tensor) -> torch.Tensor:
        """(world, *t.shape) like LightningModule.all_gather; identity without a process group."""
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return t
        out = [torch.empty_like(t) for _ in range(dist.get_world_size())]
        dist.all_gather(out, t.contiguous())
        return torch.stack(out)

    def alter_gather_cat(self, outputs, key, image_sizes):
        """interface.py:31-51 with the world>1 layout fixed: ranks are concatenated rank-major (each rank's
        images stay contiguous) instead of the reference's per-pixel interleave."""
        each = torch.cat([output[key] for output in outputs])
        allv = self.all_gather(each).detach()
        if allv.dim() == each.dim() + 1:
            allv = allv.flatten(0, 1)
        if allv.shape[-1] == 1:
            allv = allv.squeeze(-1)
        ret, curr = [], 0
        for (h, w) in image_sizes:
            chunk = allv[curr: curr + h * w]
            if chunk.shape[0] == 0:
                continue
            ret.append(chunk.reshape(h, w, 3) if allv.dim() == 2 and allv.shape[-1] == 3 else chunk.reshape(h, w))
            curr += h * w
        return ret

    @torch.no_grad()
    def psnr(self, preds, gts, i_train=None, i_val=None, i_test=None):
        """interface.py:127-140: {"name": "PSNR", "mean": m, "test": m} over per-image PSNRs."""
        m = self.psnr_each(preds, gts).mean().item()
        return {"name": "PSNR", "mean": m, "test": m}

    @torch.no_grad()
    def ssim_each(self, preds, gts):
        """interface.py:102-111: piqa's SSIM() of each (h, w, 3) pair clipped to [0,1], as one HIP call over the whole list -> (n,)."""
        from ..ops import ssim

        return ssim(preds, gts)

    @torch.no_grad()
    def ssim(self, preds, gts, i_train=None, i_val=None, i_test=None):
        """interface.py:142-157: {"name": "SSIM", "mean": m, "test": m} over per-image SSIMs."""
        m = self.ssim_each(preds, gts).mean().item()
        return {"name": "SSIM", "mean": m, "test": m}


def get_obj_rgbs_from_segmap(all_segmap, all_pred_img, all_pred_target):
    """models/utils.py:102-109: per image, the predicted / target colours of the pixels inside the instance mask."""
    objs, tgts = [], []
    for seg, pred, target in zip(all_segmap, all_pred_img, all_pred_target):
        mask = seg.bool().unsqueeze(-1).expand(-1, -1, 3)
        objs.append(pred[mask])
        tgts.append(target[mask])
    return objs, tgts


class _LogSeries(list):
    """The values one name was logged with, as floats.  ``float(tensor)`` at log time is a host synchronisation, four per training step
    (the host then enqueues the backward only after the forward has finished), so device scalars wait in a SIDE buffer and are turned into
    floats when anybody looks at the list -- any read entry point, pickling and copying included (round 5 kept the pending
    tensors inside the list itself, and ``copy()``, ``+``, ``==``, ``repr``, ``np.asarray`` handed raw device tensors out) -- or 512 at a
    time with ONE device read.  The list proper only ever holds floats."""

    def __init__(self, *a):
        super().__init__(*a)
        self._wait = []          # device scalars logged since the last read, in order (they follow everything already in the list)

    def append(self, value):
        if isinstance(value, torch.Tensor):
            self._wait.append(value.detach())
            if len(self._wait) >= 512:
                self._settle()
        else:
            self._settle()
            list.append(self, float(value))

    def _settle(self):
        wait, self._wait = getattr(self, "_wait", []), []
        if wait:
            ts = [t.reshape(()).float() for t in wait]
            vals = torch.stack(ts).tolist() if len({t.device for t in ts}) == 1 else [float(t) for t in ts]
            list.extend(self, vals)

    def __reduce_ex__(self, protocol):          # pickle / copy.copy / copy.deepcopy: a plain list of floats
        self._settle()
        return (list, (list(self),))


def _settled(name):
    base = getattr(list, name)

    def method(self, *a, **k):
        self._settle()
        return base(self, *a, **k)

    method.__name__ = name
    return method


for _name in ("__getitem__", "__iter__", "__len__", "__repr__", "__eq__", "__ne__", "__lt__", "__le__", "__gt__", "__ge__", "__contains__", "__add__", "__mul__",
              "__rmul__", "__reversed__", "__setitem__", "__delitem__", "__iadd__", "__imul__", "copy", "count", "index", "extend", "insert", "pop", "remove",
              "reverse", "sort", "clear"):
    setattr(_LogSeries, _name, _settled(_name))


class Harness(LitModel):
    """What the two LightningModules of the reference share once Lightning is removed: the ``self.log`` sink, the
    learning-rate rule of ``optimizer_step`` (model.py:391-419 == model_autodecoder.py:607-636) and the PSNR / SSIM part
    of ``test_epoch_end`` (model.py:450-485, model_autodecoder.py:665-701; LPIPS needs pretrained VGG weights and is out of
    scope)."""

    lr_init, lr_final, lr_delay_steps, lr_delay_mult = 5.0e-4, 5.0e-6, 2500, 0.01

    def _init_harness(self, hparams, defaults, lr_init, lr_final, lr_delay_steps, lr_delay_mult, randomized, near, far, white_bkgd, ray_box):
        from collections import defaultdict
        from types import SimpleNamespace

        hp = dict(defaults)
        hp.update(vars(hparams) if hparams is not None and not isinstance(hparams, dict) else (hparams or {}))
        self.hparams = SimpleNamespace(**hp)
        self.logged = defaultdict(_LogSeries)
        self.global_step = 0
        self.lr_init, self.lr_final, self.lr_delay_steps, self.lr_delay_mult = lr_init, lr_final, lr_delay_steps, lr_delay_mult
        self.randomized, self.near, self.far, self.white_bkgd = randomized, near, far, white_bkgd
        # ray_box (a side length, or (lo, hi)): per-ray near / far from the rays' intersection with that box (helper.get_ray_limits, the
        # reference's near_obj / far_obj) instead of the scalars; None: the scalars, as before
        self.ray_box = ray_box

    def log(self, name, value, **_):
        self.logged[name].append(value)

    def lr_at_step(self, step: int) -> float:
        """log-linear decay lr_init -> lr_final over run_max_steps, times a sine warm-up over lr_delay_steps."""
        if self.lr_delay_steps > 0:
            delay = self.lr_delay_mult + (1 - self.lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / self.lr_delay_steps, 0), 1))
        else:
            delay = 1.0
        t = min(max(step / self.hparams.run_max_steps, 0), 1)
        return delay * math.exp(math.log(self.lr_init) * (1 - t) + math.log(self.lr_final) * t)

    def optimizer_step(self, optimizer, closure=None):
        for pg in optimizer.param_groups:
            pg["lr"] = self.lr_at_step(self.global_step)
        optimizer.step(closure=closure)
        self.global_step += 1

    def fit_step(self, batch, batch_idx, optimizer, find_unused_parameters: bool = False):
        """One batch of Lightning's automatic optimisation under its DDP plugin (run.py:144-153): zero_grad, training_step,
        backward, the data-parallel gradient mean (ONE flat RCCL bucket, `parallel.allreduce_gradients`; a no-op without a process
        group or at world size 1), then the LR rule + optimizer step.  `find_unused_parameters` is DDPPlugin's argument (run.py:109,
        :129, :151): False -- the reference's value -- is DDP's strict contract (every rank produces gradients for the same parameters;
        a violation raises UnevenGradientsError on EVERY rank at the next exchange, or at `finish_fit()` / a checkpoint / test_epoch_end
        when there is no next one); True lets a rank whose batch did not touch a parameter adopt the others' mean."""
        from ..parallel import allreduce_gradients

        optimizer.zero_grad(set_to_none=True)
        loss = self.training_step(batch, batch_idx)
        loss.backward()
        allreduce_gradients(self, find_unused_parameters=find_unused_parameters)
        self.optimizer_step(optimizer)
        return loss.detach()

    _CHUNK_SKIP = ()   # batch keys that are never rays (a harness's scalar keys)

    def _render_chunks(self, batch, *model_args, skip=(), whole=()):
        """The model on `batch`, hparams.chunk rays at a time, without randomness -> the fine level's comp_rgb, acc, depth over all rays.
        model_args: behind near / far (the latents); skip: batch keys left out; whole: keys handed to every chunk unsliced.  A ray box's
        limits are those of the whole image -- the fallback for rays that miss the box is a property of the ray set -- sliced per chunk."""
        step = self.hparams.chunk
        limits = ops.ray_limits(batch["rays_o"], batch["rays_d"], self.ray_box) if self.ray_box is not None else None
        outs = []
        for i in range(0, batch["rays_o"].shape[0], step):
            chunk = {k: (v if k in whole else v[i: i + step]) for k, v in batch.items() if k not in skip and k not in self._CHUNK_SKIP}
            if limits is not None:
                near, far, live = (x[i: i + step] for x in limits)
                outs.append(self.model(chunk, False, self.white_bkgd, near, far, *model_args, ray_live=live)[1])
            else:
                outs.append(self.model(chunk, False, self.white_bkgd, self.near, self.far, *model_args)[1])
        return {k: torch.cat([o[j] for o in outs], 0) for j, k in enumerate(("comp_rgb", "acc", "depth"))}

    # ---- fitting poses and codes on the FROZEN network: what fit_latents and the two fit_pose hand fit.py's loop (DESIGN.md sections 4.13 - 4.15) ----
    def _fit_args(self, name, steps, batches, poses=False):
        """The checks of `steps` and `batches` and, for poses other than False (fit_pose), of one pose per view -> (batches, poses) as lists."""
        if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
            raise ValueError(f"{name}: steps must be a positive int, got {steps!r}")
        batches = list(batches)
        if not batches:
            raise ValueError(f"{name}: no batches")
        if poses is not False:
            poses = [] if poses is None else list(poses)
            if len(poses) != len(batches):
                raise ValueError(f"{name}: one (3, 4) pose per view: {len(batches)} views, {len(poses)} poses")
        return batches, poses

    def _fit_pose_batches(self, batches):
        if self.ray_box is not None:
            raise NotImplementedError("fit_pose: per-ray near / far from a ray box are not differentiated; use the scalar near / far")
        for b in batches:
            if "directions" not in b or "target" not in b:
                raise ValueError("fit_pose: every batch needs 'directions' (camera-space) and 'target'")

    def _fit_frozen(self, batches, steps, seed, poses=None, lr_pose=None, codes=None, lr_codes=None, fit_codes=False, freeze=True):
        """`steps` Adam steps on the frozen network, batch `i % len(batches)` at step i -> (corrected poses or None, codes or None, losses).
        poses: the views' initial (3, 4) matrices -- every batch is then a view ("directions", "target") whose 6-vector is fitted at rate
        lr_pose -- or None: the batches are un-batched training batches, the ray box applies.  codes: the initial codes of an articulated
        network (handed to self._frozen_loss; stepped at rate lr_codes when fit_codes) or None.  freeze=False: the network keeps its flags."""
        dev = next(self.model.parameters()).device
        views = len(batches)
        if poses is not None:
            pose0 = []
            for c2w in poses:
                c = torch.as_tensor(c2w, dtype=torch.float32).detach().to(dev)
                if c.dim() != 2 or c.shape[0] < 3 or c.shape[1] != 4:
                    raise ValueError(f"fit_pose: a pose must be a (3, 4) matrix, got {tuple(c.shape)}")
                pose0.append(c[:3].contiguous())
            pose_buf = fit.AdamBuffer(6 * views, dev)
            corr = [pose_buf.leaf(6 * v, 6) for v in range(views)]
        code_buf = leaves = None
        if codes is not None:
            code_buf = fit.CodeBuffer([codes], dev, [k for k, _ in ops._LATENT_KEYS] if fit_codes else ())
            leaves = code_buf.leaves[0]
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))

        def forward(i):
            v = i % views
            near, far = self.near, self.far
            if poses is not None:
                directions = batches[v]["directions"].to(device=dev, dtype=torch.float32)
                target = batches[v]["target"].to(device=dev, dtype=torch.float32).reshape(-1, 3)
                rays_o, rays_d = ops.rays_from_pose(directions, pose0[v], corr[v])
                rays = {"rays_o": rays_o, "rays_d": rays_d, "viewdirs": rays_d}
            else:
                rays, target = batches[v], batches[v]["target"]
                if self.ray_box is not None:
                    near, far, _ = ops.ray_limits(rays["rays_o"], rays["rays_d"], self.ray_box)
            t_rand = u = None
            if self.randomized:
                n = rays["rays_d"].shape[0]
                t_rand = torch.rand((n, self.model.num_coarse_samples + 1), device=dev, generator=gen)
                u = torch.rand((n, self.model.num_fine_samples), device=dev, generator=gen) if self.model.num_levels == 2 else None
            loss = self._frozen_loss(rays, target, near, far, leaves, t_rand, u)
            return loss, ([corr[v]] if poses is not None else []) + (code_buf.wrt if fit_codes else [])

        def apply(i, grads):
            if poses is not None:   # a view's 6-vector keeps its own step count
                v = i % views
                pose_buf.take(grads[:1], v)
                pose_buf.step(lr_pose, i // views + 1, 6 * v, 6)
                grads = grads[1:]
            if fit_codes:
                code_buf.take(grads)
                code_buf.step(lr_codes, i + 1)

        with fit.frozen(self.model, freeze):
            losses = fit.run(steps, dev, forward, apply)
        fitted = None
        if poses is not None:
            with torch.no_grad():
                fitted = [ops.apply_pose_correction(pose0[v], pose_buf.rows[0, 6 * v: 6 * v + 6]) for v in range(views)]
        return fitted, (code_buf.clones()[0] if codes is not None else None), losses

    def finish_fit(self) -> None:
        """End of a training loop (Lightning's on_train_end): the deferred check of the LAST gradient exchange, which no later
        fit_step will look at.  Also run by utils.save_checkpoint and test_epoch_end."""
        from ..parallel import check_gradient_exchange

        check_gradient_exchange()

    @torch.no_grad()
    def test_epoch_end(self, outputs, image_sizes, out_dir=None, name="image"):
        """Gather the per-image test outputs over ranks, PSNR and SSIM over whole images, PSNR over object pixels, and
        (rank 0, when ``out_dir`` is given) the JPEG dump + results.json of the reference.  Returns (psnr, psnr_obj); the
        SSIM dict is logged as ``test/ssim`` and written to results.json."""
        from ..utils import store_image, write_stats

        self.finish_fit()
        rgbs = self.alter_gather_cat(outputs, "rgb", image_sizes)
        masks = self.alter_gather_cat(outputs, "instance_mask", image_sizes)
        targets = self.alter_gather_cat(outputs, "target", image_sizes)
        psnr = self.psnr(rgbs, targets)
        ssim = self.ssim(rgbs, targets)
        objs, obj_targets = get_obj_rgbs_from_segmap(masks, rgbs, targets)
        psnr_obj = self.psnr(objs, obj_targets)
        psnr_obj["name"] = "PSNR_obj"
        self.log("test/psnr", psnr["test"])
        self.log("test/ssim", ssim["test"])
        self.log("test/psnr_obj", psnr_obj["test"])
        if out_dir is not None and (not dist.is_initialized() or dist.get_rank() == 0):
            store_image(out_dir, rgbs, name)
            write_stats(os.path.join(out_dir, "results.json"), psnr, ssim, psnr_obj)
        return psnr, psnr_obj
