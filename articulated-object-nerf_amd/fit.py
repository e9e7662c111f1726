"""Fitting a few values -- latent codes, 6-vector pose corrections -- on a FROZEN network: what fit_latents, the two fit_pose, fit_scene_codes
and fit_scene_poses share.  `frozen` clears the network's requires_grad flags for the duration; an `AdamBuffer`
holds the fitted values, their gradients and the Adam moments as one flat (4, N) tensor stepped by aon_adam_step, a `CodeBuffer` lays the
codes of K objects out on one; `run` is the loop.  An entry point checks its arguments, builds its buffers and hands `run` two closures."""
from __future__ import annotations

import contextlib

import torch

from . import ops

CODE_WIDTH = sum(d for _, d in ops._LATENT_KEYS)   # 288 floats an object


@contextlib.contextmanager
def frozen(module, freeze: bool = True):
    """Clear the requires_grad flag of every parameter of `module`; each flag is put back on the way out, after an exception too.
    freeze=False: the flags stay as they are."""
    params = list(module.parameters())
    flags = [p.requires_grad for p in params]
    try:
        if freeze:
            for p in params:
                p.requires_grad_(False)
        yield
    finally:
        for p, f in zip(params, flags):
            p.requires_grad_(f)


def lr_pair(who: str, lr):
    """One rate, or a (pose rate, code rate) pair -> the pair.  A bool is not a rate."""
    lrs = tuple(lr) if isinstance(lr, (tuple, list)) else (lr, lr)
    if len(lrs) != 2 or not all(isinstance(x, (int, float)) and not isinstance(x, bool) and x > 0 for x in lrs):
        raise ValueError(f"{who}: lr must be positive (one rate, or a pair for poses and codes), got {lr!r}")
    return lrs


class AdamBuffer:
    """`n` fitted floats as one flat (4, n) fp32 tensor -- rows: values, gradients, exp_avg, exp_avg_sq -- starting at zero.
    wrt: the leaves handed out that require grad, in the order they were asked for."""

    def __init__(self, n: int, dev):
        self.rows = torch.zeros((4, n), dtype=torch.float32, device=dev)
        self.wrt, self._slots = [], []

    def leaf(self, begin: int, count: int, shape=None, requires_grad: bool = True):
        """A leaf tensor of `shape` (flat by default) on the storage of values [begin, begin + count): a step of the buffer moves it."""
        shape = (count,) if shape is None else shape
        leaf = self.rows[0, begin: begin + count].view(shape).detach().requires_grad_(bool(requires_grad))
        if requires_grad:
            self.wrt.append(leaf)
            self._slots.append(self.rows[1, begin: begin + count].view(shape))
        return leaf

    def take(self, grads, first: int = 0) -> None:
        """The gradients of wrt[first], wrt[first + 1], ... each into its leaf's slot of the gradient row, in one launch; the slots of
        values that are not fitted stay zero."""
        torch._foreach_copy_(self._slots[first: first + len(grads)], list(grads))

    def step(self, lr, step: int, begin: int = 0, count: int | None = None) -> None:
        """One Adam step (betas 0.9 / 0.999, eps 1e-8) of values [begin, begin + count) -- the whole buffer by default -- as their step
        number `step` (1 for the first).  A value whose gradient and moments are zero stays exactly as it is."""
        count = self.rows.shape[1] - begin if count is None else count
        ops.adam_step(self.rows[0], self.rows[1], self.rows[2], self.rows[3], begin, count, float(lr), 0.9, 0.999, 1e-8, step)


class CodeBuffer(AdamBuffer):
    """The codes of K objects, 288 floats an object in ops._LATENT_KEYS order.  codes: K dicts of tensors with dim values each (copied in);
    fit_keys: the keys whose leaves require grad.  leaves: K dicts of (1, dim) leaves on the value row; wrt runs objects outer, keys inner."""

    def __init__(self, codes, dev, fit_keys=()):
        super().__init__(CODE_WIDTH * len(codes), dev)
        self.leaves, off = [], 0
        for given in codes:
            mine = {}
            for k, d in ops._LATENT_KEYS:
                self.rows[0, off: off + d].view(1, d).copy_(given[k].detach().reshape(1, d))
                mine[k] = self.leaf(off, d, (1, d), k in fit_keys)
                off += d
            self.leaves.append(mine)

    def clones(self):
        """-> K dicts of (1, dim) copies of the current values."""
        return [{k: v.detach().clone() for k, v in mine.items()} for mine in self.leaves]


def code_norm_penalty(leaves):
    """The reference's latent regulariser over K objects: 1e-4 * sum over objects, then codes, of mean ||code||."""
    return 1e-4 * sum(torch.mean(torch.norm(codes[k], dim=0)) for codes in leaves for k, _ in ops._LATENT_KEYS)


def run(steps: int, dev, forward, apply):
    """`steps` rounds of `forward(i)` -> (loss, leaves to differentiate by) and `apply(i, grads)`, which writes the gradients into their
    buffers and steps them -> the per-step losses as one (steps,) tensor on `dev`.  Nothing here reads the device back."""
    losses = torch.zeros(steps, dtype=torch.float32, device=dev)
    with torch.enable_grad():
        for i in range(steps):
            loss, wrt = forward(i)
            grads = torch.autograd.grad(loss, wrt)
            losses[i] = loss.detach()
            apply(i, grads)
    return losses
