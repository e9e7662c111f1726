"""Guard bands for the memory contract of include/aon_hip.h: inputs are never written, outputs are written inside their stated extents, and
a workspace of exactly the library's byte count is enough.  Value tests cannot see a breach: torch's caching allocator rounds every block up
and packs blocks side by side, so a store past an end lands in slack, and `torch.empty` hands back the block the previous call of the same
shape just freed, correct result included.

`GuardedAlloc` gives every buffer a band of 0xFF bytes on either side that starts at the exact byte where the payload ends; `TorchProxy`
stands in for the `torch` name of the modules that allocate what the library writes, so their `torch.empty` / `zeros` / ... go through it;
`LibRecorder` notes which `aon_*` functions a run fetched.  Nothing here imports the package at module level: tests/test_guard_cpu.py drives
the same proxy with a fake binding on the CPU."""
import contextlib
import importlib
import os
import traceback

import torch as _torch

BAND = 4096        # bytes on either side of a payload
ALIGN = 256        # the payload start keeps this alignment: the strictest include/aon_hip.h asks of any pointer
FILL = 0xFF        # NaN as fp32 / fp64, -1 as int32 / int64: a stray float read poisons the result, a stray index points next to its base

# every module of the package that allocates buffers whose pointers reach the library (found by searching for `data_ptr` / `_ptr(` and for
# what is handed on to ops.py), relative to the package
PACKAGE = "aon_amd"
ALLOCATING_MODULES = ("ops", "autograd", "arena", "occupancy", "mesh", "models.vanilla_nerf.model", "models.vanilla_nerf.model_autodecoder",
                      "models.vanilla_nerf.helper", "models.code_library")

_HERE = os.path.abspath(__file__)


def _caller() -> str:
    """file:line of the nearest frame outside this module: the line that asked for the buffer."""
    for fr in reversed(traceback.extract_stack()):
        if os.path.abspath(fr.filename) != _HERE:
            return f"{os.path.relpath(fr.filename)}:{fr.lineno}"
    return "?"


class GuardError(AssertionError):
    pass


class _Rec:
    __slots__ = ("backing", "start", "nbytes", "shape", "dtype", "where", "kind")

    def describe(self) -> str:
        return f"{self.kind} {tuple(self.shape)} {self.dtype} ({self.nbytes} B) allocated at {self.where}"


class GuardedAlloc:
    """Allocations with a 0xFF band on either side.  `prefill`: what a request that came from `empty` / `empty_like` holds, "nan" (0xFF
    bytes) or "zero"; `zeros` / `ones` / `full` get the value they asked for.  Every backing tensor is kept until reset(), so no guarded
    block is recycled inside a case."""

    def __init__(self, prefill: str = "nan", device_types=("cuda",)):
        if prefill not in ("nan", "zero"):
            raise ValueError(f"prefill must be 'nan' or 'zero', got {prefill!r}")
        self.prefill, self.device_types = prefill, tuple(device_types)
        self.records: list = []

    def guards(self, device) -> bool:
        return _torch.device(device).type in self.device_types

    def alloc(self, shape, dtype, device, value=None, kind="buffer"):
        """`value` None: an `empty` request (prefilled by mode); else the fill value.  -> tensor of `shape` / `dtype` on `device`."""
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        itemsize = _torch.empty((), dtype=dtype).element_size()
        nbytes = numel * itemsize
        backing = _torch.empty(BAND + nbytes + BAND + ALIGN, dtype=_torch.uint8, device=device)
        backing.fill_(FILL)
        start = BAND + (-(backing.data_ptr() + BAND)) % ALIGN
        payload = backing[start:start + nbytes]
        assert payload.data_ptr() % ALIGN == 0 or nbytes == 0
        t = payload.view(dtype).view(shape) if nbytes else _torch.empty(shape, dtype=dtype, device=device)
        if nbytes:
            if value is None:
                if self.prefill == "zero":
                    payload.zero_()
            else:
                t.fill_(value)
        rec = _Rec()
        rec.backing, rec.start, rec.nbytes, rec.shape, rec.dtype, rec.where, rec.kind = backing, start, nbytes, shape, dtype, _caller(), kind
        self.records.append(rec)
        return t

    def check(self) -> None:
        """Synchronise, then every band byte must still be 0xFF."""
        if any(r.backing.is_cuda for r in self.records):
            _torch.cuda.synchronize()
        for r in self.records:
            head, tail = r.backing[:r.start], r.backing[r.start + r.nbytes:]
            for name, band in (("tail", tail), ("head", head)):
                bad = band != FILL
                if bool(bad.any()):
                    idx = bad.nonzero().reshape(-1)
                    if name == "tail":
                        first = int(idx[0])
                        where = f"first damaged byte {first} B past the payload's end"
                    else:
                        first = r.start - int(idx[-1])
                        where = f"nearest damaged byte {first} B before the payload's start (the first one {r.start - int(idx[0])} B before it)"
                    raise GuardError(f"{name} band damaged ({int(bad.sum())} bytes): {where}; {r.describe()}")

    def reset(self) -> None:
        self.records.clear()

    def __len__(self) -> int:
        return len(self.records)


def _size_args(args):
    """sizes given as one tuple / list / torch.Size or as varargs -> tuple"""
    if len(args) == 1 and isinstance(args[0], (tuple, list, _torch.Size)):
        return tuple(args[0])
    return tuple(args)


class TorchProxy:
    """`torch` with the allocating functions routed through a GuardedAlloc when the target device is of a guarded type."""

    def __init__(self, real_torch, alloc: GuardedAlloc):
        object.__setattr__(self, "_real", real_torch)
        object.__setattr__(self, "_alloc", alloc)

    def __getattr__(self, name):
        return getattr(self._real, name)

    def __setattr__(self, name, value):
        setattr(self._real, name, value)

    # ---- helpers
    def _device(self, device):
        if device is None:
            get = getattr(self._real, "get_default_device", None)
            return get() if get is not None else self._real.device("cpu")
        return self._real.device(device)

    def _new(self, name, shape, value, args, kw, like=None):
        opts = dict(kw)
        dtype, device = opts.pop("dtype", None), opts.pop("device", None)
        requires_grad = opts.pop("requires_grad", False)
        if like is not None:
            dtype = like.dtype if dtype is None else dtype
            device = like.device if device is None else device
        device = self._device(device)
        # anything beyond the plain contiguous strided request goes to torch as it came
        plain = set(opts) <= {"layout", "pin_memory", "memory_format"} and all(
            v in (None, False, self._real.strided, self._real.contiguous_format, self._real.preserve_format) for v in opts.values())
        if not plain or not self._alloc.guards(device) or (like is not None and not like.is_contiguous()):
            return getattr(self._real, name)(*args, **kw)
        if dtype is None:
            if name == "full" and isinstance(value, bool):
                dtype = self._real.bool
            elif name == "full" and isinstance(value, int):
                dtype = self._real.int64
            else:
                dtype = self._real.get_default_dtype()
        t = self._alloc.alloc(shape, dtype, device, value, kind=name)
        if requires_grad:
            t.requires_grad_(True)
        return t

    # ---- the overridden functions
    def empty(self, *size, **kw):
        return self._new("empty", _size_args(size), None, size, kw)

    def zeros(self, *size, **kw):
        return self._new("zeros", _size_args(size), 0, size, kw)

    def ones(self, *size, **kw):
        return self._new("ones", _size_args(size), 1, size, kw)

    def full(self, size, fill_value, **kw):
        return self._new("full", tuple(size), fill_value, (size, fill_value), kw)

    def empty_like(self, t, **kw):
        return self._new("empty_like", tuple(t.shape), None, (t,), kw, like=t)

    def zeros_like(self, t, **kw):
        return self._new("zeros_like", tuple(t.shape), 0, (t,), kw, like=t)

    def ones_like(self, t, **kw):
        return self._new("ones_like", tuple(t.shape), 1, (t,), kw, like=t)

    def full_like(self, t, fill_value, **kw):
        return self._new("full_like", tuple(t.shape), fill_value, (t, fill_value), kw, like=t)


class LibRecorder:
    """The ctypes library, with the name of every `aon_*` function that is fetched noted in `.names`."""

    def __init__(self, lib):
        object.__setattr__(self, "_lib", lib)
        object.__setattr__(self, "names", set())

    def __getattr__(self, name):
        if name.startswith("aon_"):
            self.names.add(name)
        return getattr(self._lib, name)


@contextlib.contextmanager
def guarded(monkeypatch, prefill, modules=None, device_types=("cuda",)):
    """`with guarded(monkeypatch, "nan") as (alloc, recorder):` -- inside, the name `torch` of every allocating module is a TorchProxy over
    a fresh GuardedAlloc and their `lib` a LibRecorder.  `modules` None: the package's ALLOCATING_MODULES, and ops.release_workspaces() runs
    on entry and on exit, so every workspace of the run is allocated fresh at exactly the requested size through the proxy and nothing
    guarded outlives the block in a cache or pool.  Otherwise `modules` is a list of module objects (the CPU self-test's fake binding)."""
    release = None
    if modules is None:
        modules = [importlib.import_module(f"{PACKAGE}.{m}") for m in ALLOCATING_MODULES]
        release = importlib.import_module(f"{PACKAGE}.ops").release_workspaces
    alloc = GuardedAlloc(prefill, device_types)
    proxy = TorchProxy(_torch, alloc)
    recorder = None
    with monkeypatch.context() as m:
        for mod in modules:
            if hasattr(mod, "lib"):
                if recorder is None:
                    recorder = LibRecorder(mod.lib)
                m.setattr(mod, "lib", recorder)
            m.setattr(mod, "torch", proxy)
        if release is not None:
            release()
        try:
            yield alloc, recorder
        finally:
            if release is not None:
                release()
            alloc.reset()


def place(alloc: GuardedAlloc, tensor):
    """A copy of a test input in a guarded slot: a read past its end meets NaN, not a neighbour.  Tensors on unguarded devices, and
    anything that is not a tensor, are returned as they are.  A packed stream keeps the form it was packed in (`_aon_form`, which the
    binding re-declares for the new address on every call)."""
    if not isinstance(tensor, _torch.Tensor) or not alloc.guards(tensor.device):
        return tensor
    src = tensor.detach().contiguous()
    out = alloc.alloc(src.shape, src.dtype, src.device, None, kind="input")
    out.copy_(src)
    if hasattr(tensor, "_aon_form"):
        out._aon_form = tensor._aon_form
    if tensor.requires_grad:
        out.requires_grad_(True)
    return out


def bits(t):
    """An integer view of `t` for bitwise comparison (NaN equals NaN); a copy on the CPU, so it also serves as a before-image."""
    t = t.detach().contiguous().cpu()
    if t.dtype in (_torch.float32,):
        return t.view(_torch.int32).clone()
    if t.dtype in (_torch.float64,):
        return t.view(_torch.int64).clone()
    if t.dtype in (_torch.float16, _torch.bfloat16):
        return t.view(_torch.int16).clone()
    if t.dtype == _torch.bool:
        return t.to(_torch.uint8)
    return t.clone()


def has_unwritten_word(t) -> bool:
    """True when `t` (an output of a "nan"-prefilled run) still holds a whole aligned 32-bit word of 0xFF bytes: an element nobody wrote.
    Buffers whose size is no multiple of four bytes are checked word-wise over their whole words, and their last bytes as a group."""
    raw = t.detach().contiguous().cpu().reshape(-1).view(_torch.uint8)
    n = raw.numel()
    if n == 0:
        return False
    words = raw[:n - n % 4].reshape(-1, 4)
    if bool((words == FILL).all(dim=1).any()):
        return True
    return n % 4 != 0 and bool((raw[n - n % 4:] == FILL).all())
