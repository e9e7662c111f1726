"""CPU: the guard-band harness of tests/_guard.py discriminates.  A fake "binding" module -- plain torch on the CPU, run through the same
proxy with `cpu` guarded -- plants each of the six defects the harness exists for; each must be reported by the check meant for it, and
the correct function must pass them all.  Then: alignment and edge requests, and the completeness of tests/test_hip_extents.py's case
table against include/aon_hip.h (the half that needs no GPU)."""
import os
import re
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _guard  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------ the fake binding: out = 2 * x + sum(scratch), scratch = x[:2] squared
_FAKE = '''
import torch
def run(x, defect=None):
    n = x.numel()
    out, scratch = torch.empty(n, dtype=torch.float32, device=x.device), torch.empty(2, dtype=torch.float32, device=x.device)
    span = lambda t, lo, hi: t.as_strided((hi - lo,), (1,), t.storage_offset() + lo)   # elements [lo, hi) relative to t[0]
    scratch[: 1 if defect == "f" else 2] = x[: 1 if defect == "f" else 2] ** 2          # (f) scratch[1] is never written ...
    lo, hi = (-1 if defect == "b" else 0), (n + 1 if defect == "a" else n - 1 if defect == "c" else n)
    span(out, lo, hi).copy_(2 * span(x, lo, hi).nan_to_num(0.0) + scratch.sum())         # ... and read here
    if defect == "d": x[0] = 7.0
    if defect == "e": out[0] += span(x, n, n + 1)[0]
    return out
'''


@pytest.fixture()
def fake():
    mod = types.ModuleType("fake_binding")
    exec(_FAKE, mod.__dict__)
    return mod


def _x():
    return torch.arange(1.0, 6.0)      # 5 elements: 20 bytes, so the tail band begins inside a 16-byte vector


def _three_runs(fake, monkeypatch, defect):
    """The protocol of tests/test_hip_extents.py on the fake binding -> dict of what each check saw."""
    seen = {"band": None, "input": False, "differ": False, "unwritten": False}
    x0 = _x()
    outs = [_guard.bits(fake.run(x0.clone(), defect if defect in ("c", "d", "f") else None))]     # plain run: nothing to overrun into
    for prefill in ("nan", "zero"):
        with _guard.guarded(monkeypatch, prefill, modules=[fake], device_types=("cpu",)) as (alloc, _):
            x = _guard.place(alloc, x0)
            before = _guard.bits(x)
            out = fake.run(x, defect)
            try:
                alloc.check()
            except _guard.GuardError as e:
                seen["band"] = str(e)
            seen["input"] |= not torch.equal(_guard.bits(x), before)
            if prefill == "nan":
                seen["unwritten"] |= _guard.has_unwritten_word(out)
            outs.append(_guard.bits(out))
    seen["differ"] = not (torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2]))
    return seen


def test_correct_function_passes_every_check(fake, monkeypatch):
    seen = _three_runs(fake, monkeypatch, None)
    assert seen == {"band": None, "input": False, "differ": False, "unwritten": False}


def test_a_write_past_an_output_names_allocation_and_offset(fake, monkeypatch):
    msg = _three_runs(fake, monkeypatch, "a")["band"]
    assert msg is not None and "tail band" in msg and "first damaged byte 0 B past the payload's end" in msg
    assert "empty (5,) torch.float32" in msg and "<string>:5" in msg      # the allocation, by shape, dtype and source line


def test_b_write_before_an_output_names_allocation_and_offset(fake, monkeypatch):
    msg = _three_runs(fake, monkeypatch, "b")["band"]
    assert msg is not None and "head band" in msg and "nearest damaged byte 1 B before the payload's start" in msg and "(the first one 4 B" in msg
    assert "empty (5,) torch.float32" in msg and "<string>:5" in msg


def test_c_unwritten_last_element_is_seen(fake, monkeypatch):
    seen = _three_runs(fake, monkeypatch, "c")
    assert seen["unwritten"] and seen["differ"] and seen["band"] is None and not seen["input"]


def test_d_modified_input_is_seen(fake, monkeypatch):
    seen = _three_runs(fake, monkeypatch, "d")
    assert seen["input"] and seen["band"] is None


def test_e_read_past_an_input_reaches_the_result(fake, monkeypatch):
    seen = _three_runs(fake, monkeypatch, "e")
    assert seen["differ"] and seen["band"] is None and not seen["input"]     # the guarded runs fold a NaN in, the plain run a neighbour


def test_f_read_of_unwritten_scratch_reaches_the_result(fake, monkeypatch):
    seen = _three_runs(fake, monkeypatch, "f")
    assert seen["differ"] and seen["band"] is None and not seen["input"]     # NaN prefill against zero prefill


# ------------------------------------------------------------------ alignment and edge requests
@pytest.mark.parametrize("nbytes", [0, 1, 3, 20, 255, 256, 4096, 4097])
def test_payload_alignment_and_exact_tail(nbytes):
    alloc = _guard.GuardedAlloc("nan", ("cpu",))
    proxy = _guard.TorchProxy(torch, alloc)
    t = proxy.empty(nbytes, dtype=torch.uint8, device="cpu")
    assert t.shape == (nbytes,) and t.dtype == torch.uint8
    rec = alloc.records[-1]
    assert rec.nbytes == nbytes and rec.start >= _guard.BAND and rec.backing.numel() - rec.start - nbytes >= _guard.BAND
    if nbytes:
        assert t.data_ptr() % 256 == 0
        assert t.data_ptr() == rec.backing.data_ptr() + rec.start        # the tail band begins at the exact byte where the payload ends
        assert bool((t == 0xFF).all())
        t.zero_()
    alloc.check()
    if nbytes:
        rec.backing[rec.start + nbytes] = 0                               # one byte past the end: no rounding up hides it
        with pytest.raises(_guard.GuardError, match="first damaged byte 0 B past"):
            alloc.check()


def test_proxy_forms_and_values():
    alloc = _guard.GuardedAlloc("zero", ("cpu",))
    proxy = _guard.TorchProxy(torch, alloc)
    assert proxy.empty(2, 3).shape == (2, 3) and proxy.empty((2, 3)).shape == (2, 3) and proxy.empty(torch.Size([2, 3])).shape == (2, 3)
    assert proxy.empty(7).dtype == torch.get_default_dtype() and bool((proxy.empty(7) == 0).all())      # "zero" prefill
    assert proxy.empty((0, 3), dtype=torch.float32).shape == (0, 3) and proxy.zeros(0).numel() == 0
    z, o = proxy.zeros(3, 5, dtype=torch.int64), proxy.ones((4,), dtype=torch.float64)
    assert z.dtype == torch.int64 and bool((z == 0).all()) and o.dtype == torch.float64 and bool((o == 1).all())
    f = proxy.full((2, 2), 2.5)
    assert f.dtype == torch.float32 and bool((f == 2.5).all()) and proxy.full((3,), 4).dtype == torch.int64
    like = torch.arange(6, dtype=torch.int32).reshape(2, 3)
    assert proxy.empty_like(like).dtype == torch.int32 and proxy.empty_like(like).shape == (2, 3)
    assert bool((proxy.zeros_like(like) == 0).all()) and bool((proxy.ones_like(like) == 1).all())
    fl = proxy.full_like(like, 9, dtype=torch.float32)
    assert fl.dtype == torch.float32 and bool((fl == 9).all())
    assert proxy.empty(3, requires_grad=True).requires_grad
    n = len(alloc)
    assert proxy.empty(3, device="meta").device.type == "meta" and len(alloc) == n      # an unguarded device goes to torch as it came
    assert proxy.float32 is torch.float32 and proxy.Tensor is torch.Tensor and proxy.cuda is torch.cuda
    alloc.check()
    nan = _guard.GuardedAlloc("nan", ("cpu",))
    assert _guard.has_unwritten_word(_guard.TorchProxy(torch, nan).empty(3, dtype=torch.float32))
    assert bool(torch.isnan(_guard.TorchProxy(torch, nan).empty(3, dtype=torch.float64)).all())
    assert bool((_guard.TorchProxy(torch, nan).empty(3, dtype=torch.int64) == -1).all())


def test_place_bits_and_recorder():
    alloc = _guard.GuardedAlloc("nan", ("cpu",))
    src = torch.tensor([1.0, float("nan"), -0.0])
    src._aon_form = 1
    put = _guard.place(alloc, src)
    assert put.data_ptr() != src.data_ptr() and put.data_ptr() % 256 == 0 and put._aon_form == 1
    assert torch.equal(_guard.bits(put), _guard.bits(src)) and not torch.equal(put, src)      # NaN equals NaN bitwise only
    assert _guard.place(alloc, 3) == 3
    assert bool(torch.isnan(put.as_strided((1,), (1,), put.storage_offset() + 3)).all())       # past its end: NaN, not a neighbour
    ns = types.SimpleNamespace(aon_one=1, aon_two=2, other=3)
    rec = _guard.LibRecorder(ns)
    assert rec.aon_one == 1 and rec.other == 3 and getattr(rec, "aon_" + "two") == 2
    assert rec.names == {"aon_one", "aon_two"}


# ------------------------------------------------------------------ completeness of the case table (the half that needs no GPU)
def stream_entry_points():
    """Every entry point of include/aon_hip.h whose parameter list has a `stream` parameter (comments stripped as
    tests/test_abi_cpu.py::declared_symbols does)."""
    text = open(os.path.join(ROOT, "include", "aon_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return sorted({m.group(1) for m in re.finditer(r"\b(aon_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
                   if re.search(r"\bstream\b", m.group(2))})


def test_every_stream_entry_point_is_in_a_case_or_excluded():
    import test_hip_extents as ext

    names = stream_entry_points()
    assert len(names) >= 79 and "aon_render_fwd_ex" in names and "aon_adam_step" in names and "aon_abi_version" not in names
    reached = set().union(*(set(c.reaches) for c in ext.CASES))
    assert not reached - set(names), f"cases name entry points the header does not have: {sorted(reached - set(names))}"
    both = reached & set(ext.EXCLUDED)
    assert not both, f"both covered and excluded: {sorted(both)}"
    missing = [n for n in names if n not in reached and n not in ext.EXCLUDED]
    assert not missing, f"stream-taking entry points neither in a case's `reaches` nor excluded: {missing}"
    for name, (rule, reason) in ext.EXCLUDED.items():
        assert name in names, f"{name} is excluded but not a stream-taking entry point"
        assert rule in ("probe", "older form", "multi-gpu") and reason and "\n" not in reason
        if rule == "older form":      # the reason names the covered form tests/test_hip_entry_ladder.py shows it forwarding to
            forms = [w for w in re.findall(r"aon_[a-z_0-9]+", reason) if w != name]
            assert forms and all(f in reached for f in forms), f"{name}: {reason!r} names no covered form"
            ladder = open(os.path.join(ROOT, "tests", "test_hip_entry_ladder.py")).read()
            stem = name.replace("aon_art_", "").replace("aon_", "")
            assert stem.split("render_")[-1] in ladder
    assert len({c.name for c in ext.CASES}) == len(ext.CASES)
