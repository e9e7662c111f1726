"""Latent-only backward / fit_latents, what can be checked without a GPU: the C ABI declares and exports the new
entry points, the ctypes binding registers them, argument validation happens on the host, and fit_latents' `init` / `steps` rules."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("aon_art_render_bwd_latents", "aon_train_scratch_bytes_latents")


def test_header_declares_and_library_exports_the_new_symbols():
    from aon_amd import _lib

    header = open(os.path.join(ROOT, "include", "aon_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert getattr(_lib.lib, name) is not None
    assert re.search(r"#define AON_ABI_VERSION 5\b", header) and _lib.lib.aon_abi_version() == 5   # additive: no bump


def test_ctypes_signatures_are_registered():
    from aon_amd import _lib

    full = _lib._SIGS["aon_art_render_bwd_ex"][1]
    lat = _lib._SIGS["aon_art_render_bwd_latents"][1]
    # aon_art_render_bwd_ex minus the three latents and the two gradient arrays
    assert len(lat) == len(full) - 5 and _lib._SIGS["aon_art_render_bwd_latents"][0] is C.c_int
    assert list(_lib.lib.aon_art_render_bwd_latents.argtypes) == list(lat)
    assert _lib._SIGS["aon_train_scratch_bytes_latents"] == (C.c_int64, [C.c_int64, C.c_int, C.c_void_p])
    assert _lib.lib.aon_train_scratch_bytes_latents.restype is C.c_int64
    assert set(NEW) <= set(_lib.exported_symbols())


def test_entry_points_validate_without_gpu():
    from aon_amd import _lib

    lib = _lib.lib
    for n in (1, 37, 4096):
        for levels in (1, 2):
            small, full = lib.aon_train_scratch_bytes_latents(n, levels, None), lib.aon_train_scratch_bytes_ex(n, 1, levels, None)
            assert 0 < small < full, (n, levels)
            assert full - small >= levels * (90 << 20)     # the weight-gradient workspaces are what is left out
    assert lib.aon_train_scratch_bytes_latents(4096, 1, None) < lib.aon_train_scratch_bytes_latents(4096, 2, None)
    rc = lib.aon_art_render_bwd_latents(None, None, None, None, None, 0, 1, 2, None, None, None, None, None, None, None, None, None, 0, None, 0, None, None)
    assert rc != 0 and b"aon_art_render_bwd_latents" in lib.aon_last_error()
    rc = lib.aon_art_render_bwd_latents(None, None, None, None, None, 16, 1, 3, None, None, None, None, None, None, None, None, None, 0, None, 0, None, None)
    assert rc != 0 and b"num_levels" in lib.aon_last_error()
    rc = lib.aon_art_render_bwd_latents(None, None, None, None, None, 16, 1, 2, None, None, None, None, None, None, None, None, None, 0, None, 0, None, None)
    assert rc != 0 and b"null" in lib.aon_last_error()


@pytest.fixture(scope="module")
def lit():
    import aon_amd.synthetic as syn
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    lit = LitNeRF_AutoDecoder(hparams={"N_max_objs": 3})
    lit.code_library.load_state_dict(syn.make_code_library_state(seed=4, n_max_objs=3))
    return lit


def test_fit_latents_rejects_bad_arguments(lit):
    batch = {"rays_o": torch.zeros(4, 3), "rays_d": torch.zeros(4, 3), "viewdirs": torch.zeros(4, 3), "target": torch.zeros(4, 3)}
    for steps in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="steps"):
            lit.fit_latents([batch], steps)
    with pytest.raises(ValueError, match="no batches"):
        lit.fit_latents([], 3)
    with pytest.raises(ValueError, match="lr"):
        lit.fit_latents([batch], 3, lr=0.0)
    good = {"density": torch.zeros(1, 128), "color": torch.zeros(128), "articulation": torch.zeros(1, 32)}
    bad_inits = ["median", 5, (0,), (0, 1, 2), (3, 0), (0, 10), (-1, 0), (0.0, 1), {"density": good["density"]},
                 dict(good, articulation=torch.zeros(1, 31)), dict(good, extra=torch.zeros(1))]
    for init in bad_inits:
        with pytest.raises(ValueError, match="init"):
            lit.fit_latents([batch], 3, init=init)
    flags = [p.requires_grad for p in lit.model.parameters()]
    assert all(flags)      # nothing above froze the network


def test_initial_latents(lit):
    tables = {"density": lit.code_library.embedding_instance_shape.weight, "color": lit.code_library.embedding_instance_appearance.weight,
              "articulation": lit.code_library.embedding_instance_articulation.weight}
    mean = lit._initial_latents("mean", "cpu")
    for k, w in tables.items():
        assert mean[k].shape == (1, w.shape[1]) and mean[k].dtype == torch.float32 and not mean[k].requires_grad
        assert torch.equal(mean[k], w.detach().mean(dim=0, keepdim=True)), k
    rows = lit._initial_latents((2, 7), "cpu")
    assert torch.equal(rows["density"], tables["density"].detach()[2:3]) and torch.equal(rows["color"], tables["color"].detach()[2:3])
    assert torch.equal(rows["articulation"], tables["articulation"].detach()[7:8])
    rows["density"].zero_()     # copies: the library is untouched
    assert tables["density"].detach()[2].abs().sum() > 0
    given = {"density": torch.arange(128.0), "color": torch.ones(1, 128), "articulation": torch.full((32,), 2.0, dtype=torch.float64)}
    out = lit._initial_latents(given, "cpu")
    assert torch.equal(out["density"], torch.arange(128.0).reshape(1, 128)) and out["articulation"].dtype == torch.float32
    assert out["articulation"].shape == (1, 32)
