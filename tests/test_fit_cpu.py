"""The shared pieces of the frozen-network fits (fit.py), what can be checked without a GPU and without the
library: the freeze context manager, the code layout on the flat Adam buffer and the `lr` rule.  No Adam step is taken here."""
import pytest
import torch


def _net():
    net = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))
    net[0].bias.requires_grad_(False)
    net[1].weight.requires_grad_(False)
    return net


def test_frozen_restores_mixed_flags():
    from aon_amd import fit

    net = _net()
    flags = [p.requires_grad for p in net.parameters()]
    assert flags == [True, False, False, True]
    with fit.frozen(net):
        assert not any(p.requires_grad for p in net.parameters())
        x = torch.ones(5, 3, requires_grad=True)
        g, = torch.autograd.grad(net(x).sum(), x)
        assert g.shape == x.shape
    assert [p.requires_grad for p in net.parameters()] == flags
    assert all(p.grad is None for p in net.parameters())
    with pytest.raises(KeyError, match="inside"):
        with fit.frozen(net):
            assert not any(p.requires_grad for p in net.parameters())
            raise KeyError("inside")
    assert [p.requires_grad for p in net.parameters()] == flags
    assert all(p.grad is None for p in net.parameters())
    with fit.frozen(net, freeze=False):         # the pass-through of fit_latents(full_backward=True)
        assert [p.requires_grad for p in net.parameters()] == flags
    assert [p.requires_grad for p in net.parameters()] == flags


def _codes(K, seed=0):
    from aon_amd import ops

    gen = torch.Generator().manual_seed(seed)
    return [{k: torch.randn(1, d, generator=gen) for k, d in ops._LATENT_KEYS} for _ in range(K)]


@pytest.mark.parametrize("K", [1, 3])
def test_code_buffer_layout(K):
    from aon_amd import fit, ops

    assert [k for k, _ in ops._LATENT_KEYS] == ["density", "color", "articulation"] and fit.CODE_WIDTH == 288
    given = _codes(K)
    given[0]["color"] = given[0]["color"].reshape(-1).requires_grad_(True)      # a (dim,) tensor that requires grad is copied in all the same
    buf = fit.CodeBuffer(given, "cpu", ("density", "articulation"))
    assert buf.rows.shape == (4, 288 * K) and buf.rows.dtype == torch.float32 and not buf.rows.requires_grad
    assert not buf.rows[1:].any()                                                # gradients and moments start at zero
    assert len(buf.leaves) == K
    base = buf.rows.data_ptr()
    for j, mine in enumerate(buf.leaves):
        assert list(mine) == ["density", "color", "articulation"]
        for (k, d), off in zip(ops._LATENT_KEYS, (0, 128, 256)):
            leaf = mine[k]
            assert leaf.shape == (1, d) and leaf.is_leaf and leaf.data_ptr() == base + 4 * (288 * j + off)       # row 0's own storage
            assert leaf.requires_grad == (k != "color")
            assert torch.equal(leaf.detach(), given[j][k].detach().reshape(1, d))
    assert len(buf.wrt) == 2 * K                                                # objects outer, keys inner
    assert all(buf.wrt[2 * j] is buf.leaves[j]["density"] and buf.wrt[2 * j + 1] is buf.leaves[j]["articulation"] for j in range(K))
    # the round trip is exact, and the clones are copies
    back = buf.clones()
    assert len(back) == K
    for j in range(K):
        for k, d in ops._LATENT_KEYS:
            assert back[j][k].shape == (1, d) and not back[j][k].requires_grad and torch.equal(back[j][k], given[j][k].detach().reshape(1, d))
            assert not base <= back[j][k].data_ptr() < base + buf.rows.numel() * 4
    # a write to the value row shows through the leaves; gradients land in the fitted slots only
    with torch.no_grad():
        buf.rows[0].add_(1.0)
    assert torch.equal(buf.leaves[K - 1]["articulation"].detach(), given[K - 1]["articulation"] + 1.0)
    buf.take([torch.full_like(w, float(i + 1)) for i, w in enumerate(buf.wrt)])
    for j in range(K):
        row = buf.rows[1, 288 * j: 288 * (j + 1)]
        assert bool((row[:128] == 2 * j + 1).all()) and not row[128:256].any() and bool((row[256:] == 2 * j + 2).all())
    assert not buf.rows[2:].any()


def test_code_buffer_fit_keys_choices():
    from aon_amd import fit

    given = _codes(2, seed=1)
    none = fit.CodeBuffer(given, "cpu")
    assert none.wrt == [] and not any(v.requires_grad for mine in none.leaves for v in mine.values())
    every = fit.CodeBuffer(given, "cpu", ("density", "color", "articulation"))
    assert len(every.wrt) == 6 and all(v.requires_grad for mine in every.leaves for v in mine.values())
    assert [w.data_ptr() - every.rows.data_ptr() for w in every.wrt] == [4 * o for o in (0, 128, 256, 288, 416, 544)]


def test_adam_buffer_leaves():
    from aon_amd import fit

    buf = fit.AdamBuffer(18, "cpu")
    assert buf.rows.shape == (4, 18) and not buf.rows.any() and buf.wrt == []
    views = [buf.leaf(6 * v, 6) for v in range(2)]                              # fit_pose's per-view 6-vectors
    held = buf.leaf(12, 6, (2, 3), requires_grad=False)
    assert all(x.shape == (6,) and x.requires_grad and x.is_leaf and x.data_ptr() == buf.rows.data_ptr() + 24 * v for v, x in enumerate(views))
    assert held.shape == (2, 3) and not held.requires_grad and held.data_ptr() == buf.rows.data_ptr() + 48
    assert len(buf.wrt) == 2 and all(a is b for a, b in zip(buf.wrt, views))
    buf.take([torch.arange(6.0)], 1)                                            # view 1's gradient alone
    assert torch.equal(buf.rows[1], torch.cat([torch.zeros(6), torch.arange(6.0), torch.zeros(6)])) and not buf.rows[[0, 2, 3]].any()
    buf.take((torch.ones(6), 2.0 * torch.ones(6)))
    assert torch.equal(buf.rows[1], torch.cat([torch.ones(6), 2.0 * torch.ones(6), torch.zeros(6)]))


def test_code_norm_penalty_is_the_inline_expression():
    from aon_amd import fit, ops

    leaves = _codes(3, seed=2)
    want = 1e-4 * sum(torch.mean(torch.norm(codes[k], dim=0)) for codes in leaves for k in ("density", "color", "articulation"))
    assert torch.equal(fit.code_norm_penalty(leaves), want)
    assert [k for k, _ in ops._LATENT_KEYS] == ["density", "color", "articulation"]


@pytest.mark.parametrize("lr, want", [(5e-3, (5e-3, 5e-3)), (1, (1, 1)), ((2e-3, 5e-3), (2e-3, 5e-3)), ([2e-3, 1], (2e-3, 1))])
def test_lr_pair_accepts(lr, want):
    from aon_amd import fit

    assert fit.lr_pair("fit_pose", lr) == want


@pytest.mark.parametrize("lr", [0.0, -1e-3, True, False, None, "1e-3", (1e-3,), (1e-3, 1e-3, 1e-3), (1e-3, 0.0), (True, 1e-3), (1e-3, None), (), float("nan")])
def test_lr_pair_refuses(lr):
    from aon_amd import fit

    with pytest.raises(ValueError, match=r"who: lr must be positive \(one rate, or a pair for poses and codes\), got"):
        fit.lr_pair("who", lr)
