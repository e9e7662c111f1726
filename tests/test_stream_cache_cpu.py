"""ops.StreamCache, the one helper behind the four scratch caches of the whole-path calls (_WS_CACHE, _GWS_CACHE, _OCC_WS_CACHE, _WG_WS):
driven with fake stream handles and a counting fake allocator -- no GPU, no library call.

The property that matters is NO ALIASING: two calls in flight on two streams of one device never get the same workspace.  The rule these
caches had before (key = the device alone) is kept below in ten lines and shown to fail that property, so the test is known to tell the
two apart without a race ever being run on a GPU."""
import itertools

import pytest


class FakeBuf:
    def __init__(self, serial, nbytes):
        self.serial, self.nbytes = serial, nbytes

    def numel(self):
        return self.nbytes


class CountingAlloc:
    def __init__(self):
        self.calls = []

    def __call__(self, nbytes):
        self.calls.append(nbytes)
        return FakeBuf(len(self.calls), nbytes)


class DeviceKeyedCache:
    """The parent's rule, as _workspace / grender_fwd / _occ_workspace / the wgrad wrappers had it: ONE buffer per device, whatever the
    stream; a larger request replaces it."""

    def __init__(self):
        self._entries = {}

    def get(self, key, need, alloc):
        dev = key[0]
        ws = self._entries.get(dev)
        if ws is None or ws.numel() < need:
            ws = self._entries[dev] = alloc(need)
        return ws


S1, S2, S3 = 0x7F00_0000_1000, 0x7F00_0000_2000, 0x7F00_0000_3000   # stream handles are pointers; 0 is the null stream


def _new():
    from aon_amd import ops

    return ops.StreamCache(register=False), CountingAlloc()


def no_alias(cache, alloc):
    """Two streams of one device ask in every interleaving (and grow): do they ever hold the same buffer?"""
    held = {}
    for stream, need in [(S1, 100), (S2, 100), (S1, 100), (S2, 400), (S1, 100), (S1, 900), (S2, 400), (0, 50), (S1, 10), (S2, 10), (0, 2000), (S1, 10)]:
        held[stream] = cache.get((0, stream), need, alloc)
        assert held[stream].numel() >= need
        if any(a is b for a, b in itertools.combinations(held.values(), 2)):
            return False
    return True


def test_same_stream_reuses():
    cache, alloc = _new()
    a = cache.get((0, S1), 100, alloc)
    assert cache.get((0, S1), 100, alloc) is a and cache.get((0, S1), 7, alloc) is a    # a smaller request keeps the larger buffer
    assert alloc.calls == [100]
    assert cache.get((0, 0), 100, alloc) is cache.get((0, 0), 100, alloc)                 # the null stream (handle 0) is a key like any other
    assert alloc.calls == [100, 100]


def test_two_streams_never_alias():
    cache, alloc = _new()
    assert no_alias(cache, alloc)
    # ... and the same stream handle on another device is another key
    assert cache.get((0, S1), 8, alloc) is not cache.get((1, S1), 8, alloc)


def test_parent_rule_aliases():
    """The discrimination proof: under key = device only, the first two requests already share a buffer."""
    alloc = CountingAlloc()
    parent = DeviceKeyedCache()
    assert parent.get((0, S1), 100, alloc) is parent.get((0, S2), 100, alloc)
    assert not no_alias(DeviceKeyedCache(), CountingAlloc())


def test_growth_replaces_only_that_streams_entry():
    cache, alloc = _new()
    a, b = cache.get((0, S1), 100, alloc), cache.get((0, S2), 100, alloc)
    a2 = cache.get((0, S1), 101, alloc)
    assert a2 is not a and a2.numel() == 101 and a2 is not b
    assert cache.get((0, S2), 100, alloc) is b                  # S2's entry is untouched by S1's growth
    assert cache.get((0, S1), 101, alloc) is a2 and len(cache) == 2
    b2 = cache.get((0, S2), 5000, alloc)                        # growth on the other one
    assert b2 is not b and cache.get((0, S1), 50, alloc) is a2
    assert alloc.calls == [100, 100, 101, 5000]


def test_bound_holds_and_drops_least_recently_used():
    from aon_amd import ops

    cache, alloc = _new()
    assert cache.max_entries == ops.STREAM_CACHE_ENTRIES >= 2
    keep = cache.get((0, S1), 64, alloc)
    for i in range(10 * cache.max_entries):           # a loop of fresh handles, the kept stream used in between
        cache.get((0, 0x1000 + 16 * i), 64, alloc)
        assert cache.get((0, S1), 64, alloc) is keep
        assert len(cache) <= cache.max_entries
    assert len(cache) == cache.max_entries
    # the oldest fresh handles are gone (asking again allocates), the most recent ones are still there
    n = len(alloc.calls)
    last = 0x1000 + 16 * (10 * cache.max_entries - 1)
    cache.get((0, last), 64, alloc)
    assert len(alloc.calls) == n
    cache.get((0, 0x1000), 64, alloc)
    assert len(alloc.calls) == n + 1
    small = ops.StreamCache(max_entries=2, register=False)
    x = small.get((0, S1), 1, alloc)
    small.get((0, S2), 1, alloc)
    small.get((0, S1), 1, alloc)     # S1 is now the most recent
    small.get((0, S3), 1, alloc)     # drops S2
    assert small.get((0, S1), 1, alloc) is x and len(small) == 2 and (0, S2) not in small._entries


def test_release_workspaces_empties_every_cache():
    from aon_amd import ops

    caches = {"_WS_CACHE": ops._WS_CACHE, "_GWS_CACHE": ops._GWS_CACHE, "_OCC_WS_CACHE": ops._OCC_WS_CACHE, "_WG_WS": ops._WG_WS}
    for name, cache in caches.items():
        assert isinstance(cache, ops.StreamCache), name
        assert any(cache is c for c in ops._STREAM_CACHES), name
    alloc = CountingAlloc()
    try:
        for cache in caches.values():
            cache.get((0, S1), 16, alloc)
            cache.get((0, S2), 16, alloc)
            assert len(cache) == 2
        ops._TRAIN_POOL[(0, 16)] = []
        ops.release_workspaces()
        for name, cache in caches.items():
            assert len(cache) == 0 and cache.values() == [], name
        assert not ops._TRAIN_POOL
    finally:
        for cache in caches.values():
            cache.clear()
        ops._TRAIN_POOL.clear()


def test_workspace_on_cpu_is_refused():
    import torch

    from aon_amd import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.stream_key(torch.device("cpu"))
