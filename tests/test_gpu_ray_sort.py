"""GPU suite (-m gpu): the per-bounce ray sort (option "sort", csrc/kernels.hip k_sortg_hist / k_sortg_scatter).

The permutation itself, through rdx_debug_sort_keys -- the frame path's own launch on the caller's keys: for every capacity / live
count, key set and number of key bits the output is a permutation of [0, m) along which the reduced key
(((k >> 3) >> (15 - bits)) << 3) | (k & 7) does not decrease.  Sizes: below one 8-key load of a wave (1, 63), one wave's worth of
lanes (64), around 4096 and around 8192 paths -- a block's smallest slice, from where on a second block shares the work -- and
256 * 4096 + 17 and 256 * 8192 + 17: 129 blocks, and every block of the full grid with a slice longer than the smallest; both
end ragged.  A live count of 0 under a capacity of 4096.

Frames: the sort only changes the order in which the traversal launch hands its rays out, so a sorted frame is the unsorted
frame bit for bit -- with one sample group and with two (each group owns a sort scratch).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 4095, 4096, 4097, 8191, 8192, 8193, 256 * 4096 + 17, 256 * 8192 + 17]
KEYSETS = ["random", "equal", "largest", "increasing"]


@pytest.fixture(scope="module")
def mods(gpu):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd, scenes
    return rd, scenes


def _sort(rd, keys, live=None, key_bits=13, keys_offset=0):
    """rdx_debug_sort_keys on `keys` (their number is the capacity, the first `live` are alive), `keys_offset` bytes into their
    device buffer -> perm[0 .. live)"""
    from radiance_ray_tracing_amd import _lib
    k = np.ascontiguousarray(keys, np.uint16).reshape(-1)
    live = k.shape[0] if live is None else int(live)
    kb = rd.CreateBuffer(None, keys_offset + max(k.nbytes, 2))
    pb = rd.CreateBuffer(None, max(k.shape[0] * 4, 4))
    rd.WriteBuffer(None, kb, k.nbytes, k, keys_offset)
    if _lib.lib().rdx_debug_sort_keys(kb.handle, keys_offset, live, k.shape[0], key_bits, pb.handle, 0) != 0:
        raise rd.RadianceError(_lib.last_error())
    out = np.empty(min(live, k.shape[0]), np.uint32)
    if out.size:
        rd.ReadBuffer(None, pb, out.nbytes, out.view(np.uint8))
    return out


def _keys(kind, n):
    if kind == "random":
        return np.random.default_rng(n).integers(0, 1 << 15, n, dtype=np.uint16)
    if kind == "equal":
        return np.full(n, 0x1234, np.uint16)
    if kind == "largest":
        return np.full(n, 0x7fff, np.uint16)
    # strictly increasing as far as 15 bits go: every key once, then the largest
    return np.minimum(np.arange(n, dtype=np.int64), 0x7fff).astype(np.uint16)


def _reduced(k, bits):
    k = k.astype(np.uint32)
    return (((k >> 3) >> (15 - bits)) << 3) | (k & 7)


def _check(perm, keys, m, bits, what):
    assert perm.shape == (m,), what
    seen = np.zeros(m, np.uint8)
    assert not m or int(perm.max()) < m, (what, "an entry is not below the live count")
    seen[perm] = 1
    assert int(seen.sum()) == m, (what, "not a permutation", m - int(seen.sum()))
    r = _reduced(keys, bits)[perm]
    assert not (r[1:] < r[:-1]).any(), (what, "the reduced key decreases", int(np.flatnonzero(r[1:] < r[:-1])[0]))


@pytest.mark.parametrize("bits", [13, 14])
@pytest.mark.parametrize("kind", KEYSETS)
def test_the_permutation(mods, kind, bits):
    rd, _ = mods
    for n in SIZES:
        keys = _keys(kind, n)
        _check(_sort(rd, keys, key_bits=bits), keys, n, bits, (kind, bits, n))
    # consecutive sorts alternate between the two copies of the key totals: as the 12th and 13th sort of this test these two sizes
    # count into the other copy than they did as the 3rd and 6th
    for n in (64, 4097):
        keys = _keys(kind, n)
        _check(_sort(rd, keys, key_bits=bits), keys, n, bits, (kind, bits, n, "other phase"))


@pytest.mark.parametrize("bits", [13, 14])
def test_live_count_below_the_capacity(mods, bits):
    """the grid is sized by the capacity, the slices by the live count: nothing alive, and live counts that leave blocks without
    a slice; keys past the live count are never read as keys of a path (they hold the largest key here)"""
    rd, _ = mods
    for cap, live in ((4096, 0), (4096, 1), (4097, 63), (256 * 4096 + 17, 4097), (256 * 4096 + 17, 8193), (256 * 4096 + 17, 256 * 4096 + 9)):
        keys = _keys("random", cap)
        keys[live:] = 0x7fff
        _check(_sort(rd, keys, live=live, key_bits=bits), keys, live, bits, (cap, live, bits))
    # after a sort of nothing the next one still starts from zeroed totals
    keys = _keys("random", 4097)
    _check(_sort(rd, keys, key_bits=bits), keys, 4097, bits, "after live 0")


def test_keys_that_are_not_16_byte_aligned(mods):
    """keys two bytes into their buffer take the one-key-at-a-time loads"""
    rd, _ = mods
    for n in (63, 4097, 40000):
        keys = _keys("random", n)
        _check(_sort(rd, keys, key_bits=13, keys_offset=2), keys, n, 13, ("offset 2", n))


def test_refusals(mods):
    rd, _ = mods
    keys = _keys("random", 64)
    for kw in ({"key_bits": 11}, {"key_bits": 15}, {"live": 65}, {"keys_offset": 1}):
        with pytest.raises(rd.RadianceError):
            _sort(rd, keys, **kw)


def test_sorted_frames_are_the_unsorted_frame(mods):
    """160 x 90 x 4 spp x depth 4 of c2_atrium, 57 600 paths: imageScratch with `sort` 1 equals `sort` 0 bit for bit, with one
    sample group and with two"""
    rd, scenes = mods
    dev = scenes.DeviceScene(scenes.c2_atrium(160, 90, 4, 4, detail=0.25))
    frames = {}
    try:
        for sort, groups in ((0, 1), (1, 1), (1, 2)):
            rd.SetOption("sort", sort)
            rd.SetOption("groups", groups)
            dev.set_rtprop(totalSamples=0)
            dev.clear_scratch()
            dev.render()
            st = rd.GetTraceStats()
            assert st.groups == groups, (sort, groups, st.groups)
            frames[(sort, groups)] = dev.read_scratch().copy()
    finally:
        rd.SetOption("sort", -1)
        rd.SetOption("groups", 0)
    ref = frames[(0, 1)]
    assert np.isfinite(ref).all() and float(ref.max()) > 0.0
    assert np.array_equal(frames[(1, 1)].view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(frames[(1, 2)].view(np.uint32), ref.view(np.uint32))
