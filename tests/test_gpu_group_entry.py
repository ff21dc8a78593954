"""GPU suite (-m gpu): entry items of the shared-transform group (option "group_entry_items", csrc/traverse_pool.h ENT).

With the option on (default) a ray enters ALL pending instances of the group in one instance step, as pool items that point at
per-instance entry records; with 0 it enters one instance per step and tests the root box there.  Every case compares option 1,
option 0 and the reference-order kernel (`kernel` 0) on the same rays, at most 4096 of them: exact equality of every HitData
field for closest-hit rays; for any-hit rays the hit flag (the production engines report nothing else for them: include/rdx.h
rdx_trace_batch, mode 0).  Scenes and rays: tests/group_entry_cases.py.
"""
import numpy as np
import pytest

import group_entry_cases as gec
import ray_query_cases as rq

pytestmark = pytest.mark.gpu
N = 4096


@pytest.fixture(scope="module")
def mods(gpu):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd, scenes
    return rd, scenes


class Built:
    """the TLAS of a case on the device"""

    def __init__(self, rd, scenes, plt, case):
        self.rd, self.plt, self.case = rd, plt, case
        self.meshes, self.insts = gec.instances(scenes, case)
        self.blases = rd.BuildAccelStructs(plt, [rd.Mesh(m[0], m[1]) for m in self.meshes])
        self.tlas = rd.BuildAccelStruct(plt, self.rd_instances(self.insts))
        if case == "non_union":      # the blob with blown-up root boxes, written back: the layout is derived from what the buffer holds
            blob = rd.ReadBuffer(plt, self.tlas, self.tlas.size).tobytes()
            fat = gec.inflate_roots(blob, len(self.insts))
            assert fat != blob
            rd.WriteBuffer(plt, self.tlas, len(fat), np.frombuffer(fat, np.uint8))

    def rd_instances(self, insts):
        return [self.rd.Instance(tf, 0, cid, self.blases[mi]) for mi, tf, cid in insts]

    def blob(self):
        return self.rd.ReadBuffer(self.plt, self.tlas, self.tlas.size).tobytes()


@pytest.fixture(scope="module")
def tlases(mods, gpu):
    rd, scenes = mods
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = Built(rd, scenes, gpu, case)
        return cache[case]
    return get


def _three_ways(rd, run):
    """run() under option 1, option 0 and kernel 0 -> the three results"""
    out = []
    for opts in ({"group_entry_items": 1}, {"group_entry_items": 0}, {"kernel": 0}):
        try:
            for k, v in opts.items():
                rd.SetOption(k, v)
            out.append(run())
        finally:
            rd.SetOption("group_entry_items", 1)
            rd.SetOption("kernel", 3)
    return out


def _trace_equal(rd, tlas, o, d, what):
    for kind in (1, 2):
        on, off, ref = _three_ways(rd, lambda: rd.TraceBatch(tlas, o, d, 0.001, 1000.0, kind))
        if kind == 1:
            assert 0 < int(ref["hit"].sum()) < o.shape[0], what
            for name, got in (("group_entry_items 1", on), ("group_entry_items 0", off)):
                bad = (got.view(np.uint8).reshape(o.shape[0], -1) != ref.view(np.uint8).reshape(o.shape[0], -1)).any(1)
                assert not bad.any(), (what, name, "closest", int(bad.sum()), int(np.flatnonzero(bad)[0]))
        else:
            for name, got in (("group_entry_items 1", on), ("group_entry_items 0", off)):
                bad = got["hit"] != ref["hit"]
                assert not bad.any(), (what, name, "any", int(bad.sum()), int(np.flatnonzero(bad)[0]))


def _layout(rd, b):
    s, _ = rd.DebugAccelLayout(b.blob())
    return s


def test_forty_members_overflow_the_pool(tlases, mods):
    """case 1: a group of 40 (two bitmap words); 64 lanes x 40 entry items are several times the pool, so the per-lane quota of
    the instance step runs"""
    rd, scenes = mods
    b = tlases("stack40")
    s = _layout(rd, b)
    assert s["groupCount"] == 40 and s["topFlat"] > 0 and s["groupIdentity"] == 0
    _, need = rd.DebugAccelEntries(b.blob())
    assert 64 * 40 > 64 * (max(s["quadNeed"], need) + 8)        # more items than any pool of this scene (csrc/traverse_pool.h pool_cap)
    o, d = gec.world_rays(scenes, "stack40", N, 11)
    # ... and steps do run with a quota below a lane's pending count.  A wave takes 64 consecutive rays and they reach their first
    # instance step together.  The pool of this scene holds 256 entries (pool_cap: 64 x the need of 4), so the quota of a step
    # with more than 8 ready lanes is at most (256 - RESERVE) >> 4 = 15: in every block of 64 rays more than 8 must have over 15
    # instances pending -- counted here as the members whose world box (the engine's pre-test box) the ray passes through
    _, a = rd.DebugAccelLayout(b.blob())
    lo, hi = a["insts"]["worldMin"][:, :3].astype(np.float64), a["insts"]["worldMax"][:, :3].astype(np.float64)
    with np.errstate(all="ignore"):
        tA = (lo[None] - o[:, None].astype(np.float64)) / d[:, None].astype(np.float64)
        tB = (hi[None] - o[:, None].astype(np.float64)) / d[:, None].astype(np.float64)
    tn, tf = np.fmin(tA, tB).max(2), np.fmax(tA, tB).min(2)
    pending = (tf > np.fmax(tn, 0.0)).sum(1)
    assert max(s["quadNeed"], need) == 4 and ((pending > 15).reshape(-1, 64).sum(1) > 8).all()
    _trace_equal(rd, b.tlas, o, d, "stack40")


def test_group_beside_other_instances_and_a_leaf_root(tlases, mods):
    """case 2: group lanes take entry items, the other instances (and the inline leaf root) today's path, in the same steps"""
    rd, scenes = mods
    b = tlases("mixed")
    s = _layout(rd, b)
    assert s["groupCount"] == 3 and s["nInst"] == 6 and s["leafRoots"] == 1 and s["topFlat"] > 0
    o, d = gec.world_rays(scenes, "mixed", N, 12)
    _trace_equal(rd, b.tlas, o, d, "mixed")
    try:        # ... and with the leaf root entered like any other instance
        rd.SetOption("inline_leaf_roots", 0)
        _trace_equal(rd, b.tlas, o, d, "mixed, inline_leaf_roots 0")
    finally:
        rd.SetOption("inline_leaf_roots", 1)


@pytest.mark.parametrize("case", ["leaf_kids", "non_union"])
def test_leaf_children_and_non_union_roots(tlases, mods, case):
    """case 3: roots with one or two leaf children (pair form with leaf entries), and root boxes that are not the union of their
    children's (single-entry form)"""
    rd, scenes = mods
    b = tlases(case)
    s = _layout(rd, b)
    assert s["groupCount"] == len(b.insts) and s["topFlat"] > 0
    e, _ = rd.DebugAccelEntries(b.blob())
    pair = (e["half"][:, 0]["ld1"] & 1) != 0
    assert pair.all() if case == "leaf_kids" else not pair.any()
    o, d = gec.world_rays(scenes, case, N, 13)
    _trace_equal(rd, b.tlas, o, d, case)


@pytest.mark.parametrize("case", ["stack40", "mixed"])
def test_query_rays_with_per_ray_intervals(tlases, mods, case):
    """case 4: the same through rdx_query_rays, every ray with its own interval"""
    rd, scenes = mods
    b = tlases(case)
    o, d = gec.world_rays(scenes, case, N, 14)
    rng = np.random.default_rng(15)
    rays = np.zeros(N, rq.RAY_DTYPE)
    rays["origin"], rays["direction"] = o, d
    rays["tmin"] = np.where(rng.random(N) < 0.5, 0.001, rng.random(N) * 3.0).astype(np.float32)
    rays["tmax"] = (rays["tmin"] + np.where(rng.random(N) < 0.5, 1000.0, rng.random(N) * 6.0)).astype(np.float32)
    bR = rd.CreateBuffer(b.plt, N * 32)
    rd.WriteBuffer(b.plt, bR, N * 32, rays)
    for kind in (1, 2):
        def run():
            return rd.ReadBuffer(b.plt, rd.QueryRays(b.tlas, bR, N, kind), N * 32).view(rq.RAY_HIT_DTYPE).copy()
        on, off, ref = _three_ways(rd, run)
        assert 0 < int(ref["hit"].sum()) < N
        assert not rq.mismatches(ref, on).any(), (case, kind, "group_entry_items 1", int(rq.mismatches(ref, on).sum()))
        assert not rq.mismatches(ref, off).any(), (case, kind, "group_entry_items 0", int(rq.mismatches(ref, off).sum()))


def test_member_leaves_the_group_and_returns(mods, gpu):
    """case 5: rdx_tlas_update rotates one member out of the group, then puts it back; after each update the answers equal a fresh
    build's of the same instances (and the reference-order kernel's)"""
    rd, scenes = mods
    b = Built(rd, scenes, gpu, "mixed")
    o, d = gec.world_rays(scenes, "mixed", N, 16)
    rd.TraceBatch(b.tlas, o[:64], d[:64])                   # a layout exists before the first update
    moved = [(mi, (np.asarray(scenes.rotate_y(31), np.float32) @ tf).astype(np.float32) if k == 1 else tf, cid)
             for k, (mi, tf, cid) in enumerate(b.insts)]
    for what, insts, group in (("out", moved, 2), ("back", b.insts, 3)):
        rd.UpdateAccelStruct(gpu, b.tlas, b.rd_instances(insts))
        assert _layout(rd, b)["groupCount"] == group, what
        fresh = rd.BuildAccelStruct(gpu, b.rd_instances(insts))
        assert rd.ReadBuffer(gpu, fresh, fresh.size).tobytes() == b.blob(), what
        for kind in (1, 2):
            want = rd.TraceBatch(fresh, o, d, 0.001, 1000.0, kind)
            on, off, ref = _three_ways(rd, lambda: rd.TraceBatch(b.tlas, o, d, 0.001, 1000.0, kind))
            for name, got in (("1", on), ("0", off)):
                if kind == 1:
                    assert got.tobytes() == want.tobytes() == ref.tobytes(), (what, name)
                else:
                    assert np.array_equal(got["hit"], want["hit"]) and np.array_equal(got["hit"], ref["hit"]), (what, name)


def test_atrium_frame_is_the_same_frame(mods):
    """case 6: 160 x 90 x 4 spp x depth 8 of c2_atrium through the fused pipeline: imageScratch and the RGBA8 image, bit for bit,
    between option 1 and option 0"""
    rd, scenes = mods
    dev = scenes.DeviceScene(scenes.c2_atrium(160, 90, 4, 8, detail=0.25))
    frames = []
    for v in (1, 0):
        try:
            rd.SetOption("group_entry_items", v)
            dev.set_rtprop(totalSamples=0)
            dev.clear_scratch()
            img = dev.render().copy()
            frames.append((img, dev.read_scratch().copy()))
        finally:
            rd.SetOption("group_entry_items", 1)
    assert np.isfinite(frames[0][1]).all() and float(frames[0][1].max()) > 0.0
    assert np.array_equal(frames[0][1].view(np.uint32), frames[1][1].view(np.uint32))
    assert np.array_equal(frames[0][0], frames[1][0])
