"""Entry records (csrc/accel_layout.h AccelLayout::entries), checked on the host -- no device.

An entry record E(i) must make a pool item decide exactly what the reference decides when it enters instance slot i: the root
test of radiance.cl:61-63, then the walk below the root R.  Here a numpy walker with the decision rule of quad_half
(csrc/traverse_pool.h) and the reference's slab test (csrc/kernels.hip slab_hit, which slab_fast's decision equals) runs over the
arrays of rd.DebugAccelLayout and rd.DebugAccelEntries, for every instance with an inner root and seeded rays -- aimed at the
root box, past it, with zero direction components, from points in the planes of its faces (tests/group_entry_cases.object_rays):

  * the set of triangle slots tested by "root test, then R's quad record" equals the set tested from E(i), for every ray;
  * the second half of every entry record is inert: two empty entries, which the walker proves to contribute nothing;
  * the entry need is at least the pool growth of a depth-first walk (one item popped, its entries pushed in the engine's order)
    that starts at E(i), on every ray walked that way;
  * a leaf-root instance has an inert record, the layout without quad records has none, and the records follow their instances
    through update_accel_layout.
"""
import numpy as np
import pytest

import accel_layout_cases as alc
import group_entry_cases as gec
import tlas_update_cases as tu

F = np.float32
LEAF, PAIR = 0x80000000, 1
RAYS_PER_INSTANCE = {"c2_small": 160, "group_rotated": 1200, "leaf_root": 1200}
DFS_RAYS = 40


@pytest.fixture(scope="module")
def mods(built):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd, scenes
    return rd, scenes


def case_blob(rd, scenes, case):
    return gec.host_blob(rd, scenes, case) if case in gec.CASES else alc.blob(case)


def slab(o, d, mn, mx):
    """the reference's slab test on (m, 3) float32 arrays: fmin / fmax ignore a NaN (0 / 0), as the device functions do"""
    with np.errstate(all="ignore"):
        tA, tB = (mn - o) / d, (mx - o) / d
    t1, t2 = np.fmin(tA, tB), np.fmax(tA, tB)
    tn = np.fmax(np.fmax(t1[:, 0], t1[:, 1]), t1[:, 2])
    tf = np.fmin(np.fmin(t2[:, 0], t2[:, 1]), t2[:, 2])
    return tf > np.fmax(tn, F(0))


def exact_only(d):
    """traverse_pool.h: a direction component is (nearly) zero"""
    with np.errstate(all="ignore"):
        rcp = F(1) / d
    return ~(np.abs(d).min(1) > F(1e-20)) | ~(np.abs(rcp).max(1) < F(1e20))


def half_decide(H, o, d, ex):
    """quad_half for m items: H = their halves (structured, rd._DWIDE), o / d / ex = their rays -> per entry (A, B): push mask,
    run mask, d0, count"""
    ad0, ad1, bd0, bd1 = H["ld0"], H["ld1"], H["rd0"], H["rd1"]
    leafA, leafB, pair = (ad1 & LEAF) != 0, (bd1 & LEAF) != 0, (ad1 & PAIR) != 0
    sA, sB = slab(o, d, H["lmin"], H["lmax"]), slab(o, d, H["rmin"], H["rmax"])
    u = np.where(~leafA & ~leafB, slab(o, d, np.fmin(H["lmin"], H["rmin"]), np.fmax(H["lmax"], H["rmax"])), np.where(leafA, sA, sB))
    gate = ex & pair
    sA, sB = np.where(gate, sA & u, sA), np.where(gate, sB & u, sB)
    return ((~leafA & sA, leafA & (sA | ~pair), ad0, (ad1 >> 24) & 0x7f),
            (~leafB & sB, leafB & (sB | ~pair), bd0, (bd1 >> 24) & 0x7f))


def walk_sets(T, start, o, d):
    """all rays at once: ray r starts at record start[r] (< 0: nowhere) -> sorted unique (ray << 32 | triangle slot) tested"""
    ex = exact_only(d)
    r = np.flatnonzero(start >= 0)
    q = start[r]
    tested = []
    while r.size:
        nr, nq = [], []
        for h in (0, 1):
            for push, run, d0, cnt in half_decide(T["half"][q, h], o[r], d[r], ex[r]):
                nr.append(r[push]); nq.append(d0[push].astype(np.int64))
                run = run & (cnt > 0)
                for k in range(int(cnt[run].max()) if run.any() else 0):
                    m = run & (cnt > k)
                    tested.append((r[m].astype(np.int64) << 32) | (d0[m].astype(np.int64) + k))
        r, q = np.concatenate(nr), np.concatenate(nq)
    return np.unique(np.concatenate(tested)) if tested else np.zeros(0, np.int64)


def walk_dfs(T, start, o, d):
    """one ray, depth first as the pool's tight mode walks: pop one item, push its inner entries in the engine's order (second
    half's B, A, then the first half's B, A: entry A of the first half ends on top) -> (tested slots, largest pool size)"""
    o, d = o.reshape(1, 3), d.reshape(1, 3)
    ex = exact_only(d)
    stack, tested, top = [int(start)], set(), 0
    while stack:
        i = stack.pop()
        (pa, ra, a0, ac), (pb, rb, b0, bc) = half_decide(T["half"][i:i + 1, 0], o, d, ex)
        (pc, rc, c0, cc), (pe, re_, e0, ec) = half_decide(T["half"][i:i + 1, 1], o, d, ex)
        for p, d0 in ((pe, e0), (pc, c0), (pb, b0), (pa, a0)):
            if p[0]:
                stack.append(int(d0[0]))
        for rn, d0, c in ((ra, a0, ac), (rb, b0, bc), (rc, c0, cc), (re_, e0, ec)):
            if rn[0]:
                tested.update(range(int(d0[0]), int(d0[0]) + int(c[0])))
        top = max(top, len(stack))
    return tested, top


@pytest.fixture(scope="module")
def layouts(mods):
    rd, scenes = mods
    cache = {}

    def get(case):
        if case not in cache:
            blob = case_blob(rd, scenes, case)
            s, a = rd.DebugAccelLayout(blob)
            e, need = rd.DebugAccelEntries(blob)
            cache[case] = (blob, s, a, e, need)
        return cache[case]
    return get


ALL = ("c2_small", "group_rotated", "leaf_kids", "non_union", "mixed", "stack40")


@pytest.mark.parametrize("case", ALL)
def test_entry_walk_tests_what_the_root_walk_tests(layouts, case):
    _, s, a, e, need = layouts(case)
    insts, quad = a["insts"], a["quad"]
    assert len(e) == s["nInst"] == len(insts) and len(quad) > 0
    T = np.concatenate([quad, e])
    inner = np.flatnonzero((insts["rootDesc1"] & LEAF) == 0)
    assert inner.size >= 2
    per = RAYS_PER_INSTANCE.get(case, 600 if len(inner) < 8 else 120)
    rng = np.random.default_rng(1234)
    O, D, slot = [], [], []
    for i in inner:
        o, d = gec.object_rays(rng, insts["rootMin"][i][:3], insts["rootMax"][i][:3], per)
        O.append(o); D.append(d); slot.append(np.full(per, i))
    O, D, slot = np.concatenate(O), np.concatenate(D), np.concatenate(slot)
    n = O.shape[0]
    assert n >= 2000
    hit_root = slab(O, D, insts["rootMin"][slot][:, :3], insts["rootMax"][slot][:, :3])
    zero = (D == 0).any(1)
    assert 0.05 < (~hit_root).mean() < 0.6 and zero.sum() >= n // 8 and (hit_root & zero).any() and (~hit_root & zero).any()
    want = walk_sets(T, np.where(hit_root, insts["rootDesc0"][slot].astype(np.int64), -1), O, D)
    got = walk_sets(T, len(quad) + slot.astype(np.int64), O, D)
    assert want.size > n // 4       # the rays do reach triangles
    if not np.array_equal(want, got):
        odd = np.setxor1d(want, got)
        raise AssertionError("%s: %d (ray, slot) pairs differ; first: ray %d (instance slot %d, o %r, d %r), triangle slot %d"
                             % (case, odd.size, odd[0] >> 32, slot[odd[0] >> 32], O[odd[0] >> 32].tolist(), D[odd[0] >> 32].tolist(),
                                odd[0] & 0xffffffff))
    # a ray that misses the root box tests nothing from E(i)
    assert not np.isin(got >> 32, np.flatnonzero(~hit_root)).any()
    # the need covers a depth-first walk from E(i); the scalar walker agrees with the batched one
    growth = 0
    pick = rng.choice(np.flatnonzero(hit_root), DFS_RAYS, replace=False)
    for r in pick:
        tested, top = walk_dfs(T, len(quad) + int(slot[r]), O[r], D[r])
        assert tested == set((got[(got >> 32) == r] & 0xffffffff).tolist()), (case, int(r))
        assert top <= need, (case, int(r), top, need)
        growth = max(growth, top)
    assert 1 <= growth <= need


def check_forms(s, a, e, union_expected=True):
    """first half: the pair of R's children under R's box iff that box is bit for bit the union of theirs, else R itself under its
    own box; second half: two empty entries; a leaf root: four empty entries"""
    insts, wide = a["insts"], a["wide"]
    assert len(e) == s["nInst"]
    for i in range(len(e)):
        h0, h1 = e["half"][i]
        for h in (h1,) + ((h0,) if insts["rootDesc1"][i] & LEAF else ()):
            assert h["ld1"] == LEAF and h["rd1"] == LEAF and h["ld0"] == 0 and h["rd0"] == 0
            assert not np.any(h["lmin"]) and not np.any(h["lmax"]) and not np.any(h["rmin"]) and not np.any(h["rmax"])
        if insts["rootDesc1"][i] & LEAF:
            continue
        R = int(insts["rootDesc0"][i])
        w = wide[R]
        rmin, rmax = insts["rootMin"][i][:3], insts["rootMax"][i][:3]
        union = (np.array_equal(np.minimum(w["lmin"], w["rmin"]), rmin) and np.array_equal(np.maximum(w["lmax"], w["rmax"]), rmax))
        assert union == union_expected
        entries = [(h0["lmin"], h0["lmax"], int(h0["ld0"]), int(h0["ld1"])), (h0["rmin"], h0["rmax"], int(h0["rd0"]), int(h0["rd1"]))]
        if not union:
            (mn, mx, d0, d1), (_, _, e0, e1) = entries
            assert d1 == 0 and d0 == R and np.array_equal(mn, rmin) and np.array_equal(mx, rmax) and e1 == LEAF and e0 == 0
            continue
        kids = []
        for mn, mx, d0, d1 in ((w["lmin"], w["lmax"], int(w["ld0"]), int(w["ld1"])), (w["rmin"], w["rmax"], int(w["rd0"]), int(w["rd1"]))):
            if d1 & LEAF:        # a leaf child carries R's box (csrc/rdx_types.h, DQuad)
                kids.append((rmin.tobytes(), rmax.tobytes(), d0 & 0x1ffffff, LEAF | (((d1 >> 24) & 0x7f) << 24) | PAIR))
            else:
                kids.append((mn.tobytes(), mx.tobytes(), d0, PAIR))
        assert sorted((mn.tobytes(), mx.tobytes(), d0, d1) for mn, mx, d0, d1 in entries) == sorted(kids), i


@pytest.mark.parametrize("case", ALL + ("leaf_root",))
def test_record_form(layouts, case):
    _, s, a, e, _ = layouts(case)
    check_forms(s, a, e, case != "non_union")


def test_no_quad_records_no_entries(mods):
    rd, scenes = mods
    blob = alc.blob("group_rotated")
    for quad, cull in ((0, 0), (1, 1)):
        e, need = rd.DebugAccelEntries(blob, quad, cull)
        assert len(e) == 0 and need == 0
    e, need = rd.DebugAccelEntries(alc.blob("atrium_400"))       # unified tree: no quad records either
    assert len(e) == 0 and need == 0


@pytest.mark.parametrize("case", ["c2_small", "group_rotated", "leaf_root", "shared_blas"])
def test_entries_follow_their_instances_through_updates(mods, case):
    """after every update of tests/tlas_update_cases.py -- which re-orders the instance slots and moves members out of the group;
    the BLAS blocks stay where the first derivation put them -- the record of every slot is the one of the BLAS that the slot's
    instance record names, in the arrays as updated, and the need is a fresh derivation's"""
    rd, scenes = mods
    s = alc.scene(case)
    blases = [rd.BuildAccelStruct(None, rd.Mesh(m[0], m[1])) for m in s.meshes]
    orig = tu.instances(s)
    chain = [tu.product_blob(rd, orig, blases)]
    seen = set()
    for _, insts, _ in tu.stepped(orig):
        chain.append(tu.product_blob(rd, insts, blases))
        got, need = rd.DebugAccelEntries(chain)
        s_, a_, paths = rd.DebugAccelLayoutUpdate(chain)
        seen.update(paths)
        check_forms(s_, a_, got)
        assert need == rd.DebugAccelEntries(chain[-1])[1]
    assert 1 in seen            # (some step was incremental)
