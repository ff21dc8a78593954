"""CPU suite: the oracle against the REFERENCE's own intersectTop beyond the stock ray interval and unit directions.

tests/golden/refgpu_rayedges.npz holds what the reference's device code (oracle/_ref/ref_shader_gfx950_p.co, run on an MI355X by
tests/golden/make_golden_gpu.py rayedges) answers for every cell of tests/ray_edge_cases.py: 13 ray intervals (zero, negative,
empty, infinite and NaN bounds among them), directions scaled over 50 orders of magnitude, tmin / tmax one float32 step either
side of an exact hit distance, tmin behind the nearest surface, far origins, and degenerate rays (zero, NaN, infinite and
denormal components).  `ob.trace_batch` must reproduce all of it: hit flags everywhere, every HitData field bit for bit where the
reference hit, any-hit flags.  This pins the oracle's Tmin / Tmax, tie and degenerate-ray behaviour to the real reference.

The second half asserts the CONDITIONS ON THE INPUTS, evaluated on the reference's answers only: they keep a family from being
vacuous (a tie family in which no ray ties, a second-surface family in which no ray has a second surface)."""
import os

import numpy as np
import pytest

import golden_cases as gc
import oracle_bind as ob
import ray_edge_cases as rec

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("distance", "primitiveIndex", "instanceIndex", "instanceCustomIndex", "instanceSBTOffset", "barycentric",
          "hitPoint", "transform")


@pytest.fixture(scope="module")
def mods():
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd, scenes
    return rd, scenes


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLD, "refgpu_rayedges.npz"))


def load_cells(scenes, G, name):
    """(cells, [(reference closest-hit records, reference any-hit flags)]) of one scene, inputs rebuilt from the seed + fixture"""
    base = None
    if name in rec.GOLDEN:
        g = np.load(os.path.join(GOLD, "refgpu_%s.npz" % name))
        base = (g["ray_o"], g["ray_d"])
    cells = rec.Cases(scenes, name, base, rec.load_params(G, name), None).cells()
    return cells, rec.unpack_scene(G, name, cells, ob.HIT_DTYPE)


assert set(FIELDS) | {"hit"} == set(ob.HIT_DTYPE.names)       # FIELDS + the flag are the whole record: compared as bytes below


def mismatches(want, got, closest=True):
    """per ray: hit flags differ, or (closest hit, where the reference hit) any byte of the HitData record differs"""
    bad = want["hit"] != got["hit"]
    if closest:
        h = np.flatnonzero((want["hit"] == 1) & ~bad)
        w = np.ascontiguousarray(want).view(np.uint8).reshape(-1, ob.HIT_DTYPE.itemsize)
        g = np.ascontiguousarray(got).view(np.uint8).reshape(-1, ob.HIT_DTYPE.itemsize)
        bad[h] = (w[h] != g[h]).any(1)
    return bad


def describe(cell, want, got, bad, what):
    i = int(np.flatnonzero(bad)[0])
    return ("%s, %s: %d of %d rays differ; first: ray %d o=%r d=%r tmin=%r tmax=%r want t=%r prim=%d inst=%d hit=%d, got t=%r prim=%d inst=%d hit=%d"
            % (cell.key, what, int(bad.sum()), cell.n, i, cell.o[i].tolist(), cell.d[i].tolist(), cell.tmin, cell.tmax,
               float(want["distance"][i]), int(want["primitiveIndex"][i]), int(want["instanceIndex"][i]), int(want["hit"][i]),
               float(got["distance"][i]), int(got["primitiveIndex"][i]), int(got["instanceIndex"][i]), int(got["hit"][i])))


@pytest.mark.parametrize("name", rec.SCENES)
def test_oracle_matches_the_reference_on_every_cell(mods, fixture, name):
    rd, scenes = mods
    blob = gc.scene_blob(rd, rec.scene(scenes, name))
    assert np.array_equal(gc.sha(blob), fixture[name + "/blob_sha256"])
    cells, want = load_cells(scenes, fixture, name)
    assert len(cells) >= 17
    for c, (w1, w2) in zip(cells, want):
        got = ob.trace_batch(blob, c.o, c.d, c.tmin, c.tmax, 1)
        bad = mismatches(w1, got)
        assert not bad.any(), describe(c, w1, got, bad, "closest hit")
        got2 = ob.trace_batch(blob, c.o, c.d, c.tmin, c.tmax, 2)
        bad = w2 != got2["hit"]
        assert not bad.any(), "%s, any hit: %d of %d flags differ, first at ray %d" % (c.key, int(bad.sum()), c.n, int(np.flatnonzero(bad)[0]))


def test_fixture_lists_no_ray_the_reference_could_not_run(fixture):
    # (at most 1/8 of family F may be listed; the reference's walk terminates on all of them, so none is)
    assert fixture["notes"].shape[0] <= len(rec.DEGENERATE_KINDS) // 8
    assert len(rec.DEGENERATE_KINDS) <= 256


# ---------------------------------------------------------------------------------------------------------------------
# conditions on the inputs (reference answers only)
# ---------------------------------------------------------------------------------------------------------------------
def _by_key(cells, want):
    return {c.key: (c, w1, w2) for c, (w1, w2) in zip(cells, want)}


def _answer_differs(a, b):
    return (a["hit"] != b["hit"]) | ((a["hit"] == 1) & ((a["instanceIndex"] != b["instanceIndex"]) | (a["primitiveIndex"] != b["primitiveIndex"])))


@pytest.mark.parametrize("name", [n for n in rec.SCENES if n != "planes"])
def test_family_a_every_interval_changes_answers(mods, fixture, name):
    """per scene and non-stock interval: >= 64 rays whose reference answer differs from the stock-interval answer"""
    K = _by_key(*load_cells(mods[1], fixture, name))
    stock = K["%s/A/stock" % name][1]
    for nm, _, _ in rec.INTERVALS[1:]:
        n = int(_answer_differs(stock, K["%s/A/%s" % (name, nm)][1]).sum())
        assert n >= 64, (name, nm, n)


@pytest.mark.parametrize("name", ["c0", "c1", "planes"])
def test_family_c_boundary_is_straddled(mods, fixture, name):
    """for at least one adjacent pair of k the reference's hit flags differ on >= 64 rays, in each tie batch"""
    K = _by_key(*load_cells(mods[1], fixture, name))
    for tag in ("y", "xz"):
        best = 0
        for end in ("tmax", "tmin"):
            for k in range(-2, 2):
                a, b = K["%s/C/%s_%s%+d" % (name, tag, end, k)][1], K["%s/C/%s_%s%+d" % (name, tag, end, k + 1)][1]
                best = max(best, int((a["hit"] != b["hit"]).sum()))
        assert best >= 64, (name, tag, best)
        # ... and as tmin the same step moves rays to ANOTHER primitive (strict `>`): the answers differ, the flags need not
        a, b = K["%s/C/%s_tmin-1" % (name, tag)][1], K["%s/C/%s_tmin+0" % (name, tag)][1]
        assert int(_answer_differs(a, b).sum()) >= 64, (name, tag)


def test_family_d_rays_report_a_later_surface(mods, fixture):
    """per scene >= 24 rays, over the three golden scenes >= 400, that hit under the stock interval and hit a different
    (instance, primitive) under tmin = median t1"""
    total = 0
    for name in rec.SCENES:
        if name == "planes":
            continue
        cells, want = load_cells(mods[1], fixture, name)
        K = _by_key(cells, want)
        c, w, _ = K["%s/D/tmin_median" % name]
        t1 = rec.load_params(fixture, name)["stock_t"]
        # t1: the reference's stock-interval distance of the same rays (-1: miss).  A hit now at another distance is a hit of
        # another (instance, primitive): the same pair would give the same t.  (A lower bound: equal t on another primitive not counted.)
        n = int(((t1 >= 0) & (w["hit"] == 1) & (w["distance"] != t1)).sum())
        st = rec.N_GOLDEN // rec.N_A.get(name, 1024)
        assert np.array_equal(K["%s/A/stock" % name][1]["distance"][t1[::st] >= 0], t1[::st][t1[::st] >= 0])
        assert n >= 24, (name, n)
        if name in rec.GOLDEN:
            total += n
    assert total >= 400, total


@pytest.mark.parametrize("name", [n for n in rec.SCENES if n not in ("planes", "edges_inst_id")])
def test_family_b_hit_rates(mods, fixture, name):
    cells, want = load_cells(mods[1], fixture, name)
    seen = 0
    for c, (w1, _) in zip(cells, want):
        if c.family == "B":
            r = float((w1["hit"] == 1).mean())
            assert 0.05 <= r <= 0.95, (c.key, r)
            seen += 1
    assert seen == 2 * (len(rec.SCALES) + 1)


@pytest.mark.parametrize("name", rec.GOLDEN)
def test_family_e_hit_rates(mods, fixture, name):
    cells, want = load_cells(mods[1], fixture, name)
    misses = 0
    for c, (w1, _) in zip(cells, want):
        if c.family == "E":
            r = float((w1["hit"] == 1).mean())
            assert r >= 0.25, (c.key, r)
            misses += int((w1["hit"] == 0).sum())
    assert misses >= 64, (name, misses)


@pytest.mark.parametrize("name", ["edges_inst", "edges_inst_id"])
def test_edges_inst_rays_reach_every_group_member(mods, fixture, name):
    """the reference reports at least 64 closest hits on each of the three instances under the shared transform, on the mirrored
    and on the non-uniformly scaled instance (families A and D): a wrong instance slot or object-space ray there cannot hide"""
    cells, want = load_cells(mods[1], fixture, name)
    inst = np.concatenate([w1["instanceIndex"][w1["hit"] == 1] for c, (w1, _) in zip(cells, want) if c.family in "AD"])
    for k in rec.GROUP_MEMBERS + (0, 1):
        assert int((inst == k).sum()) >= 64, (name, k, int((inst == k).sum()))


def test_edges_inst_holds_what_it_is_for(mods):
    """non-uniform scale, a mirrored instance, three single-user BLASes under one bit-identical transform (identity in the second
    variant), a top level small enough for the flat step.  (That the product forms a transform group of these three is shown on the
    GPU: tests/test_gpu_ray_edges.py module docstring, mutation 5.)"""
    rd, scenes = mods
    for ident in (False, True):
        s = rec.edges_inst(scenes, ident)
        tfs = [np.asarray(tf, np.float64) for _, tf, _ in s.instances]
        dets = [np.linalg.det(t[:3, :3]) for t in tfs]
        assert min(dets) < 0 and len(s.instances) <= 32
        sv = np.linalg.svd(tfs[0][:3, :3], compute_uv=False)
        assert sv[0] / sv[2] > 2
        g = [s.instances[k] for k in rec.GROUP_MEMBERS]
        assert len({mi for mi, _, _ in g}) == 3
        assert all(np.asarray(tf, np.float32).tobytes() == np.asarray(g[0][1], np.float32).tobytes() for _, tf, _ in g)
        assert np.array_equal(g[0][1], np.eye(4, dtype=np.float32)) == ident
        users = [sum(1 for mi, _, _ in s.instances if mi == m) for m, _, _ in g]
        assert users == [1, 1, 1]
        assert all(s.meshes[mi][1].shape[0] > 16 for mi, _, _ in g)         # inner-node roots
