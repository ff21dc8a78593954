"""update_accel_layout (csrc/accel_layout.cpp) on the host, through rdx_debug_accel_layout_update: the layout a TLAS update
leaves behind, against the layout derived afresh from the same blob (rdx_debug_accel_layout: existing code, pinned by
tests/golden/accel_layout.json).  Scenes and moves: tests/tlas_update_cases.py; every check under all of
accel_layout_cases.SETTINGS.

An update keeps the per-BLAS blocks of bnodes / tris / wide / quad where they are, a fresh derivation orders them by instance slot.
So: where the slot order is unchanged everything is byte-identical to fresh; always, everything that does not name a block
position is; and a walk that ends where it began ends byte-identical to the fresh layout it began with.
"""
import numpy as np
import pytest

import accel_layout_cases as alc
import tlas_update_cases as tu

SMALL = ("tnodes", "ctnodes", "groupBits")


@pytest.fixture(scope="module")
def rd(built):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd
    return rd


class Case:
    def __init__(self, rd, name):
        self.rd, self.name = rd, name
        s = alc.scene(name)
        self.blases = [rd.BuildAccelStruct(None, rd.Mesh(m[0], m[1])) for m in s.meshes]
        self.insts = tu.instances(s)
        self.n = len(self.insts)
        self._blob, self._fresh = {}, {}

    def blob(self, key):
        """key: "orig", a move applied to the scene as built, or a tuple of steps (tu.stepped): the blob after the last one"""
        if key not in self._blob:
            if key == "orig":
                insts = self.insts
            elif isinstance(key, tuple):
                insts = tu.stepped(self.insts, key)[-1][1]
            else:
                insts = tu.apply(self.insts, key)
            self._blob[key] = tu.product_blob(self.rd, insts, self.blases)
        return self._blob[key]

    def fresh(self, key, quad, cull):
        k = (key, quad, cull)
        if k not in self._fresh:
            self._fresh[k] = self.rd.DebugAccelLayout(self.blob(key), quad, cull)
        return self._fresh[k]


@pytest.fixture(scope="module")
def case(rd):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Case(rd, name)
        return cache[name]
    return get


def _same(got, want, names=None):
    (gs, ga), (ws, wa) = got, want
    assert gs == ws, {k: (gs[k], ws[k]) for k in gs if gs[k] != ws[k]}
    for name in (names or [n for n, _ in ga.items()]):
        assert ga[name].shape == wa[name].shape, (name, ga[name].shape, wa[name].shape)
        if ga[name].tobytes() != wa[name].tobytes():
            bad = np.flatnonzero((ga[name].view(np.uint8).reshape(ga[name].shape[0], -1) != wa[name].view(np.uint8).reshape(wa[name].shape[0], -1)).any(1))
            raise AssertionError("%s: %d of %d records differ, first %d" % (name, bad.shape[0], ga[name].shape[0], int(bad[0])))


# ---- preconditions, from the blobs alone ------------------------------------------------------------------------------------------
def test_the_moves_do_what_the_cases_are_for(case):
    c2 = case("c2_small")
    off = {k: tu.inst_byte_offset(c2.blob(k)) for k in ("orig", "A", "B", "C")}
    assert off == {"orig": 640, "A": 640, "B": 448, "C": 544}, off
    assert tu.top_nodes(c2.blob("orig")) == 13 and tu.top_nodes(c2.blob("B")) == 9
    for k in ("A", "B", "C"):      # the BLAS region only shifts
        assert tu.blas_region(c2.blob(k), c2.n) == tu.blas_region(c2.blob("orig"), c2.n)
    at = case("atrium_400")
    assert tu.inst_byte_offset(at.blob("A")) == tu.inst_byte_offset(at.blob("orig"))
    assert at.fresh("orig", 1, 0)[0]["unifiedRoot"] > 0 and at.fresh("A", 1, 0)[0]["unifiedRoot"] == 0
    sb = case("shared_blas")
    for k in ("A", "B", "C"):
        assert tu.slot_sequence(sb.blob(k), sb.n) == tu.slot_sequence(sb.blob("orig"), sb.n)
    # somewhere the slot order does change: the block order of a fresh derivation then differs from the updated layout's
    assert any(tu.slot_sequence(case(n).blob(k), case(n).n) != tu.slot_sequence(case(n).blob("orig"), case(n).n)
               for n in ("c2_small", "c1_small") for k in ("B", "C"))
    so = case("sbt_offset")
    assert so.fresh("orig", 1, 0)[0]["sbtOffsets"] == 1 and so.fresh("S", 1, 0)[0]["sbtOffsets"] == 0


# ---- 1: same slot order -> everything identical -----------------------------------------------------------------------------------
@pytest.mark.parametrize("quad,cull", alc.SETTINGS)
@pytest.mark.parametrize("name", tu.SCENES)
def test_same_slot_order_is_byte_identical_to_fresh(rd, case, name, quad, cull):
    c = case(name)
    seq0 = tu.slot_sequence(c.blob("orig"), c.n)
    checked = 0
    for mv in tu.moves_of(name):
        if tu.slot_sequence(c.blob(mv), c.n) != seq0:
            continue
        s, a, paths = rd.DebugAccelLayoutUpdate([c.blob("orig"), c.blob(mv)], quad, cull)
        _same((s, a), c.fresh(mv, quad, cull))
        checked += 1
    if name == "shared_blas":
        assert checked == 3


# ---- 2: every step ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quad,cull", alc.SETTINGS)
@pytest.mark.parametrize("name", tu.SCENES)
def test_every_step_matches_fresh_outside_block_positions(rd, case, name, quad, cull):
    c = case(name)
    for mv in tu.moves_of(name):
        s, a, paths = rd.DebugAccelLayoutUpdate([c.blob("orig"), c.blob(mv)], quad, cull)
        ws, wa = c.fresh(mv, quad, cull)
        _same((s, a), (ws, wa), SMALL)
        for k in a:
            assert a[k].nbytes == wa[k].nbytes, (mv, k)
        # DInst bytes 140..155 are blasRoot, rootDesc0 / 1 and _p0: positions of the BLAS's blocks
        gi = a["insts"].view(np.uint8).reshape(c.n, 224).copy()
        wi = wa["insts"].view(np.uint8).reshape(c.n, 224).copy()
        gi[:, 140:156] = 0
        wi[:, 140:156] = 0
        assert np.array_equal(gi, wi), (mv, np.flatnonzero((gi != wi).any(1))[:8])
        # ... and what they name is the same BLAS: equal root boxes and triangle counts are in the compared bytes; the owner
        # words of the triangles each instance points at are this instance's slot or "none", as in the fresh layout
        for k in range(c.n):
            g0, w0 = int(a["insts"]["_p0"][k]), int(wa["insts"]["_p0"][k])
            assert int(a["tris"]["_p0"][g0]) == int(wa["tris"]["_p0"][w0]), (mv, k)
            assert int(a["tris"]["_p1"][g0]) == g0


# ---- 3: round trips ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quad,cull", alc.SETTINGS)
@pytest.mark.parametrize("name", tu.SCENES)
def test_round_trips_end_byte_identical_to_where_they_began(rd, case, name, quad, cull):
    c = case(name)
    want = c.fresh("orig", quad, cull)
    for mv in tu.moves_of(name):
        s, a, _ = rd.DebugAccelLayoutUpdate([c.blob("orig"), c.blob(mv), c.blob("orig")], quad, cull)
        _same((s, a), want)
    chain = [c.blob("orig")] + [c.blob(tu.STEPS[:i + 1]) for i in range(len(tu.STEPS))]
    assert chain[-1] == chain[0]
    s, a, _ = rd.DebugAccelLayoutUpdate(chain, quad, cull)
    _same((s, a), want)


# ---- 4: which steps are incremental -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quad,cull", alc.SETTINGS)
def test_step_paths(rd, case, quad, cull):
    c2, sb, at = case("c2_small"), case("shared_blas"), case("atrium_400")
    assert rd.DebugAccelLayoutUpdate([c2.blob("orig"), c2.blob("A")], quad, cull)[2] == [1]
    for mv in tu.MOVES:
        assert rd.DebugAccelLayoutUpdate([sb.blob("orig"), sb.blob(mv)], quad, cull)[2] == [1], mv
    # the unified tree vanishes and comes back: handed to the full derivation (an incremental answer would be as good)
    paths = rd.DebugAccelLayoutUpdate([at.blob("orig"), at.blob("A"), at.blob("orig")], quad, cull)[2]
    assert set(paths) <= {1, 2}
    # another custom id keeps the unified tree (every matrix is still the identity): incremental, and identical to fresh
    assert at.fresh("K", quad, cull)[0]["unifiedRoot"] > 0
    s, a, paths = rd.DebugAccelLayoutUpdate([at.blob("orig"), at.blob("K")], quad, cull)
    assert paths == [1]
    _same((s, a), at.fresh("K", quad, cull))
    assert a["insts"].tobytes() != at.fresh("orig", quad, cull)[1]["insts"].tobytes()


def test_another_scene_is_derived_in_full(rd, case):
    """a blob whose BLAS region is not the previous one's is no update: the seam derives it afresh and says so"""
    a, b = case("c2_small"), case("shared_blas")
    s, arr, paths = rd.DebugAccelLayoutUpdate([a.blob("orig"), b.blob("orig")], 1, 0)
    assert paths == [2]
    _same((s, arr), b.fresh("orig", 1, 0))


def test_single_blob_is_the_fresh_layout(rd, case):
    c = case("group_rotated")
    s, arr, paths = rd.DebugAccelLayoutUpdate([c.blob("orig")], 1, 0)
    assert paths == []
    _same((s, arr), c.fresh("orig", 1, 0))
    with pytest.raises(rd.RadianceError, match="does not hold a top-level acceleration structure"):
        rd.DebugAccelLayoutUpdate([c.blob("orig"), b"\0" * 64], 1, 0)


def test_update_needs_an_initialised_library(rd):
    """nothing here has created a Platform: rdx_tlas_update refuses before it looks at its arguments"""
    with pytest.raises(rd.RadianceError, match="rdx_init has not been called"):
        rd.UpdateAccelStruct(None, rd.Buffer(None, 0), [])
    st = rd.GetTlasUpdateStats()
    assert st.path == 0 and st.bytes_h2d == 0
