"""GPU suite, part 5 (-m gpu): every walk and the GPU binning pass on HOSTILE GEOMETRY (tests/mesh_edge_cases.py).

Comparand: tests/golden/refgpu_meshedges.npz -- the answers of the reference's own `intersectTop` (oracle/_ref, build p, run on
an MI355X by tests/golden/make_golden_gpu.py meshedges) for the rays of every case at the stock interval and at (0, FLT_MAX) --
and, when the code object is present, the live reference launched next to the product.  Bar, as in test_gpu_ray_edges.py
(whose Ctx-style context, check_cell, mismatches and option matrices are used here by import): fixture == live reference ==
reference-order kernel == every configuration of FULL (kernel 3 / 2 / 1 x cull x quad x group_instances; instanced cases:
FULL_INST); closest hit: hit flags everywhere and every HitData field bit for bit where the reference hit; any hit: the flag.
A NaN of the reference wants a NaN.  Nothing is filtered out of a batch.

Why hostile trees may run on persistent kernels (the argument test_gpu_ray_edges.py gives for rays, restated for geometry after
reading kernels.hip traverse / traverse_wide, traverse_coop.h and traverse_pool.h):
  * node, leaf, triangle-run and instance indices come from the structure only.  accel_layout.cpp refuses a blob whose child,
    leaf, instance, BLAS or vertex indices are out of range or not in DFS pre-order, before anything is uploaded; the derived
    records (wide, quad, entry records, the flat top level's child words) are written from those indices, never from a float.
  * a box's or a triangle's floats decide only WHICH children are entered and which candidates are accepted: slab and
    Moeller-Trumbore tests are comparisons, false on NaN; a band test that cannot decide (NaN, inf - inf) falls to the
    reference's own division form, whose answer the reference gives too.  The culled walk's gate (kernels.hip cull_gate) reads a
    cone the HOST packed into bytes -- from NaN edges too: the packing runs under UBSan in test_mesh_edges_cpu.py -- and yields
    two numbers, `safe` and a margin, that feed comparisons only.  quad_half (traverse_pool.h) turns four slab answers into up
    to four pushes of descriptors the record holds; a NaN box changes the answers, not the descriptors.  The flat top level's
    reach bits are indexed by node numbers below 64 (topFlat is 0 otherwise), set from child words of the record.
  * every loop is counted by the structure.  The per-lane walks (kernel 1, and the reference-order kernel) pop a stack that a
    visited node pushes to a bounded number of times (sized by stackNeed, which test_mesh_edges_cpu.py holds to walkers of its
    own, leaf pieces included); leaf pieces count a triangle count down.  The pool engine (kernel 3) drains integer-counted
    queues and carries an iteration bound, POOL_MAX_ITER, that the host reports as "a traversal wave exceeded its iteration
    bound" -- an error return and a finding, not something to retry.
  * the cooperative engine (kernel 2, traverse_coop.h) has NO such bound in the shipped build: COOP_MAX_ITER sits under
    COOP_WATCHDOG, which is 0, and would raise no status word anyway.  Its termination is structural.  A lane's state is a work
    item, a stack of work items, and integers (qHead, qTail, finMark, markPrev, pend[], the ray reservation).  Floats enter in
    four places only: the slab answers of the top, instance and node steps (which of the record's children become work items),
    coop_inst_pretest (which bits of a leaf's instance mask are set), the triangle test (whether a key goes to best[]), and
    "an any-hit ray with a key drops its remaining work" -- each can only REMOVE work items, never add or repeat one.  Every
    round of the loop with a work item anywhere runs one of: the leaf step (every lane with a leaf item pops it), the top step,
    the instance step, the node step -- the three weighted conditions cannot all fail while one of nTop, nInst, nNode is
    non-zero -- and each of them replaces the item of at least one lane by items lower in the tree or pops it; the instance
    step's only wait, `ready` (qHead has passed markPrev), is answered by a test step, which consumes at least one queue entry
    (markPrev <= qTail).  A steal moves an item between lanes and counts it in pend[], an integer.  With no work item left, a
    non-empty queue is drained by test steps, `done` is an integer comparison that then holds, helpers give pend[] back, owners
    finish, and the ray counter -- read against n only -- runs out.  So the number of rounds is bounded by (items of the tree
    + queued triangles + rays) whatever the boxes hold, NaN included.
  So each walk ends after at most (nodes + triangles) steps per ray, as the reference's does.  What the argument does NOT give is
  equal ANSWERS on a tree whose boxes do not enclose their children (a NaN dropped by a later min / max): that is what the
  parity below measures.

Mutations (local builds, never committed), each applied alone, and what fails under it:
  * the partition's `<` made `<=` (bvh_build.cpp): test_builder_fuzz_nine_kinds_of_hostile_soups, and dense_planes_400 in
    test_builder_blobs_where_the_strict_comparisons_decide.  None of the 52 recorded cases, plane_depth0 and plane_deeper
    included: the winning plane is the first one BEHIND a group of centroids, so it carries a centroid only where two
    neighbouring planes both do; dense_planes_400 has several centroids on every plane of the middle.
  * the axis skip at 1e-3 instead of 1e-4: thin_above_skip in the same test (a stack that only z can split: 31 nodes at an
    extent of 1.01e-4, one leaf under the mutation), and nothing else -- in extent_above_skip the SAH never chooses the thin axis.
  * cneed's swap dropped while the need keeps its formula max(1 + smaller, larger) (accel_layout.cpp):
    test_stack_needs_cover_a_walk_of_the_tests_own fails on 12 cases (blasNeed below the walk in the STORED order): nan_300,
    nan_two_axes, plane_depth0, plane_deeper, zero_mixed_40, extent_above_skip, degen_clusters_7x40 and five more.
  * `bvh_key` without its sign handling in k_bvh_bin (`b ^ 0x80000000`): test_gpu_binner_on_hostile_meshes fails on the finite
    classes flat_y_300, plane_depth0, plane_deeper, duplicates_300, zero_mixed_300 and deep_soup_leaf127 (and on the finite
    subtrees of nan_300): their GPU-assisted blob differs from the oracle's.  fltmax_300 (its root finds no split) and
    deep_left_255 (no negative coordinate) stay equal.
  * trav_threads allocating need - 1 entries: NOT run, and no test of the suite would fail under it.  No CPU test sees the
    launch's allocation, and on the GPU no case fills its per-lane stack to the last entry: stackNeed keeps a flat allowance for
    leaf pieces on top of the pieces the recurrence counts, so by the CPU walkers' count every case stays at least 2 entries
    below it (deep_left_120: reference-order walk 21 -- the kernels follow the left child without pushing it, one entry fewer
    still --, stackNeed 23).

Found by the CPU walkers: the per-lane wide kernel and the cooperative kernel keep the 8-triangle pieces of an oversized leaf on
the lane's stack while the record's other child is walked, so the pieces of every oversized leaf along a path are there
together, while stackNeed / coopNeed allowed for one such leaf: degen_clusters_7x40 needs 14 cooperative entries where 11 were
allowed, degen_clusters_5x120 47 where 33 were.  accel_layout.cpp carries the pieces through the recurrence; scenes without
leaves above 8 triangles keep their numbers."""
import ctypes
import os
import types

import numpy as np
import pytest

import golden_cases as gc
import mesh_edge_cases as mec
import oracle_bind as ob
import refgpu_bind as rg
from test_gpu_ray_edges import FULL, FULL_INST, SMALL, check_cell

pytestmark = pytest.mark.gpu
PLAIN = [n for n in mec.NAMES if not mec.case(n).instanced]
INSTANCED = [n for n in mec.NAMES if mec.case(n).instanced]


@pytest.fixture(scope="module")
def mods(gpu):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd
    return rd, gpu


@pytest.fixture(scope="module")
def ref(gpu):
    return rg.RefGpu("p") if rg.available("p") else None


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(mec.GOLD, "refgpu_meshedges.npz"))


class Ctx:
    """one case on the device + its cells and the reference's answers (the members check_cell reads)"""

    def __init__(self, rd, plt, G, ref, name):
        c = mec.case(name)
        self.rd, self.name = rd, name
        self.blas = [rd.BuildAccelStruct(plt, rd.Mesh(v, t)) for v, t in c.meshes]
        tlas = rd.BuildAccelStruct(plt, [rd.Instance(tf, 0, k, self.blas[mi]) for k, (mi, tf) in enumerate(c.instances)])
        self.dev = types.SimpleNamespace(topAccelStruct=tlas, plt=plt)
        blob = rd.ReadBuffer(plt, tlas, tlas.size).tobytes()
        assert np.array_equal(gc.sha(blob), G[name + "/blob_sha256"]), "the TLAS blob of %s changed" % name
        self.cells, self.want = mec.reference_answers(G, c, ob.HIT_DTYPE)
        self.ref, self.tl = ref, (rg.DevBuf.of(np.frombuffer(blob, np.uint8)) if ref is not None else None)


def run_case(rd, plt, G, ref, name, configs):
    c = Ctx(rd, plt, G, ref, name)
    rays = 0
    for cell, (w1, w2) in zip(c.cells, c.want):
        rays += check_cell(c, cell, w1, w2, configs)
        if name in mec.RAGGED_CASES:
            for n in mec.RAGGED:
                check_cell(c, cell, w1, w2, SMALL, n)
    return rays


@pytest.mark.parametrize("name", PLAIN)
def test_every_walk_matches_the_reference_on_hostile_meshes(mods, fixture, ref, name):
    rd, plt = mods
    assert run_case(rd, plt, fixture, ref, name, FULL) == 2 * mec.N_RAYS


@pytest.mark.parametrize("name", INSTANCED)
def test_every_walk_matches_the_reference_on_hostile_instances(mods, fixture, ref, name):
    """hostile meshes under the identity, a mirrored transform and one shared transform (a transform group); instance matrices
    with a NaN and with an infinite entry: also x unified_tree x top_flat x inline_leaf_roots"""
    rd, plt = mods
    assert run_case(rd, plt, fixture, ref, name, FULL_INST) == 2 * mec.N_RAYS


def test_gpu_binner_on_hostile_meshes(mods):
    """The binning pass of large nodes on the device (k_bvh_bin: atomic min / max on order-preserving integer keys) with the
    threshold at 64 primitives, on hostile meshes of 200 to 600 triangles: the blob equals the host path's and the oracle's byte
    for byte, one mesh at a time and through BuildAccelStructs (builder threads share the device).  On the FINITE classes (flat,
    centroids on candidate planes, duplicated centroids, mixed zeros, a FLT_MAX coordinate, a lopsided deep tree, an
    unsplittable set of 127) the device must have been asked: rdx_debug_gpu_bin_calls rises for each.  A node that holds a
    primitive with a NaN or infinite box or centroid is never sent there (its candidates are evaluated in the reference's
    literal order on the host); the finite subtrees below it are."""
    rd, plt = mods
    from radiance_ray_tracing_amd import _lib
    calls = _lib.lib().rdx_debug_gpu_bin_calls
    calls.restype = ctypes.c_ulonglong
    meshes = mec.binner_meshes()
    want = [ob.OracleBlas(v, t).blob for _, _, (v, t) in meshes]
    try:
        rd.SetOption("gpu_build", 0)
        host = [rd.BuildAccelStruct(plt, rd.Mesh(v, t)).data for _, _, (v, t) in meshes]
        rd.SetOption("gpu_build", 1); rd.SetOption("gpu_build_min", 64)
        dev, rose = [], []
        for _, _, (v, t) in meshes:
            before = calls()
            dev.append(rd.BuildAccelStruct(plt, rd.Mesh(v, t)).data)
            rose.append(calls() - before)
        many = [b.data for b in rd.BuildAccelStructs(plt, [rd.Mesh(v, t) for _, _, (v, t) in meshes])]
    finally:
        rd.SetOption("gpu_build", 1); rd.SetOption("gpu_build_min", 32768)
    for (name, finite, (v, t)), o, h, d, m, r in zip(meshes, want, host, dev, many, rose):
        assert bytes(h) == o, "%s (%d triangles): the host build differs from the oracle's" % (name, t.shape[0])
        assert bytes(d) == o, "%s (%d triangles): the GPU-assisted build differs" % (name, t.shape[0])
        assert bytes(m) == o, "%s (%d triangles): the GPU-assisted build on builder threads differs" % (name, t.shape[0])
        if finite:
            assert r >= 1, "%s: the device did not bin a node (%d calls)" % (name, r)
