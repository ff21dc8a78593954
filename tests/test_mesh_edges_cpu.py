"""CPU suite: the host builders, the layout derivation and the CPU oracle on HOSTILE GEOMETRY (tests/mesh_edge_cases.py): NaN,
infinite, overflowing and denormal coordinates, degenerate and identical triangles, flat meshes and extents either side of the
axis skip, centroids exactly on candidate planes, signed zeros, lopsided deep trees, hostile instances.

* builder blobs: for every case (and a seeded fuzz of 300 soups in nine kinds) the product's host builder gives the blob of the
  oracle's literal restatement of the reference's `Recurse` (oracle/rt_oracle.c) byte for byte, BLAS and TLAS, with equal
  max_depth.  Meshes on which the reference's split loop would not end are refused by the product ("split step underflows");
  the oracle abort()s on them, so they are asked of the product alone.
* sanitised host code: tests/mesh_edges_host.cpp + csrc/bvh_build.cpp + csrc/accel_layout.cpp, compiled with the host compiler and
  -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all, run as a program of its own on every case.
* layout: rd.DebugAccelLayout takes every blob; the structural invariants of test_accel_layout_cpu.py hold on the new cases.
* stack needs against a walk of this file's own over `tnodes` / `bnodes`, `ctnodes` and `wide` (see test_stack_needs...).
* coverage guards, counted from the blobs and the REFERENCE's answers (tests/golden/refgpu_meshedges.npz), see each docstring.
* the CPU oracle's trace_batch equals the reference's intersectTop (the fixture) bit for bit on the rays of every case.

quadNeed is not restated here: the quad record's rule (which grandchildren a half takes, eight arrangements, entry records)
does not fit a short restatement; it is held by the GPU parity of tests/test_gpu_mesh_edges.py, where an undersized pool is
reported as an error by the engine's iteration bound or shows as a wrong answer.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import accel_layout_cases as alc
import golden_cases as gc
import mesh_edge_cases as mec
import oracle_bind as ob
import test_accel_layout_cpu as tal
from test_ray_edges_cpu import describe, mismatches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = mec.GOLD
CSRC = os.path.join(ROOT, "radiance-ray-tracing_amd", "csrc")
LEAF = 0x80000000
SAN_FLAGS = ["-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def rd(built):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd
    return rd


@pytest.fixture(scope="module")
def built_cases(rd):
    """name -> (product, oracle), each (TLAS blob, [BLAS blobs], [BLAS max depths], TLAS max depth); built once, never changed"""
    with np.errstate(all="ignore"):
        return {c.name: (mec.product_blob(rd, c), mec.oracle_blob(ob, c)) for c in mec.all_cases()}


@pytest.fixture(scope="module")
def layouts(rd, built_cases):
    return {name: rd.DebugAccelLayout(b[0][0]) for name, b in built_cases.items()}


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLD, "refgpu_meshedges.npz"))


def reference_answers(G, c):
    return mec.reference_answers(G, c, ob.HIT_DTYPE)


# ---------------------------------------------------------------------------------------------------------------------
# builder blobs
# ---------------------------------------------------------------------------------------------------------------------
def _first_difference(a, b):
    if len(a) != len(b):
        return "lengths %d and %d" % (len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8))
    return "%d bytes differ, the first at %d (node %d if in the node array)" % (d.shape[0], int(d[0]), (int(d[0]) - 16) // 48)


@pytest.mark.parametrize("name", mec.NAMES)
def test_builder_blobs_equal_the_literal_restatement(built_cases, name):
    (blob_p, blas_p, depths_p, depth_p), (blob_o, blas_o, depths_o, depth_o) = built_cases[name]
    for k, (a, b) in enumerate(zip(blas_p, blas_o)):
        assert a == b, "%s, BLAS %d: %s" % (name, k, _first_difference(a, b))
    assert depths_p == depths_o
    assert blob_p == blob_o, "%s, TLAS: %s" % (name, _first_difference(blob_p, blob_o))
    assert depth_p == depth_o
    assert max(depths_p) <= 90          # the reference's bottom-level stack holds 100 entries: the comparand stays inside it
    assert len(mec.case(name).instances) <= 8       # ... and its top-level stack 8


def test_builder_blobs_where_the_strict_comparisons_decide(rd):
    """meshes made so that the builder's two thresholds decide the tree (mesh_edge_cases.builder_only_meshes): centroids ON the
    plane the root chooses (a partition with `<=` moves them to the other side), and a stack of triangles that only z can split,
    with a z extent of 1.01e-4 (split: 31 nodes) and of 9.9e-5 (axis skipped: one leaf of 16)"""
    nodes = {}
    for name, (v, t) in mec.builder_only_meshes():
        p, o = rd.BuildAccelStruct(None, rd.Mesh(v, t)), ob.OracleBlas(v, t)
        assert p.data == o.blob and p.max_depth == o.max_depth, "%s: %s" % (name, _first_difference(p.data, o.blob))
        h = np.frombuffer(o.blob[:16], np.uint32)
        nodes[name] = (int(h[2]) - int(h[1])) // 48
    assert nodes["thin_above_skip"] > 1 and nodes["thin_below_skip"] == 1, nodes


FUZZ_KINDS = ("nan", "inf", "ninf", "3e38", "tiny", "flat", "dupcentroid", "onplane", "zeros")


def fuzz_soup(kind, seed):
    rng = np.random.default_rng([seed, FUZZ_KINDS.index(kind)])
    n = int(rng.choice([8, 9, 12, 16, 24, 32, 48, 64, int(rng.integers(8, 601))]))
    v, t = mec.soup(int(rng.integers(1 << 30)), n)
    rows = lambda k: rng.integers(0, v.shape[0], k)
    if kind == "nan":
        for r in rows(int(rng.integers(1, 4))):
            v[r, rng.integers(3)] = np.nan
    elif kind in ("inf", "ninf"):
        v[rows(1)[0], rng.integers(3)] = np.inf if kind == "inf" else -np.inf
    elif kind == "3e38":
        for r in rows(2):
            v[r, rng.integers(3)] = rng.choice([3e38, -3e38])
    elif kind == "tiny":
        v = (v.astype(np.float64) * 10.0 ** float(rng.integers(-42, -3))).astype(np.float32)
    elif kind == "flat":
        v[:, rng.integers(3)] = np.float32(rng.choice([0.0, 0.5, -3.25]))
    elif kind == "dupcentroid":
        m = max(4, n // 4)
        v = np.tile(v.reshape(-1, 3, 3)[:m], (n // m + 1, 1, 1))[:n].reshape(-1, 3).copy()
    elif kind == "onplane":
        v, t = mec.on_planes(int(rng.integers(1 << 30)), max(n - 2, 6), depth_steps=bool(seed & 1))
    elif kind == "zeros":
        v, t = mec.signed_zeros(int(rng.integers(1 << 30)), n)
    return np.ascontiguousarray(v, np.float32), t


def test_builder_fuzz_nine_kinds_of_hostile_soups(rd):
    """300 seeded soups (8 to 600 triangles; NaN, +inf, -inf, +-3e38, tiny, flat, duplicated centroids, centroids on candidate
    planes, mixed zeros): product blob == oracle blob, equal max_depth.  A soup the product refuses as "split step underflows"
    is one the oracle would abort() on and is left out; at most a tenth may be (none of these 300 is: 300 compared)."""
    compared, differ = 0, []
    for seed in range(300):
        kind = FUZZ_KINDS[seed % len(FUZZ_KINDS)]
        v, t = fuzz_soup(kind, seed)
        try:
            p = rd.BuildAccelStruct(None, rd.Mesh(v, t))
        except rd.RadianceError as e:
            assert "split step underflows" in str(e), (kind, seed, str(e))
            continue
        o = ob.OracleBlas(v, t)
        compared += 1
        if p.data != o.blob or p.max_depth != o.max_depth:
            differ.append((kind, seed, t.shape[0]))
    assert not differ, "%d of %d soups differ: %r" % (len(differ), compared, differ[:12])
    assert compared >= 270


def test_product_refuses_a_mesh_the_reference_would_not_finish(rd):
    """coordinates near 1e8 (ulp 8) with an extent of about 80: the candidate step (80 / 1024) is below half an ulp,
    `testSplit += step` no longer moves and the reference's loop never ends.  The product says so
    (test_builder_rejects_bad_input has no such mesh)."""
    v, t = mec.soup(5, 16, spread=40.0, size=4.0)
    v = (v + np.float32(1e8)).astype(np.float32)
    with pytest.raises(rd.RadianceError, match="split step underflows"):
        rd.BuildAccelStruct(None, rd.Mesh(v, t))


# ---------------------------------------------------------------------------------------------------------------------
# sanitised host code, as a program of its own
# ---------------------------------------------------------------------------------------------------------------------
def _host_compiler():
    for cc in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cc and shutil.which(cc):
            return shutil.which(cc)
    return None


def test_host_builders_and_layout_under_sanitizers(tmp_path):
    """build_blas, build_tlas and derive_accel_layout under every (quad, cull) of accel_layout_cases.SETTINGS, on every case, in a
    stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer (float-cast-overflow included: converting a
    NaN bin estimate to an integer is what this catches).  Exit status 0 and one line per case and setting."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    empty = tmp_path / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    probe = subprocess.run([cxx, "-std=c++17"] + SAN_FLAGS + ["-o", str(tmp_path / "empty"), str(empty)], capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(tmp_path / "empty")], capture_output=True).returncode != 0:
        pytest.skip("the host compiler cannot link and start an empty program with %s: %s" % (" ".join(SAN_FLAGS), probe.stderr.strip()[-300:]))
    assert alc.SETTINGS == ((1, 0), (0, 0), (1, 1))          # the settings mesh_edges_host.cpp runs
    exe = tmp_path / "mesh_edges_host"
    subprocess.run([cxx, "-std=c++17", "-O0", "-g", "-pthread"] + SAN_FLAGS + ["-o", str(exe), os.path.join(ROOT, "tests", "mesh_edges_host.cpp"),
                    os.path.join(CSRC, "bvh_build.cpp"), os.path.join(CSRC, "accel_layout.cpp")], check=True)
    files = []
    for c in mec.all_cases():
        files.append(str(tmp_path / (c.name + ".raw")))
        mec.write_raw(c, files[-1])
    run = subprocess.run([str(exe)] + files, capture_output=True, text=True)
    assert run.returncode == 0, "exit status %d\n%s" % (run.returncode, run.stderr[-2000:])
    lines = run.stdout.splitlines()
    assert len(lines) == 3 * len(files) and not any("refused" in ln for ln in lines), [ln for ln in lines if "refused" in ln][:4]


# ---------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quad,cull", alc.SETTINGS)
@pytest.mark.parametrize("name", mec.NAMES)
def test_layout_accepts_every_blob(rd, built_cases, name, quad, cull):
    """every blob is taken (none of these cases is beyond a limit of the layout: <= 250 stack entries, <= 2^27 triangles), the
    record counts are the blob's, and the scene goes to the reference-order kernel exactly when a leaf exceeds 127 triangles"""
    blob = built_cases[name][0][0]
    s, a = rd.DebugAccelLayout(blob, quad, cull)
    c = mec.case(name)
    assert s["nInst"] == len(c.instances) == a["insts"].shape[0]
    used = {mi for mi, _ in c.instances}
    assert a["tris"].shape[0] == sum(c.meshes[mi][1].shape[0] for mi in used)
    leaves = blas_leaf_sizes(blob)
    assert s["sbtOffsets"] == int(max(leaves) > 127)
    assert s["stackNeed"] <= 250


@pytest.mark.parametrize("name", mec.NAMES)
def test_layout_invariants_hold_on_the_new_cases(rd, built_cases, name):
    """(a leaf above 127 triangles does not fit a wide record's count field: the record keeps its first 127, the scene is flagged
    for the reference-order kernel, which reads the blob's own nodes -- there the flag is what is asserted, not the leaf cover)"""
    blobs = {name: built_cases[name][0][0]}
    if max(blas_leaf_sizes(blobs[name])) > 127:
        assert rd.DebugAccelLayout(blobs[name])[0]["sbtOffsets"] == 1
    else:
        tal.test_every_triangle_belongs_to_one_leaf(rd, blobs, name)
    for quad, cull in alc.SETTINGS + ((-1, -1), (0, 1)):
        tal.test_quad_records_exist_by_rule_and_point_inside(rd, blobs, name, quad, cull)


# ---------------------------------------------------------------------------------------------------------------------
# blob readers of this file's own
# ---------------------------------------------------------------------------------------------------------------------
def top_parts(blob):
    """(top nodes as (n, 12) uint32, instance records as (m, 20) uint32) of a TLAS blob"""
    h = np.frombuffer(blob[:16], np.uint32)
    nodes = np.frombuffer(blob[h[1]:h[2]], np.uint32).reshape(-1, 12)
    leaf = (nodes[:, 8] & LEAF) != 0
    ninst = int((nodes[leaf, 9] + (nodes[leaf, 8] & 0x7fffffff)).max())
    return nodes, np.frombuffer(blob[h[2]: h[2] + 80 * ninst], np.uint32).reshape(-1, 20)


def blas_nodes(blob):
    """[(n, 12) uint32 node array] of every distinct BLAS of a TLAS blob"""
    _, inst = top_parts(blob)
    out = []
    for off in sorted(set(inst[:, 19].tolist())):
        h = np.frombuffer(blob[off: off + 16], np.uint32)
        out.append(np.frombuffer(blob[off + h[1]: off + h[2]], np.uint32).reshape(-1, 12))
    return out


def blas_leaf_sizes(blob):
    return sorted({int(x) for n in blas_nodes(blob) for x in (n[(n[:, 8] & LEAF) != 0, 8] & 0x7fffffff)})


# ---------------------------------------------------------------------------------------------------------------------
# stack needs against a walk of this file's own
# ---------------------------------------------------------------------------------------------------------------------
def reference_order_occupancy(a):
    """largest number of pending entries of the reference-order walk on ONE stack: at an inner node push right, push left, pop left;
    at a top-level leaf push its instances, pop one and walk its BLAS; triangles are tested where they are found.  Reads tnodes,
    insts[blasRoot] and bnodes only."""
    tn, bn, insts = a["tnodes"]["w"], a["bnodes"]["w"], a["insts"]

    def walk(nodes, i, leaf):
        w0, w1 = int(nodes[i][0]), int(nodes[i][1])
        if w0 & LEAF:
            return leaf(w0 & 0x7fffffff, w1)
        return max(2, 1 + walk(nodes, w0, leaf), walk(nodes, w1, leaf))

    blas = lambda cnt, first: 0
    top = lambda cnt, first: max(cnt, cnt - 1 + max(walk(bn, int(insts["blasRoot"][k]), blas) for k in range(first, first + cnt)))
    return walk(tn, 0, top)


def wide_walk_occupancy(a, any_order=False):
    """(largest pending count of the wide walk inside a BLAS over all instances, the same through the cooperative top level): a leaf
    child is queued, never pushed; of two inner children the one in the record's FIRST half is followed and the other pushed
    (any_order: whichever is worse).  Reads `wide`, insts[rootDesc*] and `ctnodes` only."""
    wide, insts, ct = a["wide"], a["insts"], a["ctnodes"]["w"]

    def rec_need(d0, d1):
        if d1 & tal.WIDE_LEAF:
            return 0
        w = wide[d0]
        l, r = (int(w["ld0"]), int(w["ld1"])), (int(w["rd0"]), int(w["rd1"]))
        li, ri = not (l[1] & tal.WIDE_LEAF), not (r[1] & tal.WIDE_LEAF)
        if li and ri:
            nl, nr = rec_need(*l), rec_need(*r)
            return 1 + max(nl, nr) if any_order else max(1 + nl, nr)
        return rec_need(*l) if li else (rec_need(*r) if ri else 0)

    per_inst = [rec_need(int(i["rootDesc0"]), int(i["rootDesc1"])) for i in insts]

    def top(i):
        w0, w1 = int(ct[i][0]), int(ct[i][1])
        if w0 & LEAF:
            cnt = w0 & 0x7fffffff
            return (cnt + 15) // 16 + max(per_inst[w1: w1 + cnt])
        return max(1 + top(w0), top(w1))
    return max(per_inst), top(0)


def _pieces(d1):
    """entries a leaf child of more than 8 triangles leaves on a lane's stack: all but the last of its 8-triangle pieces"""
    return (((int(d1) >> 24) & 0x7f) - 1) // 8 if (int(d1) >> 24) & 0x7f else 0


def _blas_with_pieces(wide, d0, d1, base, push_leaves):
    """peak stack occupancy inside one BLAS from `base` entries when every box is hit.  A record stacks the pieces of its
    oversized leaf children first -- they stay there while the rest of the record is walked --; then, push_leaves (the per-lane
    wide kernel): the second child is pushed whenever both children give an item, leaves included; not push_leaves (the
    cooperative kernel): only an inner second child is pushed, a leaf's last piece is queued."""
    if d1 & tal.WIDE_LEAF:
        return base + _pieces(d1)
    w = wide[d0]
    kids = [(int(w["ld0"]), int(w["ld1"])), (int(w["rd0"]), int(w["rd1"]))]
    inner = [not (k[1] & tal.WIDE_LEAF) for k in kids]
    at = base + sum(_pieces(k[1]) for k, i in zip(kids, inner) if not i)
    pushed = 1 if (push_leaves or all(inner)) else 0
    peak = at + pushed
    if inner[0]:
        peak = max(peak, _blas_with_pieces(wide, *kids[0], at + pushed, push_leaves))
    if inner[1]:
        peak = max(peak, _blas_with_pieces(wide, *kids[1], at, push_leaves))      # (popped: its own entry is gone, the pieces are not)
    return peak


def lane_walk_occupancy(a):
    """the per-lane wide kernel (kernels.hip traverse_wide) on tnodes / insts / wide: one stack for top-level nodes, waiting
    instances, wide records and leaf pieces"""
    tn, insts, wide = a["tnodes"]["w"], a["insts"], a["wide"]

    def top(i, base):
        w0, w1 = int(tn[i][0]), int(tn[i][1])
        if not w0 & LEAF:
            return max(base + 1, top(w0, base + 1), top(w1, base))
        cnt = w0 & 0x7fffffff
        return max([base + cnt - 1] + [_blas_with_pieces(wide, int(insts["rootDesc0"][w1 + k]), int(insts["rootDesc1"][w1 + k]), base + cnt - 1 - k, True)
                                       for k in range(cnt)])
    return top(0, 0)


def coop_walk_occupancy(a):
    """the cooperative kernel's stack on ctnodes / insts / wide: a top-level leaf files its instances as 16-bit masks, the entry
    in use goes back while one of its instances is walked"""
    ct, insts, wide = a["ctnodes"]["w"], a["insts"], a["wide"]

    def top(i, base):
        w0, w1 = int(ct[i][0]), int(ct[i][1])
        if not w0 & LEAF:
            return max(base + 1, top(w0, base + 1), top(w1, base))
        cnt = w0 & 0x7fffffff
        masks = (cnt + 15) // 16
        return max(_blas_with_pieces(wide, int(insts["rootDesc0"][w1 + k]), int(insts["rootDesc1"][w1 + k]), base + masks, False) for k in range(cnt))
    return top(0, 0)


@pytest.mark.parametrize("name", mec.NAMES)
def test_stack_needs_cover_the_pieces_of_oversized_leaves(layouts, name):
    """stackNeed / coopNeed >= the occupancy of the per-lane wide kernel / the cooperative kernel when the pieces of leaves above
    8 triangles are counted where those kernels put them: on the lane's stack, below whatever the record's other child needs --
    so the pieces of every oversized leaf ALONG A PATH are there together (degen_clusters_* are made for this)."""
    s, a = layouts[name]
    lane, coop = lane_walk_occupancy(a), coop_walk_occupancy(a)
    assert s["stackNeed"] >= lane, (name, s["stackNeed"], lane)
    assert s["coopNeed"] >= coop, (name, s["coopNeed"], coop)


@pytest.mark.parametrize("name", mec.NAMES)
def test_stack_needs_cover_a_walk_of_the_tests_own(layouts, name):
    """stackNeed, coopNeed, blasNeed and blasNeedAny are each >= the occupancy this file's walkers measure on the derived arrays.
    EXACT are blasNeed (the wide walk inside a BLAS in the stored order: accel_layout.cpp's cneed, whose swap puts the child with
    the smaller need into the followed half) and blasNeedAny (the same walk under the worse of the two orders at every record):
    those two are asserted equal.  stackNeed and coopNeed are bounds by rule: on top of their walk (leaf pieces along the path
    included, see the test above) they add one entry and a flat allowance for the pieces of the largest leaf, so >= is asserted
    -- and that they exceed the piece-aware walk by no more than that allowance, 1 + 2 * ceil(largest leaf / 8) entries."""
    s, a = layouts[name]
    ref = reference_order_occupancy(a)
    in_blas, coop = wide_walk_occupancy(a)
    in_blas_any, _ = wide_walk_occupancy(a, any_order=True)
    assert s["blasNeed"] == in_blas, (name, s["blasNeed"], in_blas)
    assert s["blasNeedAny"] == in_blas_any >= in_blas, (name, s["blasNeedAny"], in_blas_any)
    leaf = max(int(x) for x in (a["bnodes"]["w"][:, 0][(a["bnodes"]["w"][:, 0] & LEAF) != 0] & 0x7fffffff))
    allowance = 1 + 2 * ((leaf + 7) // 8)
    lane, coop_p = lane_walk_occupancy(a), coop_walk_occupancy(a)
    assert ref <= s["stackNeed"] and coop <= s["coopNeed"]
    assert s["stackNeed"] <= max(lane, ref, 1) + allowance + 1, (name, s["stackNeed"], lane, ref)
    assert s["coopNeed"] <= max(coop_p, 1) + allowance, (name, s["coopNeed"], coop_p)


# ---------------------------------------------------------------------------------------------------------------------
# coverage guards: counted from the blobs and the reference's answers
# ---------------------------------------------------------------------------------------------------------------------
def _node_boxes(nodes):
    return nodes[:, :8].view(np.float32)


def test_guard_a_written_node_box_holds_a_nan(built_cases):
    """found: nan_root (200 triangles) and nan_root_100, one node each -- the root, a leaf, with NaN in both corners: a NaN in a
    node's box makes its cost NaN and the node a leaf, so a written NaN always sits on a leaf box"""
    found = {name: sum(int(np.isnan(_node_boxes(n)).any(1).sum()) for n in blas_nodes(b[1][0])) for name, b in built_cases.items()}
    found = {k: v for k, v in found.items() if v}
    assert set(found) >= {"nan_root", "nan_root_100"}, found
    leaves_100 = blas_leaf_sizes(built_cases["nan_root_100"][1][0])
    assert leaves_100 == [100]          # <= 127: the production engines walk a tree whose root box is NaN


def _sequential_box(p):
    """box of a triangle as linalg.h's min / max give it: `a < b ? a : b` keeps the LATER operand on a NaN"""
    lo, hi = np.full(3, mec.FLT_MAX, np.float32), np.full(3, -mec.FLT_MAX, np.float32)
    for v in p:
        for k in range(3):
            lo[k] = lo[k] if lo[k] < v[k] else v[k]
            hi[k] = hi[k] if hi[k] > v[k] else v[k]
    return lo, hi


def test_guard_a_finite_root_over_a_primitive_box_that_is_not(built_cases):
    """found: 3 cases -- nan_first_last_z, nan_mid_last_x, nan_whole_triangle (a NaN in a triangle's LAST vertex, which its own box
    keeps and a later primitive's min / max drops again): the root box is finite and the tree has inner nodes, although one
    primitive's own box is not finite"""
    found = []
    for c in mec.all_cases():
        if c.instanced:
            continue
        v, t = c.meshes[0]
        bad = np.flatnonzero(~np.isfinite(v[t.astype(np.int64)]).all((1, 2)))
        boxes = [_sequential_box(v[t[j].astype(np.int64)]) for j in bad]
        if any(not (np.isfinite(lo).all() and np.isfinite(hi).all()) for lo, hi in boxes):
            root = _node_boxes(blas_nodes(built_cases[c.name][1][0])[0])[0]
            if np.isfinite(root).all():
                found.append(c.name)
    assert len(found) >= 3 and "nan_first_last_z" in found, found


def test_guard_leaf_sizes_either_side_of_the_engines_limits(built_cases):
    """leaves of exactly 8 and 9 triangles (one piece / two pieces of the engines' 8-triangle work items) and of 127 and 128
    (WIDE_MAX_LEAF_TRIS / the first size that sends the scene to the reference-order kernel) exist -- and 127 and 128 also
    below inner nodes (deep_soup_leaf127 / 128), not only as single-leaf meshes"""
    sizes = {name: blas_leaf_sizes(b[1][0]) for name, b in built_cases.items()}
    every = set().union(*sizes.values())
    assert {8, 9, 127, 128} <= every, sorted(every)
    for name, n in (("deep_soup_leaf127", 127), ("deep_soup_leaf128", 128), ("deep_chain_leaf127", 127)):
        assert max(sizes[name]) == n and len(blas_nodes(built_cases[name][1][0])[0]) > 3, (name, sizes[name])


def test_guard_stack_needs_reach_the_smaller_blocks(built_cases, layouts):
    """trav_threads (kernels.hip) takes 128 threads from stackNeed 41 and 64 threads from 81 (need x threads x 4 bytes > 40 KB).
    Found: three cases with leaves <= 127 -- the production engines run them -- lie in 41..80: deep_chain_leaf127 with stackNeed 56
    (a tree of depth 18 over a leaf of 127 triangles), deep_soup_leaf127 with 55, degen_clusters_5x120 with 76; deep_left_255 has
    depth 25 and stackNeed 28.  All three reach the range through the pieces of their oversized leaves, NOT through tree depth:
    the deepest tree a mesh of this kind gives (deep_left_255, depth 25) stops at 28, so "the need grows with the depth" is held
    only up to there, and the 128-thread branch is reached by leaf pieces.  No mesh within max_depth <= 90 and leaves <= 127 reaches
    81 (a chain gains about one level per decade of triangle sizes, and float32 has 38 of them), so degen_same_320 stands in: one
    leaf of 320 identical triangles, stackNeed 82, traced by the reference-order kernel, which is sized by the same function."""
    need = {n: s["stackNeed"] for n, (s, _) in layouts.items()}
    leaves = {n: max(blas_leaf_sizes(b[0][0])) for n, b in built_cases.items()}
    mid = [n for n in need if 41 <= need[n] <= 80 and leaves[n] <= 127]
    assert "deep_chain_leaf127" in mid, (mid, need["deep_chain_leaf127"])
    assert need["degen_same_320"] >= 81 and leaves["degen_same_320"] == 320
    assert max(d for b in built_cases.values() for d in b[0][2]) >= 25


@pytest.mark.parametrize("name", mec.NAMES)
def test_guard_reference_hits_and_misses(fixture, name):
    """every case's reference answers (both intervals together) hold at least 20 % closest hits and at least one miss
    (found: between 29 % -- nan_mid_mid_z -- and 76 % -- zero_mixed_300)"""
    _, want = reference_answers(fixture, mec.case(name))
    hit = np.concatenate([w1["hit"] for w1, _ in want]) == 1
    assert hit.mean() >= 0.2 and (~hit).any(), (name, float(hit.mean()))


def test_rays_are_what_the_cases_promise():
    for c in mec.all_cases():
        o, d = mec.rays(c)
        assert 192 <= o.shape[0] == mec.N_RAYS <= 256 and np.isfinite(o).all() and np.isfinite(d).all()
        assert all(t.shape[0] >= 8 for _, t in c.meshes)
    assert set(mec.RAGGED_CASES) <= set(mec.NAMES) and len(mec.RAGGED_CASES) == 2
    sizes = [t.shape[0] for _, _, (_, t) in mec.binner_meshes()]
    assert min(sizes) >= 100 and max(sizes) <= 600


# ---------------------------------------------------------------------------------------------------------------------
# the CPU oracle on the rays
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mec.NAMES)
def test_oracle_matches_the_reference_on_every_case(built_cases, fixture, name):
    blob = built_cases[name][0][0]
    assert np.array_equal(gc.sha(blob), fixture[name + "/blob_sha256"])
    cells, want = reference_answers(fixture, mec.case(name))
    assert len(cells) == 2
    for c, (w1, w2) in zip(cells, want):
        got = ob.trace_batch(blob, c.o, c.d, c.tmin, c.tmax, 1)
        bad = mismatches(w1, got)
        assert not bad.any(), describe(c, w1, got, bad, "closest hit")
        got2 = ob.trace_batch(blob, c.o, c.d, c.tmin, c.tmax, 2)
        bad = w2 != got2["hit"]
        assert not bad.any(), "%s, any hit: %d of %d flags differ, first at ray %d" % (c.key, int(bad.sum()), c.n, int(np.flatnonzero(bad)[0]))
