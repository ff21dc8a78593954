"""Shared definitions of the mesh-edge cases (tests/golden/refgpu_meshedges.npz): hostile GEOMETRY under the builders, the
layout derivation and every walk.  Like ray_edge_cases.py / shade_edge_cases.py: deterministic, seeded, float32.  The fixture
recorder (tests/golden/make_golden_gpu.py meshedges, runs the REAL reference's intersectTop on an MI355X), the CPU tests
(tests/test_mesh_edges_cpu.py) and the GPU tests (tests/test_gpu_mesh_edges.py) all build meshes and rays here, byte for byte.

A CASE is a scene: meshes [(vertices (n, 3) float32, triangles (m, 3) uint32)] and instances [(mesh, 4x4 transform)].  Every
mesh of a class has at least 8 triangles, so the builder takes its split path.  The rays aimed at a case go with it
(`cells(case)`): 224 rays through the centres of finite triangle boxes, along the axes inside box planes, at the finite
vertices of broken triangles, from inside the mesh, random ones and some that point away; at the stock interval and at
(0, FLT_MAX).  Rays are made from the case's SANE coordinates only (finite, |x| < 100): nothing of the product, the oracle or
the reference shapes an input.

Classes (names carry the class as a prefix):
  nan_     one NaN coordinate in the first / middle / last vertex of the first / a middle / the last triangle, on each axis; two
           NaNs on different axes; an all-NaN triangle; nan_root / nan_root_100: NaN in the last vertex of the LAST triangle -- the
           root box keeps it and the mesh becomes one leaf (of 200: reference-order kernel; of 100: production engines)
  inf_     +inf, -inf, +-FLT_MAX, +-3e38 in one coordinate; the whole mesh scaled by 1e30 (half-areas overflow, inf * 0 in a
           cost); a mesh of denormal size (1e-40).  The last two carry a unit companion mesh, the only thing a ray can hit there
  degen_   a repeated vertex, collinear vertices; same_N: N identical triangles, N = 8, 9, 16, 17, 127, 128, 129 and 320
           (one unsplittable leaf; 127 = WIDE_MAX_LEAF_TRIS, above it the scene goes to the reference-order kernel; 320: the
           reference-order kernel with 64 threads per block); clusters_*: several unsplittable sets in one mesh
  extent_  flat in each axis plane; extents 9.9e-5 and 1.01e-4 either side of the axis skip `fabsf(stop - start) < 1e-4`
  plane_   centroids exactly on candidate planes: multiples of extent / 1024 (depth 0) and of extent * (depth + 1) / 1024
  zero_    signed zeros mixed into vertices
  deep_    lopsided deep trees: geometric progressions of triangle sizes and their mirror images (max_depth <= 90); a soup
           and a progression next to 127 / 128 identical triangles (the largest leaf the engines serve, below inner nodes)
  inst_    a hostile mesh under the identity and under a non-identity transform; two hostile meshes under one shared
           non-identity transform (a transform group); an instance matrix with a NaN entry, one with an inf entry
builder_only_meshes(): three meshes held to the oracle's blob only (the partition's strict `<`, the axis skip); binner_meshes():
the meshes of the GPU binning test.
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
NAN, INF = float("nan"), float("inf")
STOCK = (0.001, 1000.0)
INTERVALS = (("stock",) + STOCK, ("0_fltmax", 0.0, FLT_MAX))
N_RAYS = 224
RAGGED = (1, 63, 64, 65)
RAGGED_CASES = ("nan_mid_last_x", "degen_same_17")


class Case:
    def __init__(self, name, meshes, instances=None):
        self.name = name
        self.meshes = [(np.ascontiguousarray(v, F).reshape(-1, 3), np.ascontiguousarray(t, np.uint32).reshape(-1, 3)) for v, t in meshes]
        self.instances = [(k, np.eye(4, dtype=F)) for k in range(len(self.meshes))] if instances is None else \
                         [(mi, np.ascontiguousarray(tf, F).reshape(4, 4)) for mi, tf in instances]

    @property
    def instanced(self):
        return self.name.startswith("inst_")

    def __repr__(self):
        return "<%s: %s triangles, %d instances>" % (self.name, [int(t.shape[0]) for _, t in self.meshes], len(self.instances))


# ---------------------------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------------------------
def soup(seed, n, spread=2.0, size=0.35):
    """n random triangles, a vertex triple each (no sharing: spoiling a vertex spoils one triangle)"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-spread, spread, (n, 1, 3))
    v = (c + rng.normal(size=(n, 3, 3)) * size).astype(F).reshape(-1, 3)
    return v, np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)


def _spoil(v, tri, vert, axis, value):
    v = v.copy()
    v[3 * tri + vert, axis] = F(value)
    return v


def unit_companion(offset=(0.0, 0.0, 0.0)):
    """an octahedron subdivided once (32 triangles) of radius 1: something a ray can hit next to a mesh it cannot"""
    p = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    tris = []
    for a, b, c in faces:
        A, B, Cc = p[a], p[b], p[c]
        ab, bc, ca = [(x + y) / np.linalg.norm(x + y) for x, y in ((A, B), (B, Cc), (Cc, A))]
        tris += [(A, ab, ca), (ab, B, bc), (ca, bc, Cc), (ab, bc, ca)]
    v = (np.array(tris).reshape(-1, 3) + np.array(offset)).astype(F)
    return v, np.arange(v.shape[0], dtype=np.uint32).reshape(-1, 3)


def identical(n):
    v = np.tile(np.array([[-1.0, -0.5, 0.25], [1.0, -0.5, 0.25], [0.0, 1.0, -0.25]], F), (n, 1))
    return v, np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)


def clusters(xs, n):
    """n identical triangles at each x of xs (every set a little higher than the one before)"""
    ms = []
    for k, x in enumerate(xs):
        v, t = identical(n)
        ms.append(((v * F(0.3) + np.array([x, 0.1 * k, 0], F)).astype(F), t))
    return joined(*ms)


def flat(seed, n, axis, thickness=0.0):
    """a soup squeezed onto the plane axis = 0.5, or to the given extent along the axis (two triangles span it exactly)"""
    v, t = soup(seed, n)
    v[:, axis] = F(0.5)
    if thickness:
        rng = np.random.default_rng(seed + 1)
        v[:, axis] = (F(0.5) + rng.uniform(0, 1, v.shape[0]).astype(F) * F(thickness)).astype(F)
        v[0, axis] = F(0.5); v[5, axis] = F(0.5) + F(thickness)
        v[:, axis] = np.minimum(v[:, axis], F(0.5) + F(thickness))
    return v, t


def on_planes(seed, n, depth_steps=False):
    """triangles whose box centroids are exact multiples of extent / 1024 on every axis (extent 8 = [-4, 4], step 2^-7, so
    every candidate plane start + k * step is exact): `centroid < plane` is decided on equality.  With depth_steps the
    coordinates are multiples of extent * (depth + 1) / 1024 for the depths 1..3 too (steps 2^-6, 3 * 2^-7, 2^-5: common
    multiple 3 * 2^-5 inside boxes that keep power-of-two extents after a split at the middle)."""
    rng = np.random.default_rng(seed)
    step = 3.0 / 32.0 if depth_steps else 1.0 / 128.0
    k = rng.integers(-int(3.5 / step), int(3.5 / step) + 1, (n, 3))
    c = k * step
    h = rng.integers(1, 5, (n, 3)) * (1.0 / 64.0)          # half extents, exact
    v = np.zeros((n, 3, 3))
    v[:, 0] = c - h; v[:, 1] = c + h                        # box corners: centroid (lo + hi) / 2 = c exactly
    v[:, 2] = c + h * np.array([1.0, -1.0, 0.5])
    v = v.reshape(-1, 3)
    # pin the extent to [-4, 4] on every axis with two more triangles
    pin = np.array([[-4, -4, -4], [-3.5, -4, -3.5], [-4, -3.5, -3.5], [4, 4, 4], [3.5, 4, 3.5], [4, 3.5, 3.5]], np.float64)
    v = np.concatenate([v, pin]).astype(F)
    return v, np.arange(v.shape[0], dtype=np.uint32).reshape(-1, 3)


def signed_zeros(seed, n):
    rng = np.random.default_rng(seed)
    v, t = soup(seed, n, spread=1.0, size=0.5)
    m = rng.uniform(size=v.shape) < 0.35
    z = np.where(rng.uniform(size=v.shape) < 0.5, F(0.0), F(-0.0)).astype(F)
    v = np.where(m, z, v).astype(F)
    return v, t


def progression(n, ratio, top, mirror=False):
    """n nested triangles that share the corner at the origin, sizes top * ratio^k: the box of any subset is the box of its
    largest member, so the SAH peels the few largest triangles off again and again -- a lopsided tree, about one level per
    decade of sizes (the split needs two primitives on each side and an extent of at least 1e-4).  The small triangles
    have the smaller centroids and go LEFT: the reference's walk keeps one pending right sibling per level, so its need grows
    with the depth.  The mirror image (x, y, z negated) puts the chain on the right: deep tree, small need."""
    s = top * ratio ** np.arange(n, dtype=np.float64)
    z = np.zeros(n)
    v = np.stack([np.stack([z, z, z], 1), np.stack([s, 0.25 * s, 0.5 * s], 1), np.stack([0.125 * s, s, s], 1)], 1).reshape(-1, 3)
    if mirror:
        v = -v
    return v.astype(F), np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)


def joined(*meshes):
    vs, ts, at = [], [], 0
    for v, t in meshes:
        vs.append(np.asarray(v, F)); ts.append(np.asarray(t, np.uint32) + np.uint32(at)); at += v.shape[0]
    return np.concatenate(vs), np.concatenate(ts)


def _tf(tx, ty, tz, deg, sx, sy, sz):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    T = np.eye(4); T[:3, 3] = (tx, ty, tz)
    R = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]])
    S = np.diag([sx, sy, sz, 1.0])
    return (T @ R @ S).astype(F)


def _build_cases():
    out = []
    add = lambda name, meshes, instances=None: out.append(Case(name, meshes, instances))
    # ---- NaN: (triangle position) x (vertex position) x axis, rotated so that 9 cases cover every value of each ----
    sizes = (8, 9, 40, 200)
    k = 0
    for ti, tname in enumerate(("first", "mid", "last")):
        for vi, vname in enumerate(("first", "mid", "last")):
            n = sizes[k % 4]
            axis = (ti + vi) % 3
            tri = (0, n // 2, n - 1)[ti]
            if tname == "last" and vname == "last":
                k += 1
                continue                                # the root-box case below
            v, t = soup(100 + k, n)
            add("nan_%s_%s_%s" % (tname, vname, "xyz"[axis]), [(_spoil(v, tri, vi, axis, NAN), t)])
            k += 1
    v, t = soup(120, 200)
    add("nan_root", [(_spoil(v, 199, 2, 1, NAN), t)])
    v, t = soup(121, 40)
    add("nan_two_axes", [(_spoil(_spoil(v, 7, 0, 0, NAN), 22, 1, 2, NAN), t)])
    v, t = soup(122, 40)
    v[3 * 11: 3 * 11 + 3] = F(NAN)
    add("nan_whole_triangle", [(v, t)])
    v, t = soup(123, 300)
    add("nan_300", [(_spoil(_spoil(v, 17, 0, 2, NAN), 150, 1, 0, NAN), t)])
    # the same with 100 triangles: a NaN root box over a leaf that the production engines walk (<= WIDE_MAX_LEAF_TRIS).  A NaN
    # in a node's box makes its cost NaN and the node a leaf, and a NaN primitive that is not the LAST of a node is dropped by
    # the next min / max (which then restarts from that primitive: the box no longer holds the earlier ones -- the reference's
    # behaviour, and the blob's), so a written NaN always sits on a leaf
    v, t = soup(124, 100)
    add("nan_root_100", [(_spoil(v, 99, 2, 0, NAN), t)])
    # ---- infinities and overflow ----
    for nm, val, n, seed in (("pinf", INF, 200, 130), ("ninf", -INF, 40, 131), ("pfltmax", FLT_MAX, 40, 132), ("nfltmax", -FLT_MAX, 9, 133),
                             ("p3e38", 3e38, 200, 134), ("n3e38", -3e38, 8, 135)):
        v, t = soup(seed, n)
        add("inf_" + nm, [(_spoil(v, n // 3, 1, seed % 3, val), t)])
    v, t = soup(136, 40)
    add("inf_scaled_1e30", [((v.astype(np.float64) * 1e30).astype(F), t), unit_companion()])
    v, t = soup(137, 40)
    add("inf_denormal", [((v.astype(np.float64) * 1e-40).astype(F), t), unit_companion((3.0, 0.0, 0.0))])
    # ---- degenerate triangles, unsplittable sets ----
    v, t = soup(140, 40)
    v[3 * 5 + 1] = v[3 * 5]; v[3 * 20 + 2] = v[3 * 20]; v[3 * 39 + 2] = v[3 * 39 + 1]
    add("degen_repeated_vertex", [(v, t)])
    v, t = soup(141, 40)
    for tri in (0, 13, 39):
        v[3 * tri + 2] = (v[3 * tri] + (v[3 * tri + 1] - v[3 * tri]) * F(0.25 * (1 + tri % 3))).astype(F)
    add("degen_collinear", [(v, t)])
    for n in (8, 9, 16, 17, 127, 128, 129, 320):
        add("degen_same_%d" % n, [identical(n)])
    # several unsplittable sets in one mesh, at doubling distances: a lopsided tree with an oversized leaf beside every level
    # of a path.  The per-lane and the cooperative kernel keep the 8-triangle pieces of each of them on the lane's stack at once
    add("degen_clusters_7x40", [clusters((0, 1, 3, 7, 15, 31, 63), 40)])
    add("degen_clusters_5x120", [clusters((0, 1, 3, 7, 15), 120)])
    # ---- extent either side of the axis skip ----
    # (a flat root box never passes the reference's slab test `tFar > max(tNear, 0)`: no ray ever hits a flat mesh.  The unit
    #  companion gives the rays something to hit; the flat instance must be MISSED by every walk as it is by the reference)
    for axis in range(3):
        add("extent_flat_" + "xyz"[axis], [flat(150 + axis, 40, axis), unit_companion((0.0, 0.0, 0.0))])
    add("extent_below_skip", [flat(153, 40, 1, 9.9e-5)])
    add("extent_above_skip", [flat(154, 40, 2, 1.01e-4)])
    # ---- centroids on candidate planes ----
    add("plane_depth0", [on_planes(160, 200)])
    add("plane_deeper", [on_planes(161, 400, depth_steps=True)])
    # ---- signed zeros ----
    add("zero_mixed_40", [signed_zeros(170, 40)])
    add("zero_mixed_300", [signed_zeros(171, 300)])
    # ---- lopsided deep trees ----
    for nm, n, ratio, top, mirror in DEEP:
        add(nm, [progression(n, ratio, top, mirror)])
    # a soup next to 127 identical triangles: an inner tree over a leaf of exactly WIDE_MAX_LEAF_TRIS triangles, the largest
    # the production engines serve (walked in pieces of 8); the same with 128: the smallest that goes to the reference-order kernel
    for n in (127, 128):
        v, t = identical(n)
        add("deep_soup_leaf%d" % n, [joined(soup(175, 300), ((v + np.array([9.0, 0, 0], F)).astype(F), t))])
    v, t = identical(127)
    add("deep_chain_leaf127", [joined(progression(120, 0.75, 1e12), ((v + np.array([9.0, 0, 0], F)).astype(F), t))])
    # ---- instances ----
    v, t = soup(180, 40)
    hostile = (_spoil(v, 20, 1, 0, NAN), t)
    v2, t2 = soup(181, 40)
    hostile2 = ((_spoil(v2, 3, 0, 2, INF) + np.array([6.0, 0, 0], F)).astype(F), t2)
    shared = _tf(0.5, -0.25, 1.0, 30.0, 1.25, 1.0, 0.75)
    add("inst_identity_and_moved", [hostile, unit_companion()], [(0, np.eye(4)), (0, _tf(7.0, 1.0, -2.0, 40.0, 1.5, 0.5, -1.0)), (1, _tf(-6.0, 0, 0, 0, 1, 1, 1))])
    add("inst_group", [hostile, hostile2, unit_companion()], [(0, shared), (1, shared.copy()), (2, _tf(-6.0, 2.0, 0, 15.0, 1, 2, 1))])
    m = _tf(5.0, 0.0, 0.0, 20.0, 1, 1, 1); m[1, 2] = F(NAN)
    add("inst_nan_matrix", [soup(182, 40), unit_companion()], [(0, m), (1, np.eye(4)), (0, _tf(-5.0, 0, 0, 0, 1, 1, 1))])
    m = _tf(5.0, 0.0, 0.0, 20.0, 1, 1, 1); m[0, 3] = F(INF)
    add("inst_inf_matrix", [soup(183, 40), unit_companion()], [(0, m), (1, np.eye(4)), (0, _tf(-5.0, 0, 0, 0, 1, 1, 1))])
    return out


# (name, triangles, ratio, size of the largest triangle, mirror).  With the oracle's builder: deep_left_120 and deep_right_120 have
# max_depth 20, deep_left_255 has 25 (about one level per decade of sizes: 1e12 .. 1e-3 and 1e15 .. 1e-3)
DEEP = (("deep_left_120", 120, 0.75, 1e12, False), ("deep_right_120", 120, 0.75, 1e12, True), ("deep_left_255", 255, 0.85, 1e15, False))

_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = _build_cases()
    return _ALL


NAMES = tuple(c.name for c in all_cases())


def dense_planes(seed, n):
    """centroids on the lattice k / 128, |k| <= 32, on every axis, inside an extent pinned to [-4, 4] (candidate planes of the
    root: -4 + j / 128, exact): several centroids on EVERY candidate plane of the middle, so the plane the root chooses carries
    some -- `centroid < plane` is decided on equality there"""
    rng = np.random.default_rng(seed)
    c = rng.integers(-32, 33, (n, 3)) / 128.0
    h = rng.integers(1, 5, (n, 3)) / 256.0
    v = np.zeros((n, 3, 3))
    v[:, 0] = c - h; v[:, 1] = c + h; v[:, 2] = c + h * np.array([1.0, -1.0, 0.5])
    pin = np.array([[-4, -4, -4], [-3.5, -4, -3.5], [-4, -3.5, -3.5], [4, 4, 4], [3.5, 4, 3.5], [4, 3.5, 3.5]], np.float64)
    v = np.concatenate([v.reshape(-1, 3), pin]).astype(F)
    return v, np.arange(v.shape[0], dtype=np.uint32).reshape(-1, 3)


def thin_stack(n, extent):
    """n copies of one triangle that differ only in z, spread evenly over `extent`: x and y cannot split them (equal
    centroids), z can -- if the axis is not skipped (`fabsf(stop - start) < 1e-4`)"""
    v, t = identical(n)
    v = v.reshape(n, 3, 3).copy()
    v[:, :, 2] = (F(0.5) + np.linspace(0.0, extent, n)[:, None]).astype(F)
    v[-1, :, 2] = F(0.5) + F(extent)
    return v.reshape(-1, 3).astype(F), t


def builder_only_meshes():
    """[(name, (vertices, triangles))] held to the oracle's blob only (no rays): the chosen plane carries centroids; the only
    splittable axis has an extent just above / just below the skip"""
    return [("dense_planes_400", dense_planes(165, 400)),
            ("thin_above_skip", thin_stack(16, 1.01e-4)), ("thin_below_skip", thin_stack(16, 9.9e-5))]


def binner_meshes():
    """[(name, finite, (vertices, triangles))]: hostile meshes of 200 to 600 triangles for the GPU binning pass (nodes of at
    least 64 primitives).  finite: every primitive box and centroid is finite, so the device must be asked to bin."""
    v, t = soup(190, 100)
    dup = (np.tile(v.reshape(-1, 3, 3), (3, 1, 1)).reshape(-1, 3), np.arange(900, dtype=np.uint32).reshape(-1, 3))
    v, t = soup(191, 300)
    fm = (_spoil(v, 100, 1, 0, FLT_MAX), t)
    out = [("flat_y_300", True, flat(192, 300, 1)), ("plane_depth0", True, case("plane_depth0").meshes[0]),
           ("plane_deeper", True, case("plane_deeper").meshes[0]), ("duplicates_300", True, dup),
           ("zero_mixed_300", True, case("zero_mixed_300").meshes[0]), ("fltmax_300", True, fm),
           ("deep_left_255", True, case("deep_left_255").meshes[0]), ("deep_soup_leaf127", True, case("deep_soup_leaf127").meshes[0])]
    out += [(n, False, case(n).meshes[0]) for n in ("nan_300", "nan_root", "inf_pinf")]
    return out


def case(name):
    for c in all_cases():
        if c.name == name:
            return c
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------------
# blobs
# ---------------------------------------------------------------------------------------------------------------------
def product_blob(rd, c, many=False):
    """(TLAS blob, [BLAS blobs], [BLAS max depths], TLAS max depth) of the product's host builder"""
    if many:
        blas = rd.BuildAccelStructs(None, [rd.Mesh(v, t) for v, t in c.meshes])
    else:
        blas = [rd.BuildAccelStruct(None, rd.Mesh(v, t)) for v, t in c.meshes]
    insts = [rd.Instance(tf, 0, k, blas[mi]) for k, (mi, tf) in enumerate(c.instances)]
    blob, depth = rd.BuildTopAccelStructBlob(insts)
    return blob, [b.data for b in blas], [b.max_depth for b in blas], depth


def write_raw(c, path):
    """the case as the raw file tests/mesh_edges_host.cpp reads"""
    with open(path, "wb") as f:
        f.write(np.array([len(c.meshes), len(c.instances)], np.uint32).tobytes())
        for v, t in c.meshes:
            f.write(np.array([v.shape[0], t.shape[0]], np.uint32).tobytes() + v.tobytes() + t.tobytes())
        for mi, tf in c.instances:
            f.write(np.array([mi], np.uint32).tobytes() + np.ascontiguousarray(tf, F).tobytes())


def oracle_blob(ob, c):
    blas = [ob.OracleBlas(v, t) for v, t in c.meshes]
    blob, depth = ob.tlas_build([(mi, tf, 0, k) for k, (mi, tf) in enumerate(c.instances)], blas)
    return blob, [b.blob for b in blas], [b.max_depth for b in blas], depth


# ---------------------------------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------------------------------
def _sane(x):
    with np.errstate(invalid="ignore"):
        return np.isfinite(x).all(-1) & (np.abs(x) < 100.0).all(-1)


def world_triangles(c):
    """(m, 3, 3) float64 world-space vertices of every instanced triangle whose transform is finite; broken[m]: the triangle
    has a vertex that is not sane (its sane vertices are kept, the others are NaN)"""
    tris = []
    for mi, tf in c.instances:
        tf = tf.astype(np.float64)
        if not np.isfinite(tf).all():
            continue
        v, t = c.meshes[mi]
        w = v.astype(np.float64) @ tf[:3, :3].T + tf[:3, 3]
        w[~_sane(v)] = np.nan
        tris.append(w[t.astype(np.int64)])
    return np.concatenate(tris)


def rays(c):
    """the N_RAYS rays of a case (float32 origins and directions)"""
    rng = np.random.default_rng(abs(hash_name(c.name)) % (1 << 31))
    T = world_triangles(c)
    ok_v = ~np.isnan(T).any(-1)                              # (m, 3)
    with np.errstate(invalid="ignore"):
        whole = ok_v.all(1) & ((T.max(1) - T.min(1)).max(1) > 1e-5)      # (a triangle of denormal size counts as broken)
    pts = T[whole].reshape(-1, 3)
    lo, hi = pts.min(0), pts.max(0)
    ctr, r = (lo + hi) / 2, max(float(np.linalg.norm(hi - lo)) / 2, 1e-3)
    W = T[whole]
    blo, bhi = W.min(1), W.max(1)
    def outside(n):
        u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
        return ctr + u * 2.5 * r
    def aim(o, tgt):
        d = tgt - o
        return d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-30)
    O, D = [], []
    # 64 random rays: half at points of the bounds, half at points of whole triangles
    o = outside(64)
    tgt = lo + (hi - lo) * rng.uniform(-0.05, 1.05, (64, 3))
    k = rng.integers(0, W.shape[0], 32)
    b = rng.dirichlet([1, 1, 1], 32)
    tgt[32:] = (W[k] * b[:, :, None]).sum(1)
    O.append(o); D.append(aim(o, tgt))
    # 48 through the centres of triangle boxes
    k = rng.integers(0, W.shape[0], 48)
    o = outside(48); O.append(o); D.append(aim(o, (blo[k] + bhi[k]) / 2))
    # 32 along the axes inside box planes: the origin shares two coordinates with a corner of a triangle's box
    k = rng.integers(0, W.shape[0], 32)
    ax = np.arange(32) % 3
    o = np.where(rng.uniform(size=(32, 3)) < 0.5, blo[k], bhi[k])
    sg = np.where(np.arange(32) % 2 == 0, 1.0, -1.0)
    o[np.arange(32), ax] = ctr[ax] - sg * 2.5 * r
    d = np.zeros((32, 3)); d[np.arange(32), ax] = sg
    O.append(o); D.append(d)
    # 32 at the sane vertices of broken triangles (any vertices where nothing is broken)
    bv = T[~whole][ok_v[~whole]] if (~whole).any() and ok_v[~whole].any() else pts
    k = rng.integers(0, bv.shape[0], 32)
    o = outside(32); O.append(o); D.append(aim(o, bv[k]))
    # 32 from inside
    o = ctr + rng.uniform(-0.3, 0.3, (32, 3)) * (hi - lo)
    u = rng.normal(size=(32, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    O.append(o); D.append(u)
    # 16 that point away
    o = outside(16); O.append(o); D.append(aim(ctr[None, :].repeat(16, 0), o))
    o, d = np.concatenate(O).astype(F), np.concatenate(D).astype(F)
    assert o.shape[0] == N_RAYS and np.isfinite(o).all() and np.isfinite(d).all()
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def hash_name(name):
    h = 2166136261
    for b in name.encode():
        h = ((h ^ b) * 16777619) & 0xffffffff
    return h


class Cell:
    def __init__(self, scene, name, o, d, tmin, tmax):
        self.scene, self.family, self.name, self.o, self.d = scene, "M", name, o, d
        self.tmin, self.tmax = float(F(tmin)), float(F(tmax))
        self.n = o.shape[0]

    @property
    def key(self):
        return "%s/%s" % (self.scene, self.name)


def cells(c):
    o, d = rays(c)
    return [Cell(c.name, nm, o, d, tmin, tmax) for nm, tmin, tmax in INTERVALS]


def reference_answers(G, c, hit_dtype):
    """(cells, [(reference closest-hit records, reference any-hit flags)]) of a case from the loaded fixture G"""
    import ray_edge_cases as rec
    cs = cells(c)
    return cs, rec.unpack_scene(G, c.name, cs, hit_dtype)


# ---------------------------------------------------------------------------------------------------------------------
# fixture layout (tests/golden/refgpu_meshedges.npz), per case <name>:
#   <name>/blob_sha256   SHA-256 of the TLAS blob the rays were traced through
#   <name>/hit           closest-hit flags of the cells in cells() order, one bit per ray (packbits)
#   <name>/any_xor_hit   any-hit flags, stored as the difference to the closest-hit flags
#   <name>/idx_delta, <name>/recs   the HitData records of the closest hits, as in ray_edge_cases.py
# ---------------------------------------------------------------------------------------------------------------------
