"""Shared definitions of the ray-edge cases (tests/golden/refgpu_rayedges.npz): traversal beyond the stock ray interval
(0.001, 1000) and beyond unit directions.  Like tests/golden_cases.py: deterministic, seeded, float32.  The fixture
generator (tests/golden/make_golden_gpu.py rayedges, runs the REAL reference code object on an MI355X), the CPU test
(tests/test_ray_edges_cpu.py) and the GPU tests (tests/test_gpu_ray_edges.py) all build their inputs here, byte for byte.

A CELL is one launch: (scene, family, name, origins, directions, tmin, tmax).  `Cases(scenes, name, base, params, trace)`
builds the cells of one scene in a fixed order.  Some inputs depend on the REFERENCE's answers (the most frequent t~ of the
tie family, the median t1 of the second-surface family, hit points the far rays aim at): those are `params`.  The generator
passes `trace` (the reference) and empty params, and stores what was computed in the fixture; the tests pass the stored
params and no tracer, so nothing of the product or of the CPU oracle ever shapes an input.

Families, and the kernel property each one is aimed at:
  A  golden rays x INTERVALS: the acceptance `t > 0 && t > tmin && t < tmax` with zero, negative, empty, infinite and NaN bounds
  B  directions scaled by 1e-25 .. 1e25 and by per-ray powers of two, uncut and cut at 3/4 of the stock hits: the walk's
     exactOnly switch (1e-20 / 1e20), its margins that scale with 1 / |d|, best-t bits compared as integers across 50 decades
  C  exact ties: axis-parallel rays from origins at binary-fraction distances of axis-aligned faces; tmax and, separately, tmin
     = nextafter^k(t0), k = -2..2, t0 = the most frequent t~ of the reference: the strict `<` and `>` at both ends
  D  second surface: tmin at the median of / just above the most frequent stock t1: a closer candidate that tmin rejects must
     not cull the surface behind it
  E  origins 1e6 and 1e7 away aimed at hit points; origins inside with tmax around (and a quarter of) the scene diameter
  F  degenerate rays: zero direction, signed zeros, NaN / inf components, denormal directions (192 rays, a batch of their own)
Ray counts per cell are the smallest that keep the conditions on the inputs (tests/test_ray_edges_cpu.py, second half) true.
"""
import numpy as np

import golden_cases as gc

F = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
NAN, INF = float("nan"), float("inf")
STOCK = (0.001, 1000.0)

INTERVALS = (("stock", 0.001, 1000.0), ("0_fltmax", 0.0, FLT_MAX), ("0_inf", 0.0, INF), ("neg1_1000", -1.0, 1000.0),
             ("0.001_2", 0.001, 2.0), ("2_1000", 2.0, 1000.0), ("2_2.5", 2.0, 2.5), ("5_1_empty", 5.0, 1.0),
             ("0.001_1e-30", 0.001, 1e-30), ("1e30_fltmax", 1e30, FLT_MAX), ("nan_1000", NAN, 1000.0),
             ("0.001_nan", 0.001, NAN), ("0.001_neg1", 0.001, -1.0))
# the three intervals of family A that change the most answers (measured with the reference: see the CPU test's conditions)
A_FULL_MATRIX = ("0_fltmax", "0.001_2", "2_1000")
SCALES = (1e-25, 1e-19, 1e-6, 1e-3, 7.0, 1e6, 1e19, 1e25)          # both sides of the walk's exactOnly thresholds 1e-20 / 1e20

GOLDEN = gc.SCENES
SCENES = GOLDEN + ("edges_inst", "edges_inst_id", "planes")
N_GOLDEN = 4 * gc.N_PRIMARY                                          # the golden batch of a scene: family D traces all of it
N_A = {"c0": 4096, "edges_inst": 2048, "edges_inst_id": 2048}      # rays per cell of family A (default 1024): c0's rays mostly miss
N_B = {"c0": 512}                                                  # ... of family B (default 256)
N_C = 1024
N_E = 256
RAGGED = (1, 63, 64, 65)


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def _moved(mesh, dx, dy, dz):
    """a mesh with its vertices displaced (a BLAS of its own that does not overlap its siblings under a shared transform)"""
    v, t, n, uv = mesh
    return np.ascontiguousarray(np.asarray(v, F).reshape(-1, 3) + np.array([dx, dy, dz], F)), t, n, uv


def edges_inst(scenes, identity_group=False):
    """Instanced scene: shared BLASes under a non-uniformly scaled and under a mirrored (negative determinant) transform, and three
    DISTINCT meshes (a BLAS of its own each, inner-node roots) under ONE bit-identical transform -- the product's transform group
    (accel_layout.cpp: instances with bit-identical inverse matrices whose BLAS has a single user).  With
    `identity_group` that shared transform is the identity (identity group).  14 instances: a top level far below 64 nodes."""
    s = scenes.Scene("edges_inst_id" if identity_group else "edges_inst")
    ball = s.add_mesh(scenes.icosphere(2, 0.45))
    cube = s.add_mesh(scenes.box([-0.35, -0.35, -0.35], [0.35, 0.35, 0.35]))
    g1 = s.add_mesh(_moved(scenes.icosphere(2, 0.6), -1.5, 0.0, 0.0))
    g2 = s.add_mesh(_moved(scenes.cylinder([0, -0.75, 0], 0.4, 1.5, 12, 6, 0.05, 3), 0.0, 0.0, 0.25))
    g3 = s.add_mesh(_moved(scenes.heightfield([-0.75, 0, -0.75], [1.5, 0, 0], [0, 0, 1.5], [0, 1, 0], 12, 12, 0.2, 7), 1.5, -0.25, 0.0))
    s.materials = [scenes.material((0.7, 0.7, 0.7), 0.0, 0.5), scenes.material((0.9, 0.8, 0.5), 0.9, 0.2)]
    T, R, S = scenes.translate, scenes.rotate_y, scenes.scale
    s.add_instance(ball, T(-2.5, 1.5, 0.5) @ R(20.0) @ S(1.75, 0.5, 1.0), 0)          # non-uniform scale
    s.add_instance(ball, T(2.5, 1.5, -0.5) @ R(-35.0) @ S(-1.0, 1.25, 1.0), 1)        # mirrored: determinant < 0
    s.add_instance(cube, T(0.0, 1.75, 0.0) @ R(45.0) @ S(1.0, 0.25, 2.0), 0)
    s.add_instance(cube, T(-2.5, -1.5, 0.0) @ S(-1.5, -1.0, 0.5), 1)                   # two axes flipped: determinant > 0 again
    k = 0
    for ix in range(-1, 2):
        for iz in range(-1, 2, 2):
            s.add_instance(ball if k % 2 else cube, T(1.25 * ix, -1.75, 1.5 * iz) @ R(11.0 * k) @ S(1.0 + 0.05 * k, 1.0, 1.0 - 0.04 * k), k % 2)
            k += 1
    shared = np.eye(4, dtype=F) if identity_group else (T(0.5, -0.25, 1.0) @ R(30.0) @ S(1.25, 1.0, 0.75)).astype(F)
    for m in (g1, g2, g3):
        s.add_instance(m, shared.copy(), 0)
    s.add_instance(ball, T(0.0, 0.0, -2.5), 1)
    s.camera = scenes.blender_camera(64, 48, 0.05, 0.036, 9.0, 0.0, (0.5, 9.0, 1.0), (-96.0, 180.0, 0.0))
    s.sceneProps = scenes.blender_dir_light(-45.0, 20.0, 5.0)
    s.rtprop = scenes._rtprop(0, 2, 4)
    return s


GROUP_MEMBERS = (10, 11, 12)          # instance numbers of the three group members of edges_inst / edges_inst_id


def planes(scenes):
    """identity instances of axis-aligned boxes on quarter-unit coordinates, a flat grid and a sphere: the scene of
    test_gpu_parity.test_axis_parallel_rays_in_box_planes_match_the_reference_order_walk (same seed, same construction)"""
    rng = np.random.default_rng(77)
    s = scenes.Scene("planes")
    s.materials = [scenes.material((0.7, 0.7, 0.7))]
    I = np.eye(4, dtype=F)
    for k in range(6):
        lo = np.round(rng.uniform(-3, 0, 3) * 4) / 4; hi = lo + np.round(rng.uniform(0.5, 3, 3) * 4) / 4
        s.add_instance(s.add_mesh(scenes.box(lo.tolist(), hi.tolist())), I, 0)
    s.add_instance(s.add_mesh(scenes.heightfield([-3, -1, -3], [0.25, 0, 0], [0, 0, 0.25], [0, 1, 0], 24, 24, 0.0, 1)), I, 0)
    s.add_instance(s.add_mesh(scenes.icosphere(3, 1.0)), I, 0)
    s.camera = scenes.blender_camera(64, 48, 0.05, 0.036, 9.0, 0.0, (0.5, 14.0, 1.0), (-96.0, 180.0, 0.0))
    s.sceneProps = scenes.blender_dir_light(-45.0, 20.0, 5.0)
    s.rtprop = scenes._rtprop(0, 1, 2)
    return s


def scene(scenes, name):
    if name in GOLDEN:
        return gc.small_scene(scenes, name)
    if name == "planes":
        return planes(scenes)
    return edges_inst(scenes, identity_group=(name == "edges_inst_id"))


def world_bounds(s):
    """(lo, hi) of all instanced vertices, float64"""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for mi, tf, _ in s.instances:
        v = np.asarray(s.meshes[mi][0], np.float64).reshape(-1, 3) @ np.asarray(tf, np.float64)[:3, :3].T + np.asarray(tf, np.float64)[:3, 3]
        lo, hi = np.minimum(lo, v.min(0)), np.maximum(hi, v.max(0))
    return lo, hi


def own_primary_rays(s, n):
    """n pinhole rays at a scene without golden rays: from a point outside its bounds through a jittered grid on its centre
    plane (float64, rounded; directions unit to rounding)"""
    rng = np.random.default_rng(31)
    lo, hi = world_bounds(s)
    c, r = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
    eye = c + np.array([0.3, 0.45, 1.0]) / np.linalg.norm([0.3, 0.45, 1.0]) * 2.5 * r
    tgt = c + rng.uniform(-1, 1, (n, 3)) * (hi - lo) * 0.55
    d = tgt - eye
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(np.tile(eye, (n, 1)), F), np.ascontiguousarray(d, F)


# ---------------------------------------------------------------------------------------------------------------------
# cells
# ---------------------------------------------------------------------------------------------------------------------
class Cell:
    def __init__(self, scene, family, name, o, d, tmin, tmax):
        self.scene, self.family, self.name = scene, family, name
        self.o, self.d = np.ascontiguousarray(o, F).reshape(-1, 3), np.ascontiguousarray(d, F).reshape(-1, 3)
        self.tmin, self.tmax = (float(np.asarray(v, F).reshape(-1)[0]) for v in (tmin, tmax))
        self.n = self.o.shape[0]

    @property
    def key(self):
        return "%s/%s/%s" % (self.scene, self.family, self.name)

    def __repr__(self):
        return "<%s: %d rays, tmin %r tmax %r>" % (self.key, self.n, self.tmin, self.tmax)


def _step(x, k):
    """nextafter^k of a float32"""
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


def _mode_bits(t):
    """the most frequent bit pattern among float32 values (ties: the smallest pattern)"""
    u, c = np.unique(np.ascontiguousarray(t, F).view(np.uint32), return_counts=True)
    return np.array([u[np.argmax(c)]], np.uint32).view(F)[0]


def _unit64(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def degenerate_rays(o, d):
    """family F from plain base rays (o, d): at most 256 rays; row k's kind is in DEGENERATE_KINDS[k]"""
    o, d = o.copy(), d.copy()
    kinds = []
    k = 0
    def put(kind, oo=None, dd=None):
        nonlocal k
        if oo is not None: o[k] = oo
        if dd is not None: d[k] = dd
        kinds.append(kind); k += 1
    z, nz = F(0.0), F(-0.0)
    for _ in range(16):
        put("zero direction", dd=(0, 0, 0))
    for ax in range(3):                                   # (+-0, +-0, +-1) and its two axis permutations, three origins each
        for sa in (z, nz):
            for sb in (z, nz):
                for sc in (F(1.0), F(-1.0)):
                    v = np.roll(np.array([sa, sb, sc], F), ax + 1)
                    for _ in range(3):
                        put("signed zeros", dd=v)
    for c in range(3):
        for _ in range(4):
            oo = o[k].copy(); oo[c] = np.nan; put("NaN origin", oo=oo)
        for _ in range(4):
            dd = d[k].copy(); dd[c] = np.nan; put("NaN direction", dd=dd)
    for c in range(3):
        for sg in (np.inf, -np.inf):
            for _ in range(3):
                oo = o[k].copy(); oo[c] = sg; put("inf origin", oo=oo)
            for _ in range(3):
                dd = d[k].copy(); dd[c] = sg; put("inf direction", dd=dd)
    tiny = F(1e-40)                                       # a float32 denormal
    for c in range(3):
        for sg in (tiny, -tiny):
            for _ in range(2):
                dd = d[k].copy(); dd[c] = sg; put("denormal component", dd=dd)
            dd = np.full(3, sg, F); dd[c] = F(1.0) if sg > 0 else F(-1.0); put("two denormal components", dd=dd)
            dd = np.full(3, sg, F); put("denormal direction", dd=dd)
    while k < 192:
        put("plain")
    return np.ascontiguousarray(o[:k]), np.ascontiguousarray(d[:k]), tuple(kinds)


class Cases:
    """cells of one scene.  base: (ray_o, ray_d) of the scene's 4096 golden rays or None; params: dict of reference-derived
    inputs (filled when `trace` is given); trace(o, d, tmin, tmax, rec) -> HitData records of the reference"""

    def __init__(self, scenes, name, base=None, params=None, trace=None):
        self.scenes, self.name, self.trace = scenes, name, trace
        self.params = {} if params is None else params
        self.s = scene(scenes, name)
        self.base = base

    def p(self, key, fn):
        if key not in self.params:
            if self.trace is None:
                raise KeyError("the fixture holds no parameter %r for scene %s" % (key, self.name))
            self.params[key] = np.asarray(fn())
        return self.params[key]

    # -- the rays of family A ------------------------------------------------------------------------------------
    def golden_rays(self):
        if self.base is None:
            po, pd = own_primary_rays(self.s, gc.N_PRIMARY)
            ph = self.p("primary_hit_t", lambda: (lambda h: np.where(h["hit"] == 1, h["distance"], F(-1.0)).astype(F))(self.trace(po, pd, *STOCK, 1)))
            self.base = gc.derived_rays(5, po, pd, (ph >= 0).astype(np.uint32), np.where(ph >= 0, ph, F(np.inf)).astype(F))
        o, d = self.base
        assert o.shape[0] == N_GOLDEN
        return np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)

    def stock_t(self, o, d):
        """the reference's stock-interval t of the golden rays, -1 where it misses"""
        return self.p("stock_t", lambda: (lambda h: np.where(h["hit"] == 1, h["distance"], F(-1.0)).astype(F))(self.trace(o, d, *STOCK, 1)))

    def tie_rays(self, axes):
        rng = np.random.default_rng(41 + sum(axes))
        o = rng.uniform(-3, 3, (N_C, 3)).astype(F)
        d = np.zeros((N_C, 3), F)
        a = np.array(axes)[np.arange(N_C) % len(axes)]
        o[np.arange(N_C), a] = F(8.0)
        d[np.arange(N_C), a] = F(-1.0)
        return o, d

    def cells(self, families="ABCDEF"):
        name, out = self.name, []
        add = lambda fam, nm, o, d, tmin, tmax: out.append(Cell(name, fam, nm, o, d, tmin, tmax))
        if name == "planes":
            families = [f for f in families if f == "C"]
        if name != "planes":
            go, gd = self.golden_rays()                       # all 4096; families take every k-th ray: all four kinds of derived_rays
            t1 = self.stock_t(go, gd)
            st = N_GOLDEN // N_A.get(name, 1024)
            ao, ad = go[::st], gd[::st]
            t_cut = F(np.percentile(t1[t1 >= 0], 75))         # three quarters of the stock hits lie in front of it
        if "A" in families:
            for nm, tmin, tmax in INTERVALS:
                add("A", nm, ao, ad, tmin, tmax)
        if "B" in families and name != "edges_inst_id":
            st = N_GOLDEN // N_B.get(name, 256)
            bo, bd = go[::st], gd[::st]
            rng = np.random.default_rng(43)
            per_ray = np.ldexp(F(1.0), rng.integers(-60, 61, bo.shape[0])).astype(F)
            for nm, sc in [("%g" % s, F(s)) for s in SCALES] + [("pow2", per_ray)]:
                ds = (bd * (sc[:, None] if np.ndim(sc) else sc)).astype(F)
                add("B", "x%s_full" % nm, bo, ds, 0.0, FLT_MAX)
                if not np.ndim(sc):
                    add("B", "x%s_cut" % nm, bo, ds, 0.0, t_cut / sc)
            add("B", "xpow2_cut", bo, (bd * per_ray[:, None]).astype(F), 0.0, t_cut)
        if "C" in families and name in ("c0", "c1", "planes"):
            for tag, axes in (("y", (1,)), ("xz", (0, 2))):
                co, cd = self.tie_rays(axes)
                t0 = self.p("tie_t0_" + tag, lambda: (lambda h: _mode_bits(h["distance"][h["hit"] == 1]))(self.trace(co, cd, 0.0, FLT_MAX, 1)))
                for k in range(-2, 3):
                    v = _step(F(t0), k)
                    add("C", "%s_tmax%+d" % (tag, k), co, cd, 0.0, v)
                for k in range(-2, 3):
                    v = _step(F(t0), k)
                    add("C", "%s_tmin%+d" % (tag, k), co, cd, v, FLT_MAX)
        if "D" in families:
            add("D", "tmin_median", go, gd, F(np.median(t1[t1 >= 0])), 1000.0)
            add("D", "tmin_above_mode", go, gd, _step(_mode_bits(t1[t1 >= 0]), 1), 1000.0)
        if "E" in families and name in GOLDEN:
            h = np.flatnonzero(t1 >= 0)
            hp = go[h].astype(np.float64) + gd[h].astype(np.float64) * t1[h].astype(np.float64)[:, None]
            rng = np.random.default_rng(47)
            tgt = hp[rng.integers(0, hp.shape[0], N_E)]
            u = _unit64(rng.normal(size=(N_E, 3)))
            for nm, R in (("far1e6", 1e6), ("far1e7", 1e7)):
                eo = (tgt + u * R).astype(F)
                add("E", nm, eo, _unit64(tgt - eo.astype(np.float64)).astype(F), 0.0, FLT_MAX)
            lo, hi = world_bounds(self.s)
            diam = float(np.linalg.norm(hi - lo))
            m = N_E
            io = (lo + (hi - lo) * rng.uniform(0.05, 0.95, (m, 3))).astype(F)
            idir = _unit64(tgt[:m] - io.astype(np.float64))
            idir[m // 2:] = _unit64(rng.normal(size=(m - m // 2, 3)))
            add("E", "inside_short", io, idir.astype(F), 0.0, F(diam * 0.98))
            add("E", "inside_beyond", io, idir.astype(F), 0.0, F(diam * 1.02))
            add("E", "inside_half", io, idir.astype(F), 0.0, F(diam * 0.25))
        if "F" in families:
            base = np.argsort(t1 < 0, kind="stable")[:: max(1, int((t1 >= 0).sum()) // 256)][:256]      # plain rays that hit, to be spoilt
            fo, fd, _ = degenerate_rays(go[base], gd[base])
            add("F", "stock", fo, fd, *STOCK)
            add("F", "0_fltmax", fo, fd, 0.0, FLT_MAX)
        return out


DEGENERATE_KINDS = degenerate_rays(np.zeros((256, 3), F), np.ones((256, 3), F))[2]


# ---------------------------------------------------------------------------------------------------------------------
# fixture layout (tests/golden/refgpu_rayedges.npz)
#   <scene>/blob_sha256          SHA-256 of the TLAS blob the rays were traced through
#   <scene>/par/<key>            reference-derived input parameters (Cases.params)
#   <scene>/hit                  closest-hit flags of all cells in Cases.cells() order, one bit per ray (packbits)
#   <scene>/any_xor_hit          any-hit flags, stored as the difference to the closest-hit flags
#   <scene>/idx_delta            for every closest hit in that order: row of its HitData in the record table (first differences)
#   <scene>/recs                 table of the distinct HitData records (28 words each) in order of first use, transposed (byte planes)
# ---------------------------------------------------------------------------------------------------------------------
def pack_scene(name, sha, params, results):
    """results: [(closest HIT records, any-hit HIT records)] in cell order -> dict of arrays"""
    hit = np.concatenate([(r1["hit"] == 1) for r1, _ in results])
    anyh = np.concatenate([(r2["hit"] == 1) for _, r2 in results])
    recs = np.concatenate([r1[r1["hit"] == 1] for r1, _ in results])
    raw = np.ascontiguousarray(recs).view(np.uint8).reshape(-1, 112)
    table, first, idx = np.unique(raw, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")          # rows in order of first use: consecutive hits then have consecutive rows
    rank = np.empty_like(order); rank[order] = np.arange(order.shape[0])
    idx = rank[idx.reshape(-1)].astype(np.int64)
    out = {name + "/blob_sha256": sha, name + "/hit": np.packbits(hit), name + "/any_xor_hit": np.packbits(anyh ^ hit),
           name + "/idx_delta": np.diff(idx, prepend=0).astype(np.int32), name + "/recs": np.ascontiguousarray(table[order].T)}
    for k, v in params.items():
        out["%s/par/%s" % (name, k)] = np.asarray(v)
    return out


def load_params(G, name):
    pre = name + "/par/"
    return {k[len(pre):]: G[k] for k in G.files if k.startswith(pre)}


def unpack_scene(G, name, cells, hit_dtype):
    """-> [(closest HIT records -- zeros where the reference missed --, any-hit flags uint32)] per cell"""
    total = sum(c.n for c in cells)
    hit = np.unpackbits(G[name + "/hit"])[:total].astype(bool)
    anyh = (np.unpackbits(G[name + "/any_xor_hit"])[:total].astype(bool) ^ hit).astype(np.uint32)
    table = np.ascontiguousarray(G[name + "/recs"].T)
    recs = np.ascontiguousarray(table[np.cumsum(G[name + "/idx_delta"].astype(np.int64))]).view(hit_dtype).reshape(-1)
    assert recs.shape[0] == int(hit.sum())
    full = np.zeros(total, hit_dtype)
    full[hit] = recs
    out, at = [], 0
    for c in cells:
        out.append((full[at: at + c.n], anyh[at: at + c.n]))
        at += c.n
    return out
