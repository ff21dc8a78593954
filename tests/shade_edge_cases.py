"""Shared definitions of the shading edge cases (tests/golden/refgpu_shade_edges.npz): the closest-hit shader, the BRDF pair,
the camera and the tone map at the edges of their inputs.  Like tests/ray_edge_cases.py: deterministic, seeded, float32, no GPU.
The fixture generator (tests/golden/make_golden_gpu.py shadeedges, runs the REAL reference code object on an MI355X), the CPU
test (tests/test_shade_edges_cpu.py) and the GPU tests (tests/test_gpu_shade_edges.py) build their inputs here, byte for byte.

THE EDGE SCENE: one instance per case, each a unit quad of two triangles in the plane z = 0 of its own space (front: +z), laid
out as a grid in the world plane z = 0 that CAMERA sees from z = 20; INSTANCES[k] = (family, name) of instance k:
  material   the plain quad (unit normals, a translation) with one Material record each: roughness -1 .. 2 and NaN, metallic up to
             5, transmission up to 2, ior 0 .. 50, albedo 0 / 1 / above 1 / negative, and one with normalTexIdx = 0 (textures off:
             texel 0) on the plain quad and on quads whose world normal is (+-1, 0, 0)
  normal     one mesh per vertex-normal set: zero, cancelling, 1e-30, 1e-42, 1e30, 3e38, 7.5, opposed, tilted, (+-1, 0, 0) and
             both sides of GetNormalSpace's 1e-6 threshold
  transform  the plain quad under rotate_y(+-90), uniform scale 1e-15 and 1e15, a mirror, scale(1e6, 1, 1e-6)
  aux        a wall beyond the grid's right edge that shadows its right half (the light comes from +x +z)
RAYS: per quad 24 rays of six direction classes at the stock interval (batch "main"), and the front rays with their direction
scaled by 1e-25 and by 1e25, the interval scaled to match (batches "s-25", "s+25").  A ray is stated in the quad's own space and
carried to the world by the instance's transform (direction by its linear part, NOT renormalised: under a scale of 1e-15 a
world-space ray of unit direction would meet the quad at t = 1e-15, below tmin); class "x" is stated in world space.
Batch "keys" aims at three materials (diffuse, metallic, transmissive) from the front and from inside with the keys of KEY_KINDS;
batch "light" is every sixth ray of "main", the batch every light buffer is run on.
In every batch the key of row i is (frameID, pixel = i, depth): the reference's `material` draws its random input from
get_global_id(0), so the pixel of a row cannot be chosen (and no key can carry 0xffffffff there).
"""
import numpy as np

import golden_cases as gc

F = np.float32
NAN, INF = float("nan"), float("inf")
FLT_MAX = float(np.finfo(np.float32).max)
SPACING, COLS = 1.5, 10
STOCK = (0.001, 1000.0)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# the comparison rule
# ---------------------------------------------------------------------------------------------------------------------
def compare(got, want):
    """THE rule: float32 arrays of one shape are equal where their bits are (signs of zero and infinities included), or where the
    reference `want` is NaN and `got` is NaN too (payload and sign free).  -> (equal per row: bool (n,), NaN share, inf share of
    the reference's components)"""
    g, w = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert g.shape == w.shape, (g.shape, w.shape)
    wn = np.isnan(w)
    ok = (g.view(np.uint32) == w.view(np.uint32)) | (wn & np.isnan(g))
    ok = ok.reshape(ok.shape[0], int(np.prod(ok.shape[1:]))).all(1) if ok.ndim else ok
    size = max(w.size, 1)
    return ok, float(wn.sum()) / size, float(np.isinf(w).sum()) / size


def nan_rows(*arrays):
    """rows with a NaN in any of the arrays (each (n, ...))"""
    out = None
    for a in arrays:
        a = np.ascontiguousarray(a, F)
        r = np.isnan(a.reshape(a.shape[0], int(np.prod(a.shape[1:])))).any(1)
        out = r if out is None else (out | r)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the scene
# ---------------------------------------------------------------------------------------------------------------------
def _material(rd, albedo, metallic, roughness, transmission, ior, normal_tex=-1):
    m = np.zeros((), rd.Material)
    m["albedo"] = (albedo[0], albedo[1], albedo[2], 1.0)
    m["metallic"], m["roughness"], m["transmission"], m["ior"] = metallic, roughness, transmission, ior
    m["albedoTexIdx"] = m["metallicTexIdx"] = m["roughnessTexIdx"] = -1
    m["normalTexIdx"] = normal_tex
    return m


ROUGHNESS = (-1.0, 0.0, 1e-3, 0.05, 1.0, 2.0, NAN)
METALLIC = (0.0, 0.5, 1.0, 5.0)
TRANSMISSION = (0.0, 0.5, 1.0, 2.0)
IOR = (0.0, 0.5, 1.0, 1.45, 10.0, 50.0)
ALBEDOS = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2.5, 1.0, 0.5), (-0.5, 0.3, 1.0))
MID = ((0.8, 0.6, 0.4), 0.2, 0.3, 0.5, 1.45)            # the material of the normal / transform / aux instances: every lobe occurs
KEY_MATERIALS = ("diffuse", "metallic", "transmissive")


def materials(rd):
    """[(name, Material)]: 76 records; the first three are the materials of batch "keys" """
    grey = (0.7, 0.65, 0.6)
    out = [("diffuse", _material(rd, grey, 0.0, 0.5, 0.0, 1.45)), ("metallic", _material(rd, grey, 1.0, 0.3, 0.0, 1.45)),
           ("transmissive", _material(rd, grey, 0.0, 0.2, 0.5, 1.45))]
    for r in ROUGHNESS:                                   # roughness x {diffuse, metallic, glass}
        for tag, me, tr in (("d", 0.0, 0.0), ("m", 1.0, 0.0), ("t", 0.0, 1.0)):
            out.append(("rough%g%s" % (r, tag), _material(rd, grey, me, r, tr, 1.45)))
    for me in METALLIC:                                   # metallic x transmission at the clamp's floor of roughness / just above it
        for k, tr in enumerate(TRANSMISSION):
            out.append(("met%g_tr%g" % (me, tr), _material(rd, grey, me, 0.0 if k % 2 else 0.05, tr, 1.45)))
    for io in IOR:                                        # ior x transmission
        for tr in (0.5, 1.0, 2.0):
            out.append(("ior%g_tr%g" % (io, tr), _material(rd, grey, 0.0, 1e-3, tr, io)))
    for k, a in enumerate(ALBEDOS):
        out.append(("albedo%d_d" % k, _material(rd, a, 0.0, 0.4, 0.0, 1.45)))
        out.append(("albedo%d_t" % k, _material(rd, a, 0.5, 0.4, 0.5, 1.45)))
    for io, r, tr in ((10.0, 0.05, 1.0), (10.0, 0.3, 1.0), (10.0, 0.05, 2.0), (0.5, 0.3, 1.0), (50.0, 0.3, 1.0), (0.0, 0.3, 1.0), (1.0, 0.3, 1.0)):
        out.append(("ior%g_rough%g_tr%g" % (io, r, tr), _material(rd, grey, 0.0, r, tr, io)))     # rough glass: total internal reflection
    out.append(("met5_rough0.3", _material(rd, grey, 5.0, 0.3, 0.0, 1.45)))
    out.append(("roughnan_met0.5", _material(rd, grey, 0.5, NAN, 0.5, 1.45)))
    out.append(("albedo3_m", _material(rd, ALBEDOS[3], 1.0, 0.3, 0.0, 1.45)))
    out.append(("normal_tex0", _material(rd, grey, 0.2, 0.3, 0.5, 1.45, normal_tex=0)))
    out.append(("mid", _material(rd, *MID)))
    assert len(out) >= 60 and len({n for n, _ in out}) == len(out)
    return out


def _quad(normals):
    """the unit quad in z = 0, counter-clockwise seen from +z; normals: one (3,) for all four vertices, or (4, 3)"""
    v = np.array([[-0.5, -0.5, 0], [0.5, -0.5, 0], [0.5, 0.5, 0], [-0.5, 0.5, 0]], F)
    t = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    n = np.ascontiguousarray(np.broadcast_to(np.asarray(normals, F), (4, 3)), F)
    uv = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F)
    return v, t, n, uv


_TILT = (0.30000001192092896, 0.20000000298023224, 0.9327379465103149)
NORMAL_SETS = (
    ("zero", (0.0, 0.0, 0.0)),
    ("cancel", ((0, 0, 1), (0, 0, -1), (0, 0, 1), (0, 0, -1))),          # zero along b1 = 1/2 (b3 = 1/2 in the second triangle)
    ("1e-30", (0.0, 0.0, 1e-30)),                                        # |v|^2 below FLT_MIN: the 2^86 path
    ("1e-42", (0.0, 1e-42, 1e-42)),                                      # denormal components
    ("1e30", (0.0, 1e30, 1e30)),                                         # |v|^2 infinite
    ("3e38", (3e38, 3e38, 3e38)),                                        # ... and still infinite after 2^-66
    ("7.5", (0.0, 0.0, 7.5)),
    ("opposed", (0.0, 0.0, -1.0)),
    ("tilted", _TILT),
    ("+x", (1.0, 0.0, 0.0)), ("-x", (-1.0, 0.0, 0.0)),
    ("+x_5e-7", (1.0, 1e-3, 0.0)), ("+x_2e-6", (1.0, 2e-3, 0.0)),        # 1 - |N.x| = 5e-7 and 2e-6 after normalize
    ("-x_5e-7", (-1.0, 0.0, 1e-3)), ("-x_2e-6", (-1.0, 0.0, 2e-3)),
)
ZERO_NORMAL_SETS = ("zero", "cancel")                   # the meshes on which an interpolated normal can be exactly (0, 0, 0)


def transforms(scenes):
    """[(name, linear part or None for the identity, z of the quad's centre)]"""
    R, S = scenes.rotate_y, scenes.scale
    return (("scale1e-15", S(1e-15, 1e-15, 1e-15), 0.0), ("translate", None, 0.0), ("rot+90", R(90.0), 0.0), ("rot-90", R(-90.0), 0.0),
            ("scale1e15", S(1e15, 1e15, 1e15), -5.0), ("mirror", S(-1.0, 1.0, 1.0), 0.0), ("scale1e6_1_1e-6", S(1e6, 1.0, 1e-6), 0.0))


LIGHT_DIRECTION = (-0.6, -0.1, -0.78)                   # towards -x -z: L points to +x +z, the wall shadows the grid's right half
CAMERA_Z = 20.0


def edge_scene(scenes):
    """-> (Scene, INSTANCES: [(family, name)] per instance).  Instance 0 is the 1e-15 quad: it sits at the world's origin, the only
    place where a float32 origin can come within 1e-15 of it."""
    rd = scenes.rd
    s = scenes.Scene("shade_edges")
    mats = materials(rd)
    s.materials = [m for _, m in mats]
    mat_no = {n: k for k, (n, _) in enumerate(mats)}
    plain = s.add_mesh(_quad((0.0, 0.0, 1.0)))
    inst = []

    def cell(k):
        return (k % COLS) * SPACING, (k // COLS) * SPACING

    def put(family, name, mesh, lin, mat, z=0.0):
        x, y = cell(len(inst))
        tf = scenes.translate(x, y, z)
        if lin is not None:
            tf = (tf @ lin).astype(F)
        s.add_instance(mesh, tf, mat)
        inst.append((family, name))
    tfs = transforms(scenes)
    put("transform", tfs[0][0], plain, tfs[0][1], mat_no["mid"], tfs[0][2])
    for name, _ in mats[:-1]:
        put("material", name, plain, None, mat_no[name])
    px, mx = s.add_mesh(_quad((1.0, 0.0, 0.0))), s.add_mesh(_quad((-1.0, 0.0, 0.0)))
    put("material", "normal_tex0/+x", px, None, mat_no["normal_tex0"])
    put("material", "normal_tex0/-x", mx, None, mat_no["normal_tex0"])
    for name, n in NORMAL_SETS:
        mesh = px if name == "+x" else mx if name == "-x" else s.add_mesh(_quad(n))
        put("normal", name, mesh, None, mat_no["mid"])
    for name, lin, z in tfs[1:]:
        put("transform", name, plain, lin, mat_no["mid"], z)
    rows = (len(inst) + COLS - 1) // COLS
    xw = (COLS - 1) * SPACING + 2.0
    ytop = (rows - 2) * SPACING + 0.7                       # the last row (the quad scaled by 1e6 along x) stays clear of the wall
    wall = s.add_mesh((np.array([[xw, -2, -1], [xw, ytop, -1], [xw, ytop, 8], [xw, -2, 8]], F),
                       np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.tile(np.array([-1, 0, 0], F), (4, 1)), np.zeros((4, 3), F)))
    s.add_instance(wall, np.eye(4, dtype=F), mat_no["mid"])
    inst.append(("aux", "wall"))
    assert len(inst) <= 160 and inst[(rows - 1) * COLS] == ("transform", "scale1e6_1_1e-6") and len(inst) == (rows - 1) * COLS + 2
    cam = np.zeros((), rd.PhysicalCamera)
    cam["widthPixel"], cam["heightPixel"] = 64, 64
    cam["focalLength"], cam["sensorWidth"], cam["focalDistance"], cam["fStop"] = 0.05, 0.04, CAMERA_Z, 0.0
    cam["x"], cam["y"], cam["z"] = (COLS - 1) * SPACING / 2, (rows - 1) * SPACING / 2, CAMERA_Z
    s.camera = cam
    sp = np.zeros((), rd.SceneProperties)
    sp["lightCount"][0] = 1
    sp["lights"][0]["direction"] = LIGHT_DIRECTION + (0.0,)
    sp["lights"][0]["color"] = (4.0, 3.5, 3.0, 1.0)
    s.sceneProps = sp
    s.rtprop = scenes._rtprop(0, 2, 4)
    return s, tuple(inst)


def instance_numbers(instances, family, name=None):
    return [k for k, (f, n) in enumerate(instances) if f == family and (name is None or n == name)]


# ---------------------------------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------------------------------
CLASSES = ("front", "normal", "behind", "graze+", "graze-", "x", "s-25", "s+25")
_TARGETS = ((0.0, 0.0), (0.1, -0.2), (-0.3, 0.25), (0.2, 0.3), (-0.15, -0.35))
_FRONT = ((0.5, 0.3, 0.8), (-0.6, 0.2, 0.7), (0.1, -0.7, 0.6), (-0.3, -0.4, 0.85), (0.75, 0.0, 0.5))


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _local_rays():
    """[(class number, origin, direction)] in the quad's own space, float64: 20 rays of classes front .. graze-"""
    out = []
    for p, u in zip(_TARGETS, _FRONT):
        u = _unit(u)
        out.append((0, np.array([p[0], p[1], 0.0]) + u, -u))
    for p in _TARGETS[:4]:
        out.append((1, np.array([p[0], p[1], 1.0]), np.array([0.0, 0.0, -1.0])))
    for p, u in zip(_TARGETS, _FRONT):
        u = _unit(u) * np.array([1.0, -1.0, -1.0])
        out.append((2, np.array([p[0], p[1], 0.0]) + u, -u))
    for cls, sg in ((3, 1.0), (4, -1.0)):
        for k, p in enumerate(_TARGETS[:3]):
            phi = 0.7 + 2.1 * k
            u = np.array([np.cos(phi) * np.cos(1e-3), np.sin(phi) * np.cos(1e-3), sg * np.sin(1e-3)])
            out.append((cls, np.array([p[0], p[1], 0.0]) + 0.3 * u, -u))
    return out


_X_OFFSETS = ((0.0, 0.0), (0.1, 0.25), (-0.2, -0.25), (0.05, 1e-3))      # (dy, dz) of the world-x rays: in the plane, above, below


class Batch:
    def __init__(self, name, o, d, tmin, tmax, cls, target, frames, depths):
        self.name = name
        self.o, self.d = np.ascontiguousarray(o, F).reshape(-1, 3), np.ascontiguousarray(d, F).reshape(-1, 3)
        self.tmin, self.tmax = float(F(tmin)), float(F(tmax))
        self.cls, self.target = np.asarray(cls, np.int32), np.asarray(target, np.int32)
        self.frames, self.depths = np.asarray(frames, np.uint32), np.asarray(depths, np.int32)
        self.n = self.o.shape[0]
        assert all(a.shape[0] == self.n for a in (self.d, self.cls, self.target, self.frames, self.depths))

    @property
    def pixels(self):
        return np.arange(self.n, dtype=np.uint32)

    def take(self, name, rows, frames=None, depths=None):
        f, dp = gc.material_inputs(len(rows))
        return Batch(name, self.o[rows], self.d[rows], self.tmin, self.tmax, self.cls[rows], self.target[rows],
                     f if frames is None else frames, dp if depths is None else depths)


def _world(tf, o, d):
    tf = np.asarray(tf, np.float64)
    return tf[:3, :3] @ o + tf[:3, 3], tf[:3, :3] @ d


def main_rays(scene, instances):
    """-> (o, d, cls, target) float64 / int of the 24 rays per instance of classes front .. x, instance after instance"""
    local = _local_rays()
    O, D, C, T = [], [], [], []
    for k, (mi, tf, _) in enumerate(scene.instances):
        if instances[k][0] == "aux":
            continue
        for cls, o, d in local:
            ow, dw = _world(tf, o, d)
            O.append(ow); D.append(dw); C.append(cls); T.append(k)
        c = np.asarray(tf, np.float64)[:3, 3]
        for dy, dz in _X_OFFSETS:
            O.append(c + np.array([-1.0, dy, dz])); D.append(np.array([1.0, 0.0, 0.0])); C.append(5); T.append(k)
    return np.array(O), np.array(D), np.array(C), np.array(T)


# ---- keys -----------------------------------------------------------------------------------------------------------
# kinds of batch "keys"; each is used on the three KEY_MATERIALS from the front and from inside, three rays each (18 rows)
KEY_KINDS = ("y_min", "y_max", "z_below_half", "z_above_half", "2z_below_t", "2z_above_t", "x_min", "x_max",
             "frame_ffffffff", "depth_ffffffff", "both_ffffffff")
N_SEARCHED = 8
ROWS_PER_KIND = 18
KEY_EPS = 2e-6


def key_property(kind, rnd):
    """the stated property of a searched key kind on rnd = pcg3d(frameID, pixel, depth) (n, 3) float32 -> bool (n,)"""
    x, y, z = (np.asarray(rnd, np.float64)[:, k] for k in range(3))
    return {"y_min": y < KEY_EPS, "y_max": y > 1 - KEY_EPS,
            "z_below_half": (z < 0.5) & (z > 0.5 - KEY_EPS), "z_above_half": (z >= 0.5) & (z < 0.5 + KEY_EPS),
            "2z_below_t": (2 * z < 0.5) & (2 * z > 0.5 - 2 * KEY_EPS), "2z_above_t": (2 * z >= 0.5) & (2 * z < 0.5 + 2 * KEY_EPS),
            "x_min": x < KEY_EPS, "x_max": x > 1 - KEY_EPS}[kind]


def key_score(kind, rnd):
    """what the search minimises (float64; inf where the side is wrong)"""
    x, y, z = (np.asarray(rnd, np.float64)[:, k] for k in range(3))
    inf = np.inf
    return {"y_min": y, "y_max": 1 - y, "z_below_half": np.where(z < 0.5, 0.5 - z, inf), "z_above_half": np.where(z >= 0.5, z - 0.5, inf),
            "2z_below_t": np.where(2 * z < 0.5, 0.5 - 2 * z, inf), "2z_above_t": np.where(2 * z >= 0.5, 2 * z - 0.5, inf),
            "x_min": x, "x_max": 1 - x}[kind]


def search_keys(pcg3d, span=1 << 22):
    """the frameID below `span` that serves each searched row best (pixel = row, depth = row % 5) -> SEARCHED_FRAMES"""
    out = []
    f = np.arange(span, dtype=np.uint32)
    for kind_no, kind in enumerate(KEY_KINDS[:N_SEARCHED]):
        for j in range(ROWS_PER_KIND):
            row = kind_no * ROWS_PER_KIND + j
            rnd = pcg3d(np.stack([f, np.full(span, row, np.uint32), np.full(span, row % 5, np.uint32)], 1))
            out.append(int(np.argmin(key_score(kind, rnd))))
    return tuple(out)


# found by search_keys(oracle_bind.pcg3d) on the CPU; tests/test_shade_edges_cpu.py re-checks the property of every one
SEARCHED_FRAMES = (
    3589940, 3709187, 1701590, 1763913, 566965, 2155631, 3541828, 4059412, 1408488,
    3880144, 104206, 3767419, 1802578, 2570590, 2597736, 3200228, 465210, 3333466,
    3319487, 536040, 1986047, 796752, 206467, 3543283, 33501, 855515, 3709220,
    2015948, 2917261, 493499, 1175386, 609027, 671113, 2816029, 309017, 2170435,
    3714202, 1007086, 1748884, 1530133, 173841, 1031147, 2716065, 1494971, 2130055,
    1923111, 616976, 164611, 155160, 893161, 1590542, 450217, 2588691, 626156,
    1027861, 899141, 495468, 2212793, 1719378, 804185, 503452, 2109921, 460213,
    2407097, 3616102, 3322769, 3931660, 145283, 3843452, 238111, 4024761, 3888887,
    1720051, 3607598, 150846, 3217230, 758082, 530683, 2782752, 683132, 2336296,
    2660015, 2212339, 3030759, 1195127, 4185521, 4033727, 2615042, 714213, 1471301,
    4011433, 1108279, 1942752, 3712172, 84154, 2682674, 2752966, 2262078, 1901880,
    1925109, 1055199, 3812461, 1214466, 3059072, 617826, 1696286, 1819589, 1294242,
    1568248, 1338061, 3171078, 1106780, 595181, 898445, 2926257, 3439385, 2478172,
    3607848, 4145303, 2572046, 1369034, 2246912, 4172872, 2541181, 3907580, 82384,
    3864198, 3495266, 1632893, 213855, 2475709, 390805, 751686, 370664, 4190222,
    3635586, 1028544, 1200570, 2018871, 317787, 1226086, 3001730, 2946721, 1275494,
)


def key_rows():
    """(frames uint32, depths int32, kind number) of the rows of batch "keys" """
    n = len(KEY_KINDS) * ROWS_PER_KIND
    row = np.arange(n)
    kind = row // ROWS_PER_KIND
    frames = (row % 7).astype(np.uint32)
    depths = (row % 5).astype(np.int32)
    ns = N_SEARCHED * ROWS_PER_KIND
    assert len(SEARCHED_FRAMES) == ns, "run search_keys and paste its result into SEARCHED_FRAMES"
    frames[:ns] = np.array(SEARCHED_FRAMES, np.uint32)
    k = np.array(KEY_KINDS)[kind]
    frames[(k == "frame_ffffffff") | (k == "both_ffffffff")] = 0xffffffff
    depths[(k == "depth_ffffffff") | (k == "both_ffffffff")] = -1
    return frames, depths, kind


def batches(scenes):
    """-> (scene, INSTANCES, {name: Batch}) in the order main, s-25, s+25, keys, light"""
    s, inst = edge_scene(scenes)
    o, d, cls, tgt = main_rays(s, inst)
    f, dp = gc.material_inputs(o.shape[0])
    out = {"main": Batch("main", o, d, *STOCK, cls, tgt, f, dp)}
    front = np.flatnonzero(cls == 0).reshape(-1, len(_FRONT))[:, :4].reshape(-1)
    for name, sc, c in (("s-25", 1e-25, 6), ("s+25", 1e25, 7)):
        with np.errstate(over="ignore"):
            ds = (d[front] * sc).astype(F)
        f, dp = gc.material_inputs(front.shape[0])
        out[name] = Batch(name, o[front], ds, F(0.001) / F(sc), F(1000.0) / F(sc), np.full(front.shape[0], c), tgt[front], f, dp)
    # keys: per kind 3 materials x (front, behind) x 3 rays
    rows = []
    for _ in KEY_KINDS:
        for m in KEY_MATERIALS:
            k = instance_numbers(inst, "material", m)[0]
            mine = np.flatnonzero(tgt == k)
            rows += list(mine[cls[mine] == 0][:3]) + list(mine[cls[mine] == 2][:3])
    frames, depths, _ = key_rows()
    out["keys"] = out["main"].take("keys", np.array(rows), frames, depths)
    out["light"] = out["main"].take("light", np.arange(0, out["main"].n, 6))
    return s, inst, out


# ---------------------------------------------------------------------------------------------------------------------
# lights
# ---------------------------------------------------------------------------------------------------------------------
def light_variants():
    """[(name, direction (3,), colour (3,))]; variant 0 is the scene's own light"""
    own_c = (4.0, 3.5, 3.0)
    return (("own", LIGHT_DIRECTION, own_c), ("dir_zero", (0.0, 0.0, 0.0), own_c), ("dir_1e-30", (-6e-31, -1e-31, -7.8e-31), own_c),
            ("dir_1e30", (-6e29, -1e29, -7.8e29), own_c), ("dir_3e38", (-3e38, -3e38, -3e38), own_c),
            ("dir_in_plane", (-1.0, 0.0, 0.0), own_c),                  # L = (1, 0, 0): in the plane of the z-facing quads
            ("dir_minus_v", (0.0, 0.0, 1.0), own_c),                    # L = (0, 0, -1) = -V of the normal-incidence rays: H = normalize(0)
            ("col_zero", LIGHT_DIRECTION, (0.0, 0.0, 0.0)), ("col_negative", LIGHT_DIRECTION, (-1.0, -2.0, 0.5)),
            ("col_inf", LIGHT_DIRECTION, (INF, 1.0, INF)), ("col_nan", LIGHT_DIRECTION, (NAN, 1.0, 2.0)))


def light_buffers(rd):
    """one SceneProperties per variant: slot k of buffer j holds variant (j + k) mod 11, so every variant sits in slot 0 once and
    in each of the slots 1 .. 4 once"""
    V = light_variants()
    out = np.zeros(len(V), rd.SceneProperties)
    for j in range(len(V)):
        out[j]["lightCount"][0] = 5
        for k in range(5):
            _, d, c = V[(j + k) % len(V)]
            out[j]["lights"][k]["direction"] = tuple(d) + (0.0,)
            out[j]["lights"][k]["color"] = tuple(c) + (1.0,)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# (d) the bare BRDF on caller-filled material records
# ---------------------------------------------------------------------------------------------------------------------
def _dot3_f32(v):
    """dot(v, v) as the fma chain fma(z, z, fma(y, y, x * x)) in float32; products of float32 are exact in float64"""
    v = np.asarray(v, F).astype(np.float64)
    a = (v[:, 0] * v[:, 0]).astype(F).astype(np.float64)
    b = (v[:, 1] * v[:, 1] + a).astype(F).astype(np.float64)
    return (v[:, 2] * v[:, 2] + b).astype(F)


def exact_unit_vectors(rng, n):
    """n float32 vectors whose restated squared length is exactly 1.0f: normalize leaves them as they are"""
    out = np.zeros((0, 3), F)
    while out.shape[0] < n:
        v = rng.normal(size=(4 * n, 3))
        v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
        out = np.concatenate([out, v[_dot3_f32(v) == F(1.0)]])
    return np.ascontiguousarray(out[:n])


N_BRDF_L, N_BRDF_V, N_BRDF = 10, 40, 2000


def brdf_grid():
    """-> dict: L (10, 3) and V (40, 3) exact unit vectors, and per row (2000): l, v (indices), N, albedo, metallic, roughness,
    transmission, ior; row i uses light l[i] -- rows are sorted by it, one rd.LightHits call per light"""
    rng = np.random.default_rng(20261019)
    L, V = exact_unit_vectors(rng, N_BRDF_L), exact_unit_vectors(rng, N_BRDF_V)
    n = N_BRDF
    l = np.sort(rng.integers(0, N_BRDF_L, n))
    v = rng.integers(0, N_BRDF_V, n)
    N = rng.normal(size=(n, 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    toward = np.sign((N * (L[l].astype(np.float64) + V[v].astype(np.float64))).sum(1, keepdims=True))
    N = np.where(rng.uniform(size=(n, 1)) < 0.8, N * np.where(toward == 0, 1, toward), N)      # most normals face the half vector
    kind = rng.integers(0, 4, n)
    N[kind == 1] *= rng.uniform(0.5, 2.0, (int((kind == 1).sum()), 1))                          # slightly non-unit
    N[kind == 2] = [1.0, 0.0, 0.0]
    N[kind == 3] = [-1.0, 0.0, 0.0]
    N[(kind == 3) & (np.arange(n) % 2 == 0)] = [1.0, 1e-3, 0.0]
    rough = rng.choice(np.array([-1.0, 0.0, 1e-3, 0.05, 0.5, 1.0, 2.0, NAN]), n, p=[0.1, 0.15, 0.15, 0.15, 0.16, 0.15, 0.1, 0.04])
    albedo = rng.uniform(-0.5, 2.5, (n, 3))
    albedo[::5] = rng.uniform(0.0, 1.0, (albedo[::5].shape[0], 3))
    return dict(L=L, V=V, l=l, v=v, N=N.astype(F), albedo=albedo.astype(F), metallic=rng.choice(np.array(METALLIC), n).astype(F),
                roughness=rough.astype(F), transmission=rng.choice(np.array(TRANSMISSION), n).astype(F),
                ior=rng.choice(np.array(IOR), n).astype(F))


def brdf_packed(g):
    """the 19 floats per row k_ref_brdf takes (the random triple is not used by microfacetBRDF: 0.5)"""
    n = g["l"].shape[0]
    return np.ascontiguousarray(np.concatenate([g["L"][g["l"]], g["V"][g["v"]], g["N"], g["albedo"], g["metallic"][:, None], g["roughness"][:, None],
                                                g["transmission"][:, None], g["ior"][:, None], np.full((n, 3), 0.5, F)], 1), F)


# ---------------------------------------------------------------------------------------------------------------------
# (h) cameras
# ---------------------------------------------------------------------------------------------------------------------
N_CAMERA_RAYS = 96
PI_2 = float(F(np.pi / 2))


def cameras(rd):
    """[(name, PhysicalCamera)]; the last two may give all-NaN rays"""
    base = dict(widthPixel=16, heightPixel=12, focalLength=0.05, sensorWidth=0.036, focalDistance=5.0, fStop=0.0, x=1.0, y=2.0, z=3.0,
                wx=0.3, wy=-0.2, wz=0.1)
    lens = dict(fStop=2.8)
    table = [("pinhole", {}), ("lens", lens), ("fstop_1e-30", dict(fStop=1e-30)), ("fstop_1e30", dict(fStop=1e30)), ("fstop_-2.8", dict(fStop=-2.8)),
             ("fstop_inf", dict(fStop=INF)), ("focal_0", dict(focalLength=0.0)), ("sensor_0", dict(sensorWidth=0.0)),
             ("sensor_0_lens", dict(sensorWidth=0.0, **lens)), ("sensor_negative", dict(sensorWidth=-0.036)),
             ("sensor_negative_lens", dict(sensorWidth=-0.036, **lens)), ("focal_0_sensor_0", dict(focalLength=0.0, sensorWidth=0.0)),
             ("distance_0", dict(focalDistance=0.0, **lens)), ("distance_1e30", dict(focalDistance=1e30, **lens)),
             ("angles_0", dict(wx=0.0, wy=0.0, wz=0.0)), ("angles_pi_2", dict(wx=PI_2, wy=PI_2, wz=PI_2, **lens)),
             ("angles_1e6", dict(wx=1e6, wy=-1e6, wz=1e6)), ("angles_1e10", dict(wx=1e10, wy=1e10, wz=-1e10, **lens)),
             ("1x1", dict(widthPixel=1, heightPixel=1)), ("1x64_lens", dict(widthPixel=1, heightPixel=64, **lens)),
             ("7.5x7.5", dict(widthPixel=7.5, heightPixel=7.5, **lens)), ("1e9x1e9", dict(widthPixel=1e9, heightPixel=1e9)),
             ("position_1e30", dict(x=1e30, y=-1e30, z=1e30, **lens)), ("position_1e30_pinhole", dict(x=1e30, y=-1e30, z=1e30)),
             ("angle_inf", dict(wy=INF)), ("fstop_nan", dict(fStop=NAN))]
    out = []
    for name, kw in table:
        c = np.zeros((), rd.PhysicalCamera)
        for k, v in dict(base, **kw).items():
            c[k] = v
        out.append((name, c))
    return out


MAY_BE_ALL_NAN = ("angle_inf", "fstop_nan")


def camera_seeds():
    """(96, 3) uint32: four all-zero, four all-0xffffffff, the rest random"""
    r = gc.generate_inputs(N_CAMERA_RAYS, 11)
    r[4:8] = 0xffffffff
    return r


# ---------------------------------------------------------------------------------------------------------------------
# (g) colours for the tone map, frameIDs for the running mean
# ---------------------------------------------------------------------------------------------------------------------
FRAME_IDS = (1, 1 << 24, (1 << 24) + 1, 1 << 31, 0xfffffffe, 0xffffffff)


def tone_values(debug=False):
    """float32 values: 2048 magnitudes log-spaced over 1e-10 .. 1e10 with both signs, then the specials"""
    mag = np.logspace(-10, 10, 2048).astype(F)
    one = F(1.0)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, FLT_MAX, -FLT_MAX, INF, -INF, NAN, 2.0 ** 23, 2.0 ** 24, 8421505.0, 8421504.0,
                        1e7, -1e7, 3e9, -3e9, 2.0 ** 31, 0.5, 1.0 / 255, 254.5 / 255], F)
    special = np.concatenate([special, np.array([0xffc00000, 0x7fc00000, 0xff800001, 0x7f800001], np.uint32).view(F)])     # NaN of both signs
    if debug:
        special = np.concatenate([special, np.array([1.0, np.nextafter(one, F(2.0)), F(256.0) / F(255.0), -0.5, -1.0, 2.0, 255.9 / 255,
                                                     257.0 / 255, 128.5, -128.5, 16909320.0 / 255], F)])
    return np.ascontiguousarray(np.concatenate([mag, -mag, special]), F)


def tone_pixels(debug=False):
    """the values as float4 pixels (rgb from consecutive values, padded with 0.25; w = 7): (npix, 4) float32"""
    v = tone_values(debug)
    npix = (v.shape[0] + 2) // 3
    rgb = np.full(npix * 3, 0.25, F)
    rgb[:v.shape[0]] = v
    out = np.full((npix, 4), 7.0, F)
    out[:, :3] = rgb.reshape(npix, 3)
    return out


TONE_NPIX = tone_pixels(True).shape[0]                  # the frame of (g): TONE_NPIX x 1 pixels


def tone_frame(debug=False):
    """(TONE_NPIX, 4): tone_pixels padded to the frame of (g)"""
    p = tone_pixels(debug)
    out = np.full((TONE_NPIX, 4), 7.0, F)
    out[:, :3] = 0.25
    out[:p.shape[0]] = p
    return out


def mean_frame():
    """the prefilled imageScratch of the running-mean cases: the debug tone frame (every special, both signs, 20 decades)"""
    return tone_frame(True)


def tone_scene(scenes):
    """the smallest scene whose frame is TONE_NPIX x 1: one quad before a pinhole camera"""
    rd = scenes.rd
    s = scenes.Scene("shade_edges_tone")
    s.materials = [_material(rd, (0.7, 0.7, 0.7), 0.0, 0.5, 0.0, 1.45)]
    s.add_instance(s.add_mesh(_quad((0.0, 0.0, 1.0))), scenes.translate(0.0, 0.0, -3.0), 0)
    cam = np.zeros((), rd.PhysicalCamera)
    cam["widthPixel"], cam["heightPixel"] = TONE_NPIX, 1
    cam["focalLength"], cam["sensorWidth"], cam["focalDistance"], cam["fStop"] = 0.05, 0.036, 3.0, 0.0
    s.camera = cam
    sp = np.zeros((), rd.SceneProperties)
    sp["lightCount"][0] = 1
    sp["lights"][0]["direction"] = (0.0, 0.0, -1.0, 0.0)
    sp["lights"][0]["color"] = (1.0, 1.0, 1.0, 1.0)
    s.sceneProps = sp
    s.rtprop = scenes._rtprop(0, 0, 0)
    return s


# ---------------------------------------------------------------------------------------------------------------------
# fixture layout (tests/golden/refgpu_shade_edges.npz); every array is an output of the reference code object
#   blob_sha256                SHA-256 of the edge scene's TLAS blob
#   <batch>/hit                closest-hit flags of the batch (packbits); <batch>/inst, /prim (uint8), /t, /bary of the hits
#   <batch>/pay                `material` payloads of the hits under light buffer 0 (13 words each)
#   light/color                (11, hits of batch "light", 3): payload.color under every light buffer
#   brdf                       (2000, 3): microfacetBRDF of the rows of brdf_grid
#   frame/scratch<f>, image<f> the edge scene's two progressive frames
#   tone/image<debug>          RGBA8 of the tone frame at batchSize 0; mean/<k> imageScratch.rgb after the running-mean frame k
#   cam/o, cam/d               (cameras, 96, 3) rays of generateRay
# ---------------------------------------------------------------------------------------------------------------------
def pack_batch(name, hits, pay):
    k = hits["hit"] == 1
    assert int(hits["instanceIndex"][k].max(initial=0)) < 256 and int(hits["primitiveIndex"][k].max(initial=0)) < 256
    return {name + "/hit": np.packbits(k), name + "/inst": hits["instanceIndex"][k].astype(np.uint8), name + "/prim": hits["primitiveIndex"][k].astype(np.uint8),
            name + "/t": hits["distance"][k].astype(F), name + "/bary": hits["barycentric"][k].astype(F),
            name + "/pay": np.ascontiguousarray(pay[k]).view(np.uint32).reshape(-1, 13)}


def unpack_batch(G, name, n, payload_dtype):
    """-> dict: hit bool (n,), and per hit inst, prim, t, bary, pay (PAYLOAD_DTYPE)"""
    hit = np.unpackbits(G[name + "/hit"])[:n].astype(bool)
    pay = np.ascontiguousarray(G[name + "/pay"]).view(payload_dtype).reshape(-1)
    assert pay.shape[0] == int(hit.sum())
    return dict(hit=hit, inst=G[name + "/inst"].astype(np.int64), prim=G[name + "/prim"].astype(np.int64), t=G[name + "/t"], bary=G[name + "/bary"], pay=pay)


def full_payloads(u, n, payload_dtype):
    """payload records of all n rows of a batch: the fixture's on the hits, zeros on the misses"""
    pay = np.zeros(n, payload_dtype)
    pay[u["hit"]] = u["pay"]
    return pay


def zero_normal_rows(scene, instances, inst, prim, bary):
    """hits on which the reference's interpolated vertex normal is exactly (0, 0, 0) -- `bary.x * n0 + bary.y * n1 + bary.z * n2`
    in float32, left to right (shader.cl:359-361) -- on the meshes of ZERO_NORMAL_SETS: the rows of "What may be left out" """
    out = np.zeros(inst.shape[0], bool)
    for name in ZERO_NORMAL_SETS:
        k = instance_numbers(instances, "normal", name)[0]
        rows = np.flatnonzero(inst == k)
        v, t, n, _ = scene.meshes[scene.instances[k][0]]
        tri = t[prim[rows]]
        b = np.ascontiguousarray(bary[rows], F)
        s = (b[:, 0:1] * n[tri[:, 0]]).astype(F)
        s = (s + (b[:, 1:2] * n[tri[:, 1]]).astype(F)).astype(F)
        s = (s + (b[:, 2:3] * n[tri[:, 2]]).astype(F)).astype(F)
        out[rows] = (s == 0).all(1)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the recordings: what tests/golden/make_golden_gpu.py stores and what the GPU tests recompute where oracle/_ref is present
# ---------------------------------------------------------------------------------------------------------------------
def reference_recordings(ref, rg, rd, scenes):
    """every array of the fixture from the live reference code object `ref` (refgpu_bind.RefGpu; rg = the refgpu_bind module)"""
    out = {}
    s, inst, B = batches(scenes)
    blob = gc.scene_blob(rd, s)
    out["blob_sha256"] = gc.sha(blob)
    rs = rg.RefScene(ref, s, blob)
    L = light_buffers(rd)
    rs.set_props(L[0])
    for name, b in B.items():
        h = rs.trace(b.o, b.d, b.tmin, b.tmax)
        out.update(pack_batch(name, h, rs.material_batch(h, b.d, b.frames, b.depths)))
    b = B["light"]
    h = rs.trace(b.o, b.d, b.tmin, b.tmax)
    k = h["hit"] == 1
    colours = []
    for j in range(L.shape[0]):
        rs.set_props(L[j])
        pay = rs.material_batch(h, b.d, b.frames, b.depths)[k]
        colours.append(pay["color"])
        if j == 0:
            first = pay
        for f in ("nextFactor", "nextRayOrigin", "nextRayDirection"):      # the light decides the colour alone
            assert compare(pay[f], first[f])[0].all(), (j, f)
    out["light/color"] = np.ascontiguousarray(np.stack(colours), F)
    out["brdf"] = np.ascontiguousarray(ref.brdf(brdf_packed(brdf_grid()))[:, :3], F)
    rf = rg.RefScene(ref, s, blob)                          # the scene's own SceneProperties and RTProp: two progressive frames
    for f in range(2):
        rf.frame()
        out["frame/scratch%d" % f], out["frame/image%d" % f] = rf.read_scratch(), rf.read_image()
    ts = tone_scene(scenes)
    rt = rg.RefScene(ref, ts, gc.scene_blob(rd, ts))
    for debug in (0, 1):
        rt.set_rtprop(totalSamples=0, batchSize=0, depth=0, debug=debug)
        rt.write_scratch(tone_frame(bool(debug)))
        rt.raygen()
        assert np.array_equal(bits(rt.read_scratch()), bits(tone_frame(bool(debug)).reshape(-1))), "batchSize 0 changed imageScratch"
        out["tone/image%d" % debug] = rt.read_image()
    for fid in FRAME_IDS:
        rt.set_rtprop(totalSamples=fid, batchSize=1, depth=0, debug=0)
        rt.write_scratch(mean_frame())
        rt.raygen()
        sc = rt.read_scratch().reshape(-1, 4)
        assert np.array_equal(bits(sc[:, 3]), bits(mean_frame()[:, 3]))
        out["mean/%d" % fid], out["mean/image%d" % fid] = np.ascontiguousarray(sc[:, :3]), rt.read_image()
    seeds = camera_seeds()
    co, cd = [], []
    for _, cam in cameras(rd):
        rt.set_camera(cam)
        o, d = rt.generate(seeds)
        co.append(o); cd.append(d)
    out["cam/o"], out["cam/d"] = np.stack(co), np.stack(cd)
    return out


def recordings_differ(a, b):
    """names of the arrays of two recordings that differ: floats under the NaN rule, everything else exactly"""
    bad = [k for k in sorted(set(a) | set(b)) if k not in a or k not in b]
    for k in sorted(set(a) & set(b)):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype:
            bad.append(k)
        elif x.dtype == F:
            if not compare(x.reshape(-1, 1), y.reshape(-1, 1))[0].all():
                bad.append(k)
        elif k.endswith("/pay"):                          # payload words: colours and rays are floats, word 3 is the hit flag
            if not compare(x.view(F).reshape(-1, 1), y.view(F).reshape(-1, 1))[0].all():
                bad.append(k)
        elif not np.array_equal(x, y):
            bad.append(k)
    return bad
