"""CPU suite: the inputs of tests/test_gpu_shade_edges.py are what they claim to be, so that the GPU tests cannot pass by testing
nothing -- and the CPU oracle against the reference's recordings of them (tests/golden/refgpu_shade_edges.npz).

First half: the builders of tests/shade_edge_cases.py (the value tables of the issue, the searched RNG keys, the exact unit vectors).
Second half: coverage counts and caps, evaluated on the reference's answers: every predicate is restated in float64 from the
inputs and the recorded hit (instance, triangle, barycentrics), with a margin where a sign decides.
Third: `OracleRef` / `OracleRefScene` give the CPU oracle the calling convention of refgpu_bind.RefGpu / RefScene, so that
shade_edge_cases.reference_recordings makes the same recordings on the CPU; glibc against OCML on edge inputs is unbounded, so the
bulk bound of test_oracle_brdf_matches_reference_gpu is gated and the worst case is printed.  The gate is the GPU's bit parity.

The two transforms of scale 1e-15 and 1e15 cannot be hit in the reference's arithmetic: intersectTop inverts the instance matrix
in float32 (radiance.cl:166-169), whose determinant 1e-45 / 1e45 rounds to a denormal / to infinity, so 1 / det is infinite /
zero and the local ray is NaN.  They stay in the scene (a quad that poisons nothing), and what is asserted of them is that.
"""
import os
import types

import numpy as np
import pytest

import oracle_bind as ob
import shade_edge_cases as se

F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MIN_ROWS = 16
UNHITTABLE = ("scale1e-15", "scale1e15")


@pytest.fixture(scope="module")
def mods():
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd, scenes
    return rd, scenes


@pytest.fixture(scope="module")
def G():
    return dict(np.load(os.path.join(GOLD, "refgpu_shade_edges.npz")))


@pytest.fixture(scope="module")
def cases(mods):
    return se.batches(mods[1])


# ---- the builders ---------------------------------------------------------------------------------------------------------------
def test_the_edge_scene_holds_the_listed_cases(mods, cases):
    rd, scenes = mods
    s, inst, B = cases
    mats = np.array([m for _, m in se.materials(rd)])
    assert mats.shape[0] >= 60 and len(inst) <= 160 and len(inst) == len(s.instances)
    for field, values in (("roughness", se.ROUGHNESS), ("metallic", se.METALLIC), ("transmission", se.TRANSMISSION), ("ior", se.IOR)):
        have = mats[field]
        for v in values:
            assert (np.isnan(have).any() if np.isnan(v) else (have == F(v)).any()), (field, v)
    a = mats["albedo"][:, :3]
    assert (a == 0).any() and (a == 1).any() and (a > 1).any() and (a < 0).any()
    assert int((mats["normalTexIdx"] == 0).sum()) == 1 and (mats["albedoTexIdx"] == -1).all()
    tex = [n for f, n in inst if f == "material" and n.startswith("normal_tex0")]
    assert tex == ["normal_tex0", "normal_tex0/+x", "normal_tex0/-x"]
    assert [n for f, n in inst if f == "normal"] == [n for n, _ in se.NORMAL_SETS] and len(se.NORMAL_SETS) >= 13
    assert sorted(n for f, n in inst if f == "transform") == sorted(n for n, _, _ in se.transforms(scenes))
    # one instance per Material record but the last ("mid", shared by the other families), in table order
    names = [n for n, _ in se.materials(rd)]
    assert [n for f, n in inst if f == "material"][:len(names) - 1] == names[:-1]
    assert sum(b.n for k, b in B.items() if k != "light") <= 5000
    assert set(B["main"].cls.tolist()) == set(range(6)) and (B["s-25"].cls == 6).all() and (B["s+25"].cls == 7).all()
    assert B["s-25"].tmax == float(F(1000.0) / F(1e-25)) and B["s+25"].tmin == float(F(0.001) / F(1e25))


def test_the_normal_space_threshold_is_probed_on_either_side(cases):
    s, inst, _ = cases
    for name, want in (("+x", 0.0), ("-x", 0.0), ("+x_5e-7", 5e-7), ("+x_2e-6", 2e-6), ("-x_5e-7", 5e-7), ("-x_2e-6", 2e-6)):
        k = se.instance_numbers(inst, "normal", name)[0]
        n = s.meshes[s.instances[k][0]][2][0].astype(np.float64)
        gap = 1.0 - abs(n[0]) / np.linalg.norm(n)
        assert abs(gap - want) < 0.02 * max(want, 1e-9), (name, gap)
        assert abs(gap - 1e-6) > 4e-7                   # float32 resolves 1 - |N.x| to 6e-8: the side is not in doubt


def test_every_searched_key_has_its_property():
    frames, depths, kind = se.key_rows()
    n = frames.shape[0]
    assert n == len(se.KEY_KINDS) * se.ROWS_PER_KIND and se.ROWS_PER_KIND >= MIN_ROWS
    rnd = ob.pcg3d(np.stack([frames, np.arange(n, dtype=np.uint32), depths.view(np.uint32)], 1))
    for k, name in enumerate(se.KEY_KINDS[:se.N_SEARCHED]):
        ok = se.key_property(name, rnd[kind == k])
        assert ok.all(), (name, rnd[kind == k][~ok])
    k = np.array(se.KEY_KINDS)[kind]
    assert (frames[k == "frame_ffffffff"] == 0xffffffff).all() and (depths[k == "depth_ffffffff"] == -1).all()
    assert (frames[k == "both_ffffffff"] == 0xffffffff).all() and (depths[k == "both_ffffffff"] == -1).all()


def test_the_directions_of_the_brdf_grid_are_left_alone_by_normalize():
    g = se.brdf_grid()
    for v in (g["L"], g["V"]):
        assert (se._dot3_f32(v) == F(1.0)).all() and np.unique(v, axis=0).shape[0] == v.shape[0]
    assert g["L"].shape == (se.N_BRDF_L, 3) and g["V"].shape == (se.N_BRDF_V, 3) and (np.diff(g["l"]) >= 0).all()
    n = np.linalg.norm(g["N"].astype(np.float64), axis=1)
    assert n.min() >= 0.49 and n.max() <= 2.01          # no normal small enough for GetNormalSpace's determinant to underflow
    assert np.isnan(g["roughness"]).any() and (g["roughness"] == -1).any() and (g["roughness"] == 2).any() and (g["metallic"] == 5).any()
    assert ((g["N"] == F([1, 0, 0])).all(1)).sum() >= MIN_ROWS and ((g["N"] == F([-1, 0, 0])).all(1)).sum() >= MIN_ROWS
    rng = np.random.default_rng(3)
    v = rng.normal(size=(4096, 3)); v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
    print("share of random float32 unit vectors whose restated squared length is exactly 1: %.3f" % float((se._dot3_f32(v) == F(1.0)).mean()))


def test_lights_cameras_colours_and_frame_ids(mods):
    rd, _ = mods
    V = se.light_variants()
    L = se.light_buffers(rd)
    assert L.shape[0] == len(V) == 11 and V[0][0] == "own"
    for j in range(L.shape[0]):                          # every variant sits in slot 0 of one buffer and in the slots 1 .. 4 of four others
        for k in range(5):
            want = np.array(V[(j + k) % len(V)][1] + (0.0,), F)
            assert np.array_equal(se.bits(L[j]["lights"][k]["direction"]), se.bits(want))
    d = np.array([v[1] for v in V], np.float64)
    c = np.array([v[2] for v in V], np.float64)
    assert (d == 0).all(1).any() and (np.abs(d).max(1) < 1e-29).sum() == 2 and (np.abs(d).max(1) > 1e29).sum() == 2
    assert (c == 0).all(1).any() and (c < 0).any() and np.isinf(c).any() and np.isnan(c).any()
    cams = se.cameras(rd)
    assert 22 <= len(cams) <= 28 and [n for n, _ in cams][-2:] == list(se.MAY_BE_ALL_NAN)
    rec = np.array([cm for _, cm in cams])
    for field, values in (("fStop", (0.0, 1e-30, 1e30, -2.8, np.inf)), ("focalLength", (0.0,)), ("sensorWidth", (0.0, -0.036)),
                          ("focalDistance", (0.0, 1e30)), ("wx", (0.0, se.PI_2, 1e6, 1e10)), ("widthPixel", (1.0, 7.5, 1e9)), ("x", (1e30,))):
        for v in values:
            assert (rec[field] == F(v)).any(), (field, v)
    seeds = se.camera_seeds()
    assert not seeds[:4].any() and (seeds[4:8] == 0xffffffff).all() and se.N_CAMERA_RAYS > 16 * 12 // 4
    assert sum(se.N_CAMERA_RAYS > int(r["widthPixel"]) * int(r["heightPixel"]) for r in rec) >= 3       # pixel numbers run off the small frames
    for debug in (False, True):
        v = se.tone_values(debug)
        fin = v[np.isfinite(v)]
        assert v.shape[0] >= 4096 and (fin > 0).sum() >= 2048 and (fin < 0).sum() >= 2048
        assert abs(fin).max() == F(se.FLT_MAX) and np.isinf(v).sum() == 2 and np.isnan(v).sum() >= 5
        assert (np.signbit(v) & np.isnan(v)).any() and (~np.signbit(v) & np.isnan(v)).any() and (se.bits(v) == 0x80000000).any()
        assert ((v != 0) & (np.abs(v) < 1e-38)).sum() >= 3 and (np.abs(fin.astype(np.float64)) * 255 > 2.0 ** 31).sum() >= 4
    dv = se.tone_values(True)
    for x in (1.0, np.nextafter(F(1.0), F(2.0)), F(256.0) / F(255.0), -0.5, -1.0):
        assert (dv == F(x)).any(), x
    assert se.FRAME_IDS == (1, 2 ** 24, 2 ** 24 + 1, 2 ** 31, 0xfffffffe, 0xffffffff)
    assert se.tone_frame(True).shape == se.tone_frame(False).shape == (se.TONE_NPIX, 4)


# ---- coverage and caps, on the reference's answers ---------------------------------------------------------------------------------
def _unit(v):
    return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-300)


class Rows:
    """every hit row of the fixture's batches main, s-25, s+25 and keys with what the predicates need, float64"""

    def __init__(self, rd, cases, G):
        s, inst, B = cases
        self.inst_names = inst
        mats = np.array(s.materials)
        info = s.buffers()["meshInfo"]
        cols = {k: [] for k in ("batch", "inst", "N", "V", "rnd", "cls", "nan", "left_out", "color", "kind")}
        L = _unit(-np.array(se.LIGHT_DIRECTION, np.float64)[None])[0]
        for name in ("main", "s-25", "s+25", "keys"):
            b = B[name]
            u = se.unpack_batch(G, name, b.n, ob.PAYLOAD_DTYPE)
            h = u["hit"]
            m = int(h.sum())
            rnd = ob.pcg3d(np.stack([b.frames, b.pixels, b.depths.view(np.uint32)], 1))[h]
            nrm = np.zeros((m, 3))
            for r in range(m):
                mi, tf, _ = s.instances[int(u["inst"][r])]
                v, t, n, _ = s.meshes[mi]
                tri = t[int(u["prim"][r])]
                nl = (u["bary"][r].astype(np.float64)[:, None] * n[tri].astype(np.float64)).sum(0)
                nrm[r] = np.asarray(tf, np.float64)[:3, :3] @ nl
            pay = u["pay"]
            cols["batch"].append(np.full(m, name)); cols["inst"].append(u["inst"]); cols["N"].append(_unit(nrm))
            cols["V"].append(_unit(-b.d[h].astype(np.float64))); cols["rnd"].append(rnd.astype(np.float64)); cols["cls"].append(b.cls[h])
            cols["nan"].append(se.nan_rows(pay["color"], pay["nextFactor"], pay["nextRayOrigin"], pay["nextRayDirection"]))
            cols["left_out"].append(se.zero_normal_rows(s, inst, u["inst"], u["prim"], u["bary"]))
            cols["color"].append(pay["color"])
            kind = np.full(m, -1)
            if name == "keys":
                kind = se.key_rows()[2][h]
            cols["kind"].append(kind)
        for k, v in cols.items():
            setattr(self, k, np.concatenate(v))
        self.n = self.inst.shape[0]
        self.mat = mats[info["materialIndex"][self.inst]]
        self.family = np.array([inst[k][0] for k in self.inst])
        self.name = np.array([inst[k][1] for k in self.inst])
        self.L = L
        with np.errstate(invalid="ignore"):
            tr = np.clip(np.nan_to_num(self.mat["transmission"].astype(np.float64)), 0, 1)
        x, y, z = self.rnd.T
        self.lower = z < 0.5
        self.transm = self.lower & (2 * z < tr)
        self.diffuse = self.lower & ~self.transm
        self.specular = ~self.lower
        self.plain_normal = (self.mat["normalTexIdx"] == -1) & (np.linalg.norm(self.N, axis=1) > 0.5)
        self.VN = (self.V * self.N).sum(1)


@pytest.fixture(scope="module")
def rows(mods, cases, G):
    return Rows(mods[0], cases, G)


def test_every_instance_group_is_hit(rows):
    R = rows
    for k, (family, name) in enumerate(R.inst_names):
        n = int((R.inst == k).sum())
        if family == "transform" and name in UNHITTABLE:
            assert n == 0, (name, n)                   # see the module docstring
        elif family != "aux":
            assert n >= MIN_ROWS, (family, name, n)
    assert R.n >= 2000


def test_every_lobe_and_special_case_has_rows(rows):
    R = rows
    sure = R.plain_normal & (np.abs(R.VN) > 1e-4)
    counts = {"diffuse lobe": int(R.diffuse.sum()), "specular lobe": int(R.specular.sum()),
              "transmission lobe from outside": int((R.transm & sure & (R.VN > 0)).sum()),
              "transmission lobe from inside": int((R.transm & sure & (R.VN < 0)).sum())}
    # total internal reflection in refract3: H of the sampled microfacet normal restated in float64 (GetNormalSpace, then the
    # GGX angle); counted where 1 - sin2Theta_t is below zero by a margin
    with np.errstate(invalid="ignore", divide="ignore"):
        rough = np.clip(np.nan_to_num(R.mat["roughness"].astype(np.float64)), 0, 1)
        ior = np.clip(np.nan_to_num(R.mat["ior"].astype(np.float64)), 0, 10)
        fn = np.where((R.VN < 0)[:, None], -R.N, R.N)
        eta = np.where(R.VN < 0, 1.0 / ior, ior)
        special = 1.0 - np.abs(fn[:, 0]) <= 1e-6
        t = np.where(special[:, None], np.array([0.0, 1.0, 0.0]), _unit(np.cross(np.array([1.0, 0.0, 0.0]), fn)))
        bt = np.cross(fn, t)
        x, y, _ = R.rnd.T
        a = rough * rough
        theta = np.arccos(np.sqrt(np.clip((1 - y) / (1 + (a * a - 1) * y), 0, 1)))
        phi = 2 * np.pi * x
        H = t * (np.sin(theta) * np.cos(phi))[:, None] + bt * (np.sin(theta) * np.sin(phi))[:, None] + fn * np.cos(theta)[:, None]
        ci = (H * R.V).sum(1)
        s2t = np.maximum(0.0, 1 - ci * ci) / (eta * eta)
        tir = R.transm & sure & np.isfinite(s2t) & (1 - s2t < -1e-3)
    counts["total internal reflection, inside at ior 10"] = int((tir & (R.VN < 0) & (R.mat["ior"] == 10)).sum())
    counts["total internal reflection, outside at ior 0.5"] = int((tir & (R.VN > 0) & (R.mat["ior"] == 0.5)).sum())
    gap = 1.0 - np.abs(R.N[:, 0])
    facing = R.plain_normal
    counts["GetNormalSpace special case"] = int((facing & (gap < 1e-6 - 4e-7)).sum())
    counts["just inside the 1e-6 threshold (5e-7)"] = int((facing & (np.abs(gap - 5e-7) < 1e-7)).sum())
    counts["just outside the 1e-6 threshold (2e-6)"] = int((facing & (np.abs(gap - 2e-6) < 1e-7)).sum())
    for k, name in enumerate(se.KEY_KINDS):
        counts["key " + name] = int((R.kind == k).sum())
    # the shadow test: a diffuse surface that faces the light and the viewer shows the direct term, or the ambient term alone
    albedo = R.mat["albedo"][:, :3]
    plainmat = (R.family == "material") & R.plain_normal & (R.mat["metallic"] < 1) & (R.mat["transmission"] < 1) & (albedo > 0).all(1)
    shows = plainmat & ((R.N * R.L).sum(1) > 1e-2) & (R.VN > 1e-2) & (R.batch == "main")
    ambient = (np.zeros(3, F) + (albedo * F(0.1)).astype(F)).astype(F)
    is_ambient = (se.bits(R.color) == se.bits(ambient)).all(1)
    counts["shadow test: lit"] = int((shows & ~is_ambient).sum())
    counts["shadow test: occluded"] = int((shows & is_ambient).sum())
    for k, v in counts.items():
        print("%-50s %5d rows" % (k, v))
    few = {k: v for k, v in counts.items() if v < MIN_ROWS}
    assert not few, few


def test_caps_on_nan_rows_and_rows_left_out(mods, rows, G):
    rd, _ = mods
    R = rows
    shares = {"family " + f: float(R.nan[R.family == f].mean()) for f in ("material", "normal", "transform")}
    for c, name in enumerate(se.CLASSES):
        shares["class " + name] = float(R.nan[R.cls == c].mean())
    shares["keys"] = float(R.nan[R.batch == "keys"].mean())
    shares["lights"] = float(se.nan_rows(G["light/color"].reshape(-1, 3)).mean())
    shares["brdf grid"] = float(se.nan_rows(G["brdf"]).mean())
    cam = se.nan_rows(G["cam/o"].reshape(-1, 3), G["cam/d"].reshape(-1, 3)).reshape(G["cam/o"].shape[:2])
    names = [n for n, _ in se.cameras(rd)]
    all_nan = [names[k] for k in range(len(names)) if cam[k].all()]
    assert len(all_nan) <= 2 and set(all_nan) <= set(se.MAY_BE_ALL_NAN), all_nan
    shares["cameras"] = float(cam.mean())
    shares["frames"] = float(np.mean([se.nan_rows(G["frame/scratch%d" % f].reshape(-1, 4)).mean() for f in range(2)]))
    shares["running mean"] = float(np.mean([se.nan_rows(G["mean/%d" % k]).mean() for k in se.FRAME_IDS]))
    total = [R.nan, se.nan_rows(G["light/color"].reshape(-1, 3)), se.nan_rows(G["brdf"]), cam.reshape(-1)] + \
            [se.nan_rows(G["frame/scratch%d" % f].reshape(-1, 4)) for f in range(2)] + [se.nan_rows(G["mean/%d" % k]) for k in se.FRAME_IDS]
    overall = float(np.concatenate(total).mean())
    for k, v in shares.items():
        print("NaN rows, %-24s %.4f" % (k, v))
    print("NaN rows overall %.4f; rows left out %d of %d hits (%.4f); all-NaN cameras %s" % (overall, int(R.left_out.sum()), R.n, float(R.left_out.mean()), all_nan))
    assert max(shares.values()) <= 0.25, shares
    assert overall <= 0.10
    assert R.left_out.mean() <= 0.05
    assert R.left_out[R.name == "zero"].all() and not R.left_out[~np.isin(R.name, se.ZERO_NORMAL_SETS)].any()


def test_fixture_size():
    size = os.path.getsize(os.path.join(GOLD, "refgpu_shade_edges.npz"))
    largest = max(os.path.getsize(os.path.join(GOLD, f)) for f in os.listdir(GOLD) if f != "refgpu_shade_edges.npz")
    assert size <= largest, (size, largest)


# ---- the CPU oracle through the calling convention of refgpu_bind ------------------------------------------------------------------
class OracleRef:
    def brdf(self, packed19):
        x = np.ascontiguousarray(packed19, F).reshape(-1, 19)
        L = ob.lib()
        out = np.zeros((x.shape[0], 9), F)
        for i in range(x.shape[0]):
            r, f, nf, nd = x[i], np.zeros(3, F), np.zeros(3, F), np.zeros(3, F)
            L.orc_microfacet_brdf(r[0:3].ctypes.data, r[3:6].ctypes.data, r[6:9].ctypes.data, r[9:12].ctypes.data,
                                  float(r[12]), float(r[13]), float(r[14]), float(r[15]), f.ctypes.data)
            L.orc_sample_brdf_transm(r[3:6].ctypes.data, r[6:9].ctypes.data, r[9:12].ctypes.data, float(r[12]), float(r[13]),
                                     float(r[14]), float(r[15]), r[16:19].ctypes.data, nf.ctypes.data, nd.ctypes.data)
            out[i] = np.concatenate([f, nd, nf])
        return out


class OracleRefScene:
    def __init__(self, ref, scene, blob):
        self.osc = ob.OracleScene(scene, blob)
        self.blob = bytes(blob)

    def trace(self, o, d, tmin=0.001, tmax=1000.0, sbtRecordOffset=1):
        return ob.trace_batch(self.blob, o, d, tmin, tmax, sbtRecordOffset)

    def material_batch(self, hits, ray_dirs, frame_ids, depths):
        n = np.asarray(hits).shape[0]
        return self.osc.material_batch(hits, ray_dirs, np.arange(n, dtype=np.uint32), frame_ids, depths)

    def set_props(self, sp):
        self.osc.sceneProps[0] = np.array(sp).reshape(1)[0]

    def set_camera(self, cam):
        self.osc.camera[0] = np.array(cam).reshape(1)[0]

    def set_rtprop(self, **kw):
        self.osc.set_rtprop(**kw)

    def write_scratch(self, values):
        self.osc.scratch[:] = np.ascontiguousarray(values, F).reshape(-1)

    def raygen(self):
        self.osc.render()

    def frame(self):
        self.osc.frame()

    def read_scratch(self):
        return self.osc.scratch.copy()

    def read_image(self):
        return self.osc.image.copy()

    def generate(self, rand3):
        r = np.ascontiguousarray(rand3, np.uint32).reshape(-1, 3)
        return self.osc.generate_rays(np.arange(r.shape[0], dtype=np.uint32), r)


def oracle_recordings(rd, scenes):
    with np.errstate(all="ignore"):
        return se.reference_recordings(OracleRef(), types.SimpleNamespace(RefScene=OracleRefScene), rd, scenes)


def test_oracle_against_the_reference_recordings(mods, G):
    """hit flags, instances and triangles of every batch exactly; on the values finite in both, the 0.99 quantile of the relative
    error below 2e-5 (the bulk bound of test_oracle_brdf_matches_reference_gpu); worst case and NaN / inf agreement printed"""
    rd, scenes = mods
    O = oracle_recordings(rd, scenes)
    assert set(O) == set(G)
    for name in ("main", "s-25", "s+25", "keys", "light"):
        for f in ("hit", "inst", "prim"):
            assert np.array_equal(O["%s/%s" % (name, f)], G["%s/%s" % (name, f)]), (name, f)
    assert np.array_equal(O["blob_sha256"], G["blob_sha256"])
    for key in sorted(G):
        if key.endswith(("/hit", "/inst", "/prim")) or key == "blob_sha256" or G[key].dtype == np.uint8:
            continue
        got, want = (a.view(F) if a.dtype == np.uint32 else a for a in (np.ascontiguousarray(O[key]), np.ascontiguousarray(G[key])))
        if key.endswith("/pay"):
            got, want = np.delete(got, 3, 1), np.delete(want, 3, 1)         # word 3 is the hit flag
        got, want = got.astype(np.float64).reshape(-1), want.astype(np.float64).reshape(-1)
        both = np.isfinite(got) & np.isfinite(want)
        same_class = (np.isnan(got) == np.isnan(want)) & (np.isinf(got) == np.isinf(want))
        rel = np.abs(got[both] - want[both]) / np.maximum(1.0, np.abs(want[both]))
        q = float(np.quantile(rel, 0.99)) if rel.size else 0.0
        print("%-16s %7d values, finite in both %.4f, NaN / inf class agrees on %.4f, rel. error: 0.99 quantile %.3g, worst %.3g"
              % (key, got.size, float(both.mean()), float(same_class.mean()), q, float(rel.max()) if rel.size else 0.0))
        assert q < 2e-5, (key, q)
    for key in sorted(G):
        if G[key].dtype == np.uint8 and "image" in key:
            d = np.abs(O[key].astype(np.int32) - G[key].astype(np.int32))
            print("%-16s %7d bytes, equal on %.4f, worst difference %d" % (key, d.size, float((d == 0).mean()), int(d.max())))
