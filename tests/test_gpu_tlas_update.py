"""GPU suite (-m gpu): rd.UpdateAccelStruct (rdx_tlas_update) -- other transforms for the instances of a built TLAS, in place.

Per scene of tests/tlas_update_cases.py: build once, then step through [B, A, C, orig] (each move on top of the last).  After
every step
  * the blob read back, and its size, equal the CPU oracle's builder's blob of the stepped instances (not the product's builder);
  * rd.QueryRays, closest and any hit, equals the reference's own device code run live on that blob (refgpu_bind.RefGpu.trace;
    that leg alone is left out where oracle/_ref was not built, and on `singular`, whose matrix without inverse the reference
    leaves undefined) and the CPU oracle (oracle_bind.trace_batch) -- on a batch of
    8192 rays, a quarter aimed at the touched instance's new world box, a quarter at its old one, half scattered over the
    scene, fixed seed; on c2_small under kernel {0, 1, 2, 3} x cull {0, 1} x quad {0, 1};
  * the frame (64 x 36, 2 spp, depth 3): imageScratch bit-identical to the reference's raygen on the stepped blob (not on
    `sbt_offset`, where the reference's own picture is undefined) and to a fresh DeviceScene built with the stepped transforms;
  * where the update was incremental (path 1): bytes_h2d <= 4096 + 1024 * instances.
Free device memory is read with hipMemGetInfo through the HIP runtime the library itself uses (refgpu_bind.hip()), not through
torch: a second runtime client initialised after the library is what tests/test_gpu_ray_query.py moves into a child process.
"""
import ctypes as C
import os

import numpy as np
import pytest

import accel_layout_cases as alc
import oracle_bind as ob
import ray_edge_cases as rec
import ray_query_cases as rq
import refgpu_bind as rg
import tlas_update_cases as tu

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_RAYS = 8192
DEFAULTS = {"kernel": 3, "cull": -1, "quad": 1}
MATRIX = [{"kernel": k, "cull": c, "quad": q} for k in (0, 1, 2, 3) for c in (0, 1) for q in (0, 1)]
FIELDS = ("distance", "primitiveIndex", "instanceIndex", "instanceCustomIndex", "instanceSBTOffset", "barycentric", "hitPoint", "transform")


@pytest.fixture(scope="module")
def mods(gpu):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd, scenes
    return rd, scenes


@pytest.fixture(scope="module")
def ref(gpu):
    return rg.RefGpu("p") if rg.available("p") else None


def gpu_scene(scenes, name):
    """the scene of accel_layout_cases.scene(name) with a 64 x 36 camera, 2 spp, depth 3 (bare cases get a camera, a light and
    one material per custom id)"""
    if name == "c1_small":
        return scenes.c1_cornell(64, 36, 2, 3, sphere_subdiv=3)
    if name == "c2_small":
        return scenes.c2_atrium(64, 36, 2, 3, detail=0.2)
    if name == "atrium_400":
        return scenes.c2_atrium_400(64, 36, 2, 3, detail=0.3)
    s = alc.scene(name)
    nmat = 1 + max(mat for _, _, mat in s.instances)
    s.materials = [scenes.material((0.25 + 0.07 * (k % 9), 0.8 - 0.06 * (k % 7), 0.3 + 0.05 * (k % 5)), 0.1 * (k % 3), 0.4 + 0.05 * (k % 4)) for k in range(nmat)]
    s.camera = scenes.blender_camera(64, 36, 0.05, 0.036, 12.0, 0.0, (1.0, 12.0, 2.5), (-100.0, 180.0, 0.0))
    s.sceneProps = scenes.blender_dir_light(-45.0, 20.0, 5.0)
    s.rtprop = scenes._rtprop(0, 2, 3)
    return s


def with_instances(scenes, s, insts):
    """a scenes.Scene like s with the instance list of a step"""
    t = scenes.Scene(s.name)
    t.meshes, t.materials, t.camera, t.sceneProps, t.rtprop = s.meshes, s.materials, s.camera, s.sceneProps, s.rtprop
    for mi, tf, sbt, mat in insts:
        t.add_instance(mi, tf, mat, sbt)
    return t


def aimed(rng, lo, hi, n):
    """n rays from points around the box [lo, hi] at points inside it (float64, rounded)"""
    c, r = (lo + hi) / 2, max(float(np.linalg.norm(hi - lo)) / 2, 1e-3)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    eye = c + v * r * rng.uniform(1.5, 4.0, (n, 1))
    d = rng.uniform(lo, hi, (n, 3)) - eye
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return eye, d


def scattered(rng, lo, hi, n):
    """n rays over the whole scene the way ray_edge_cases.own_primary_rays makes them: from one point outside the bounds through
    a jittered cloud around the centre"""
    c, r = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
    eye = c + np.array([0.3, 0.45, 1.0]) / np.linalg.norm([0.3, 0.45, 1.0]) * 2.5 * r
    d = c + rng.uniform(-1, 1, (n, 3)) * (hi - lo) * 0.55 - eye
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.tile(eye, (n, 1)), d


def batch(seed, new_box, old_box, bounds):
    rng = np.random.default_rng(seed)
    parts = [aimed(rng, *new_box, N_RAYS // 4), aimed(rng, *old_box, N_RAYS // 4), scattered(rng, *bounds, N_RAYS // 2)]
    o = np.ascontiguousarray(np.concatenate([p[0] for p in parts]), np.float32)
    d = np.ascontiguousarray(np.concatenate([p[1] for p in parts]), np.float32)
    rays = np.zeros(N_RAYS, rq.RAY_DTYPE)
    rays["origin"], rays["direction"], rays["tmin"], rays["tmax"] = o, d, 0.001, 1000.0
    return o, d, rays


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1)


class Ctx:
    """one scene on the device and, per step, what the checks compare against -- computed once, from the oracle's blob"""

    def __init__(self, rd, scenes, ref, name, shader_text=None):
        self.rd, self.scenes, self.ref, self.name = rd, scenes, ref, name
        self.s = gpu_scene(scenes, name)
        self.dev = scenes.DeviceScene(self.s, shader_text=shader_text) if shader_text else scenes.DeviceScene(self.s)
        self.plt = self.dev.plt
        self.insts = tu.instances(self.s)
        self.n = len(self.insts)
        self.oblases = [ob.OracleBlas(m[0], m[1]) for m in self.s.meshes]
        self.blob0 = tu.oracle_blob(self.insts, self.oblases)
        self.bounds = rec.world_bounds(self.s)
        self.bRays = rd.CreateBuffer(self.plt, N_RAYS * 32)
        self.bHits = rd.CreateBuffer(self.plt, N_RAYS * 32)
        self.steps = []
        prev_blob = self.blob0
        for k, (step, insts, touched) in enumerate(tu.stepped(self.insts)):
            blob = tu.oracle_blob(insts, self.oblases)
            o, d, rays = batch(1000 + k, tu.world_box(blob, self.n, touched), tu.world_box(prev_blob, self.n, touched), self.bounds)
            w = {}
            for kind in (1, 2):
                w["orc%d" % kind] = ob.trace_batch(blob, o, d, sbtRecordOffset=kind)
                w["orc_prev%d" % kind] = ob.trace_batch(prev_blob, o, d, sbtRecordOffset=kind)
                if ref is not None and self.ref_defined(insts) and self.ref_defined(tu.blob_insts_of(prev_blob, self.n)):
                    w["ref%d" % kind] = ref.trace(rg.DevBuf.of(np.frombuffer(blob, np.uint8)), o, d, 0.001, 1000.0, kind)
                    w["ref_prev%d" % kind] = ref.trace(rg.DevBuf.of(np.frombuffer(prev_blob, np.uint8)), o, d, 0.001, 1000.0, kind)
            self.steps.append(dict(step=step, insts=insts, touched=touched, blob=blob, o=o, d=d, rays=rays, want=w))
            prev_blob = blob

    @staticmethod
    def ref_defined(insts):
        """does the reference define what rays do with these instances?  Not where a matrix has no inverse: its InverseMat4x4
        leaves the result unwritten (math.cl:56-183; the product and the oracle define it as zeros) -- the
        oracle is the comparand there"""
        return all(np.linalg.det(np.asarray(tf, np.float64).reshape(4, 4)) != 0.0 for _, tf, _, _ in insts)

    def read_blob(self):
        t = self.dev.topAccelStruct
        return self.rd.ReadBuffer(self.plt, t, t.size).tobytes()

    def update(self, insts):
        rd = self.rd
        rd.UpdateAccelStruct(self.plt, self.dev.topAccelStruct, tu.rd_instances(rd, insts, self.dev.blas))
        return rd.GetTlasUpdateStats()

    def query(self, rays, kind):
        rd = self.rd
        rd.WriteBuffer(self.plt, self.bRays, N_RAYS * 32, rays)
        rd.WriteBuffer(self.plt, self.bHits, N_RAYS * 32, np.full(N_RAYS * 8, 0xA5A5A5A5, np.uint32))
        rd.QueryRays(self.dev.topAccelStruct, self.bRays, N_RAYS, kind, self.bHits)
        return rd.ReadBuffer(self.plt, self.bHits, N_RAYS * 32).view(rq.RAY_HIT_DTYPE).reshape(-1)

    def check_preconditions(self, st):
        """from the reference's answers alone (the oracle's where the reference's code object is absent): the batch looks at the
        touched instance and sees the step"""
        src = "ref" if "ref1" in st["want"] else "orc"
        now, before = st["want"][src + "1"], st["want"][src + "_prev1"]
        on = int(((now["hit"] == 1) & (now["instanceIndex"] == st["touched"])).sum())
        changed = int(rq.mismatches(rq.query_records(now), rq.query_records(before)).sum())
        print("%s step %s: %d rays end on instance %d, %d answers differ from the step before" % (self.name, st["step"], on, st["touched"], changed))
        m = np.asarray(st["insts"][st["touched"]][1], np.float64)
        if np.linalg.det(m) == 0.0:
            # an instance whose matrix has no inverse is never hit, by the reference's own answers, wherever it is moved (case
            # `singular`, move A): the step can change no answer, and the checks below hold the product to exactly that
            assert on == 0 and changed == 0, (self.name, st["step"], on, changed)
            return
        assert on >= 64 and changed >= 64, (self.name, st["step"], on, changed)

    def check_blob(self, st):
        got = self.read_blob()
        assert self.dev.topAccelStruct.size == len(st["blob"]) == self.rd._lib.lib().rdx_buffer_size(self.dev.topAccelStruct.handle)
        assert got == st["blob"], "%s step %s: the blob read back differs from the oracle builder's" % (self.name, st["step"])

    def check_queries(self, st, tag=""):
        for kind in (1, 2):
            got = self.query(st["rays"], kind)
            for src in ("ref", "orc"):
                h = st["want"].get("%s%d" % (src, kind))
                if h is None:
                    continue
                want = rq.query_records(h) if kind == 1 else rq.any_records(h["hit"].astype(np.uint32))
                bad = rq.mismatches(want, got)
                if bad.any():
                    i = int(np.flatnonzero(bad)[0])
                    raise AssertionError("%s step %s %s kind %d vs %s: %d of %d records differ; first: ray %d want %r got %r"
                                         % (self.name, st["step"], tag, kind, src, int(bad.sum()), N_RAYS, i, want[i].tolist(), got[i].tolist()))

    def check_frame(self, st):
        dev = self.dev
        dev.bind()
        dev.set_rtprop(totalSamples=0); dev.clear_scratch()
        dev.render()
        got = dev.read_scratch().reshape(-1).copy()
        # (instances with an SBT offset: the reference's picture is undefined -- a shadow ray that hits one dispatches row 3, which
        # has no hit shader, and the reference reads its payload uninitialised; tests/test_gpu_reference.py
        # test_instance_sbt_offset_like_the_reference says so -- the fresh scene below is the comparand there)
        if self.ref is not None and self.ref_defined(st["insts"]) and not any(sbt for _, _, sbt, _ in st["insts"]):
            rs = rg.RefScene(self.ref, self.s, st["blob"])
            rs.frame()
            assert np.array_equal(got.view(np.uint32), rs.read_scratch().view(np.uint32)), "%s step %s: frame differs from the reference's" % (self.name, st["step"])
        fresh = self.scenes.DeviceScene(with_instances(self.scenes, self.s, st["insts"]))
        fresh.render()
        assert np.array_equal(got.view(np.uint32), fresh.read_scratch().reshape(-1).view(np.uint32)), "%s step %s: frame differs from a fresh scene's" % (self.name, st["step"])
        dev.bind()

    def check_stats(self, stats, st):
        print("%s step %s: path %d, top nodes %d -> %d, h2d %d B, d2d %d B, %d owner words, host %.3f ms, device %.3f ms"
              % (self.name, st["step"], stats.path, stats.top_nodes_before, stats.top_nodes_after, stats.bytes_h2d, stats.bytes_d2d,
                 stats.tri_slots_rewritten, stats.ms_host, stats.ms_device))
        assert stats.path in (0, 1, 2)
        assert stats.top_nodes_after == tu.top_nodes(st["blob"])
        if stats.path == 1:
            assert stats.bytes_h2d <= 4096 + 1024 * self.n, (stats.bytes_h2d, self.n)


@pytest.fixture(scope="module")
def ctx(mods, ref):
    rd, scenes = mods
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Ctx(rd, scenes, ref, name)
        return cache[name]
    return get


@pytest.mark.parametrize("name", tu.SCENES)
def test_steps_under_default_options(ctx, mods, name):
    rd, _ = mods
    c = ctx(name)
    assert c.read_blob() == c.blob0
    c.query(c.steps[0]["rays"], 1)                  # a layout is derived before the first update
    paths = []
    for st in c.steps:
        c.check_preconditions(st)
        stats = c.update(st["insts"])
        paths.append(stats.path)
        c.check_stats(stats, st)
        c.check_blob(st)
        c.check_queries(st)
        c.check_frame(st)
    assert c.read_blob() == c.blob0                 # the step `orig` restores the blob byte for byte
    assert all(p in (1, 2) for p in paths), paths
    if name in ("shared_blas", "c2_small"):
        assert paths == [1, 1, 1, 1], paths
    if name == "atrium_400":
        # the unified tree goes with the first non-identity instance and is back after `orig`
        assert rd.DebugAccelLayout(c.read_blob())[0]["unifiedRoot"] > 0
        assert rd.DebugAccelLayout(c.steps[1]["blob"])[0]["unifiedRoot"] == 0 and paths[1] in (1, 2)


@pytest.mark.parametrize("cfg", MATRIX, ids=lambda c: "k%d-cull%d-quad%d" % (c["kernel"], c["cull"], c["quad"]))
def test_c2_small_option_matrix(ctx, mods, cfg):
    rd, _ = mods
    c = ctx("c2_small")
    try:
        for k, v in cfg.items():
            rd.SetOption(k, v)
        tag = " ".join("%s %d" % kv for kv in cfg.items())
        for st in c.steps:
            stats = c.update(st["insts"])
            c.check_stats(stats, st)
            c.check_blob(st)
            c.check_queries(st, tag)
    finally:
        for k in cfg:
            rd.SetOption(k, DEFAULTS[k])
        c.update(c.insts)


def test_update_before_any_layout_is_blob_only(mods):
    """path 0: nothing had been traced against the TLAS yet; the first query then derives the layout of the updated blob"""
    rd, scenes = mods
    c = Ctx(rd, scenes, None, "group_rotated")
    st = c.steps[0]
    stats = c.update(st["insts"])
    assert stats.path == 0 and stats.tri_slots_rewritten == 0
    c.check_blob(st)
    c.check_queries(st)


def _free_bytes():
    free, total = C.c_size_t(0), C.c_size_t(0)
    h = rg.hip()
    h.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    assert h.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_fifty_updates_lose_no_device_memory(ctx):
    """B and `orig` in turn: every update moves the blob to an allocation of another size and rewrites the owner words"""
    c = ctx("c2_small")
    b, o = c.steps[0], c.steps[3]
    c.update(b["insts"])
    c.query(b["rays"], 1)
    first = _free_bytes()
    for k in range(50):
        st = o if k % 2 == 0 else b
        stats = c.update(st["insts"])
        assert stats.path == 1 and stats.bytes_d2d > 0
        if k % 10 == 0:
            c.query(st["rays"], 1)
    c.update(o["insts"])
    c.update(b["insts"])
    last = _free_bytes()
    print("free device memory after the first update %d B, after 50 more %d B (blob %d B)" % (first, last, len(b["blob"])))
    assert abs(first - last) <= len(c.blob0), (first, last)
    c.update(c.insts)
    c.check_blob(o)
    c.check_queries(o)


def test_refusals_touch_nothing(ctx, mods, tmp_path):
    rd, scenes = mods
    c = ctx("c2_small")
    c.update(c.insts)
    st = c.steps[3]
    tl, plt = c.dev.topAccelStruct, c.plt
    good = tu.rd_instances(rd, st["insts"], c.dev.blas)
    moved = tu.rd_instances(rd, c.steps[0]["insts"], c.dev.blas)
    other = ctx("shared_blas")
    swapped = list(moved)
    swapped[3] = rd.Instance(moved[3].transform, 0, moved[3].customInstanceID, c.dev.blas[(st["insts"][3][0] + 1) % len(c.dev.blas)])
    foreign = list(moved)
    foreign[0] = rd.Instance(moved[0].transform, 0, 0, other.dev.blas[0])
    nothing = list(moved)
    nothing[5] = rd.Instance(moved[5].transform, 0, 0, None)
    path = str(tmp_path / "tlas.bin")
    rd.TopAccelStructToFile(plt, tl, path)
    assert open(path, "rb").read() == st["blob"]
    cases = [
        ("null handle", lambda: rd.UpdateAccelStruct(plt, rd.Buffer(None, 0), moved), "invalid TLAS handle"),
        ("unknown handle", lambda: rd.UpdateAccelStruct(plt, rd.Buffer(0x10, 0), moved), "invalid TLAS handle"),
        ("plain buffer", lambda: rd.UpdateAccelStruct(plt, rd.CreateBuffer(plt, len(st["blob"])), moved), "not a TLAS built by rdx_tlas_build"),
        ("wrapped memory", lambda: rd.UpdateAccelStruct(plt, rd.WrapDeviceMemory(plt, tl.device_ptr, tl.size), moved), "not a TLAS built by rdx_tlas_build"),
        ("cache file", lambda: rd.UpdateAccelStruct(plt, rd.FileToTopAccelStruct(plt, path), moved), "not a TLAS built by rdx_tlas_build"),
        ("one instance fewer", lambda: rd.UpdateAccelStruct(plt, tl, moved[:-1]), "instances"),
        ("one instance more", lambda: rd.UpdateAccelStruct(plt, tl, moved + moved[:1]), "instances"),
        ("another BLAS of the scene", lambda: rd.UpdateAccelStruct(plt, tl, swapped), "instance 3 refers to another BLAS"),
        ("a BLAS of another scene", lambda: rd.UpdateAccelStruct(plt, tl, foreign), "instance 0 refers to another BLAS"),
        ("no BLAS", lambda: rd.UpdateAccelStruct(plt, tl, nothing), "instance 5 refers to another BLAS"),
    ]
    ptr = tl.device_ptr
    for what, call, word in cases:
        with pytest.raises(rd.RadianceError) as e:
            call()
        assert word in str(e.value) and "rdx_tlas_update" in str(e.value), (what, str(e.value))
        assert tl.device_ptr == ptr and tl.size == len(st["blob"]), what
        c.check_blob(st)
        c.check_queries(st, what)
    rd.UpdateAccelStruct(plt, tl, good)
    c.check_blob(st)


def test_user_megakernel_sees_the_moved_blob(mods, ref):
    """a user raygen (tests/golden/user_trace.cl: traceRay() on the rays of slot 6, HitData to slot 1) after an update that moved
    the blob to another allocation: every HitData field, against the reference's live answers / the oracle's"""
    rd, scenes = mods
    text = open(os.path.join(GOLD, "user_trace.cl")).read()
    rd.SetShaderIncludePath("")
    c = Ctx(rd, scenes, ref, "c2_small", shader_text=text)
    dev, plt = c.dev, c.plt
    bRays = rd.CreateBuffer(plt, N_RAYS * 24)
    bOut = rd.CreateBuffer(plt, N_RAYS * 28 * 4)
    before = (dev.topAccelStruct.device_ptr, dev.topAccelStruct.size)
    for st in (c.steps[0], c.steps[3]):
        c.update(st["insts"])
        assert dev.topAccelStruct.size != before[1] or st is c.steps[3]
        c.check_blob(st)
        rd.WriteBuffer(plt, bRays, N_RAYS * 24, np.concatenate([st["o"], st["d"]], 1).reshape(-1).astype(np.float32))
        for kind in (1, 2):
            prop = np.zeros((), rd.RayTraceProperties)
            prop["batchSize"], prop["depth"] = N_RAYS, kind
            rd.WriteBuffer(plt, dev.rdRTProp, 16, np.array(prop))
            rd.WriteBuffer(plt, bOut, N_RAYS * 28 * 4, np.zeros(N_RAYS * 28, np.uint32))
            rd.BindDescriptorSet(plt, rd.CreateDescriptorSet([dev.rdRTProp, bOut, dev.rdImage, dev.rdCamData, dev.rdSceneData, dev.meshInfoData, bRays,
                                                               dev.indexData, dev.uvData, dev.normalData, dev.materialData, None, None, dev.topAccelStruct]))
            rd.TraceRays(plt, 0, 0, 0, N_RAYS, 1)
            got = rd.ReadBuffer(plt, bOut, N_RAYS * 28 * 4).view(ob.HIT_DTYPE).reshape(-1)
            for src in ("ref", "orc"):
                want = st["want"].get("%s%d" % (src, kind))
                if want is None:
                    continue
                assert np.array_equal(want["hit"], got["hit"]), (st["step"], kind, src)
                if kind == 1:
                    h = want["hit"] == 1
                    assert h.sum() > 500
                    for f in FIELDS:
                        assert np.array_equal(_bits(want[f][h]), _bits(got[f][h])), (st["step"], src, f)
    assert (dev.topAccelStruct.device_ptr, dev.topAccelStruct.size)[1] == before[1]
