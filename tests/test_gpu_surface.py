"""GPU suite (-m gpu): rd.ResolveHits / rd.ResolveHitsTorch (rdx_resolve_hits) -- surface records for the hits of a closest-hit
ray query, on the device.

Comparands, in this order of authority:
  * the reference's own device code, recorded (tests/golden/refgpu_c{0,1,2}.npz: HitData `mat_hits` of the primary rays
    gen_o / gen_d at golden_cases.spread(npix, N_MATERIAL), its `material` payloads `mat_payload`; HitData `hits` of the 4096
    scattered / axis-aligned / grazing rays ray_o / ray_d) and, where oracle/_ref is built, run live on a scene of instances;
  * the numpy restatement of tests/surface_cases.py, which tests/test_surface_cpu.py holds to the same recordings.
Bars (surface_cases.check_records / check_next_origin): hit flags equal; position, above / below (from the record's own position
and normal), u, v bit for bit; materialIndex equal; normal within 8 * 2^-24 per component of the float64 restatement; every miss
64 zero bytes; for EVERY hit the recorded nextRayOrigin has the bits of `above` or of `below`, each at least 30 times a scene.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_cases as gc
import oracle_bind as ob
import ray_query_cases as rq
import refgpu_bind as rg
import surface_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def mods(gpu):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd, scenes
    return rd, scenes


def upload(rd, plt, arr, slack=0):
    arr = np.ascontiguousarray(arr)
    buf = rd.CreateBuffer(plt, max(arr.nbytes + slack, 16))
    rd.WriteBuffer(plt, buf, arr.nbytes, arr)
    return buf


def resolve(rd, plt, tlas, rays, sb, hits=None):
    """QueryRays (closest) + ResolveHits of a RAY_DTYPE batch -> (query records, surface records, invalid); `hits`: records to
    resolve instead of the query's"""
    n = rays.shape[0]
    bR = upload(rd, plt, rays)
    bH = rd.QueryRays(tlas, bR, n, rd.QUERY_CLOSEST) if hits is None else upload(rd, plt, hits)
    out, invalid = rd.ResolveHits(tlas, bR, bH, n, sb)
    assert out.size == 64 * n
    return (rd.ReadBuffer(plt, bH, 32 * n).view(rq.RAY_HIT_DTYPE).reshape(-1).copy(),
            rd.ReadBuffer(plt, out, 64 * n).view(sc.SURFACE_DTYPE).reshape(-1).copy(), invalid)


class Golden:
    """one golden scene on the device"""

    def __init__(self, rd, scenes, name):
        self.name = name
        self.G = np.load(os.path.join(GOLD, "refgpu_%s.npz" % name))
        self.s = gc.small_scene(scenes, name)
        self.b = self.s.buffers()
        self.dev = scenes.DeviceScene(self.s)
        blob = rd.ReadBuffer(self.dev.plt, self.dev.topAccelStruct, self.dev.topAccelStruct.size).tobytes()
        assert np.array_equal(gc.sha(blob), self.G["blob_sha256"]), "the TLAS blob of %s changed" % name
        sel = gc.spread(self.s.width * self.s.height, gc.N_MATERIAL)
        self.mat_rays = sc.rays_of(self.G["gen_o"][sel], self.G["gen_d"][sel])
        self.mat_hits = np.ascontiguousarray(self.G["mat_hits"]).view(ob.HIT_DTYPE).reshape(-1)
        self.mat_pay = np.ascontiguousarray(self.G["mat_payload"]).view(ob.PAYLOAD_DTYPE).reshape(-1)


@pytest.fixture(scope="module")
def golden(mods):
    rd, scenes = mods
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Golden(rd, scenes, name)
        return cache[name]
    return get


@pytest.mark.parametrize("name", gc.SCENES)
def test_material_batch_matches_the_references_recordings(mods, golden, name):
    """the 2048 primary rays the reference's `material` was recorded on: every field, and its nextRayOrigin on EVERY hit"""
    rd, _ = mods
    c = golden(name)
    q, got, invalid = resolve(rd, c.dev.plt, c.dev.topAccelStruct, c.mat_rays, c.dev.surface_buffers())
    assert not rq.mismatches(rq.query_records(c.mat_hits), q).any()
    assert invalid == 0
    sc.check_records(got, c.mat_hits, c.b, name)
    sc.check_next_origin(got, c.mat_hits, c.mat_pay, name)


@pytest.mark.parametrize("name", gc.SCENES)
def test_scattered_axis_aligned_and_grazing_rays(mods, golden, name):
    """the 4096-ray traversal batch (primary, scattered from hit points, axis-aligned, grazing) against the recorded HitData"""
    rd, _ = mods
    c = golden(name)
    h = np.ascontiguousarray(c.G["hits"]).view(ob.HIT_DTYPE).reshape(-1)
    q, got, invalid = resolve(rd, c.dev.plt, c.dev.topAccelStruct, sc.rays_of(c.G["ray_o"], c.G["ray_d"]), c.dev.surface_buffers())
    assert not rq.mismatches(rq.query_records(h), q).any()
    assert invalid == 0 and 0 < int((h["hit"] == 1).sum()) < h.shape[0]
    sc.check_records(got, h, c.b, name + " rays")


# ---- a scene of instances ------------------------------------------------------------------------------------------------------------
def rd_instances(rd, scene, blas):
    return [rd.Instance(tf, scene.sbt_offsets.get(k, 0), mat, blas[mi]) for k, (mi, tf, mat) in enumerate(scene.instances)]


def test_instanced_scene_against_the_live_reference(mods):
    """five instances of one icosphere BLAS and a heightfield, rotated, scaled non-uniformly and translated: 4096 rays against the
    reference's own device code run here (RefScene.trace -> HitData, material_batch -> nextRayOrigin)"""
    rd, scenes = mods
    if not rg.available("p"):
        pytest.skip("oracle/_ref/ref_shader_gfx950_p.co is not built (needs the reference's sources: `make -C oracle`)")
    s = sc.instanced_scene(scenes)
    dev = scenes.DeviceScene(s)
    o, d = sc.instanced_rays()
    blob = rd.ReadBuffer(dev.plt, dev.topAccelStruct, dev.topAccelStruct.size).tobytes()
    rs = rg.RefScene(rg.RefGpu("p"), s, blob)
    h = rs.trace(o, d)
    frames, depths = gc.material_inputs(o.shape[0])
    pay = rs.material_batch(h, d, frames, depths)
    q, got, invalid = resolve(rd, dev.plt, dev.topAccelStruct, sc.rays_of(o, d), dev.surface_buffers())
    assert not rq.mismatches(rq.query_records(h), q).any()
    assert invalid == 0
    hit = h["hit"] == 1
    assert (np.bincount(h["instanceIndex"][hit], minlength=6) >= 50).all()
    sc.check_records(got, h, s.buffers(), "instanced")
    sc.check_next_origin(got, h, pay, "instanced")


def test_after_update_accel_struct(mods, golden):
    """c2: two instances are carried across the scene (incremental path of rdx_tlas_update: the top-level tree is rebuilt with
    another slot order), then two more move while option "quad" changes (full derivation).  Each time the resolve is bitwise what
    a freshly built TLAS gives, and the hits on the moved instances have another position than before the moves"""
    rd, scenes = mods
    c = golden("c2")
    first, second = sc.moves(scenes)
    dev = scenes.DeviceScene(c.s)          # (a scene of its own: the module's c2 stays as built)
    rays = sc.rays_of(c.G["ray_o"], c.G["ray_d"])
    sb = dev.surface_buffers()
    _, before, invalid = resolve(rd, dev.plt, dev.topAccelStruct, rays, sb)
    assert invalid == 0
    try:
        for step, (moved, want_path) in enumerate(((first, 1), ({**first, **second}, 2))):
            if want_path == 2:
                rd.SetOption("quad", 0)          # the quad records vanish: rdx_tlas_update derives the layout again in full
            s1 = sc.moved_scene(scenes, c.s, moved)
            rd.UpdateAccelStruct(dev.plt, dev.topAccelStruct, rd_instances(rd, s1, dev.blas))
            assert rd.GetTlasUpdateStats().path == want_path, (step, rd.GetTlasUpdateStats().path)
            q, got, invalid = resolve(rd, dev.plt, dev.topAccelStruct, rays, sb)
            fresh = scenes.DeviceScene(s1)
            qf, want, invalid_f = resolve(rd, fresh.plt, fresh.topAccelStruct, rays, fresh.surface_buffers())
            assert invalid == 0 and invalid_f == 0
            assert not rq.mismatches(qf, q).any(), step
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), step
            on_moved = (q["hit"] == 1) & np.isin(q["instanceIndex"], list(moved))
            same = (sc.bits(got["position"][on_moved]) == sc.bits(before["position"][on_moved])).all(1)
            print("step %d: %d hits on the moved instances %s, %d with the position of before" % (step, int(on_moved.sum()), sorted(moved), int(same.sum())))
            assert int(on_moved.sum()) >= 100 and not same.any(), step
    finally:
        rd.SetOption("quad", 1)


# ---- bounds -------------------------------------------------------------------------------------------------------------------------
SLACK = 4096


def test_records_that_point_outside_a_buffer_are_zeroed_and_counted(mods, golden):
    """Every scene stream lives in an allocation 4 KiB larger than its content (the slack holds plausible values), the library
    gets a view of the content alone.  64 of c1's 2048 records are rewritten so that each breaks exactly one rule by less than the
    slack -- a kernel that did not check would read memory this test owns and fail by value: the 64 come back as zeros and
    counted, the other 1984 bit for bit as before.

    The streams are c1's with: three trap triangles and one pad word appended to the indices, one pad vertex appended to the
    normals, and uvOffset 0 for instance B -- so that a vertex number can leave the normal stream alone (B, trap 1) or the uv
    stream alone (the last mesh's instance A, trap 0)."""
    rd, _ = mods
    c = golden("c1")
    plt, b = c.dev.plt, c.b
    mi = b["meshInfo"].copy()
    ninst, nidx0, nfl = mi.shape[0], b["index"].shape[0], b["normal"].shape[0]
    assert b["uv"].shape[0] == nfl and nidx0 % 3 == 0
    A = int(np.flatnonzero(mi["normalOffset"] == mi["normalOffset"].max())[-1])          # an instance of the last mesh
    B = int(np.flatnonzero((mi["normalOffset"] >= 6) & (mi["normalOffset"] < mi["normalOffset"].max()))[0])
    mi[B]["uvOffset"] = 0
    nvA = (nfl - int(mi[A]["normalOffset"])) // 3                  # vertex one past A's mesh: its normal is the pad vertex, its uv is outside
    vB = (nfl + 3 - int(mi[B]["normalOffset"])) // 3               # from B: normal one past the pad vertex, uv (offset 0) inside
    assert int(mi[B]["normalOffset"]) % 3 == 0 and 3 * vB + 1 < nfl
    index = np.concatenate([b["index"], np.array([0, 1, nvA, 0, 1, vB, 0, 1, 2, 0], np.uint32)])
    normal = np.concatenate([b["normal"], np.array([0.0, 1.0, 0.0], np.float32)])
    uv = b["uv"]
    nidx = index.shape[0]                                          # 3 * triangles + 1: the triangle at the end has ONE index inside
    trap = lambda inst, k: (nidx0 - int(mi[inst]["indexOffset"])) // 3 + k

    def view(content, slack_fill):
        content = np.ascontiguousarray(content)
        whole = np.concatenate([content.view(np.uint8).reshape(-1), np.resize(np.ascontiguousarray(slack_fill).view(np.uint8).reshape(-1), SLACK)])
        buf = upload(rd, plt, whole)
        assert buf.size == content.nbytes + SLACK
        return rd.WrapDeviceMemory(plt, buf.device_ptr, content.nbytes, keepalive=buf)
    sb = rd.SurfaceBuffers(view(mi, mi[:1]), view(index, np.arange(3, dtype=np.uint32)), view(uv, np.float32([0.25, 0.75, 0.0])),
                           view(normal, np.float32([0.6, 0.0, 0.8])))

    q, base, invalid = resolve(rd, plt, c.dev.topAccelStruct, c.mat_rays, sb)
    assert invalid == 0 and (q["hit"] == 1).all()
    own = resolve(rd, plt, c.dev.topAccelStruct, c.mat_rays, c.dev.surface_buffers())[1]
    for f in ("position", "normal", "above", "below", "hit", "materialIndex"):       # (uv differs on B by construction)
        assert np.array_equal(base[f].view(np.uint32), own[f].view(np.uint32)), f
    # the traps themselves are resolvable where they break no rule: trap 2 is an ordinary triangle
    ok = q.copy()
    ok["instanceIndex"][:8], ok["primitiveIndex"][:8] = A, trap(A, 2)
    assert resolve(rd, plt, c.dev.topAccelStruct, c.mat_rays, sb, hits=ok)[2] == 0

    rng = np.random.default_rng(9)
    rows = np.sort(rng.choice(q.shape[0], 64, replace=False))
    bad = q.copy()
    kinds = []
    for j, r in enumerate(rows):
        inst = int(bad["instanceIndex"][r])
        k = j % 8
        if k == 0:      # instanceIndex: the first past the instance count (= the MeshInfo count), and further
            bad["instanceIndex"][r] = ninst + j // 8
        elif k == 1:    # ... and further ones whose MeshInfo would still be read from the slack (4096 / 32 = 128 records)
            bad["instanceIndex"][r] = ninst + 8 + 15 * (j // 8)
        elif k == 2:    # the triangle at the end of the index stream: one index inside, two outside
            bad["primitiveIndex"][r] = trap(inst, 3)
        elif k == 3:    # triangles past it, by less than the slack
            bad["primitiveIndex"][r] = trap(inst, 4 + 37 * (j // 8))
        elif k == 4:    # 3 * primitiveIndex wraps in 32 bits to the triangle before the mesh / into the stream
            bad["primitiveIndex"][r] = (0xffffffff, 0x55555556, 0x7fffffff, 0xaaaaaaab)[(j // 8) % 4]
        elif k == 5:    # a vertex whose normal lies past the normal stream, its uv inside
            bad["instanceIndex"][r], bad["primitiveIndex"][r] = B, trap(B, 1)
        elif k == 6:    # a vertex whose uv lies past the uv stream, its normal inside
            bad["instanceIndex"][r], bad["primitiveIndex"][r] = A, trap(A, 0)
        else:           # a triangle far into the slack, its three indices still inside it
            bad["primitiveIndex"][r] = trap(inst, 3 + 300)
        kinds.append(k)
    assert 3 * (3 + 300) + 2 < SLACK // 4 and 8 + 15 * 7 < SLACK // 32
    poisoned = np.zeros(q.shape[0], bool)
    poisoned[rows] = True
    # first through the host seam -- the same function the kernel compiles: every poisoned record invalid, every other valid
    for r in range(q.shape[0]):
        inst, prim = int(bad["instanceIndex"][r]), int(bad["primitiveIndex"][r])
        first = int(mi[inst]["indexOffset"]) + 3 * prim if inst < ninst else -1
        idx3 = index[first:first + 3] if 0 <= first and first + 3 <= nidx else None
        assert rd.DebugSurfaceInBounds(mi, ninst, inst, prim, idx3, nidx, normal.shape[0], uv.shape[0]) is (not poisoned[r]), (r, inst, prim)
    _, got, invalid = resolve(rd, plt, c.dev.topAccelStruct, c.mat_rays, sb, hits=bad)
    nz = got[poisoned].view(np.uint32).reshape(64, 16).any(1)
    assert not nz.any(), "poisoned records came back non-zero: kinds %s" % sorted({kinds[i] for i in np.flatnonzero(nz)})
    assert invalid == 64
    assert np.array_equal(got[~poisoned].view(np.uint32), base[~poisoned].view(np.uint32))


def test_null_uv_stream_gives_zero_uv(mods, golden):
    rd, _ = mods
    c = golden("c0")
    dev = c.dev
    _, full, _ = resolve(rd, dev.plt, dev.topAccelStruct, c.mat_rays, dev.surface_buffers())
    _, got, invalid = resolve(rd, dev.plt, dev.topAccelStruct, c.mat_rays, (dev.meshInfoData, dev.indexData, None, dev.normalData))
    assert invalid == 0 and not got["u"].view(np.uint32).any() and not got["v"].view(np.uint32).any()
    for f in ("position", "hit", "normal", "materialIndex", "above", "below"):
        assert np.array_equal(got[f].view(np.uint32), full[f].view(np.uint32)), f


# ---- offsets and refusals ---------------------------------------------------------------------------------------------------------------
def test_offsets_and_refusals(mods, golden):
    """n = 200 of c1's records at rays_offset 96, hits_offset 160, out_offset 192 in buffers filled with 0xA5: the records equal the
    plain call's and no byte outside the 64 n output range is touched; then every refusal, after each of which the call still works"""
    rd, _ = mods
    c = golden("c1")
    dev, plt, tl = c.dev, c.dev.plt, c.dev.topAccelStruct
    sb = dev.surface_buffers()
    n, ro, ho, oo, tail = 200, 96, 160, 192, 128
    q, base, _ = resolve(rd, plt, tl, c.mat_rays, sb)
    fill = lambda buf: rd.WriteBuffer(plt, buf, buf.size, np.full(buf.size, 0xA5, np.uint8))
    bR, bH, bO = rd.CreateBuffer(plt, ro + 32 * n + tail), rd.CreateBuffer(plt, ho + 32 * n + tail), rd.CreateBuffer(plt, oo + 64 * n + tail)
    for buf in (bR, bH, bO):
        fill(buf)
    rd.WriteBuffer(plt, bR, 32 * n, c.mat_rays[:n], offset=ro)
    rd.WriteBuffer(plt, bH, 32 * n, q[:n], offset=ho)
    before = [rd.ReadBuffer(plt, buf, buf.size).copy() for buf in (bR, bH)]
    ret, invalid = rd.ResolveHits(tl, bR, bH, n, sb, bO, rays_offset=ro, hits_offset=ho, out_offset=oo)
    assert ret is bO and invalid == 0
    raw = rd.ReadBuffer(plt, bO, bO.size)
    assert np.array_equal(raw[oo:oo + 64 * n].view(np.uint32), base[:n].view(np.uint32))
    assert (raw[:oo] == 0xA5).all() and (raw[oo + 64 * n:] == 0xA5).all()
    assert all(np.array_equal(rd.ReadBuffer(plt, buf, buf.size), was) for buf, was in zip((bR, bH), before))
    # out=None: a buffer of out_offset + 64 n bytes; n == 0 touches nothing
    made, _ = rd.ResolveHits(tl, bR, bH, n, sb, None, rays_offset=ro, hits_offset=ho, out_offset=oo)
    assert made.size == oo + 64 * n
    assert np.array_equal(rd.ReadBuffer(plt, made, 64 * n, offset=oo).view(np.uint32), base[:n].view(np.uint32))
    fill(bO)
    assert rd.ResolveHits(tl, bR, bH, 0, sb, bO)[1] == 0 and (rd.ReadBuffer(plt, bO, bO.size) == 0xA5).all()

    # one buffer that holds rays, records and room for the output, for the overlap cases
    one = rd.CreateBuffer(plt, 32 * n + 32 * n + 64 * n)
    rd.WriteBuffer(plt, one, 32 * n, c.mat_rays[:n])
    rd.WriteBuffer(plt, one, 32 * n, q[:n], offset=32 * n)
    null = rd.Buffer(None, 1 << 20)

    def ok():
        fill(bO)
        assert rd.ResolveHits(tl, bR, bH, n, sb, bO, rays_offset=ro, hits_offset=ho, out_offset=oo)[1] == 0
        assert np.array_equal(rd.ReadBuffer(plt, bO, 64 * n, offset=oo).view(np.uint32), base[:n].view(np.uint32))

    call = lambda *a, **k: (lambda: rd.ResolveHits(*a, **k))
    cases = [
        ("rays_offset 8", call(tl, bR, bH, 8, sb, bO, rays_offset=8), "16"),
        ("hits_offset 8", call(tl, bR, bH, 8, sb, bO, hits_offset=8), "16"),
        ("out_offset 8", call(tl, bR, bH, 8, sb, bO, out_offset=8), "16"),
        ("rays past the end", call(tl, bR, bH, n, sb, bO, rays_offset=ro + tail + 16), "ray buffer"),
        ("records past the end", call(tl, bR, bH, n, sb, bO, hits_offset=ho + tail + 16), "hit buffer"),
        ("output past the end", call(tl, bR, bH, n, sb, bO, out_offset=oo + tail + 16), "output buffer"),
        ("output one record short", call(tl, one, one, n, sb, rd.CreateBuffer(plt, 64 * n - 16), hits_offset=32 * n), "output buffer"),
        ("output over the rays", call(tl, one, one, n, sb, one, hits_offset=32 * n, out_offset=32 * n - 64), "overlap"),
        ("output over the first ray's tail", call(tl, one, one, 1, sb, one, hits_offset=32 * n, out_offset=16), "overlap"),
        ("output over the records", call(tl, one, one, n, sb, one, hits_offset=32 * n, out_offset=64 * n - 64), "overlap"),
        ("output = the records", call(tl, one, one, n, sb, one, hits_offset=32 * n, out_offset=32 * n), "overlap"),
        ("null tlas", call(null, bR, bH, n, sb, bO), "TLAS"),
        ("null rays", call(tl, null, bH, n, sb, bO), "ray buffer handle"),
        ("null hits", call(tl, bR, null, n, sb, bO), "hit buffer handle"),
        ("null out", call(tl, bR, bH, n, sb, null), "output buffer handle"),
        ("null meshInfo", call(tl, bR, bH, n, (null, dev.indexData, dev.uvData, dev.normalData), bO), "meshInfo"),
        ("null index", call(tl, bR, bH, n, (dev.meshInfoData, null, dev.uvData, dev.normalData), bO), "index"),
        ("null normal", call(tl, bR, bH, n, (dev.meshInfoData, dev.indexData, dev.uvData, null), bO), "normal"),
    ]
    for what, fn, word in cases:
        with pytest.raises(rd.RadianceError) as e:
            fn()
        assert word in str(e.value) and "rdx_resolve_hits" in str(e.value), (what, str(e.value))
        ok()
    from radiance_ray_tracing_amd import _lib
    assert _lib.lib().rdx_resolve_hits(tl.handle, bR.handle, 0, bH.handle, 0, n, None, bO.handle, 0, None) != 0      # scene NULL
    assert "scene" in _lib.last_error()
    ok()
    # adjacent ranges of one buffer are fine: rays, then records, then the output
    _, invalid = rd.ResolveHits(tl, one, one, n, sb, one, hits_offset=32 * n, out_offset=64 * n)
    assert invalid == 0
    assert np.array_equal(rd.ReadBuffer(plt, one, 64 * n, offset=64 * n).view(np.uint32), base[:n].view(np.uint32))
    for what, fn in (("a list", lambda: rd.ResolveHits(tl, bR, bH, n, [dev.meshInfoData], bO)), ("not a Buffer", lambda: rd.ResolveHits(tl, bR, bH, n, (1, 2, 3, 4), bO))):
        with pytest.raises(rd.RadianceError):
            fn()


# ---- torch --------------------------------------------------------------------------------------------------------------------------
_TORCH_CHILD = r"""
import os, sys
ROOT = sys.argv[1]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
assert torch.cuda.is_available()
torch.zeros(1, device="cuda").cpu()                      # torch initialises the GPU first (tests/test_cpu_oracle._gpu_present)
import numpy as np
import rrt_amd
from radiance_ray_tracing_amd import rd, scenes
import golden_cases as gc
import surface_cases as sc
G = np.load(os.path.join(ROOT, "tests", "golden", "refgpu_c1.npz"))
s = gc.small_scene(scenes, "c1")
dev = scenes.DeviceScene(s)
sel = gc.spread(s.width * s.height, gc.N_MATERIAL)
rays = sc.rays_of(G["gen_o"][sel], G["gen_d"][sel])
n = rays.shape[0]
sb = dev.surface_buffers()
# the buffer route
bR = rd.CreateBuffer(dev.plt, 32 * n); rd.WriteBuffer(dev.plt, bR, 32 * n, rays)
bH = rd.QueryRays(dev.topAccelStruct, bR, n, 1)
out, invalid = rd.ResolveHits(dev.topAccelStruct, bR, bH, n, sb)
want = rd.ReadBuffer(dev.plt, out, 64 * n).view(np.uint32).reshape(n, 16).copy()
assert invalid == 0 and want[:, 3].all()
# the tensor route, on tensors a torch op produced
t = (torch.from_numpy(rays.view(np.float32).reshape(n, 8).copy()).cuda() * torch.ones(8, device="cuda")).contiguous()
h = rd.QueryRaysTorch(dev.topAccelStruct, t, 1)
got, invalid = rd.ResolveHitsTorch(dev.topAccelStruct, t, h, sb)
assert got.dtype == torch.float32 and tuple(got.shape) == (n, 16) and got.is_cuda and got.is_contiguous() and invalid == 0
assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
pre = torch.full((n, 16), -1.0, dtype=torch.float32, device="cuda")
ptr = pre.data_ptr()
ret, _ = rd.ResolveHitsTorch(dev.topAccelStruct, t, h.view(torch.float32), sb, out=pre)
assert ret is pre and pre.data_ptr() == ptr and np.array_equal(pre.cpu().numpy().view(np.uint32), want)
e, _ = rd.ResolveHitsTorch(dev.topAccelStruct, t[:0], h[:0], sb)
assert tuple(e.shape) == (0, 16)
bad = [(t[:, :7], h, None), (t.double(), h, None), (t.cpu(), h, None), (t, h[:, :7], None), (t, h.long(), None), (t, h.cpu(), None),
       (t, h[:-1], None), (t, h, pre[:-1]), (t, h, pre.double()), (t, h, pre.cpu()), (t, h, pre.view(n * 2, 8)), (rays, h, None)]
for k, (r_, h_, o_) in enumerate(bad):
    try:
        rd.ResolveHitsTorch(dev.topAccelStruct, r_, h_, sb, out=o_)
    except rd.RadianceError:
        continue
    raise AssertionError("bad argument set %d was accepted" % k)
print("TORCH-RESOLVE-OK", n)
"""


def test_torch_tensors_in_a_fresh_process(gpu):
    """rd.ResolveHitsTorch equals the buffer route bit for bit; wrong dtype, shape or device is refused in Python.  torch is
    initialised first, in a process of its own (as tests/test_gpu_ray_query.py does)"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _TORCH_CHILD, ROOT]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "TORCH-RESOLVE-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
