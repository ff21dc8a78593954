"""GPU suite (-m gpu): rdx_camera_view and rdx_temporal_accumulate through radiance_ray_tracing_amd.temporal -- a frame's history
reprojected through the previous view, tested against its own guide and folded into exponential means with a variance estimate.

The reference has no temporal accumulation.  The comparand is temporal_cases.temporal_reference, the numpy restatement that takes
one IEEE float32 operation at a time; every bar is equality of bits with it (a NaN compares as a NaN -- denoise_cases.canon), and
what is copied rather than computed -- invalid pixels, w, the guide planes -- is compared bit for bit.  Views of real cameras are the
records rdx_camera_view wrote, read back and handed to the restatement, so the device's cos and sin are never restated.  The RGBA8
image is held to rd.Accumulate, byte for byte."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_cases as dc
import temporal_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
F4 = np.dtype(("<f4", 4))
OFF = dict(color=48, mat=64, surf=16, prev=32, view=16, pview=80, hin=96, hout=32, image=12)
INPUTS, OUTPUTS = ("color", "mat", "surf", "prev", "view", "pview", "hin"), ("hout", "image")
TAIL = 80
DEPTH = 4


@pytest.fixture(scope="module")
def mods(gpu):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import _lib, denoise, rd, scenes, temporal
    return rd, scenes, temporal, denoise, _lib


class Frame:
    """the nine ranges of one call at non-zero offsets in buffers filled with 0xA5"""

    def __init__(self, rd, plt, W, H):
        self.rd, self.plt, self.W, self.H, n = rd, plt, W, H, W * H
        self.size = dict(color=16 * n, mat=64 * n, surf=64 * n, prev=16 * n, view=64, pview=64, hin=64 * n, hout=64 * n, image=4 * n)
        self.B = {k: rd.CreateBuffer(plt, OFF[k] + self.size[k] + TAIL) for k in OFF}
        for k in self.B:
            self.fill(k)

    def fill(self, k):
        self.rd.WriteBuffer(self.plt, self.B[k], self.B[k].size, np.full(self.B[k].size, 0xA5, np.uint8))

    def put(self, k, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes == self.size[k], (k, arr.nbytes, self.size[k])
        if arr.nbytes:
            self.rd.WriteBuffer(self.plt, self.B[k], arr.nbytes, arr, offset=OFF[k])

    def whole(self, k):
        return self.rd.ReadBuffer(self.plt, self.B[k], self.B[k].size).copy()

    def arguments(self, with_previous_view=True, with_previous_positions=True, with_history_in=True, with_image=True, **kw):
        B = self.B
        a = dict(color=B["color"], materials=B["mat"], surfaces=B["surf"], view=B["view"], width=self.W, height=self.H,
                 history_in=B["hin"] if with_history_in else None, history_out=B["hout"], previous_view=B["pview"] if with_previous_view else None,
                 previous_positions=B["prev"] if with_previous_positions else None, image=B["image"] if with_image else None,
                 color_offset=OFF["color"], materials_offset=OFF["mat"], surfaces_offset=OFF["surf"], view_offset=OFF["view"], history_in_offset=OFF["hin"],
                 history_out_offset=OFF["hout"], previous_view_offset=OFF["pview"], previous_positions_offset=OFF["prev"], image_offset=OFF["image"])
        a.update(kw)
        return a

    def call(self, tp, settings, **kw):
        a = self.arguments(**kw)
        return tp.TemporalAccumulate(a.pop("color"), a.pop("materials"), a.pop("surfaces"), a.pop("view"), a.pop("width"), a.pop("height"), settings, **a)

    def run(self, tp, settings, color, mat, surf, view, previous_view=None, previous_positions=None, history_in=None, image=False, refill=True):
        """-> (history (4, n, 4) float32, image (n, 4) uint8 or None); no input and nothing outside the written ranges has changed"""
        for k, arr in (("color", color), ("mat", mat), ("surf", surf), ("view", view), ("pview", previous_view), ("prev", previous_positions), ("hin", history_in)):
            if arr is not None:
                self.put(k, arr)
        if refill:
            for k in OUTPUTS:
                self.fill(k)
        before = {k: self.whole(k) for k in INPUTS}
        assert self.call(tp, settings, with_previous_view=previous_view is not None, with_previous_positions=previous_positions is not None,
                         with_history_in=history_in is not None, with_image=image) is self.B["hout"]
        for k in INPUTS:
            assert np.array_equal(self.whole(k), before[k]), k
        got = {}
        for k in OUTPUTS:
            raw = self.whole(k)
            lo, hi = OFF[k], OFF[k] + self.size[k]
            assert (raw[:lo] == 0xA5).all() and (raw[hi:] == 0xA5).all(), k
            got[k] = raw[lo:hi]
        if not image:
            assert (got["image"] == 0xA5).all()
        return got["hout"].view(F).reshape(4, -1, 4), got["image"].reshape(-1, 4) if image else None


def show(got, want, W):
    bad = np.flatnonzero((dc.canon(got) != dc.canon(want)).any((0, 2)))
    return [(int(p % W), int(p // W), got[:, p].tolist(), want[:, p].tolist()) for p in bad[:3]], int(bad.size)


def held(got, want, color, mat, surf):
    """the device's history has the restatement's bits; what is copied has its source's"""
    if not dc.same(got, want):
        return False
    invalid = ~dc.validity(mat.reshape(-1), surf.reshape(-1))
    return (np.array_equal(dc.bits(got[0][:, 3]), dc.bits(color[:, 3])) and np.array_equal(dc.bits(got[0][invalid]), dc.bits(color[invalid]))
            and np.array_equal(dc.bits(got[2:]), dc.bits(want[2:])) and not got[1][invalid].view(np.uint32).any())


# ---- 1. synthetic records ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", tc.GPU_SIZES, ids=lambda s: "%dx%d" % s)
def test_synthetic_hostile_records_have_the_restatements_bits(mods, gpu, size):
    """three chained frames under a fractional pan, every size around the 64 x 4 block and the 7 x 7 window's reach, with and without
    previous_positions, every term on and each off, history_in absent on the first frame, on records a caller may have filled with
    anything.  The cap: from 37 x 19 on more than half of frame 3's pixels have N' >= 2, all four taps count somewhere, and every
    consistency test fails somewhere"""
    rd, _, tp, _, _ = mods
    W, H = size
    seq = tc.hostile_sequence(W, H, 300 + W)
    fr = Frame(rd, gpu, W, H)
    for name, terms in tc.GPU_TERMS:
        st = tp.TemporalSettings(**terms)
        for with_prev in (False, True):
            h, fails = None, {k: 0 for k in ("fail_material", "fail_normal", "fail_position")}
            for f, (color, mat, surf, view, previous, prev) in enumerate(seq):
                info = {}
                pp = prev if with_prev else None
                want = tc.temporal_reference(color, mat, surf, W, H, st, view, previous, h, pp, info)
                got, _ = fr.run(tp, st, color, mat, surf, view, previous, pp, h)
                assert held(got, want, color, mat, surf), (size, name, with_prev, f, show(got, want, W))
                for k in fails:
                    fails[k] += int(info[k].sum())
                h = got
            if W * H >= 37 * 19:
                N = tc.history_length(h)
                assert (N >= 2).sum() > W * H // 2 and (info["counted"].sum(1) == 4).any(), (size, name, with_prev)
                assert fails["fail_material"] and fails["fail_normal"] and (fails["fail_position"] or st.position_tolerance == 0.0), (size, name, fails)
                assert np.isnan(color[:, :3]).any() and (mat["hit"] == 2).any() and (surf["hit"] == 0).any()
    assert rd.GetTraceStats().ms_accumulate > 0.0


# ---- 2. the exact pan and the still camera -----------------------------------------------------------------------------------------------
def test_the_exact_pan_and_the_still_camera_on_the_device(mods, gpu):
    rd, _, tp, _, _ = mods
    W = H = 64
    st = tp.TemporalSettings(max_history=32, alpha_min=0.0, alpha_moments_min=0.0, normal_cos_min=0.9, position_tolerance=0.5, variance_min_history=0)
    fr = Frame(rd, gpu, W, H)
    xs = np.arange(W * H) % W
    h = previous = None
    for f in range(4):
        color, mat, surf, view = tc.pan_wall(f)
        want = tc.temporal_reference(color, mat, surf, W, H, st, view, previous, h)
        got, _ = fr.run(tp, st, color, mat, surf, view, previous, None, h)
        assert held(got, want, color, mat, surf), (f, show(got, want, W))
        N = tc.history_length(got)
        assert (N == np.minimum(W - xs, f + 1)).all(), "N + 1 from the right-hand neighbour; the entering column starts at 1"
        if f:
            moved = xs < W - 1
            src = np.arange(W * H)[moved] + 1
            with np.errstate(all="ignore"):
                carried = h[0][src, :3] + (color[moved, :3] - h[0][src, :3]) * (F(1) / N[moved].astype(F))[:, None]
            assert np.array_equal(dc.bits(got[0][moved, :3]), dc.bits(carried))
        h, previous = got, view
    # the still camera: the plain mean of each pixel, previous_view absent and bit-equal alike
    W, H = 16, 8
    frames = tc.noisy_frames(W, H, 16, 21)
    view = tc.wall_view(W, H)
    st = tp.TemporalSettings(max_history=16, alpha_min=0.0, alpha_moments_min=0.0, variance_min_history=0)
    fr = Frame(rd, gpu, W, H)
    h = None
    for f, (color, mat, surf) in enumerate(frames):
        want = tc.temporal_reference(color, mat, surf, W, H, st, view, None, h)
        got, _ = fr.run(tp, st, color, mat, surf, view, view if f % 2 else None, None, h)
        assert held(got, want, color, mat, surf) and (tc.history_length(got) == f + 1).all(), f
        h = got
    mean = np.stack([c[:, :3] for c, _, _ in frames]).astype(np.float64).mean(0)
    assert np.abs(h[0][:, :3] - mean).max() <= 2.0 ** -16


# ---- real frames -------------------------------------------------------------------------------------------------------------------------
def read(rd, plt, buf, n, dtype, offset=0):
    raw = rd.ReadBuffer(plt, buf, n * dtype.itemsize, offset=offset)
    return raw.view(F).reshape(n, 4).copy() if dtype.subdtype else raw.view(dtype).reshape(-1).copy()


class Real:
    """a stock scene at 64 x 32 and its frames through the public calls: GenerateRays -> QueryRays -> ResolveHits + ResolveMaterials ->
    TracePaths at depth 4; everything stays on the device, the records are downloaded for the restatement"""

    def __init__(self, rd, scenes, tp, name, W=64, H=32):
        make = dict(c1=lambda: scenes.c1_cornell(W, H, spp=1, depth=DEPTH, sphere_subdiv=3), c2=lambda: scenes.c2_atrium(W, H, spp=1, depth=DEPTH, detail=0.2))[name]
        self.dev = dev = scenes.DeviceScene(make())
        self.rd, self.tp, self.plt, self.W, self.H, self.n = rd, tp, dev.plt, W, H, W * H
        self.tlas, self.sb, self.cam = dev.topAccelStruct, dev.shading_buffers(), dev.frame_buffers()[0]
        blob = rd.ReadBuffer(dev.plt, self.tlas, self.tlas.size).tobytes()
        s = rd.DebugAccelLayout(blob)[0]
        self.diagonal = float(np.linalg.norm(np.array(s["sceneHi"], np.float64) - np.array(s["sceneLo"], np.float64)))

    def view(self):
        b = self.tp.CameraView(self.cam)
        return b, self.rd.ReadBuffer(self.plt, b, 64).view(tc.VIEW_DTYPE)[0].copy()

    def frame(self, f, trace=True):
        """-> the device buffers and host copies of frame f: dict(bC, bM, bS, color, mat, surf, hits)"""
        rd, n = self.rd, self.n
        rays, keys = rd.GenerateRays(self.cam, n, f, f)
        bH = rd.QueryRays(self.tlas, rays, n, rd.QUERY_CLOSEST)
        bS, inv_s = rd.ResolveHits(self.tlas, rays, bH, n, self.dev.surface_buffers())
        bM, inv_m = rd.ResolveMaterials(self.tlas, rays, bH, n, self.sb)
        assert inv_s == 0 and inv_m == 0
        out = dict(bS=bS, bM=bM, mat=read(rd, self.plt, bM, n, dc.MATERIAL_DTYPE), surf=read(rd, self.plt, bS, n, dc.SURFACE_DTYPE),
                   hits=read(rd, self.plt, bH, n, rd.RAY_HIT_DTYPE))
        if trace:
            out["bC"] = rd.TracePaths(self.tlas, rays, keys, n, DEPTH, self.sb)
            out["color"] = read(rd, self.plt, out["bC"], n, F4)
        return out


@pytest.fixture(scope="module")
def real(mods):
    rd, scenes, tp, _, _ = mods
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Real(rd, scenes, tp, name)
        return cache[name]
    return get


# ---- 3. rdx_camera_view ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c1", "c2"))
def test_the_camera_view_inverts_the_devices_own_rays(mods, real, name):
    """right, up and back are orthonormal within 2^-20, and every primary hit projects to within 0.5 + 1e-3 of its pixel's centre in
    both axes: the jitter lies in [0, 1) and the cameras have fStop == 0"""
    rd, _, tp, _, _ = mods
    r = real(name)
    cam = rd.ReadBuffer(r.plt, r.cam, 48).view(rd.PhysicalCamera)[0]
    assert float(cam["fStop"]) == 0.0
    _, v = r.view()
    assert (float(v["widthPixel"]), float(v["heightPixel"])) == (r.W, r.H)
    assert v["kx"] == F(cam["focalLength"]) / F(cam["sensorWidth"]) and v["ky"] == F(cam["focalLength"]) / (F(cam["sensorWidth"]) * (F(r.H) / F(r.W)))
    assert np.array_equal(dc.bits(v["eye"]), dc.bits(np.array([cam["x"], cam["y"], cam["z"]], F)))
    m = np.stack([v["right"], v["up"], v["back"]]).astype(np.float64)
    assert np.abs(m @ m.T - np.eye(3)).max() <= 2.0 ** -20, m @ m.T
    assert np.abs(m - np.stack([tc.view_of_camera(np.array([cam[k] for k in cam.dtype.names], np.float64))[k] for k in ("right", "up", "back")])).max() <= 2.0 ** -20
    fr = r.frame(0, trace=False)
    hit = dc.validity(fr["mat"], fr["surf"])
    assert hit.sum() >= r.n // 4
    u, t, dz = tc.project(v, fr["surf"]["position"])
    ys, xs = np.divmod(np.arange(r.n), r.W)
    eu, et = np.abs(u - (xs + 0.5))[hit].max(), np.abs(t - (ys + 0.5))[hit].max()
    print("largest distance from the pixel centre: %.4f, %.4f" % (eu, et))
    assert (dz[hit] > 0).all() and eu <= 0.5 + 1e-3 and et <= 0.5 + 1e-3, (eu, et)
    # a view in a range of its own, at an offset, beside the camera in one buffer; nothing else is written
    both = rd.CreateBuffer(r.plt, 48 + 16 + 64 + 16)
    rd.WriteBuffer(r.plt, both, both.size, np.full(both.size, 0xA5, np.uint8))
    rd.WriteBuffer(r.plt, both, 48, rd.ReadBuffer(r.plt, r.cam, 48))
    assert tp.CameraView(both, both, 64) is both
    raw = rd.ReadBuffer(r.plt, both, both.size)
    assert np.array_equal(raw[64:128].view(tc.VIEW_DTYPE)[0].tobytes(), v.tobytes()) and (raw[48:64] == 0xA5).all() and (raw[128:] == 0xA5).all()
    for args, text in (((both, both, 32), "overlap"), ((both, both, 8), "16"), ((both, both, 96), "view buffer"), ((rd.Buffer(None, 48), both, 64), "camera buffer handle"),
                       ((both, rd.Buffer(1234567, 64), 0), "view buffer handle")):
        assert mods[4].lib().rdx_camera_view(args[0].handle, args[1].handle, args[2]) != 0
        err = mods[4].last_error()
        assert "rdx_camera_view" in err and text in err, err
    assert np.array_equal(rd.ReadBuffer(r.plt, both, both.size), raw)


# ---- 4. a real frame sequence ------------------------------------------------------------------------------------------------------------
def test_a_real_sequence_with_a_camera_nudge(mods, real):
    """c1, four frames at one sample per pixel; camera.x is rewritten in the buffer between frames 2 and 3 and the views come from
    rdx_camera_view.  After every frame the device's history has the restatement's bits; after the nudge some pixels keep N' = 3 and
    some restart; plane 0 then goes into denoise.Denoise as `color` at offset 0 and gives denoise_reference's bits on it"""
    rd, _, tp, dn, _ = mods
    r = real("c1")
    st = tp.TemporalSettings(max_history=32, alpha_min=0.05, alpha_moments_min=0.2, normal_cos_min=0.9, position_tolerance=0.01 * r.diagonal, variance_min_history=4)
    cam0 = rd.ReadBuffer(r.plt, r.cam, 48).copy()
    try:
        hb = [rd.CreateBuffer(r.plt, tp.HistorySize(r.W, r.H)) for _ in range(2)]
        image = rd.CreateBuffer(r.plt, 4 * r.n)
        h = bprev = vprev = None
        for f in range(4):
            if f == 2:
                cam = cam0.view(rd.PhysicalCamera).copy()
                cam["x"] += F(0.35)
                rd.WriteBuffer(r.plt, r.cam, 48, cam)
            bview, view = r.view()
            fr = r.frame(f)
            out = tp.TemporalAccumulate(fr["bC"], fr["bM"], fr["bS"], bview, r.W, r.H, st, hb[(f + 1) % 2] if f else None, hb[f % 2], bprev, None, image)
            assert out is hb[f % 2]
            got = rd.ReadBuffer(r.plt, out, 64 * r.n).view(F).reshape(4, r.n, 4).copy()
            want = tc.temporal_reference(fr["color"], fr["mat"], fr["surf"], r.W, r.H, st, view, vprev, h)
            assert held(got, want, fr["color"], fr["mat"], fr["surf"]), (f, show(got, want, r.W))
            N = tc.history_length(got)
            valid = dc.validity(fr["mat"], fr["surf"])
            if f < 2:
                assert (N[valid] >= 1).all() and (N[valid] == f + 1).sum() > valid.sum() // 2, (f, np.bincount(N))
            if f == 2:
                kept, restarted = int((N[valid] == 3).sum()), int((N[valid] == 1).sum())
                print("after the nudge: %d pixels keep N' = 3, %d restart, of %d" % (kept, restarted, int(valid.sum())))
                assert kept > 0 and restarted > 0 and not np.array_equal(view.tobytes(), vprev.tobytes())
            h, bprev, vprev = got, bview, view
        dst = dn.DenoiseSettings(sigma_position=0.01 * r.diagonal, sigma_colour=0.5)
        filtered = read(rd, r.plt, dn.Denoise(out, fr["bM"], fr["bS"], r.W, r.H, dst), r.n, F4)
        assert dc.same(filtered, dc.denoise_reference(h[0], fr["mat"], fr["surf"], r.W, r.H, dst)) and not dc.same(filtered, h[0])
    finally:
        rd.WriteBuffer(r.plt, r.cam, 48, cam0)


# ---- 5. a moved instance -----------------------------------------------------------------------------------------------------------------
def test_a_moved_instance_keeps_its_history_through_previous_positions(mods, real):
    """one instance of c2 is translated with rd.UpdateAccelStruct; previous_positions is the current position minus the translation
    on that instance's pixels (picked by the hit records' instance number).  The device has the restatement's bits either way;
    with previous_positions the instance's pixels keep their history, without they lose it where the plane test says so"""
    rd, _, tp, _, _ = mods
    r = real("c2")
    scene, dev = r.dev.scene, r.dev
    instances = lambda moved, t: [rd.Instance(np.asarray(tf, F) + (t if k == moved else 0), scene.sbt_offsets.get(k, 0), mat, dev.blas[mi])
                                  for k, (mi, tf, mat) in enumerate(scene.instances)]
    st = tp.TemporalSettings(max_history=32, alpha_min=0.05, alpha_moments_min=0.2, normal_cos_min=0.9, position_tolerance=0.004 * r.diagonal, variance_min_history=4)
    bview, view = r.view()
    f0 = r.frame(0)
    valid0 = dc.validity(f0["mat"], f0["surf"])
    counts = np.bincount(f0["hits"]["instanceIndex"][valid0], minlength=len(scene.instances))
    moved = int(np.argsort(counts)[-2]) if (counts > 0).sum() > 1 else int(np.argmax(counts))       # a well-seen instance, not the most seen (the floor)
    assert counts[moved] >= 8, counts
    shift = np.zeros((4, 4), F)
    shift[:3, 3] = F(0.012 * r.diagonal)            # row-major object -> world: the translation is the last column (scenes.translate)
    t = shift[:3, 3]
    h0 = tp.TemporalAccumulate(f0["bC"], f0["bM"], f0["bS"], bview, r.W, r.H, st)
    first = rd.ReadBuffer(r.plt, h0, 64 * r.n).view(F).reshape(4, r.n, 4).copy()
    assert held(first, tc.temporal_reference(f0["color"], f0["mat"], f0["surf"], r.W, r.H, st, view), f0["color"], f0["mat"], f0["surf"])
    try:
        rd.UpdateAccelStruct(r.plt, r.tlas, instances(moved, shift))
        f1 = r.frame(1)
        on = dc.validity(f1["mat"], f1["surf"]) & (f1["hits"]["instanceIndex"] == moved)
        assert on.sum() >= 8 and not np.array_equal(f1["surf"]["position"][on], f0["surf"]["position"][on])
        prev = np.zeros((r.n, 4), F)
        prev[:, :3] = f1["surf"]["position"]
        prev[on, :3] = f1["surf"]["position"][on] - t
        bprev = rd.CreateBuffer(r.plt, 16 * r.n)
        rd.WriteBuffer(r.plt, bprev, 16 * r.n, prev)
        kept = {}
        for with_prev in (True, False):
            info = {}
            out = tp.TemporalAccumulate(f1["bC"], f1["bM"], f1["bS"], bview, r.W, r.H, st, h0, None, None, bprev if with_prev else None)
            got = rd.ReadBuffer(r.plt, out, 64 * r.n).view(F).reshape(4, r.n, 4).copy()
            want = tc.temporal_reference(f1["color"], f1["mat"], f1["surf"], r.W, r.H, st, view, None, first, prev if with_prev else None, info)
            assert held(got, want, f1["color"], f1["mat"], f1["surf"]), (with_prev, show(got, want, r.W))
            kept[with_prev] = (int((tc.history_length(got)[on] == 2).sum()), int(info["fail_position"][on].any(1).sum()))
            assert (tc.history_length(got)[~on & dc.validity(f1["mat"], f1["surf"])] == 2).sum() > 0
        print("instance %d, %d pixels: (kept, failed the plane test) with previous_positions %s, without %s" % (moved, int(on.sum()), kept[True], kept[False]))
        assert kept[True][0] > kept[False][0] and kept[False][1] > kept[True][1], kept
    finally:
        rd.UpdateAccelStruct(r.plt, r.tlas, instances(-1, shift))


# ---- 6. the RGBA8 image ------------------------------------------------------------------------------------------------------------------
def test_the_image_is_accumulates(mods, gpu):
    """image = what rd.Accumulate writes for plane 0 of history_out at frameID 0 into a fresh scratch, with and without the debug bit,
    invalid pixels and colours above 1 included"""
    rd, _, tp, _, _ = mods
    W, H = 65, 5
    n = W * H
    seq = tc.hostile_sequence(W, H, 55, frames=2)
    for c, *_ in seq:
        with np.errstate(all="ignore"):
            c[:, :3] = np.where(np.isfinite(c[:, :3]), c[:, :3] * F(2.5), F(0.5))    # above 1: the debug image wraps, the tone-mapped one saturates
        c[::9, :3] = F(0.01)
    fr = Frame(rd, gpu, W, H)
    images = []
    for debug in (False, True):
        st = tp.TemporalSettings(position_tolerance=0.125, debug=debug)
        h = None
        for color, mat, surf, view, previous, prev in seq:
            h, image = fr.run(tp, st, color, mat, surf, view, previous, prev, h, image=True)
        assert dc.same(h, tc.temporal_reference(color, mat, surf, W, H, st, view, previous, fr.whole("hin")[OFF["hin"]:OFF["hin"] + 64 * n].view(F).reshape(4, n, 4), prev))
        scratch, ref = rd.CreateBuffer(gpu, 16 * n), rd.CreateBuffer(gpu, 4 * n)
        assert rd.Accumulate(fr.B["hout"], n, 0, scratch, ref, debug=debug, colors_offset=OFF["hout"]) == 0
        want = rd.ReadBuffer(gpu, ref, 4 * n).reshape(n, 4)
        assert np.array_equal(image, want), (debug, np.flatnonzero((image != want).any(1))[:8])
        assert (image[:, 3] == 255).all()
        images.append(image)
    assert not np.array_equal(images[0], images[1])


# ---- 7. repeatability, aliasing, refusals ------------------------------------------------------------------------------------------------
def test_repeatability_shapes_and_refusals(mods, gpu):
    rd, _, tp, _, _lib = mods
    L = _lib.lib()
    W, H = 37, 19
    n = W * H
    seq = tc.hostile_sequence(W, H, 77, frames=2)
    st = tp.TemporalSettings(position_tolerance=0.125)
    fr = Frame(rd, gpu, W, H)
    (c0, m0, s0, v0, p0, q0), (color, mat, surf, view, previous, prev) = seq
    first, _ = fr.run(tp, st, c0, m0, s0, v0, p0, q0, None)
    got, _ = fr.run(tp, st, color, mat, surf, view, previous, prev, first, image=True)
    again, _ = fr.run(tp, st, color, mat, surf, view, previous, prev, first, image=True, refill=False)
    assert np.array_equal(dc.bits(got), dc.bits(again)), "two calls give equal bits, a reused history_out what a fresh one gives"
    assert held(got, tc.temporal_reference(color, mat, surf, W, H, st, view, previous, first, prev), color, mat, surf)
    for k in OUTPUTS:
        fr.fill(k)
    untouched = lambda: all((fr.whole(k) == 0xA5).all() for k in OUTPUTS)
    inputs = {k: fr.whole(k) for k in INPUTS}

    def raw(settings="default", **kw):
        """the library itself: no wrapper decides anything"""
        a = fr.arguments(**kw)
        s = st._struct() if isinstance(settings, str) else settings
        h = lambda b: b.handle if b is not None else None
        return L.rdx_temporal_accumulate(h(a["color"]), a["color_offset"], h(a["materials"]), a["materials_offset"], h(a["surfaces"]), a["surfaces_offset"],
                                         h(a["previous_positions"]), a["previous_positions_offset"], h(a["view"]), a["view_offset"], h(a["previous_view"]),
                                         a["previous_view_offset"], a["width"], a["height"], C.byref(s) if s is not None else None, h(a["history_in"]),
                                         a["history_in_offset"], h(a["history_out"]), a["history_out_offset"], h(a["image"]), a["image_offset"])

    # a frame of no pixels succeeds and touches nothing, in the library and through the wrapper
    for w, h in ((0, H), (W, 0), (0, 0), (0, 100000)):
        assert raw(width=w, height=h) == 0, _lib.last_error()
        fr.call(tp, st, width=w, height=h)
    assert untouched()

    def settings(**kw):
        s = st._struct()
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    null, unknown = rd.Buffer(None, 1 << 20), rd.Buffer(12345678, 1 << 20)
    wrapped = lambda k, shift: rd.WrapDeviceMemory(gpu, fr.B[k].device_ptr + shift, fr.B[k].size - shift, keepalive=fr.B[k])
    cases = [
        ("a null colour", dict(color=null), "colour buffer handle"), ("an unknown material buffer", dict(materials=unknown), "material-record buffer handle"),
        ("a null surface buffer", dict(surfaces=null), "surface-record buffer handle"), ("a null view", dict(view=null), "view buffer handle"),
        ("a null history_out", dict(history_out=null), "history-out buffer handle"), ("an unknown history_in", dict(history_in=unknown), "history-in buffer handle"),
        ("an unknown previous view", dict(previous_view=unknown), "previous-view buffer handle"), ("unknown previous positions", dict(previous_positions=unknown), "previous-position buffer handle"),
        ("an unknown image", dict(image=unknown), "image buffer handle"),
        ("no settings", dict(settings=None), "settings"), ("max_history 0", dict(settings=settings(max_history=0)), "max_history"),
        ("max_history 65536", dict(settings=settings(max_history=65536)), "max_history"), ("a negative alpha_min", dict(settings=settings(alpha_min=-0.5)), "alpha_min"),
        ("alpha_min above 1", dict(settings=settings(alpha_min=1.5)), "alpha_min"), ("a NaN alpha_min", dict(settings=settings(alpha_min=float("nan"))), "alpha_min"),
        ("a NaN alpha_moments_min", dict(settings=settings(alpha_moments_min=float("nan"))), "alpha_moments_min"),
        ("an infinite normal_cos_min", dict(settings=settings(normal_cos_min=float("inf"))), "normal_cos_min"),
        ("a NaN normal_cos_min", dict(settings=settings(normal_cos_min=float("nan"))), "normal_cos_min"),
        ("a negative position_tolerance", dict(settings=settings(position_tolerance=-1.0)), "position_tolerance"),
        ("an infinite position_tolerance", dict(settings=settings(position_tolerance=float("inf"))), "position_tolerance"),
        ("a NaN position_tolerance", dict(settings=settings(position_tolerance=float("nan"))), "position_tolerance"),
        ("variance_min_history 256", dict(settings=settings(variance_min_history=256)), "variance_min_history"),
        ("non-zero padding", dict(settings=settings(_0=1)), "padding"), ("an unknown flag", dict(settings=settings(flags=2)), "flags"),
        ("a width above the limit", dict(width=16385, height=1), "outside the supported"), ("too many pixels", dict(width=16384, height=4097), "outside the supported"),
        ("a colour offset off 16", dict(color_offset=OFF["color"] + 8), "16"), ("a material offset off 16", dict(materials_offset=OFF["mat"] + 4), "16"),
        ("a surface offset off 16", dict(surfaces_offset=OFF["surf"] + 8), "16"), ("a view offset off 16", dict(view_offset=OFF["view"] + 8), "16"),
        ("a previous view offset off 16", dict(previous_view_offset=OFF["pview"] + 4), "16"), ("a previous positions offset off 16", dict(previous_positions_offset=OFF["prev"] + 8), "16"),
        ("a history_in offset off 16", dict(history_in_offset=OFF["hin"] + 8), "16"), ("a history_out offset off 16", dict(history_out_offset=OFF["hout"] + 4), "16"),
        ("an image offset off 4", dict(image_offset=OFF["image"] + 2), "4"),
        ("colours that overrun", dict(color_offset=OFF["color"] + TAIL + 16), "colour buffer"), ("materials that overrun", dict(materials_offset=OFF["mat"] + TAIL + 16), "material-record buffer"),
        ("surfaces that overrun", dict(surfaces_offset=OFF["surf"] + TAIL + 16), "surface-record buffer"), ("a view that overruns", dict(view_offset=OFF["view"] + TAIL + 16), "view buffer"),
        ("a previous view that overruns", dict(previous_view_offset=OFF["pview"] + TAIL + 16), "previous-view buffer"),
        ("previous positions that overrun", dict(previous_positions_offset=OFF["prev"] + TAIL + 16), "previous-position buffer"),
        ("a history_in that overruns", dict(history_in_offset=OFF["hin"] + TAIL + 16), "history-in buffer"),
        ("a history_out that overruns", dict(history_out_offset=OFF["hout"] + TAIL + 16), "history-out buffer"),
        ("an image that overruns", dict(image_offset=OFF["image"] + TAIL + 4), "image buffer"), ("a frame larger than the buffers", dict(height=2 * H), "buffer"),
        ("history_out over history_in", dict(history_out=fr.B["hin"], history_out_offset=OFF["hin"] + 16), "overlap"),
        ("history_out over the last plane of history_in", dict(history_out=fr.B["hin"], history_out_offset=64 * 32 - 16, history_in_offset=0, width=8, height=4), "overlap"),
        ("history_out over the colours", dict(history_out=fr.B["color"], history_out_offset=0, width=8, height=4), "overlap"),
        ("history_out over the view", dict(history_out=fr.B["view"], history_out_offset=0, width=1, height=1), "overlap"),
        ("the image over the surfaces", dict(image=fr.B["surf"], image_offset=OFF["surf"] + 64), "overlap"),
        ("the image over the previous positions", dict(image=fr.B["prev"], image_offset=OFF["prev"]), "overlap"),
        ("the image over history_out", dict(image=fr.B["hout"], image_offset=OFF["hout"] + 32 * n), "overlap"),
        ("misaligned wrapped colours", dict(color=wrapped("color", 8), color_offset=0), "aligned"), ("a misaligned wrapped history_out", dict(history_out=wrapped("hout", 4), history_out_offset=0), "aligned"),
        ("a misaligned wrapped view", dict(view=wrapped("view", 8), view_offset=0), "aligned"), ("a misaligned wrapped image", dict(image=wrapped("image", 2), image_offset=0), "aligned"),
    ]
    for what, kw, text in cases:
        kw = dict(kw)
        s = kw.pop("settings", "default")
        assert raw(settings=s, **kw) != 0, what
        err = _lib.last_error()
        assert "rdx_temporal_accumulate" in err and text in err, (what, err)
        assert untouched(), what
    assert all(np.array_equal(fr.whole(k), inputs[k]) for k in INPUTS)
    # the wrapper carries the library's refusals, and refuses what it can decide itself
    for kw in (dict(color=null), dict(history_out=fr.B["hin"], history_out_offset=OFF["hin"] + 16), dict(width=2 * W), dict(history_out=wrapped("hout", 8), history_out_offset=0)):
        with pytest.raises(rd.RadianceError, match="[Tt]emporal"):
            fr.call(tp, st, **kw)
    assert untouched()
    after, _ = fr.run(tp, st, color, mat, surf, view, previous, prev, first)
    assert np.array_equal(dc.bits(after), dc.bits(got)), "after the refusals the call is what it was"
    # a created history_out is the call's own
    out = tp.TemporalAccumulate(fr.B["color"], fr.B["mat"], fr.B["surf"], fr.B["view"], W, H, st, fr.B["hin"], None, fr.B["pview"], fr.B["prev"], color_offset=OFF["color"],
                                materials_offset=OFF["mat"], surfaces_offset=OFF["surf"], view_offset=OFF["view"], history_in_offset=OFF["hin"], previous_view_offset=OFF["pview"],
                                previous_positions_offset=OFF["prev"])
    assert out.size == 64 * n and np.array_equal(rd.ReadBuffer(gpu, out, 64 * n).view(np.uint32), dc.bits(got).reshape(-1))


# ---- 8. torch tensors and the README's snippet -------------------------------------------------------------------------------------------
_TORCH_CHILD = r"""
import os, sys
ROOT = sys.argv[1]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
assert torch.cuda.is_available()
torch.zeros(1, device="cuda").cpu()                      # torch initialises the GPU first
import numpy as np
import rrt_amd
from radiance_ray_tracing_amd import denoise, rd, scenes, temporal
import denoise_cases as dc
import temporal_cases as tc
width, height, max_depth = 64, 32, 4
dev = scenes.DeviceScene(scenes.c1_cornell(width, height, spp=1, depth=max_depth, sphere_subdiv=3))
plt, tlas, sb, sf, camera = dev.plt, dev.topAccelStruct, dev.shading_buffers(), dev.surface_buffers(), dev.frame_buffers()[0]
blob = rd.ReadBuffer(dev.plt, tlas, tlas.size).tobytes()
s = rd.DebugAccelLayout(blob)[0]
scene_diagonal = float(np.linalg.norm(np.array(s["sceneHi"], np.float64) - np.array(s["sceneLo"], np.float64)))
eye_path = [np.array(dev.scene.camera).copy() for _ in range(4)]
for f, cam in enumerate(eye_path):
    cam["x"] += np.float32(0.05 * f)
record = []
# ---- the README's snippet
settings = temporal.TemporalSettings(position_tolerance=0.01 * scene_diagonal)
denoise_settings = denoise.DenoiseSettings(sigma_position=0.01 * scene_diagonal)
history = previous_view = None
for frame, cam in enumerate(eye_path):                              # the camera moves: its buffer is rewritten, nothing else
    rd.WriteBuffer(plt, camera, 48, cam)
    view = temporal.CameraViewTorch(camera)
    rays, keys = rd.GenerateRaysTorch(camera, width * height, frame, frame)
    hits = rd.QueryRaysTorch(tlas, rays, rd.QUERY_CLOSEST)
    surfaces, _ = rd.ResolveHitsTorch(tlas, rays, hits, sf)
    materials, _ = rd.ResolveMaterialsTorch(tlas, rays, hits, sb)
    radiance = rd.TracePathsTorch(tlas, rays, keys, max_depth, sb)
    history = temporal.TemporalAccumulateTorch(radiance, materials, surfaces, view, width, height, settings, history, previous_view)
    filtered = denoise.DenoiseTorch(history[0], materials, surfaces, width, height, denoise_settings)
    previous_view = view
    record.append((radiance, materials, surfaces, view, history, filtered))        # (this line is the test's: every frame is checked below)
# ----
n = width * height
h = pv = None
for radiance, materials, surfaces, view, history, filtered in record:
    assert isinstance(history, torch.Tensor) and history.dtype == torch.float32 and tuple(history.shape) == (4, n, 4) and history.is_cuda
    mat = materials.cpu().numpy().view(dc.MATERIAL_DTYPE).reshape(-1)
    surf = surfaces.cpu().numpy().view(dc.SURFACE_DTYPE).reshape(-1)
    v = view.cpu().numpy().reshape(-1).view(tc.VIEW_DTYPE)[0]
    want = tc.temporal_reference(radiance.cpu().numpy(), mat, surf, width, height, settings, v, pv, h)
    assert dc.same(history.cpu().numpy(), want)
    assert dc.same(filtered.cpu().numpy(), dc.denoise_reference(history[0].cpu().numpy(), mat, surf, width, height, denoise_settings))
    h, pv = history.cpu().numpy(), v
N = tc.history_length(h)
assert (N == 4).sum() > n // 4 and (N[dc.validity(mat, surf)] < 4).any(), np.bincount(N)
# the Buffer route on the same memory, and the image against rd.Accumulate
radiance, materials, surfaces, view, history, filtered = record[-1]
before, pview = record[-2][4], record[-2][3]
up = lambda t: rd.WrapDeviceMemory(None, t.data_ptr(), t.numel() * t.element_size(), keepalive=t)
out = temporal.TemporalAccumulate(up(radiance), up(materials), up(surfaces), up(view), width, height, settings, up(before), None, up(pview))
assert np.array_equal(rd.ReadBuffer(plt, out, 64 * n).view(np.uint32), history.cpu().numpy().view(np.uint32).reshape(-1))
image = torch.empty((n, 4), dtype=torch.uint8, device="cuda")
again = temporal.TemporalAccumulateTorch(radiance, materials, surfaces, view, width, height, settings, before, pview, image=image)
assert torch.equal(again.view(torch.int32), history.view(torch.int32))
scratch, ref = torch.zeros((n, 4), device="cuda"), torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
assert rd.AccumulateTorch(history[0], 0, scratch, ref) == 0 and torch.equal(ref, image) and int(image[:, :3].max()) > 0
positions = surfaces[:, :4].contiguous()
same = temporal.TemporalAccumulateTorch(radiance, materials, surfaces, view, width, height, settings, before, pview, previous_positions=positions)
assert torch.equal(same.view(torch.int32), history.view(torch.int32)), "previous_positions equal to the positions change nothing"
empty = temporal.TemporalAccumulateTorch(radiance[:0], materials[:0], surfaces[:0], view, 0, 7, settings)
assert tuple(empty.shape) == (4, 0, 4)
T = temporal.TemporalAccumulateTorch
bad = [lambda: T(radiance, materials, surfaces, view, width, height + 1, settings), lambda: T(radiance.double(), materials, surfaces, view, width, height, settings),
       lambda: T(radiance, materials[:-1], surfaces, view, width, height, settings), lambda: T(radiance, materials, surfaces[:, :8], view, width, height, settings),
       lambda: T(radiance, materials.cpu(), surfaces, view, width, height, settings), lambda: T(radiance, materials, surfaces, view, width, height, None),
       lambda: T(radiance, materials, surfaces, view[:3], width, height, settings), lambda: T(radiance, materials, surfaces, view.cpu(), width, height, settings),
       lambda: T(radiance, materials, surfaces, None, width, height, settings), lambda: T(radiance, materials, surfaces, view, width, height, settings, before[:3]),
       lambda: T(radiance, materials, surfaces, view, width, height, settings, before.reshape(n, 16)), lambda: T(radiance, materials, surfaces, view, width, height, settings, before, view.double()),
       lambda: T(radiance, materials, surfaces, view, width, height, settings, previous_positions=positions[:-1]),
       lambda: T(radiance, materials, surfaces, view, width, height, settings, image=image[:-1]), lambda: T(radiance, materials, surfaces, view, width, height, settings, image=image.float()),
       lambda: T(radiance, materials, surfaces, view, 2.5, height, settings)]
for j, fn in enumerate(bad):
    try:
        fn()
    except rd.RadianceError:
        continue
    raise AssertionError("bad argument set %d was accepted" % j)
print("TORCH-TEMPORAL-OK", n)
"""


def test_torch_tensors_and_the_readme_snippet_in_a_fresh_process(gpu):
    """the torch route equals the restatement and the Buffer route bit for bit, through the README's snippet -- trace -> temporal ->
    denoise over a camera move; a wrong dtype, shape or device is refused in Python.  torch is initialised first, in a process of
    its own (as tests/test_gpu_denoise.py)"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _TORCH_CHILD, ROOT]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "TORCH-TEMPORAL-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
