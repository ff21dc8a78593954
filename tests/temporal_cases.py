"""The numpy restatement of rdx_temporal_accumulate (include/rdx.h) and the synthetic frames its tests run on.

temporal_reference takes one IEEE float32 operation at a time, in the order the header states, with the exactly rounded fma, dot3
and lum of denoise_cases (whose `canon` compares a NaN as a NaN: IEEE 754 leaves the payload of a NaN an operation produces to the
implementation).  Everything that is copied rather than computed -- invalid pixels, w, the guide planes -- is compared bit for bit.
A view is a VIEW_DTYPE record: the tests that need the device's trigonometry read the record rdx_camera_view wrote and hand it in,
so cos and sin are never restated; view_of_camera is the float64 formula for the CPU tests."""
import collections

import numpy as np

import denoise_cases as dc
from denoise_cases import F, U, MATERIAL_DTYPE, SURFACE_DTYPE, bits, canon, same, dot3, lum, validity  # noqa: F401

VIEW_DTYPE = np.dtype([("eye", "<f4", 3), ("widthPixel", "<f4"), ("right", "<f4", 3), ("heightPixel", "<f4"), ("up", "<f4", 3), ("kx", "<f4"),
                       ("back", "<f4", 3), ("ky", "<f4")])
SETTINGS_DTYPE = np.dtype([("max_history", "<u4"), ("alpha_min", "<f4"), ("alpha_moments_min", "<f4"), ("normal_cos_min", "<f4"), ("position_tolerance", "<f4"),
                           ("variance_min_history", "<u4"), ("flags", "<u4"), ("_0", "<u4")])
assert VIEW_DTYPE.itemsize == 64 and SETTINGS_DTYPE.itemsize == 32

# what temporal_reference reads of its `settings`: these attributes (a temporal.TemporalSettings has them too)
Settings = collections.namedtuple("Settings", "max_history alpha_min alpha_moments_min normal_cos_min position_tolerance variance_min_history",
                                  defaults=(32, 0.05, 0.2, 0.9, 0.0, 4))


def ubits(a):
    return np.ascontiguousarray(a, F).view(U)


def project(view, Q):
    """-> (u, t, dz) of the world points Q (n, 3) under the VIEW_DTYPE record `view`"""
    view = np.asarray(view, VIEW_DTYPE).reshape(())
    eye, right, up, back = (np.asarray(view[k], F) for k in ("eye", "right", "up", "back"))
    W, H, kx, ky = (F(view[k]) for k in ("widthPixel", "heightPixel", "kx", "ky"))
    with np.errstate(all="ignore"):
        v = np.ascontiguousarray(Q, F) - eye
        dz = -dot3(back, v)
        u = W * F(0.5) + (W * kx) * (dot3(right, v) / dz)
        t = H * F(0.5) - (H * ky) * (dot3(up, v) / dz)
    return u.astype(F), t.astype(F), dz.astype(F)


def temporal_reference(color, mat, surf, W, H, settings, view, previous_view=None, history_in=None, previous_positions=None, info=None):
    """-> (4, W H, 4) float32: `history_out` of rdx_temporal_accumulate.  info: a dict that receives, per pixel and tap (j outer, i
    inner), `weights`, `counted`, and the taps that reached a consistency test and failed it: `fail_material`, `fail_normal`,
    `fail_position`"""
    n = W * H
    color = np.ascontiguousarray(color, F).reshape(n, 4)
    mat, surf = mat.reshape(n), surf.reshape(n)
    valid = validity(mat, surf)
    Nrm, P = np.ascontiguousarray(mat["normal"], F), np.ascontiguousarray(surf["position"], F)
    mi = np.ascontiguousarray(mat["materialIndex"], U)
    c = color[:, :3]
    ys, xs = np.divmod(np.arange(n), W)
    Q = P if previous_positions is None else np.ascontiguousarray(np.asarray(previous_positions, F).reshape(n, 4)[:, :3])
    pv = view if previous_view is None else previous_view
    ncm, tol = F(settings.normal_cos_min), F(settings.position_tolerance)
    vmh, maxh = int(settings.variance_min_history), int(settings.max_history)
    sw, sc, s1, s2 = np.zeros(n, F), np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, F)
    Nh = np.full(n, 0xffffffff, np.uint64)
    record = {k: np.zeros((n, 4), bool) for k in ("counted", "fail_material", "fail_normal", "fail_position")}
    record["weights"] = np.zeros((n, 4), F)
    with np.errstate(all="ignore"):
        if history_in is not None:
            hin = np.ascontiguousarray(history_in, F).reshape(4, n, 4)
            h_c, h_m1, h_m2, h_N = np.ascontiguousarray(hin[0, :, :3]), hin[1, :, 0].copy(), hin[1, :, 1].copy(), ubits(hin[1, :, 3]).astype(np.uint64)
            h_n, h_mi, h_P, h_valid = np.ascontiguousarray(hin[2, :, :3]), ubits(hin[2, :, 3]), np.ascontiguousarray(hin[3, :, :3]), ubits(hin[3, :, 3])
            uc, tc, dzc = project(view, P)
            up, tp, dzp = project(pv, Q)
            du, dt = up - uc, tp - tc
            ok = (dzc > 0) & (dzp > 0) & np.isfinite(du) & np.isfinite(dt)
            hx, hy = xs.astype(F) + du, ys.astype(F) + dt
            x0f, y0f = np.floor(hx), np.floor(hy)
            fx, fy = hx - x0f, hy - y0f
            near = ok & (x0f >= F(-1)) & (x0f <= F(W)) & (y0f >= F(-1)) & (y0f <= F(H))
            x0, y0 = np.where(near, x0f, 0).astype(np.int64), np.where(near, y0f, 0).astype(np.int64)
            wx, wy = (F(1) - fx, fx), (F(1) - fy, fy)
            for j in range(2):
                for i in range(2):
                    qx, qy = x0 + i, y0 + j
                    inside = near & valid & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    q = np.where(inside, qy * W + qx, 0)
                    w = (wx[i] * wy[j]).astype(F)
                    base = inside & (h_valid[q] == 1) & (h_N[q] >= 1)
                    okm = h_mi[q] == mi
                    okn = dot3(Nrm, h_n[q]) >= ncm
                    okp = np.ones(n, bool) if tol == 0 else (np.abs(dot3(Nrm, h_P[q] - Q)) <= tol)
                    take = base & okm & okn & okp & (w > 0) & np.isfinite(h_c[q]).all(1)
                    sc = np.where(take[:, None], sc + h_c[q] * w[:, None], sc)
                    s1 = np.where(take, s1 + h_m1[q] * w, s1)
                    s2 = np.where(take, s2 + h_m2[q] * w, s2)
                    sw = np.where(take, sw + w, sw)
                    Nh = np.where(take, np.minimum(Nh, h_N[q]), Nh)
                    k = 2 * j + i
                    record["weights"][:, k], record["counted"][:, k] = np.where(inside, w, 0), take
                    record["fail_material"][:, k], record["fail_normal"][:, k], record["fail_position"][:, k] = base & ~okm, base & ~okn, base & ~okp
        fin = np.isfinite(c).all(1)
        l = lum(c)
        has = sw > 0
        h, m1h, m2h = sc / sw[:, None], s1 / sw, s2 / sw
        Nn = np.minimum(Nh + 1, maxh)
        Nf = Nn.astype(F)
        al, am = np.fmax(F(1) / Nf, F(settings.alpha_min)), np.fmax(F(1) / Nf, F(settings.alpha_moments_min))
        lerp = h + (c - h) * al[:, None]
        m1l, m2l = m1h + (l - m1h) * am, m2h + (l * l - m2h) * am
        N = np.where(has, np.where(fin, Nn, Nh), np.where(fin, 1, 0)).astype(np.uint64)
        co = np.where((has & fin)[:, None], lerp, np.where(has[:, None], h, c)).astype(F)
        m1 = np.where(has & fin, m1l, np.where(has, m1h, np.where(fin, l, F(0)))).astype(F)
        m2 = np.where(has & fin, m2l, np.where(has, m2h, np.where(fin, l * l, F(0)))).astype(F)
        N, m1, m2 = np.where(valid, N, 0), np.where(valid, m1, F(0)), np.where(valid, m2, F(0))
        var = np.fmax(m2 - m1 * m1, F(0))
        need = valid & (N < vmh)
        if need.any():
            a1, a2, aw = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    qx, qy = xs + dx, ys + dy
                    inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    q = np.where(inside, qy * W + qx, 0)
                    w = np.fmax(dot3(Nrm, Nrm[q]), F(0)).astype(F)
                    take = need & inside & (N[q] >= 1) & (mi[q] == mi) & (w > 0) & np.isfinite(w) & np.isfinite(m1[q]) & np.isfinite(m2[q])
                    a1 = np.where(take, a1 + m1[q] * w, a1)
                    a2 = np.where(take, a2 + m2[q] * w, a2)
                    aw = np.where(take, aw + w, aw)
            some = aw > 0
            M1, M2 = np.where(some, a1 / aw, m1), np.where(some, a2 / aw, m2)
            boost = F(vmh) / np.maximum(N, 1).astype(F)
            var = np.where(need, np.fmax(M2 - M1 * M1, F(0)) * boost, var).astype(F)
    out = np.zeros((4, n, 4), F)
    out[0] = color
    out[0, valid, :3] = co[valid]
    out[1, :, 0], out[1, :, 1], out[1, :, 2] = m1, m2, var
    out[1, :, 3] = N.astype(U).view(F)
    out[1, ~valid] = 0
    out[2, :, :3], out[2, :, 3] = Nrm, mi.view(F)
    out[3, :, :3], out[3, :, 3] = P, valid.astype(U).view(F)
    if info is not None:
        info.update(record)
    return out


def history_length(history):
    return ubits(np.asarray(history, F).reshape(4, -1, 4)[1, :, 3])


# ---- views ---------------------------------------------------------------------------------------------------------------------------------
def make_view(eye, right, up, back, width, height, kx, ky):
    v = np.zeros((), VIEW_DTYPE)
    v["eye"], v["right"], v["up"], v["back"] = eye, right, up, back
    v["widthPixel"], v["heightPixel"], v["kx"], v["ky"] = width, height, kx, ky
    return v


def view_of_camera(cam):
    """the view record of a PhysicalCamera (an array of 12 numbers: widthPixel, heightPixel, focalLength, sensorWidth, focalDistance,
    fStop, x, y, z, wx, wy, wz) by the header's formula, in float64 with numpy's cos and sin, rounded once: for the CPU tests"""
    cam = np.asarray(cam, np.float64)
    wp, hp, focal, sensor = cam[:4]
    cx, sx, cy, sy, cz, sz = np.cos(cam[9]), np.sin(cam[9]), np.cos(cam[10]), np.sin(cam[10]), np.cos(cam[11]), np.sin(cam[11])
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    m = rx @ (ry @ rz)
    return make_view(cam[6:9], m[:, 0], m[:, 1], m[:, 2], wp, hp, focal / sensor, focal / (sensor * (hp / wp)))


def wall_view(W, H, shift=(0.0, 0.0)):
    """the hand-filled view under which pixel (x, y) of denoise_cases' frames -- 0.1 world units per pixel in the plane z = 0 -- lies
    at sample position (x + shift[0], y + shift[1]): right = +x, up = -y, looking along +z from 0.1 W away; with the current view
    unshifted and the previous one shifted by (a, b), a pixel of the wall finds its history at (x + a, y + b)"""
    eye = (0.05 * W - 0.1 * shift[0], 0.05 * H - 0.1 * shift[1], -0.1 * W)
    return make_view(eye, (1, 0, 0), (0, -1, 0), (0, 0, -1), W, H, 1.0, W / H)


# ---- synthetic frames ----------------------------------------------------------------------------------------------------------------------
def noisy_frames(W, H, frames, seed, grey=False):
    """`frames` frames of one wall (denoise_cases.wall) with random colours in [0, 1): -> [(color, mat, surf)]"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(frames):
        color, mat, surf = dc.wall(W, H)
        u = rng.random((W * H, 1 if grey else 3))
        color[:, :3] = u.astype(F)
        out.append((color, mat, surf))
    return out


def pan_wall(frame):
    """frame `frame` of the exact one-pixel pan: a 64 x 64 view with kx = ky = 1 faces the wall z = -64, whose point under pixel
    (x, y)'s corner is (x - 32 + frame, 32 - y, -64); the eye is at (frame, 0, 0): it moves by exactly 1 along right per frame.
    Every quantity is an integer or a dyadic fraction.  -> (color, mat, surf, view)"""
    W = H = 64
    n = W * H
    rng = np.random.default_rng(900 + frame)
    mat, surf = dc.records(n)
    ys, xs = np.divmod(np.arange(n), W)
    mat["hit"], surf["hit"] = 1, 1
    mat["normal"] = (0.0, 0.0, 1.0)
    mat["materialIndex"] = 3
    surf["position"] = np.stack([xs - 32.0 + frame, 32.0 - ys, np.full(n, -64.0)], 1).astype(F)
    color = np.zeros((n, 4), F)
    color[:, :3] = (rng.integers(0, 256, (n, 3)) / 256.0).astype(F)
    color[:, 3] = 1.0
    return color, mat, surf, make_view((float(frame), 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), W, H, 1.0, 1.0)


def hostile(W, H, seed, stride=101):
    """a frame in the style of denoise_cases.hostile, with its three facets, exact normals and material numbers, but sparser: about
    1 % of the pixels of each kind -- invalid pixels (either record, hit = 0 and hit = 2), NaN / inf / zero / 3e38 normals and
    positions, NaN / inf / -inf / 3e38 / zero colours -- and distinct bits in every w (NaN patterns among them).  Every kind is present
    from 37 x 19 on"""
    rng = np.random.default_rng(seed)
    n = W * H
    mat, surf = dc.records(n)
    ys, xs = np.divmod(np.arange(n), W)
    facet = ((xs * 3) // max(W, 1) + (ys * 2) // max(H, 1)) % 3
    normals = np.array([(0.0, 0.0, 1.0), (0.6, 0.0, 0.8), (0.0, 0.28, 0.96)], F)
    mat["normal"] = normals[facet]
    mat["hit"], surf["hit"] = 1, 1
    mat["albedo"] = rng.uniform(0.05, 1.0, (n, 3)).astype(F)
    mat["materialIndex"] = facet + 1
    depth = (0.05 * xs * (facet == 1) + 0.03 * ys * (facet == 2) + rng.normal(0.0, 0.002, n)).astype(F)
    surf["position"] = np.stack([xs * 0.1, ys * 0.1, depth], 1).astype(F)
    surf["normal"] = mat["normal"]
    color = np.zeros((n, 4), F)
    color[:, :3] = (rng.uniform(0.2, 0.8, (n, 1)) * rng.uniform(0.5, 1.5, (n, 3))).astype(F)
    wbits = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U)
    wbits[::7] |= U(0x7fc00001)                                   # NaNs with payloads
    color[:, 3] = wbits.view(F)
    kinds = rng.permutation(n)
    pick = lambda k: kinds[k::stride]                             # disjoint pixel sets

    def put(field, k, value):
        field[pick(k)] = value
    put(mat["hit"], 0, 0)
    put(surf["hit"], 1, 0)
    put(mat["hit"], 2, 2)
    put(surf["hit"], 3, 2)
    put(mat["normal"], 4, (np.nan, 0.0, 1.0))
    put(mat["normal"], 5, (np.inf, 0.0, 1.0))
    put(mat["normal"], 6, (0.0, 0.0, 0.0))
    put(mat["normal"], 7, (3e38, 3e38, 3e38))
    put(surf["position"], 8, (np.nan, 1.0, 1.0))
    put(surf["position"], 9, (np.inf, -np.inf, 1.0))
    put(surf["position"], 10, (0.0, 0.0, 0.0))
    put(surf["position"], 11, (3e38, -3e38, 3e38))
    color[pick(12), 0] = np.nan
    color[pick(13), 1] = np.inf
    color[pick(14), 2] = -np.inf
    color[pick(15), :3] = 3e38
    color[pick(16), :3] = 0.0
    put(mat["materialIndex"], 17, 9)                              # a stray material number inside a facet
    # invalid pixels carry hostile colours too: they must neither change nor be read as a tap
    color[pick(0)[::2], :3] = (1e30, np.nan, -np.inf)
    return color, mat, surf


def hostile_sequence(W, H, seed, frames=3):
    """`frames` chained frames of `hostile` under a pair of hand-filled views with a fractional pan of (0.37, 0.61) pixels per frame, so
    that all four bilinear taps carry weight; the facets, their normals and material numbers stay where they are, the hostile pixels
    move with the frame.  previous_positions are the positions, jittered, with hostile values of their own.
    -> [(color, mat, surf, view, previous_view, previous_positions)]"""
    rng = np.random.default_rng(seed)
    out = []
    for f in range(frames):
        color, mat, surf = hostile(W, H, seed + 17 * f)
        n = W * H
        view, previous = wall_view(W, H, (0.37 * f, 0.61 * f)), wall_view(W, H, (0.37 * (f - 1), 0.61 * (f - 1)))
        prev = np.zeros((n, 4), F)
        prev[:, :3] = surf["position"] + rng.normal(0.0, 0.004, (n, 3)).astype(F)
        prev[:, 3] = rng.random(n).astype(F)
        kinds = rng.permutation(n)
        prev[kinds[0::127], 0] = np.nan
        prev[kinds[1::127], 1] = np.inf
        prev[kinds[2::127], :3] = 3e38
        prev[kinds[3::127], :3] = 0.0
        prev[kinds[4::127], 2] = -1000.0        # behind the previous camera
        out.append((color, mat, surf, view, previous, prev))
    return out


GPU_SIZES = ((1, 1), (5, 3), (7, 7), (37, 19), (64, 4), (65, 5), (130, 33))
# every consistency term on, each of the two with a switch off, and the plain running mean without the spatial variance
GPU_TERMS = (("all", dict(max_history=32, alpha_min=0.05, alpha_moments_min=0.2, normal_cos_min=0.9, position_tolerance=0.125, variance_min_history=4)),
             ("normal-off", dict(max_history=2, alpha_min=0.0, alpha_moments_min=0.0, normal_cos_min=-1e30, position_tolerance=0.125, variance_min_history=2)),
             ("position-off", dict(max_history=32, alpha_min=0.2, alpha_moments_min=0.0, normal_cos_min=0.9, position_tolerance=0.0, variance_min_history=0)))


def run_sequence(seq, W, H, settings, with_previous_positions):
    """the chained histories of hostile_sequence under the restatement; history_in is absent on the first frame.  -> [history], [info]"""
    hist, infos, h = [], [], None
    for color, mat, surf, view, previous, prev in seq:
        info = {}
        h = temporal_reference(color, mat, surf, W, H, settings, view, previous, h, prev if with_previous_positions else None, info)
        hist.append(h)
        infos.append(info)
    return hist, infos
