"""The numpy restatement of rdx_svgf_filter (include/rdx.h) and the synthetic frames its tests run on.

svgf_reference takes one IEEE float32 operation at a time, in the order the header states, built from denoise_cases' fma, dot3, lum,
canon and same (see there for how a NaN is compared).  np.sqrt on float32 is the correctly rounded square root, as the device's
sqrtf is."""
import collections

import numpy as np

import denoise_cases as dc

F = np.float32
U = np.uint32
G3 = (F(0.25), F(0.5), F(0.25))
SETTINGS_DTYPE = np.dtype([("passes", "<u4"), ("normal_squarings", "<u4"), ("sigma_position", "<f4"), ("sigma_luminance", "<f4"), ("epsilon", "<f4"),
                           ("feedback_pass", "<u4"), ("flags", "<u4"), ("_0", "<u4")])
assert SETTINGS_DTYPE.itemsize == 32

# what svgf_reference reads of its `settings`: these attributes (a svgf.FilterSettings has them too)
Settings = collections.namedtuple("Settings", "passes normal_squarings sigma_position sigma_luminance epsilon feedback_pass demodulate",
                                  defaults=(5, 5, 0.0, 4.0, 1e-6, 0, True))
Result = collections.namedtuple("Result", "out variance feedback")


def svgf_reference(color, moments, mat, surf, W, H, settings, info=None):
    """-> Result(out (W H, 4), variance_out (W H,), feedback (W H, 4) or None) of rdx_svgf_filter for (W H, 4) float32 colours and
    moments, MATERIAL_DTYPE and SURFACE_DTYPE records.  info (a dict): info["lost"][j] is the mask of valid pixels whose v_j, the
    variance pass j reads, is not finite"""
    n = W * H
    color = np.ascontiguousarray(color, F).reshape(n, 4)
    vz = np.ascontiguousarray(moments, F).reshape(n, 4)[:, 2]
    mat, surf = mat.reshape(n), surf.reshape(n)
    valid = dc.validity(mat, surf)
    den = dc.den_of(mat, settings.demodulate)
    N, P = np.ascontiguousarray(mat["normal"], F), np.ascontiguousarray(surf["position"], F)
    sp0, sl, eps = F(settings.sigma_position), F(settings.sigma_luminance), F(settings.epsilon)
    ys, xs = np.divmod(np.arange(n), W)
    feedback = None

    def emit(it):
        o = color.copy()
        o[valid, :3] = (it * den)[valid]
        return o

    def neighbour(dx, dy):
        qx, qy = xs + dx, ys + dy
        inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        return inside, np.where(inside, qy * W + qx, 0)

    with np.errstate(all="ignore"):
        ld = dc.lum(den) if settings.demodulate else np.ones(n, F)
        it = color[:, :3].copy()
        it[valid] = color[valid, :3] / den[valid]
        v = np.where(valid & (vz > 0) & (vz < np.inf), vz / (ld * ld), F(0)).astype(F)
        for j in range(int(settings.passes)):
            s = 1 << j
            if info is not None:
                info.setdefault("lost", []).append(valid & ~np.isfinite(v))
            sp = sp0 * F(s)
            lp = dc.lum(it)
            dl = np.zeros(n, F)
            if sl != 0:
                gs, gw = np.zeros(n, F), np.zeros(n, F)
                for dy in range(-1, 2):
                    for dx in range(-1, 2):
                        inside, q = neighbour(dx, dy)
                        k = G3[dy + 1] * G3[dx + 1]
                        take = inside & valid[q]
                        gs = np.where(take, gs + k * v[q], gs)
                        gw = np.where(take, gw + k, gw)
                dl = (sl * np.sqrt(gs / gw) + eps).astype(F)
            acc, accv, accw = np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    inside, q = neighbour(dx * s, dy * s)
                    k = dc.H5[dy + 2] * dc.H5[dx + 2]
                    t = np.fmax(dc.dot3(N, N[q]), F(0))
                    for _ in range(int(settings.normal_squarings)):
                        t = t * t
                    wz = F(1) if sp0 == 0 else np.fmax(F(1) - np.abs(dc.dot3(N, P[q] - P)) / sp, F(0))
                    if sl == 0:
                        wc = F(1)
                    else:
                        x = np.abs(lp - lp[q]) / dl
                        wc = F(1) / (F(1) + x * x)
                    w = (((k * t) * wz) * wc).astype(F)
                    take = valid & inside & valid[q] & (w > 0) & np.isfinite(it[q]).all(1) & np.isfinite(v[q])
                    acc = np.where(take[:, None], acc + it[q] * w[:, None], acc)
                    accv = np.where(take, accv + v[q] * (w * w), accv)
                    accw = np.where(take, accw + w, accw)
            done = valid & (accw > 0)
            it = np.where(done[:, None], acc / accw[:, None], it).astype(F)
            v = np.where(done, accv / (accw * accw), v).astype(F)
            if j + 1 == int(settings.feedback_pass):
                feedback = emit(it)
        out = emit(it)
        variance = np.where(valid, v * (ld * ld), F(0)).astype(F)
    return Result(out, variance, feedback)


def reach_of_lost_variance(lost, W, H):
    """-> the mask of pixels a variance outside float32's range can have reached: rdx_svgf_filter drops a tap whose v_j is not finite
    (w * w or sumw * sumw over- or underflowed where sum / sumw did not), which rdx_denoise keeps.  A pixel is reached in pass j if
    one of its 25 taps at step 1 << j has lost its variance or was reached before"""
    reached = np.zeros((H, W), bool)
    for j, mask in enumerate(lost):
        src = reached | mask.reshape(H, W)
        s = 1 << j
        nxt = np.zeros((H, W), bool)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                if abs(oy) >= H or abs(ox) >= W:
                    continue
                nxt[max(0, -oy):H - max(0, oy), max(0, -ox):W - max(0, ox)] |= src[max(0, oy):H - max(0, -oy), max(0, ox):W - max(0, -ox)]
        reached = nxt
    return reached.reshape(-1)


# ---- synthetic frames --------------------------------------------------------------------------------------------------------------------
def moments_of(variance):
    """a moments plane (m1 | m2 | variance | N) that carries `variance` and distinct bits in what is not read"""
    variance = np.asarray(variance, F).reshape(-1)
    m = np.zeros((variance.size, 4), F)
    m[:, 0], m[:, 1], m[:, 2] = F(0.5), np.nan, variance
    m[:, 3] = np.arange(variance.size, dtype=U).view(F)
    return m


def benign_variance(n, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, n).astype(F)


def hostile_variance(n, seed):
    """variances between 1e-4 and 0.1, sprinkled with what a caller may hand in: 0, -0, NaN, +inf, -inf, negative, 3e38, a denormal.
    Every kind is present from 37 x 19 on"""
    rng = np.random.default_rng(seed)
    v = (10.0 ** rng.uniform(-4.0, -1.0, n)).astype(F)
    kinds = rng.permutation(n)
    for k, value in enumerate((0.0, -0.0, np.nan, np.inf, -np.inf, -0.25, 3e38, 1e-41)):
        v[kinds[k::29]] = value
    return v


def step_wall(W=64, H=32, lo=0.2, hi=0.8, amp=0.05, seed=5):
    """the wall of the issue: a luminance step lo | hi at x = W / 2, grey uniform noise of +- amp, the true variance amp^2 / 3 as
    guide -> colour, moments, mat, surf, the noise-free colours (W H, 3)"""
    rng = np.random.default_rng(seed)
    color, mat, surf = dc.wall(W, H)
    xs = np.arange(W * H) % W
    base = np.where(xs < W // 2, lo, hi)[:, None] * np.ones((1, 3))
    color[:, :3] = (base + rng.uniform(-amp, amp, (W * H, 1))).astype(F)
    return color, moments_of(np.full(W * H, amp * amp / 3.0)), mat, surf, base


def checker(W, H, lo=0.25, hi=0.75):
    """a noise-free checker pattern on the flat wall"""
    color, mat, surf = dc.wall(W, H)
    ys, xs = np.divmod(np.arange(W * H), W)
    color[:, :3] = np.where((xs + ys) % 2 == 0, lo, hi)[:, None].astype(F)
    return color, mat, surf


# every term off, each term on alone, and all of them
GPU_TERMS = (("off", dict(normal_squarings=0, sigma_position=0.0, sigma_luminance=0.0, demodulate=False)),
             ("normal", dict(normal_squarings=5, sigma_position=0.0, sigma_luminance=0.0, demodulate=False)),
             ("position", dict(normal_squarings=0, sigma_position=0.05, sigma_luminance=0.0, demodulate=False)),
             ("luminance", dict(normal_squarings=0, sigma_position=0.0, sigma_luminance=4.0, demodulate=False)),
             ("demodulate", dict(normal_squarings=0, sigma_position=0.0, sigma_luminance=0.0, demodulate=True)),
             ("all", dict(normal_squarings=3, sigma_position=0.08, sigma_luminance=2.5, epsilon=1e-3, demodulate=True)))
