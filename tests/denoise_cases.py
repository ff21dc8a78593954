"""The numpy restatement of rdx_denoise (include/rdx.h) and the synthetic frames its tests run on.

denoise_reference takes one IEEE float32 operation at a time, in the order the header states: float32 arrays keep numpy's + - * /
in float32, np.fmax is fmaxf (a NaN operand is dropped), and fma -- the device's dot3 is fma(z, z', fma(y, y', x x')) -- is the
exactly rounded one: the product of two float32 is exact in float64, the sum is taken in float64 and forced to round-to-odd with
the error term of TwoSum, and a round-to-odd double rounds to the float32 a single rounding gives (53 >= 2 * 24 + 2).
IEEE 754 leaves the payload and the sign of a NaN that an operation produces to the implementation (x86 makes 0xffc00000 of inf
- inf, the GPU 0x7fc00000), so `canon` compares a NaN as a NaN: the bits of every other value, and of everything that is copied
rather than computed -- invalid pixels, w -- are compared as they are."""
import collections

import numpy as np

F = np.float32
U = np.uint32
H5 = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))
MIN_ALBEDO = F(0.015625)
MATERIAL_DTYPE = np.dtype([("normal", "<f4", 3), ("hit", "<u4"), ("albedo", "<f4", 3), ("materialIndex", "<u4"), ("metallic", "<f4"), ("roughness", "<f4"),
                           ("transmission", "<f4"), ("ior", "<f4"), ("above", "<f4", 3), ("_0", "<u4")])
SURFACE_DTYPE = np.dtype([("position", "<f4", 3), ("hit", "<u4"), ("normal", "<f4", 3), ("materialIndex", "<u4"), ("above", "<f4", 3), ("u", "<f4"),
                          ("below", "<f4", 3), ("v", "<f4")])
assert MATERIAL_DTYPE.itemsize == 64 and SURFACE_DTYPE.itemsize == 64
SETTINGS_DTYPE = np.dtype([("passes", "<u4"), ("normal_squarings", "<u4"), ("sigma_position", "<f4"), ("sigma_colour", "<f4"), ("flags", "<u4"), ("_0", "<u4", 3)])
assert SETTINGS_DTYPE.itemsize == 32

# what denoise_reference reads of its `settings`: these attributes (a denoise.DenoiseSettings has them too)
Settings = collections.namedtuple("Settings", "passes normal_squarings sigma_position sigma_colour demodulate", defaults=(5, 5, 0.0, 0.0, True))


def bits(a):
    return np.ascontiguousarray(a, F).view(U)


def canon(a):
    """the bits of float32 `a`, every NaN as 0x7fc00000"""
    a = np.ascontiguousarray(a, F)
    return np.where(np.isnan(a), U(0x7fc00000), a.view(U))


def same(a, b):
    return np.array_equal(canon(a), canon(b))


def fma(a, b, c):
    """the correctly rounded float32 a * b + c"""
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                        # exact: 48 bits
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)  # TwoSum: s + err is the exact sum where both are finite
        odd = (s.view(np.uint64) & np.uint64(1)).astype(bool)
        nudge = np.isfinite(s) & np.isfinite(err) & (err != 0.0) & ~odd
        toward = np.where(err > 0.0, np.inf, -np.inf)
        s = np.where(nudge, np.nextafter(s, toward), s)
        return s.astype(F)


def dot3(a, b):
    """device_math.h: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))"""
    with np.errstate(all="ignore"):
        return fma(a[..., 2], b[..., 2], fma(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def lum(c):
    with np.errstate(all="ignore"):
        return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def validity(mat, surf):
    return (mat["hit"] == 1) & (surf["hit"] == 1)


def den_of(mat, demodulate):
    n = mat.shape[0]
    if not demodulate:
        return np.ones((n, 3), F)
    return np.fmax(mat["albedo"].astype(F), MIN_ALBEDO)


def denoise_reference(color, mat, surf, W, H, settings):
    """-> (W H, 4) float32: `out` of rdx_denoise for (W H, 4) float32 colours, MATERIAL_DTYPE and SURFACE_DTYPE records"""
    n = W * H
    color = np.ascontiguousarray(color, F).reshape(n, 4)
    mat, surf = mat.reshape(n), surf.reshape(n)
    valid = validity(mat, surf)
    den = den_of(mat, settings.demodulate)
    N, P = np.ascontiguousarray(mat["normal"], F), np.ascontiguousarray(surf["position"], F)
    sp0, sc0 = F(settings.sigma_position), F(settings.sigma_colour)
    ys, xs = np.divmod(np.arange(n), W)
    with np.errstate(all="ignore"):
        it = color[:, :3].copy()
        it[valid] = color[valid, :3] / den[valid]
        for j in range(int(settings.passes)):
            s = 1 << j
            sp, sc = sp0 * F(s), sc0 * F(2.0 ** -j)
            lp = lum(it)
            acc, accw = np.zeros((n, 3), F), np.zeros(n, F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qx, qy = xs + dx * s, ys + dy * s
                    inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    q = np.where(inside, qy * W + qx, 0)
                    k = H5[dy + 2] * H5[dx + 2]
                    t = np.fmax(dot3(N, N[q]), F(0))
                    for _ in range(int(settings.normal_squarings)):
                        t = t * t
                    wz = F(1) if sp0 == 0 else np.fmax(F(1) - np.abs(dot3(N, P[q] - P)) / sp, F(0))
                    if sc0 == 0:
                        wc = F(1)
                    else:
                        x = np.abs(lp - lp[q]) / sc
                        wc = F(1) / (F(1) + x * x)
                    w = (((k * t) * wz) * wc).astype(F)
                    take = valid & inside & valid[q] & (w > 0) & np.isfinite(it[q]).all(1)
                    acc = np.where(take[:, None], acc + it[q] * w[:, None], acc)
                    accw = np.where(take, accw + w, accw)
            done = valid & (accw > 0)
            it = np.where(done[:, None], acc / accw[:, None], it).astype(F)
        out = color.copy()
        out[valid, :3] = (it * den)[valid]
    return out


# ---- synthetic frames --------------------------------------------------------------------------------------------------------------------
def records(n):
    mat, surf = np.zeros(n, MATERIAL_DTYPE), np.zeros(n, SURFACE_DTYPE)
    return mat, surf


def wall(W, H, colour=(0.25, 0.5, 0.75), albedo=(0.5, 0.5, 0.5)):
    """a flat wall z = 0 facing +z, 0.1 world units per pixel, of one colour: every pixel valid"""
    n = W * H
    mat, surf = records(n)
    ys, xs = np.divmod(np.arange(n), W)
    mat["hit"], surf["hit"] = 1, 1
    mat["normal"] = (0.0, 0.0, 1.0)
    mat["albedo"] = albedo
    surf["position"] = np.stack([xs * 0.1, ys * 0.1, np.zeros(n)], 1).astype(F)
    color = np.zeros((n, 4), F)
    color[:, :3] = colour
    color[:, 3] = 1.0
    return color, mat, surf


def two_halves(W, H, seed=3):
    """left half: a wall facing +z; right half: one facing +x, perpendicular to it; random colours of two disjoint ranges"""
    rng = np.random.default_rng(seed)
    color, mat, surf = wall(W, H)
    n = W * H
    xs = np.arange(n) % W
    right = xs >= W // 2
    mat["normal"][right] = (1.0, 0.0, 0.0)
    color[:, :3] = rng.uniform(0.1, 0.4, (n, 3)).astype(F)
    color[right, :3] = rng.uniform(2.0, 3.0, (int(right.sum()), 3)).astype(F)
    return color, mat, surf, right


def noisy_wall(W, H, seed=7):
    rng = np.random.default_rng(seed)
    color, mat, surf = wall(W, H)
    color[:, :3] = rng.uniform(0.0, 1.0, (W * H, 3)).astype(F)
    return color, mat, surf


def hostile(W, H, seed):
    """a frame of three facets with exact normals and noisy colours, sprinkled with what a caller may hand in: invalid pixels (either
    record, hit = 0 and hit = 2), albedo 0 / NaN / negative, NaN / inf / zero / 3e38 normals and positions, NaN / inf / huge
    colours, and distinct bits in every w (NaN patterns among them).  Every kind is present from 37 x 19 on"""
    rng = np.random.default_rng(seed)
    n = W * H
    mat, surf = records(n)
    ys, xs = np.divmod(np.arange(n), W)
    facet = ((xs * 3) // max(W, 1) + (ys * 2) // max(H, 1)) % 3
    normals = np.array([(0.0, 0.0, 1.0), (0.6, 0.0, 0.8), (0.0, 0.28, 0.96)], F)      # float32 vectors a few ulps from unit length
    mat["normal"] = normals[facet]
    mat["hit"], surf["hit"] = 1, 1
    mat["albedo"] = rng.uniform(0.05, 1.0, (n, 3)).astype(F)
    mat["materialIndex"] = facet
    depth = (0.05 * xs * (facet == 1) + 0.03 * ys * (facet == 2) + rng.normal(0.0, 0.002, n)).astype(F)
    surf["position"] = np.stack([xs * 0.1, ys * 0.1, depth], 1).astype(F)
    surf["normal"] = mat["normal"]
    color = np.zeros((n, 4), F)
    color[:, :3] = (rng.uniform(0.2, 0.8, (n, 1)) * rng.uniform(0.5, 1.5, (n, 3))).astype(F)
    wbits = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U)
    wbits[::7] |= U(0x7fc00001)                                   # NaNs with payloads
    color[:, 3] = wbits.view(F)
    kinds = rng.permutation(n)
    pick = lambda k: kinds[k::23]                                 # disjoint pixel sets, about 4 % each

    def put(field, k, value):
        field[pick(k)] = value
    put(mat["hit"], 0, 0)
    put(surf["hit"], 1, 0)
    put(mat["hit"], 2, 2)
    put(surf["hit"], 3, 2)
    put(mat["albedo"], 4, (0.0, 0.0, 0.0))
    put(mat["albedo"], 5, (np.nan, 0.5, np.nan))
    put(mat["albedo"], 6, (-0.5, -0.0, 0.25))
    put(mat["normal"], 7, (np.nan, 0.0, 1.0))
    put(mat["normal"], 8, (np.inf, 0.0, 1.0))
    put(mat["normal"], 9, (0.0, 0.0, 0.0))
    put(mat["normal"], 10, (3e38, 3e38, 3e38))
    put(surf["position"], 11, (np.nan, 1.0, 1.0))
    put(surf["position"], 12, (np.inf, -np.inf, 1.0))
    put(surf["position"], 13, (0.0, 0.0, 0.0))
    put(surf["position"], 14, (3e38, -3e38, 3e38))
    color[pick(15), 0] = np.nan
    color[pick(16), 1] = np.inf
    color[pick(17), 2] = -np.inf
    color[pick(18), :3] = 3e38
    color[pick(19), :3] = 0.0
    # invalid pixels carry hostile colours too: they must neither change nor be read as a neighbour
    color[pick(0)[::2], :3] = (1e30, np.nan, -np.inf)
    return color, mat, surf


GPU_SIZES = ((1, 1), (5, 3), (37, 19), (64, 4), (65, 5), (130, 33))
GPU_PASSES = (0, 1, 2, 3, 5, 8)
# every term off, each term on alone, and all of them
GPU_TERMS = (("off", dict(normal_squarings=0, sigma_position=0.0, sigma_colour=0.0, demodulate=False)),
             ("normal", dict(normal_squarings=5, sigma_position=0.0, sigma_colour=0.0, demodulate=False)),
             ("position", dict(normal_squarings=0, sigma_position=0.05, sigma_colour=0.0, demodulate=False)),
             ("colour", dict(normal_squarings=0, sigma_position=0.0, sigma_colour=0.35, demodulate=False)),
             ("demodulate", dict(normal_squarings=0, sigma_position=0.0, sigma_colour=0.0, demodulate=True)),
             ("all", dict(normal_squarings=3, sigma_position=0.08, sigma_colour=0.5, demodulate=True)))
