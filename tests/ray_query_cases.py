"""Shared inputs of the ray-query tests (tests/test_ray_query_cpu.py, tests/test_gpu_ray_query.py): ONE batch per scene that holds
every cell of tests/ray_edge_cases.py at once, each ray carrying the interval of the cell it comes from, in a fixed random order --
so that neighbouring lanes of a wave hold different intervals (13 to 30 distinct ones per aligned block of 64 rays).  The wanted
records are the reference's own answers from tests/golden/refgpu_rayedges.npz, permuted alike; nothing of the product shapes them.
"""
import numpy as np

import oracle_bind as ob
from test_ray_edges_cpu import load_cells

RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("direction", "<f4", 3), ("tmax", "<f4")])          # rdx_ray
RAY_HIT_DTYPE = np.dtype([("t", "<f4"), ("b1", "<f4"), ("b2", "<f4"), ("hit", "<u4"), ("primitiveIndex", "<u4"),
                          ("instanceIndex", "<u4"), ("instanceCustomIndex", "<u4"), ("instanceSBTOffset", "<u4")])   # rdx_ray_hit
SEED = 53
# rays / closest hits per scene, computed on the CPU from the fixture when this file was written
SIZES = {"c0": (92800, 8335), "c1": (48256, 22266), "c2": (27776, 13611), "edges_inst": (39808, 3681),
         "edges_inst_id": (35200, 3316), "planes": (20480, 5134)}


def query_records(h):
    """HitData records (ob.HIT_DTYPE; zeros where the reference missed) -> the 32-byte records rdx_query_rays writes"""
    out = np.zeros(h.shape[0], RAY_HIT_DTYPE)
    m = h["hit"] == 1
    out["hit"] = h["hit"]
    out["t"][m] = h["distance"][m]
    out["b1"][m] = h["barycentric"][m, 1]
    out["b2"][m] = h["barycentric"][m, 2]
    for f in ("primitiveIndex", "instanceIndex", "instanceCustomIndex", "instanceSBTOffset"):
        out[f][m] = h[f][m]
    return out


def mixed_batch(scenes, G, name):
    """-> (rays RAY_DTYPE, wanted closest-hit records RAY_HIT_DTYPE, wanted any-hit flags uint32) of one scene"""
    cells, want = load_cells(scenes, G, name)
    n = sum(c.n for c in cells)
    rays = np.zeros(n, RAY_DTYPE)
    rays["origin"] = np.concatenate([c.o for c in cells])
    rays["direction"] = np.concatenate([c.d for c in cells])
    rays["tmin"] = np.concatenate([np.full(c.n, c.tmin, np.float32) for c in cells])
    rays["tmax"] = np.concatenate([np.full(c.n, c.tmax, np.float32) for c in cells])
    w1 = query_records(np.concatenate([a for a, _ in want]))
    w2 = np.concatenate([b for _, b in want]).astype(np.uint32)
    assert w1.shape[0] == n == w2.shape[0]
    perm = np.random.default_rng(SEED).permutation(n)
    return np.ascontiguousarray(rays[perm]), np.ascontiguousarray(w1[perm]), np.ascontiguousarray(w2[perm])


def any_records(flags):
    """the records an any-hit query writes: the flag, everything else 0"""
    out = np.zeros(flags.shape[0], RAY_HIT_DTYPE)
    out["hit"] = flags
    return out


def words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, 8)


def mismatches(want, got):
    """per ray: any of the eight words differs (hit flag everywhere, the other seven bit for bit: the reference's on a hit, 0 else)"""
    return (words(want) != words(got)).any(1)


def interval_keys(rays):
    return (rays["tmin"].view(np.uint32).astype(np.uint64) << np.uint64(32)) | rays["tmax"].view(np.uint32).astype(np.uint64)


def distinct_per_block(rays, block=64):
    """distinct (tmin, tmax) bit patterns in every aligned block of `block` consecutive rays (the last, partial block included)"""
    k = interval_keys(rays)
    return np.array([np.unique(k[i:i + block]).shape[0] for i in range(0, k.shape[0], block)])
