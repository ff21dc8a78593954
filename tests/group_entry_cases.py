"""Scenes, rays and blob helpers of the entry-record tests (test_group_entry_cpu.py, test_gpu_group_entry.py).

An entry record E(i) (csrc/accel_layout.h AccelLayout::entries) stands for the BLAS root R of instance slot i: a pool item that
points at it decides the root test and -- when R's box is the union of its children's boxes -- one level below.  The scenes here
have what the two forms of the record and the instance step that pushes such items (csrc/traverse_pool.h) can get wrong:

    stack40      40 small overlapping meshes, a BLAS each, under ONE non-identity transform: a group of 40 (two bitmap words), far
                 more entry items per wave than the pool holds
    mixed        a group of three, two instances with transforms of their own and a leaf-root instance
    leaf_kids    a group whose roots have one leaf child (a box: 12 triangles) or two (a strip of 8 triangles)
    non_union    leaf_kids and a sphere with every BLAS root box blown up in the blob: the root box is then NOT the union of its
                 children's boxes, and the entry record is the single-entry form
"""
import struct

import numpy as np

F = np.float32
CASES = ("stack40", "mixed", "leaf_kids", "non_union")


def strip(scenes, n, dz=0.2):
    """n disjoint triangles in a row along x (8 and more: a root with two leaf children)"""
    v, t = [], []
    for k in range(n):
        x = 1.5 * k
        v += [[x, 0, 0], [x + 1, 0, dz * k], [x, 1, 0]]
        t.append([3 * k, 3 * k + 1, 3 * k + 2])
    return scenes._finish(np.array(v, float), t, np.array([[0, 0, 1]] * len(v), float))


def shared_transform(scenes):
    return (scenes.translate(0.5, 1.0, -2.0) @ scenes.rotate_y(30.0)).astype(F)


def instances(scenes, case):
    """(meshes, [(mesh index, 4x4 float32, custom id)]) of a case"""
    tf = shared_transform(scenes)
    meshes, insts = [], []

    def add(mesh, m, cid=0):
        meshes.append(mesh)
        insts.append((len(meshes) - 1, np.asarray(m, F).copy(), cid))
    if case == "stack40":
        rng = np.random.default_rng(5)
        for k in range(40):         # boxes and small spheres threaded on the object-space z axis, overlapping their neighbours
            c = np.array([0.15 * rng.standard_normal(), 0.15 * rng.standard_normal(), 0.3 * k])
            if k % 3 == 2:
                v, t, n, uv = scenes.icosphere(1, 0.45)
                add((v + c.astype(F), t, n, uv), tf, k)
            else:
                add(scenes.box(list(c - 0.4), list(c + 0.4)), tf, k)
    elif case == "mixed":
        add(scenes.icosphere(2, 0.5), tf, 0)
        add(scenes.box([1, -1, -1], [2, 1, 1]), tf, 1)
        add(strip(scenes, 9), tf, 2)
        add(scenes.box([-3, -1, -1], [-2, 1, 1]), scenes.translate(0, 0, 4), 3)
        add(scenes.icosphere(1, 0.7), scenes.translate(1.0, 0.5, 1.0) @ scenes.rotate_y(-50.0), 4)
        add(scenes.quad([0, 0, 0], [1, 0, 0], [1, 0, 1], [0, 0, 1], [0, 1, 0]), scenes.rotate_y(20), 5)      # leaf root
    elif case in ("leaf_kids", "non_union"):
        add(scenes.box([-1, -1, -1], [1, 1, 1]), tf, 0)
        add(strip(scenes, 8), tf, 1)
        add(scenes.box([0.5, -0.5, 0.5], [2.5, 0.5, 1.5]), tf, 2)
        add(strip(scenes, 11, 0.1), tf, 3)
        if case == "non_union":
            add(scenes.icosphere(2, 0.8), tf, 4)
    else:
        raise KeyError(case)
    return meshes, insts


def inflate_roots(blob, n, by=0.25):
    """the blob with the box of every BLAS root grown by `by` on all sides (reference blob format, data.cl:237-278: a BLAS is a
    16-byte header and its nodes -- min[3], pad, max[3], pad, four words -- the root first).  The top level is left alone: a root
    box that sticks out of its top-level leaf only makes the walk miss what every engine misses alike."""
    b = bytearray(blob)
    inst_off = struct.unpack_from("<I", b, 8)[0]
    seen = set()
    for k in range(n):
        off = struct.unpack_from("<I", b, inst_off + 80 * k + 76)[0]
        if off in seen:
            continue
        seen.add(off)
        node = off + struct.unpack_from("<I", b, off + 4)[0]
        box = np.frombuffer(bytes(b[node:node + 32]), "<f4").copy()
        box[0:3] -= F(by)
        box[4:7] += F(by)
        b[node:node + 32] = box.tobytes()
    return bytes(b)


def host_blob(rd, scenes, case):
    """the product builder's blob of a case, on the host"""
    meshes, insts = instances(scenes, case)
    blases = [rd.BuildAccelStruct(None, rd.Mesh(m[0], m[1])) for m in meshes]
    blob = rd.BuildTopAccelStructBlob([rd.Instance(tf, 0, cid, blases[mi]) for mi, tf, cid in insts])[0]
    return inflate_roots(blob, len(insts)) if case == "non_union" else blob


def object_rays(rng, lo, hi, n):
    """n rays (float32 origin, direction) around the box [lo, hi]: aimed at points inside it from outside and from inside, a
    quarter of them aimed past it (they miss the box or graze it), and -- every eighth -- with one or two direction components
    exactly zero, some of those starting ON a face of the box or in the plane of one"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, e = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1e-3)
    o = c + (rng.random((n, 3)) * 2 - 1) * e * np.where(rng.random((n, 1)) < 0.3, 0.9, 3.0)
    tgt = c + (rng.random((n, 3)) * 2 - 1) * e * np.where(rng.random((n, 1)) < 0.25, 2.5, 1.0)
    d = tgt - o
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9)
    k = np.arange(n)
    z = k % 8 == 0
    ax = rng.integers(0, 3, n)
    d[z, ax[z]] = 0.0
    z2 = k % 32 == 0
    d[z2, (ax[z2] + 1) % 3] = 0.0
    face = k % 16 == 0               # ... the origin in the plane of a face, along the zeroed axis
    o[face, ax[face]] = np.where(rng.random(face.sum()) < 0.5, lo[ax[face]], hi[ax[face]])
    dead = ~np.any(d != 0.0, axis=1)
    d[dead] = [0.0, 0.0, 1.0]
    return o.astype(F), d.astype(F)


def world_rays(scenes, case, n, seed):
    """n world-space rays for a case: object_rays around the boxes of its meshes, taken through the instances' transforms (float64,
    rounded once), round robin over the instances; every fifth ray runs along the group's object-space z axis through its members"""
    meshes, insts = instances(scenes, case)
    rng = np.random.default_rng(seed)
    O, D = np.zeros((n, 3), F), np.zeros((n, 3), F)
    per = [np.flatnonzero(np.arange(n) % len(insts) == k) for k in range(len(insts))]
    for k, idx in enumerate(per):
        mi, tf, _ = insts[k]
        v = meshes[mi][0].astype(np.float64)
        o, d = object_rays(rng, v.min(0), v.max(0), len(idx))
        m = tf.astype(np.float64)
        O[idx] = (o.astype(np.float64) @ m[:3, :3].T + m[:3, 3]).astype(F)
        D[idx] = (d.astype(np.float64) @ m[:3, :3].T).astype(F)
    allv = np.concatenate([meshes[mi][0] for mi, tf, _ in insts if np.array_equal(tf, insts[0][1])]).astype(np.float64)
    lo, hi = allv.min(0), allv.max(0)
    thru = np.flatnonzero(np.arange(n) % 5 == 0)
    m = insts[0][1].astype(np.float64)
    mid = lambda k: lo[k] + (hi[k] - lo[k]) * (0.3 + 0.4 * rng.random(len(thru)))      # (the middle of the extent: through most members)
    p = np.stack([mid(0), mid(1), np.full(len(thru), lo[2] - 1.0)], 1)
    q = np.stack([mid(0), mid(1), np.full(len(thru), hi[2] + 1.0)], 1)
    dd = q - p
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    O[thru] = (p @ m[:3, :3].T + m[:3, 3]).astype(F)
    D[thru] = (dd @ m[:3, :3].T).astype(F)
    return O, D
