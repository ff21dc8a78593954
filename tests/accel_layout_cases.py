"""Scenes, settings and fingerprints of the traversal-layout tests (test_accel_layout_cpu.py), and the recorder of their
fixture tests/golden/accel_layout.json.

The fixture holds, per case and (quad, cull) setting, the scalars of the derived layout and the FNV-1a-64 hash of each derived
array's bytes.  It was recorded from the commit BEFORE the derivation moved into csrc/accel_layout.cpp -- a build of that commit
with a throwaway export of the vectors it was about to upload, behind the signature of rdx_debug_accel_layout -- not from the
code under test:

    python tests/accel_layout_cases.py --lib <librdx.so of that build> --out tests/golden/accel_layout.json

Recording from a current build is only right after a deliberate change of the layout.
"""
import json
import os
import sys

import numpy as np

SETTINGS = ((1, 0), (0, 0), (1, 1))      # (quad, cull)
BUILDER_CASES = ("one_triangle", "cube", "c0", "c1_small", "shared_blas", "c2_small", "signed_zero")
CASES = BUILDER_CASES + ("leaf_root", "group_rotated", "singular", "sbt_offset", "atrium_400")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "accel_layout.json")


def scene(case):
    """the scenes.Scene of a case; instances may carry SBT offsets (Scene.sbt_offsets)"""
    from radiance_ray_tracing_amd import scenes
    tri = lambda: scenes._finish(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), [[0, 1, 2]], np.array([[0, 0, 1]] * 3))
    if case == "one_triangle":
        s = scenes.Scene("tri")
        s.add_instance(s.add_mesh(tri()), None, 0)
    elif case == "cube":
        s = scenes.Scene("cube")
        s.add_instance(s.add_mesh(scenes.box([-1, -2, -3], [1, 2, 3])), scenes.translate(1, 2, 3) @ scenes.rotate_y(33), 0)
    elif case == "c0":
        s = scenes.c0_two_boxes(32, 32)
    elif case == "c1_small":
        s = scenes.c1_cornell(32, 18, sphere_subdiv=3)
    elif case == "shared_blas":          # 9-instance grid sharing two BLAS (dedup path, bvh.cpp:575-588)
        s = scenes.Scene("grid")
        a = s.add_mesh(scenes.icosphere(2, 0.5)); b = s.add_mesh(scenes.box([-.4, -.4, -.4], [.4, .4, .4]))
        for k in range(9):
            s.add_instance(a if k % 2 else b, scenes.translate(1.5 * (k % 3), 0.3 * k, 1.5 * (k // 3)) @ scenes.rotate_y(10 * k), k)
    elif case == "c2_small":
        s = scenes.c2_atrium(32, 18, detail=0.2)
    elif case == "signed_zero":          # mixed +0 / -0 coordinates keep their sign through every min/max
        v = np.array([[0.0, 0, 0], [-0.0, 1, 0], [1, -0.0, 0], [1, 1, -0.0]] * 4, np.float32)
        v[4:] += np.arange(12, dtype=np.float32)[:, None] * 0.25
        t = np.array([[0, 1, 2], [1, 2, 3], [4, 5, 6], [5, 6, 7], [8, 9, 10], [9, 10, 11], [12, 13, 14], [13, 14, 15],
                      [0, 5, 10], [3, 6, 9]], np.uint32)
        s = scenes.Scene("zeros")
        s.meshes.append((v, t, np.zeros_like(v), np.zeros_like(v)))
        s.add_instance(0, None, 0)
    elif case == "leaf_root":            # a mesh of <= 8 triangles: its BLAS is a single leaf
        s = scenes.Scene("leaf_root")
        s.add_instance(s.add_mesh(scenes.icosphere(2, 0.5)), scenes.translate(2, 0, 0), 0)
        s.add_instance(s.add_mesh(scenes.quad([0, 0, 0], [1, 0, 0], [1, 0, 1], [0, 0, 1], [0, 1, 0])), scenes.rotate_y(20), 1)
    elif case == "group_rotated":        # two distinct meshes under one non-identity transform: a group, not the identity
        s = scenes.Scene("group_rotated")
        tf = scenes.translate(0.5, 1, -2) @ scenes.rotate_y(30)
        s.add_instance(s.add_mesh(scenes.icosphere(2, 0.5)), tf, 0)
        s.add_instance(s.add_mesh(scenes.box([1, -1, -1], [2, 1, 1])), tf, 1)
        s.add_instance(s.add_mesh(scenes.box([-3, -1, -1], [-2, 1, 1])), scenes.translate(0, 0, 4), 2)
    elif case == "singular":             # an instance whose matrix has no inverse: its inverse stays zero
        s = scenes.Scene("singular")
        s.add_instance(s.add_mesh(scenes.icosphere(2, 0.5)), scenes.scale(1, 0, 1), 0)
        s.add_instance(s.add_mesh(scenes.box([1, -1, -1], [2, 1, 1])), None, 1)
    elif case == "sbt_offset":           # a non-zero SBT offset whose rows are not the stock ones: reference-order kernel
        s = scenes.Scene("sbt_offset")
        s.add_instance(s.add_mesh(scenes.icosphere(2, 0.5)), None, 0)
        s.add_instance(s.add_mesh(scenes.box([1, -1, -1], [2, 1, 1])), scenes.translate(0, 2, 0), 1, sbt_offset=1)
    elif case == "atrium_400":           # > 256 identity instances, a BLAS each: unified tree
        s = scenes.c2_atrium_400(32, 18, detail=0.3)
    else:
        raise KeyError(case)
    return s


def blob(case):
    """the product builder's TLAS blob of a case"""
    from radiance_ray_tracing_amd import rd
    s = scene(case)
    blases = [rd.BuildAccelStruct(None, rd.Mesh(m[0], m[1])) for m in s.meshes]
    insts = [rd.Instance(tf, s.sbt_offsets.get(k, 0), mat, blases[mi]) for k, (mi, tf, mat) in enumerate(s.instances)]
    return rd.BuildTopAccelStructBlob(insts)[0]


def fnv1a64(data):
    h = 0xcbf29ce484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def fingerprint(scalars, arrays):
    """what the fixture records of one derivation: the scalars (floats by their bits) and a hash per array"""
    sc = {k: ([int(x) for x in np.array(v, np.float32).view(np.uint32)] if isinstance(v, list) else v) for k, v in scalars.items()}
    return {"scalars": sc, "hashes": {k: "%016x" % fnv1a64(a.tobytes()) for k, a in arrays.items()}}


def record(lib_path=None):
    import ctypes
    from radiance_ray_tracing_amd import rd
    lib = None
    if lib_path:
        lib = ctypes.CDLL(lib_path)
        lib.rdx_last_error.restype = ctypes.c_char_p
        lib.rdx_debug_accel_layout.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p]
    out = {}
    for case in CASES:
        b = blob(case)
        for quad, cull in SETTINGS:
            out["%s/quad%d/cull%d" % (case, quad, cull)] = fingerprint(*rd.DebugAccelLayout(b, quad, cull, lib=lib))
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import rrt_amd  # noqa: F401  (makes the package importable)
    args = dict(zip(sys.argv[1::2], sys.argv[2::2]))
    rec = record(args.get("--lib"))
    text = "{\n" + ",\n".join('"%s": %s' % (k, json.dumps(rec[k], sort_keys=True, separators=(",", ":"))) for k in sorted(rec)) + "\n}\n"
    with open(args.get("--out", GOLDEN), "w") as f:
        f.write(text)
    print("wrote", args.get("--out", GOLDEN), "fnv1a64 of the text: %016x" % fnv1a64(text.encode()))
