"""Scenes, moves and blob helpers of the TLAS-update tests (test_tlas_update_cpu.py, test_gpu_tlas_update.py).

A scene is one of tests/accel_layout_cases.scene(); a move multiplies ONE instance's matrix from the left, in float32:

    A  translate(0.37, 0, 0)   on instance 0        (a nudge: the top-level tree usually keeps its shape)
    B  translate(25, 3, -17)   on the last instance (far away: the tree is rebuilt around it, leaves merge or split)
    C  rotate_y(31)            on instance 1        (leaves the shared-transform group of identity instances)
    S  (sbt_offset only) instance 1's SBT offset 1 -> 0: the scene leaves the reference-order kernel
    K  instance 1's customInstanceID + 7: no matrix changes (the only kind of update a unified tree survives: it needs every
       instance to be the identity)

A step sequence applies its moves one on top of the other ("orig" goes back to the scene as built), so the instance lists of
[B, A, C, orig] are B(orig), A(B(orig)), C(A(B(orig))), orig.
"""
import struct

import numpy as np

import accel_layout_cases as alc

F = np.float32
SCENES = ("shared_blas", "c1_small", "c2_small", "group_rotated", "leaf_root", "singular", "sbt_offset", "atrium_400")
MOVES = ("A", "B", "C")
STEPS = ("B", "A", "C", "orig")


def moves_of(case):
    return MOVES + (("S",) if case == "sbt_offset" else ())


def instances(scene):
    """[[mesh index, 4x4 float32, SBT offset, custom id]] of a scenes.Scene, by instance number"""
    return [[mi, np.array(tf, F).reshape(4, 4), int(scene.sbt_offsets.get(k, 0)), int(mat)] for k, (mi, tf, mat) in enumerate(scene.instances)]


def target(move, n):
    """the instance a move touches, of n"""
    return {"A": 0, "B": n - 1, "C": 1, "S": 1, "K": 1}[move]


def apply(insts, move):
    """a new instance list: `move` applied to `insts`"""
    from radiance_ray_tracing_amd import scenes
    out = [[mi, tf.copy(), sbt, mat] for mi, tf, sbt, mat in insts]
    k = target(move, len(out))
    if move == "S":
        out[k][2] = 0 if out[k][2] else 1
        return out
    if move == "K":
        out[k][3] += 7
        return out
    m = {"A": scenes.translate(0.37, 0, 0), "B": scenes.translate(25, 3, -17), "C": scenes.rotate_y(31)}[move]
    out[k][1] = np.matmul(np.asarray(m, F), out[k][1]).astype(F)
    return out


def stepped(insts, steps=STEPS):
    """[(step name, instance list, touched instance)] of a step sequence; "orig" restores `insts` (touched: the last instance,
    which comes home from where B put it)"""
    cur, out = insts, []
    for s in steps:
        cur = [[mi, tf.copy(), sbt, mat] for mi, tf, sbt, mat in insts] if s == "orig" else apply(cur, s)
        out.append((s, cur, target("B" if s == "orig" else s, len(insts))))
    return out


def rd_instances(rd, insts, blases):
    return [rd.Instance(tf, sbt, mat, blases[mi]) for mi, tf, sbt, mat in insts]


def product_blob(rd, insts, blases):
    """the product builder's blob (held to the reference's builder by tests/test_cpu_oracle.py)"""
    return rd.BuildTopAccelStructBlob(rd_instances(rd, insts, blases))[0]


def oracle_blob(insts, oblases):
    """the CPU oracle's blob of the same instances (oblases: oracle_bind.OracleBlas per mesh)"""
    import oracle_bind as ob
    return ob.tlas_build([(mi, tf, sbt, mat) for mi, tf, sbt, mat in insts], oblases)[0]


# ---- the reference blob format (radiance/shader/data.cl:237-278) ----------------------------------------------------------------
def inst_byte_offset(blob):
    return struct.unpack_from("<I", blob, 8)[0]


def top_nodes(blob):
    return (inst_byte_offset(blob) - 16) // 48


def blob_instances(blob, n):
    """the n instance records, in slot order"""
    dt = np.dtype([("m", "<f4", 16), ("SBTOffset", "<u4"), ("instanceID", "<u4"), ("customInstanceID", "<u4"), ("instanceOffset", "<u4")])
    return np.frombuffer(blob, dt, n, inst_byte_offset(blob))


def blob_insts_of(blob, n):
    """[[None, 4x4, SBT offset, custom id]] read from a blob's instance records, by slot"""
    return [[None, r["m"].reshape(4, 4).copy(), int(r["SBTOffset"]), int(r["customInstanceID"])] for r in blob_instances(blob, n)]


def slot_sequence(blob, n):
    """instanceID by slot"""
    return blob_instances(blob, n)["instanceID"].tolist()


def blas_region(blob, n):
    return blob[inst_byte_offset(blob) + 80 * n:]


def world_box(blob, n, inst):
    """world-space box of instance `inst`: its BLAS root box (first node behind the 16-byte BLAS header) through its matrix, in
    float64 -> (lo[3], hi[3])"""
    rec = blob_instances(blob, n)
    r = rec[[int(x) for x in rec["instanceID"]].index(inst)]
    node = np.frombuffer(blob, "<f4", 8, int(r["instanceOffset"]) + 16).astype(np.float64)
    lo, hi = node[0:3], node[4:7]
    m = r["m"].astype(np.float64).reshape(4, 4)
    c = np.array([[(hi if (k >> a) & 1 else lo)[a] for a in range(3)] + [1.0] for k in range(8)])
    w = c @ m.T
    return w[:, :3].min(0), w[:, :3].max(0)
