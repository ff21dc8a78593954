"""The traversal layout derived from a TLAS blob (csrc/accel_layout.cpp), checked on the host through rdx_debug_accel_layout.

* fingerprints: scalars and per-array hashes equal tests/golden/accel_layout.json, which was recorded from the commit before the
  derivation became a unit of its own (accel_layout_cases.py says how) -- the move changed no record;
* rejections: every corruption the validator names is refused with its message;
* invariants that hold for any correct layout, read off the arrays.
"""
import json
import struct

import numpy as np
import pytest

import accel_layout_cases as alc

WIDE_LEAF = 0x80000000
CULL_AUTO_MIN_WIDE = 1 << 20


@pytest.fixture(scope="module")
def rd(built):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd
    return rd


@pytest.fixture(scope="module")
def blobs(rd):
    return {case: alc.blob(case) for case in alc.CASES}


@pytest.fixture(scope="module")
def golden():
    with open(alc.GOLDEN) as f:
        return json.load(f)


def test_seam_needs_no_device(rd, blobs):
    """the seam runs before (and without) rdx_init: nothing here has created a Platform"""
    scalars, arrays = rd.DebugAccelLayout(blobs["cube"])
    assert scalars["nInst"] == 1 and arrays["groupBits"].shape == (9,)
    with pytest.raises(rd.RadianceError, match="TLAS buffer too small"):
        rd.DebugAccelLayout(b"\0" * 8)


@pytest.mark.parametrize("quad,cull", alc.SETTINGS)
@pytest.mark.parametrize("case", alc.CASES)
def test_fingerprint(rd, blobs, golden, case, quad, cull):
    want = golden["%s/quad%d/cull%d" % (case, quad, cull)]
    scalars, arrays = rd.DebugAccelLayout(blobs[case], quad, cull)
    got = alc.fingerprint(scalars, arrays)
    assert got["scalars"] == want["scalars"]
    for name, _ in rd.ACCEL_ARRAYS:
        assert got["hashes"][name] == want["hashes"][name], "%s: %d records" % (name, arrays[name].shape[0])


def test_cases_cover_what_they_are_for(golden):
    """the special cases reach the branches they were made for (read from the recorded scalars)"""
    s = lambda case: golden[case + "/quad1/cull0"]["scalars"]
    assert s("leaf_root")["leafRoots"] == 1
    assert s("group_rotated")["groupCount"] == 2 and s("group_rotated")["groupIdentity"] == 0
    assert s("c2_small")["groupCount"] == 25 and s("c2_small")["groupIdentity"] == 1
    assert s("sbt_offset")["sbtOffsets"] == 1 and s("singular")["sbtOffsets"] == 0
    assert s("atrium_400")["nInst"] > 256 and s("atrium_400")["unifiedRoot"] > 0 and s("atrium_400")["unifiedNeed"] > 0
    assert s("c2_small")["unifiedRoot"] == 0


def test_singular_instance_keeps_zero_inverse(rd, blobs):
    _, arrays = rd.DebugAccelLayout(blobs["singular"])
    assert not arrays["insts"]["inv"][0].any() and arrays["insts"]["worldMin"][0][3] == -1.0
    assert np.array_equal(arrays["insts"]["inv"][1], np.eye(4, dtype=np.float32).reshape(-1))


# ---- rejections ---------------------------------------------------------------------------------------------------------------
def _u32(blob, off):
    return struct.unpack_from("<I", blob, off)[0]


def _poke(blob, off, value):
    b = bytearray(blob)
    struct.pack_into("<I", b, off, value)
    return bytes(b)


def _nodes(blob, off, n):
    """[(byte offset of w0, w0, w1)] of n 48-byte nodes at `off`"""
    return [(off + 48 * i + 32, _u32(blob, off + 48 * i + 32), _u32(blob, off + 48 * i + 36)) for i in range(n)]


def test_corrupted_blobs_are_refused(rd, blobs):
    blob = blobs["shared_blas"]          # 9 instances: inner top-level nodes, and BLASes with inner nodes
    inst_off = _u32(blob, 8)
    top = _nodes(blob, 16, (inst_off - 16) // 48)
    assert not top[0][1] & 0x80000000
    blas = _u32(blob, inst_off + 76)      # instance 0: instanceOffset
    node_off, face_off, vert_off = (_u32(blob, blas + 4 * k) for k in (1, 2, 3))
    bn = _nodes(blob, blas + node_off, (face_off - node_off) // 48)
    assert not bn[0][1] & 0x80000000
    tleaf = next(i for i, n in enumerate(top) if n[1] & 0x80000000)
    bleaf = next(i for i, n in enumerate(bn) if n[1] & 0x80000000)
    cases = [
        (_poke(blob, top[0][0], len(top) + 5), "TLAS blob: child index out of range"),
        (_poke(blob, bn[0][0], len(bn)), "BLAS blob: child index out of range"),
        (_poke(blob, top[0][0], 2), "TLAS blob: node 0 is not in DFS pre-order (children 2, %u)" % top[0][2]),
        (_poke(blob, bn[0][0] + 4, 1), "BLAS blob: node 0 is not in DFS pre-order (children 1, 1)"),
        (_poke(blob, top[tleaf][0] + 4, top[tleaf][2] + 1),
         "TLAS blob: leaf %u does not list its instances in leaf order (start %u, expected %u)" % (tleaf, top[tleaf][2] + 1, top[tleaf][2])),
        (_poke(blob, bn[bleaf][0] + 4, bn[bleaf][2] + 1),
         "BLAS blob: leaf %u does not list its triangles in leaf order (start %u, expected %u)" % (bleaf, bn[bleaf][2] + 1, bn[bleaf][2])),
        (_poke(blob, inst_off + 76, len(blob)), "TLAS blob: BLAS offset out of range"),
        (_poke(blob, blas + face_off, 0x0fffffff), "BLAS blob: vertex index out of range"),
    ]
    rd.DebugAccelLayout(blob)            # the blob itself is fine
    for bad, message in cases:
        with pytest.raises(rd.RadianceError) as e:
            rd.DebugAccelLayout(bad)
        assert str(e.value) == message


# ---- invariants ---------------------------------------------------------------------------------------------------------------
def _leaf_run(d0, d1):
    return int(d0) & ((1 << 25) - 1), (int(d1) >> 24) & 0x7f


@pytest.mark.parametrize("case", alc.CASES)
def test_every_triangle_belongs_to_one_leaf(rd, blobs, case):
    """every triangle slot is referenced by exactly one leaf descriptor of the wide records reachable from the instance roots"""
    _, a = rd.DebugAccelLayout(blobs[case])
    wide, refs = a["wide"], np.zeros(a["tris"].shape[0], np.int64)
    seen = set()
    todo = sorted({(int(i["rootDesc0"]), int(i["rootDesc1"])) for i in a["insts"]})      # instances of one BLAS share its root
    while todo:
        d0, d1 = todo.pop()
        if d1 & WIDE_LEAF:
            start, count = _leaf_run(d0, d1)
            refs[start:start + count] += 1
            continue
        assert d0 < wide.shape[0] and d0 not in seen, "record %d: out of range or reached twice" % d0
        seen.add(d0)
        w = wide[d0]
        todo += [(int(w["ld0"]), int(w["ld1"])), (int(w["rd0"]), int(w["rd1"]))]
    assert refs.shape[0] > 0 and (refs == 1).all(), np.flatnonzero(refs != 1)[:8]


@pytest.mark.parametrize("quad,cull", alc.SETTINGS + ((-1, -1), (0, 1)))
@pytest.mark.parametrize("case", alc.CASES)
def test_quad_records_exist_by_rule_and_point_inside(rd, blobs, case, quad, cull):
    s, a = rd.DebugAccelLayout(blobs[case], quad, cull)
    culled = cull > 0 or (cull < 0 and s["nWide"] >= CULL_AUTO_MIN_WIDE)
    want = quad != 0 and not culled and not s["unifiedRoot"]
    assert a["quad"].shape[0] == (s["nWide"] if want else 0)
    assert s["nWide"] == a["wide"].shape[0] and s["nInst"] == a["insts"].shape[0]
    if not want:
        assert s["quadNeed"] == 0
        return
    for h in (0, 1):
        for side in ("l", "r"):
            d0, d1 = a["quad"]["half"][:, h][side + "d0"], a["quad"]["half"][:, h][side + "d1"]
            inner = (d1 & WIDE_LEAF) == 0
            assert (d0[inner] < s["nWide"]).all()
            leaf = ~inner
            assert ((d0[leaf].astype(np.int64) + ((d1[leaf] >> 24) & 0x7f)) <= a["tris"].shape[0]).all()
