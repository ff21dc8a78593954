"""CPU suite: the one rule every device-resident call (rdx_query_rays .. rdx_trace_paths_lights) applies to the byte ranges it is
given, through the host seam rdx_debug_check_ranges: a table of refusals, and the seam against a restatement of the rule over
seeded random tables.  The calls themselves refuse to run before rdx_init; their own refusal tables are in tests/test_gpu_*.py."""
import collections
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Row = collections.namedtuple("Row", "name address size offset bytes align present")      # the order rd.DebugCheckRanges takes
STAGE_WORDS = (("offset", "multiple of"), ("size", "run past"), ("address", "aligned"), ("overlap", "overlap"))


@pytest.fixture(scope="module")
def mods(built):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import _lib, rd
    return _lib, rd


def row(name, address=0x10000, size=1024, offset=0, nbytes=0, align=16, present=True):
    return Row(name, address, size, offset, nbytes, align, present)


def stage_of(message):
    """None (accepted) or the stage whose words the refusal carries -- exactly one"""
    if message is None:
        return None
    assert message.startswith("rdx_debug_check_ranges: "), message
    found = [stage for stage, words in STAGE_WORDS if words in message]
    assert len(found) == 1, message
    return found[0]


def restated(rows, first_out, n):
    """the rule: None, or the stage that refuses"""
    live = [r for r in rows if r.present]
    if any(r.offset % r.align for r in live):
        return "offset"
    if any(r.offset > r.size or r.bytes > r.size - r.offset for r in live):
        return "size"
    if n == 0:
        return None
    if any(r.address % r.align for r in live):
        return "address"
    span = lambda r: (r.address + r.offset, r.address + r.offset + r.bytes)
    for o in range(first_out, len(rows)):
        for k in range(o):
            (a0, a1), (b0, b1) = span(rows[o]), span(rows[k])
            if rows[o].present and rows[k].present and a0 < a1 and b0 < b1 and a0 < b1 and b0 < a1:
                return "overlap"
    return None


A, B = 0x10000, 0x20000         # two buffers' addresses
IN = lambda **kw: row("ray", **kw)
OUT = lambda **kw: row("hit", **kw)
# (what, rows, first_out, n, the stage that refuses or None, words the refusal must contain)
CASES = [
    # offsets and sizes
    ("offset 8 in a row of 16", [IN(offset=8, nbytes=32), row("pixel", B, offset=4, nbytes=4, align=4)], 2, 1, "offset", ("16 for ray",)),
    ("offset 6 in a row of 4", [IN(offset=16, nbytes=32), row("pixel", B, offset=6, nbytes=4, align=4)], 2, 1, "offset", ("4 for pixel",)),
    ("offset 4 in a row of 4", [IN(offset=16, nbytes=32), row("pixel", B, offset=4, nbytes=4, align=4)], 2, 1, None, ()),
    ("offset == size, 0 bytes", [IN(offset=1024, nbytes=0)], 1, 0, None, ()),
    ("offset == size + align", [IN(offset=1024 + 16, nbytes=0)], 1, 0, "size", ("ray buffer",)),
    ("bytes == size - offset", [IN(offset=64, nbytes=960)], 1, 30, None, ()),
    ("one record more", [IN(offset=64, nbytes=960 + 32)], 1, 31, "size", ("ray buffer",)),
    ("one byte more", [IN(offset=64, nbytes=961)], 1, 1, "size", ("ray buffer",)),
    ("offset 2**64 - 16 into a small buffer", [IN(offset=2 ** 64 - 16, nbytes=32)], 1, 1, "size", ("ray buffer",)),
    ("bytes 2**64 - 16 in a small buffer", [IN(offset=16, nbytes=2 ** 64 - 16)], 1, 1, "size", ("ray buffer",)),
    # n == 0: never an address or an overlap, still an offset or a size
    ("n 0: a misaligned address, coincident outputs", [IN(address=A + 8, nbytes=64), OUT(address=B, nbytes=64), row("key", B, nbytes=64)], 1, 0, None, ()),
    ("n 0: a bad offset", [IN(address=A + 8, offset=4, nbytes=64)], 1, 0, "offset", ("16 for ray",)),
    ("n 0: a bad size", [IN(), OUT(address=B, offset=1024, nbytes=32)], 1, 0, "size", ("hit buffer",)),
    # n != 0: addresses
    ("address & 15 in a row of 16", [IN(address=A + 8, nbytes=32)], 1, 1, "address", ("16-byte aligned", "ray buffer")),
    ("address & 3 == 0 in a row of 16", [IN(address=A + 4, nbytes=32)], 1, 1, "address", ("16-byte aligned", "ray buffer")),
    ("address & 3 == 0 in a row of 4", [row("src", A + 4, nbytes=32, align=4)], 1, 1, None, ()),
    ("address & 3 in a row of 4", [row("src", A + 2, nbytes=32, align=4)], 1, 1, "address", ("4-byte aligned", "src buffer")),
    # overlaps
    ("ranges that touch", [IN(nbytes=64), OUT(offset=64, nbytes=64)], 1, 2, None, ()),
    ("ranges that touch, the output first in memory", [IN(offset=64, nbytes=64), OUT(nbytes=64)], 1, 2, None, ()),
    ("overlapping by one byte", [IN(nbytes=65), OUT(offset=64, nbytes=64)], 1, 2, "overlap", ("the hit range", "the ray range")),
    ("overlapping by one byte, the output first in memory", [IN(offset=64, nbytes=64), OUT(nbytes=65)], 1, 2, "overlap", ("the hit range", "the ray range")),
    ("one memory under two buffers", [IN(size=1024, nbytes=64), OUT(size=512, nbytes=64)], 1, 2, "overlap", ("hit", "ray")),
    ("one memory under two buffers, apart", [IN(size=1024, nbytes=64), OUT(size=512, offset=64, nbytes=64)], 1, 2, None, ()),
    ("two inputs that overlap", [IN(nbytes=64), row("key", nbytes=64), OUT(address=B, nbytes=64)], 2, 2, None, ()),
    ("an output over an earlier output", [IN(nbytes=64), OUT(address=B, nbytes=64), row("next-ray", B, offset=32, nbytes=64)], 1, 2, "overlap",
     ("the next-ray range", "the hit range")),
    ("an absent row between them", [IN(nbytes=64), row("key", nbytes=64, present=False), OUT(address=B, nbytes=64)], 1, 2, None, ()),
    ("an absent output over everything, misplaced", [IN(nbytes=64), row("shadow-ray", A + 2, 16, offset=3, nbytes=4096, present=False), OUT(address=B, nbytes=64)],
     1, 2, None, ()),
    ("a present row of 0 bytes inside an output", [IN(offset=32, nbytes=0), OUT(nbytes=64)], 1, 2, None, ()),
    ("a present output of 0 bytes inside an input", [IN(nbytes=64), OUT(offset=32, nbytes=0)], 1, 2, None, ()),
    # order
    ("an offset in the last row before a size in the first", [IN(offset=2048, nbytes=32), OUT(address=B, offset=8, nbytes=32)], 1, 1, "offset", ("16 for hit",)),
    ("a size before an address", [IN(address=A + 8, nbytes=32), OUT(address=B, offset=1024, nbytes=32)], 1, 1, "size", ("hit buffer",)),
    ("an address before an overlap", [IN(nbytes=64), OUT(nbytes=64), row("src", B + 8, nbytes=4)], 1, 1, "address", ("src buffer",)),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_refusal_table(mods, case):
    rd = mods[1]
    what, rows, first_out, n, stage, words = case
    message = rd.DebugCheckRanges(rows, first_out, n)
    assert stage_of(message) == stage == restated(rows, first_out, n), (what, message)
    for w in words:
        assert w in message, (what, w, message)


def test_the_seam_follows_the_restated_rule_on_random_tables(mods):
    """400 small tables (sizes <= 4096, addresses on a 4-byte grid, up to 6 rows, n in {0, 1, 7}), drawn so that most rows are sound
    and every stage refuses often enough to be seen: accept / refuse and the refusing stage are the restatement's"""
    rd = mods[1]
    rng = np.random.default_rng(0)
    seen = collections.Counter()
    for t in range(400):
        n = int(rng.choice([0, 1, 7]))
        rows = []
        for k in range(int(rng.integers(1, 7))):
            align = int(rng.choice([4, 16]))
            rec = int(rng.choice([4, 16, 32, 64]))
            address = 0x10000 + 16 * int(rng.integers(0, 24)) + (4 * int(rng.integers(1, 4)) if rng.random() < 0.06 else 0)
            offset = align * int(rng.integers(0, 8)) + (int(rng.integers(1, 4)) if rng.random() < 0.04 else 0)
            nbytes = n * rec if rng.random() < 0.8 else int(rng.integers(0, 600))
            size = min(offset + nbytes + int(rng.choice([0, 0, 16, 1000])), 4096)       # the range ends at or before the buffer's end,
            if rng.random() < 0.08:
                size = max(size - int(rng.integers(1, 40)), 0)                          # or the buffer ends a little early
            rows.append(Row("row%d" % k, address, size, offset, nbytes, align, bool(rng.random() < 0.85)))
        first_out = int(rng.integers(0, len(rows) + 1))
        want = restated(rows, first_out, n)
        assert stage_of(rd.DebugCheckRanges(rows, first_out, n)) == want, (t, rows, first_out, n)
        seen[want] += 1
    assert all(seen[s] >= 15 for s in (None, "offset", "size", "address", "overlap")), seen


def test_every_symbol_is_present(mods):
    _lib, rd = mods
    import ctypes as C
    assert "rdx_debug_check_ranges" in _lib.SIGNATURES and _lib.lib().rdx_debug_check_ranges
    hdr = open(os.path.join(ROOT, "include", "rdx.h")).read()
    assert re.search(r"\brdx_debug_check_ranges\(", hdr)
    assert re.search(r"typedef struct rdx_debug_range\s*\{\s*uint64_t address, size, offset, bytes;\s*uint32_t align, present;\s*\}", hdr)
    assert [f for f, _ in _lib.rdx_debug_range._fields_] == ["address", "size", "offset", "bytes", "align", "present"]
    assert C.sizeof(_lib.rdx_debug_range) == 40
    assert hasattr(rd, "DebugCheckRanges")
    assert rd.DebugCheckRanges([], 0, 1) is None


def test_every_header_of_csrc_is_a_dependency_of_the_library(built):
    """editing any csrc/*.h must rebuild librdx.so: build.py compares the library's time stamp with SOURCES + HEADERS only"""
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import build
    csrc = os.path.join(ROOT, "radiance-ray-tracing_amd", "csrc")
    on_disk = sorted(f for f in os.listdir(csrc) if f.endswith(".h"))
    assert len(on_disk) >= 20 and all(os.path.exists(os.path.join(csrc, h)) for h in build.HEADERS)
    assert [h for h in on_disk if h not in build.HEADERS] == []
    assert len(set(build.HEADERS)) == len(build.HEADERS)
