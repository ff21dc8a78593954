"""GPU suite, part 5 (-m gpu): the device-resident ray query (rdx_query_rays, rd.QueryRays / rd.QueryRaysTorch), whose rays carry
their OWN interval.

Comparand: tests/golden/refgpu_rayedges.npz, the reference's own answers, through tests/ray_query_cases.mixed_batch: per scene
ONE batch of every cell of tests/ray_edge_cases.py, each ray with its cell's interval, in a fixed random order (13 to 30 distinct
intervals per 64 consecutive rays; tests/test_ray_query_cpu.py asserts the conditions on these inputs).  Bar, nothing filtered: all
eight words of every record -- the hit flag everywhere; t, b1, b2 and the four integers bit for bit where the reference hit
(kind 1); 0 in the other seven words on misses and for kind 2.

That these tests notice a wrong engine was checked with local mutations (never committed), each run against this file -- the
outcomes are in profiles/ray_query_kernels.txt.
"""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_cases as gc
import ray_edge_cases as rec
import ray_query_cases as rq
from test_ray_edges_cpu import GOLD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = {"kernel": 3, "cull": -1, "quad": 1, "group_instances": 1, "unified_tree": 1, "top_flat": 1, "inline_leaf_roots": 1}


def _matrix(**axes):
    keys = list(axes)
    return [dict(zip(keys, v)) for v in itertools.product(*axes.values())]


POOL = _matrix(kernel=(3,), cull=(0, 1), quad=(0, 1), group_instances=(0, 1))
POOL_INST = _matrix(kernel=(3,), cull=(0, 1), quad=(0, 1), group_instances=(0, 1), unified_tree=(0, 1), top_flat=(0, 1), inline_leaf_roots=(0, 1))
OTHERS = [{"kernel": 2}, {"kernel": 1}, {"kernel": 0}]


@pytest.fixture(scope="module")
def mods(gpu):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd, scenes
    return rd, scenes


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLD, "refgpu_rayedges.npz"))


class Ctx:
    """one scene on the device, its mixed batch in a device buffer, the reference's answers"""

    def __init__(self, rd, scenes, G, name):
        self.rd, self.name = rd, name
        self.dev = scenes.DeviceScene(rec.scene(scenes, name))
        self.plt = self.dev.plt
        blob = rd.ReadBuffer(self.plt, self.dev.topAccelStruct, self.dev.topAccelStruct.size).tobytes()
        assert np.array_equal(gc.sha(blob), G[name + "/blob_sha256"]), "the TLAS blob of %s changed" % name
        self.rays, self.want1, self.want2 = rq.mixed_batch(scenes, G, name)
        self.n = self.rays.shape[0]
        self.bRays = rd.CreateBuffer(self.plt, self.n * 32)
        rd.WriteBuffer(self.plt, self.bRays, self.n * 32, self.rays)
        self.bHits = rd.CreateBuffer(self.plt, self.n * 32)

    def query(self, kind, n=None):
        n = self.n if n is None else n
        self.rd.QueryRays(self.dev.topAccelStruct, self.bRays, n, kind, self.bHits)
        return self.rd.ReadBuffer(self.plt, self.bHits, n * 32).view(rq.RAY_HIT_DTYPE).reshape(-1)

    def want(self, kind):
        return self.want1 if kind == 1 else rq.any_records(self.want2)


@pytest.fixture(scope="module")
def ctx(mods, fixture):
    rd, scenes = mods
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Ctx(rd, scenes, fixture, name)
        return cache[name]
    return get


def _fail(c, kind, what, want, got, bad):
    i = int(np.flatnonzero(bad)[0])
    r = c.rays[i]
    raise AssertionError("%s kind %d, %s: %d of %d records differ; first: ray %d o=%r d=%r tmin=%r tmax=%r want %r, got %r"
                         % (c.name, kind, what, int(bad.sum()), bad.shape[0], i, r["origin"].tolist(), r["direction"].tolist(),
                            float(r["tmin"]), float(r["tmax"]), want[i].tolist(), got[i].tolist()))


def _run(c, configs):
    rd = c.rd
    for cfg in configs:
        try:
            for k, v in cfg.items():
                rd.SetOption(k, v)
            for kind in (1, 2):
                rd.WriteBuffer(c.plt, c.bHits, c.n * 32, np.full(c.n * 8, 0xA5A5A5A5, np.uint32))
                got = c.query(kind)
                bad = rq.mismatches(c.want(kind), got)
                if bad.any():
                    _fail(c, kind, " ".join("%s %d" % kv for kv in cfg.items()), c.want(kind), got, bad)
        finally:
            for k in cfg:
                rd.SetOption(k, DEFAULTS[k])


@pytest.mark.parametrize("name", rec.SCENES)
def test_mixed_intervals_match_the_reference_pool_engine(ctx, name):
    """the pool engine's per-ray variant under every option that selects another kernel or another walk"""
    _run(ctx(name), POOL_INST if name.startswith("edges_inst") else POOL)


@pytest.mark.parametrize("name", rec.SCENES)
def test_mixed_intervals_match_the_reference_other_kernels(ctx, name):
    """`kernel` 2 and 1 (per-lane wide-node kernel) and 0 (reference order), default options otherwise"""
    _run(ctx(name), OTHERS)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_ragged_sizes_and_offsets(ctx, n):
    """the first n rays of c1's batch, read at rays_offset 96 and written at hits_offset 160 of buffers filled with 0xA5: the n
    records equal those of the full batch and no byte outside them is touched"""
    c = ctx("c1")
    rd, plt = c.rd, c.plt
    ro, ho, tail = 32 * 3, 32 * 5, 32 * 4
    bR = rd.CreateBuffer(plt, ro + 65 * 32 + tail)
    bH = rd.CreateBuffer(plt, ho + 65 * 32 + tail)
    fill = lambda b: rd.WriteBuffer(plt, b, b.size, np.full(b.size, 0xA5, np.uint8))
    fill(bR)
    rd.WriteBuffer(plt, bR, 65 * 32, c.rays[:65], offset=ro)
    rays_before = rd.ReadBuffer(plt, bR, bR.size).copy()
    for kind in (1, 2):
        fill(bH)
        ret = rd.QueryRays(c.dev.topAccelStruct, bR, n, kind, bH, rays_offset=ro, hits_offset=ho)
        assert ret is bH
        raw = rd.ReadBuffer(plt, bH, bH.size)
        got = raw[ho:ho + 32 * n].view(rq.RAY_HIT_DTYPE)
        bad = rq.mismatches(c.want(kind)[:n], got)
        assert not bad.any(), (kind, n, int(bad.sum()))
        assert (raw[:ho] == 0xA5).all() and (raw[ho + 32 * n:] == 0xA5).all(), (kind, n)
        assert np.array_equal(rd.ReadBuffer(plt, bR, bR.size), rays_before)
    # hits=None: a buffer of hits_offset + 32 n bytes is created
    h = rd.QueryRays(c.dev.topAccelStruct, bR, n, 1, None, rays_offset=ro, hits_offset=ho)
    assert h.size == max(ho + 32 * n, 1)
    if n:
        got = rd.ReadBuffer(plt, h, 32 * n, offset=ho).view(rq.RAY_HIT_DTYPE)
        assert not rq.mismatches(c.want1[:n], got).any()


def test_agrees_with_the_trace_batch_seam_at_the_stock_interval(ctx, mods):
    """c2's golden rays at (0.001, 1000): every field both records have, against rd.TraceBatch's production kernel"""
    rd, _ = mods
    c = ctx("c2")
    g = np.load(os.path.join(GOLD, "refgpu_c2.npz"))
    o, d = np.ascontiguousarray(g["ray_o"], np.float32), np.ascontiguousarray(g["ray_d"], np.float32)
    n = o.shape[0]
    rays = np.zeros(n, rq.RAY_DTYPE)
    rays["origin"], rays["direction"], rays["tmin"], rays["tmax"] = o, d, 0.001, 1000.0
    bR = rd.CreateBuffer(c.plt, n * 32)
    rd.WriteBuffer(c.plt, bR, n * 32, rays)
    for kind in (1, 2):
        seam = rd.TraceBatch(c.dev.topAccelStruct, o, d, 0.001, 1000.0, kind)
        want = rq.query_records(seam) if kind == 1 else rq.any_records(seam["hit"])
        got = rd.ReadBuffer(c.plt, rd.QueryRays(c.dev.topAccelStruct, bR, n, kind), n * 32).view(rq.RAY_HIT_DTYPE)
        assert 0 < int(want["hit"].sum()) < n
        bad = rq.mismatches(want, got)
        assert not bad.any(), (kind, int(bad.sum()), int(np.flatnonzero(bad)[0]))
        assert rd.GetTraceStats().ms_extend > 0.0


def test_refusals_leave_the_library_usable(ctx, mods):
    rd, _ = mods
    c = ctx("c1")
    tl, plt = c.dev.topAccelStruct, c.plt
    bR = rd.CreateBuffer(plt, 64 * 32)
    rd.WriteBuffer(plt, bR, 64 * 32, c.rays[:64])
    bH = rd.CreateBuffer(plt, 64 * 32)
    both = rd.CreateBuffer(plt, 128 * 32)
    rd.WriteBuffer(plt, both, 64 * 32, c.rays[:64])
    rd.WriteBuffer(plt, both, 64 * 32, np.full(64 * 32, 0xA5, np.uint8), offset=64 * 32)
    null = rd.Buffer(None, 64 * 32)

    def ok():
        got = rd.ReadBuffer(plt, rd.QueryRays(tl, bR, 64, 1, bH), 64 * 32).view(rq.RAY_HIT_DTYPE)
        assert not rq.mismatches(c.want1[:64], got).any()

    ok()
    cases = [
        ("kind", lambda: rd.QueryRays(tl, bR, 64, 3, bH), "kind"),
        ("kind 0", lambda: rd.QueryRays(tl, bR, 64, 0, bH), "kind"),
        ("rays_offset 8", lambda: rd.QueryRays(tl, bR, 8, 1, bH, rays_offset=8), "16"),
        ("hits_offset 8", lambda: rd.QueryRays(tl, bR, 8, 1, bH, hits_offset=8), "16"),
        ("one ray past the rays", lambda: rd.QueryRays(tl, bR, 65, 1, both), "ray buffer"),
        ("one ray past the rays (offset)", lambda: rd.QueryRays(tl, bR, 64, 1, both, rays_offset=32), "ray buffer"),
        ("one record past the hits", lambda: rd.QueryRays(tl, both, 65, 1, bH), "hit buffer"),
        ("one record past the hits (offset)", lambda: rd.QueryRays(tl, bR, 64, 1, bH, hits_offset=32), "hit buffer"),
        ("overlap", lambda: rd.QueryRays(tl, both, 64, 1, both, rays_offset=0, hits_offset=63 * 32), "overlap"),
        ("same range", lambda: rd.QueryRays(tl, both, 64, 1, both), "overlap"),
        ("null rays", lambda: rd.QueryRays(tl, null, 64, 1, bH), "ray buffer handle"),
        ("null hits", lambda: rd.QueryRays(tl, bR, 64, 1, null), "hit buffer handle"),
        ("null tlas", lambda: rd.QueryRays(null, bR, 64, 1, bH), "TLAS"),
    ]
    for what, call, word in cases:
        with pytest.raises(rd.RadianceError) as e:
            call()
        assert word in str(e.value) and "rdx_query_rays" in str(e.value), (what, str(e.value))
        ok()
    # adjacent ranges of one buffer are fine: rays in the first half, records in the second
    rd.QueryRays(tl, both, 64, 1, both, rays_offset=0, hits_offset=64 * 32)
    got = rd.ReadBuffer(plt, both, 64 * 32, offset=64 * 32).view(rq.RAY_HIT_DTYPE)
    assert not rq.mismatches(c.want1[:64], got).any()
    assert np.array_equal(rd.ReadBuffer(plt, both, 64 * 32).view(rq.RAY_DTYPE).view(np.uint32), c.rays[:64].view(np.uint32))


_TORCH_CHILD = r"""
import os, sys
ROOT = sys.argv[1]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
assert torch.cuda.is_available()
torch.zeros(1, device="cuda").cpu()                      # torch initialises the GPU first (tests/test_cpu_oracle._gpu_present)
import numpy as np
import rrt_amd
from radiance_ray_tracing_amd import rd, scenes
import ray_edge_cases as rec
import ray_query_cases as rq
G = np.load(os.path.join(ROOT, "tests", "golden", "refgpu_rayedges.npz"))
rays, w1, w2 = rq.mixed_batch(scenes, G, "c1")
n = rays.shape[0]
dev = scenes.DeviceScene(rec.scene(scenes, "c1"))
t = torch.from_numpy(rays.view(np.float32).reshape(n, 8).copy()).cuda()
scale = torch.ones(8, device="cuda"); scale[4:7] = 1.0
t = (t * scale).contiguous()                             # produced by a torch op on torch's stream (x 1.0: the same bits)
assert np.array_equal(t.cpu().numpy().view(np.uint32), rays.view(np.uint32).reshape(n, 8))
for kind, want in ((1, w1), (2, rq.any_records(w2))):
    out = rd.QueryRaysTorch(dev.topAccelStruct, t, kind)
    assert out.dtype == torch.int32 and tuple(out.shape) == (n, 8) and out.is_cuda
    got = out.cpu().numpy().view(np.uint32)
    bad = (got != rq.words(want)).any(1)
    assert not bad.any(), (kind, int(bad.sum()), int(np.flatnonzero(bad)[0]))
    assert np.array_equal(out.view(torch.float32)[:, 0].cpu().numpy().view(np.uint32), want["t"].view(np.uint32))
pre = torch.full((n, 8), -1, dtype=torch.int32, device="cuda")
ptr = pre.data_ptr()
ret = rd.QueryRaysTorch(dev.topAccelStruct, t, 1, out=pre)
assert ret is pre and pre.data_ptr() == ptr
assert np.array_equal(pre.cpu().numpy().view(np.uint32), rq.words(w1))
for bad_in in (t[:, :7], t.double(), t.cpu()):
    try:
        rd.QueryRaysTorch(dev.topAccelStruct, bad_in, 1)
    except rd.RadianceError:
        continue
    raise AssertionError("a tensor that is not a contiguous float32 CUDA (n, 8) tensor was accepted")
print("TORCH-QUERY-OK", n)
"""


def test_torch_tensors_in_a_fresh_process(gpu):
    """rd.QueryRaysTorch on c1's mixed batch as a CUDA tensor made by a torch op; torch is initialised first, in a process of its own"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _TORCH_CHILD, ROOT]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "TORCH-QUERY-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
