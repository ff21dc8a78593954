"""GPU suite, part 4 (-m gpu): traversal parity BEYOND the stock ray interval (0.001, 1000) and beyond unit directions.

Comparand: tests/golden/refgpu_rayedges.npz -- the answers of the reference's own `intersectTop` (oracle/_ref, build p, run on
an MI355X by tests/golden/make_golden_gpu.py rayedges) for every cell of tests/ray_edge_cases.py -- and, when the code object is
present, the live reference launched next to the product.  Bar: hit flags everywhere, every HitData field bit for bit where the
reference hit (closest hit, sbtRecordOffset 1); the hit flag (any hit, sbtRecordOffset 2).  Nothing is filtered out of a batch.

Which cell gets which option matrix (every cell also runs the reference-order kernel, rd.TraceBatch(reference_order=True)):

  FULL   kernel 3 / 2 / 1  x  cull 0 / 1  x  quad 0 / 1  x  group_instances 0 / 1, and on edges_inst / edges_inst_id also
         x unified_tree 0 / 1  x  top_flat 0 / 1  x  inline_leaf_roots 0 / 1
             family A at the three intervals that change the most answers (0, FLT_MAX), (0.001, 2), (2, 1000);
             family C (exact ties at tmin / tmax);  family D (second surface)
  SMALL  kernel 3 / 2 / 1  x  cull 0 / 1
             the other ten intervals of family A;  families B (scaled directions), E (far / large), F (degenerate rays)
  Families C and D also run at 1, 63, 64 and 65 rays (SMALL matrix).

The user-library test runs a program that calls traceRay() with an interval read from a buffer (tests/golden/
user_trace_interval.cl) over families A, C and D of scene c1; the fuzz test runs tools/fuzz_parity.py with intervals and scales.

That these tests notice a wrong kernel was checked with local mutations (never committed), each run against this file:
`t < tmax` -> `t <= tmax` in coop_triangle_regs: families A (c0, c1) and C fail; `t > tmin` -> `t >= tmin`: A, C and D fail;
`float tlim = tmax` -> `1000.0f` in traverse_pool.h: B, E and the fuzz test fail; Tmax ignored in intersectBot of
shader/radiance.cl: the user-program test fails (433 of 1024 rays of c1 / A / (0.001, 2)); the exactOnly threshold 1e-20 ->
1e-10 survives -- rightly: a larger threshold only sends MORE rays down the exact path (the reference's own division form, no leaf
skip), which is the reference's arithmetic by construction; it costs speed, not answers.

Transform groups: no statistic exposes the group the product forms on edges_inst, so it was shown indirectly, with two local
mutations (never committed).  (a) the layout derivation (accel_layout.cpp) writing the group's FIRST member into the `_p0` instance slot of every member's
triangles: every kernel-3 cell of edges_inst / edges_inst_id then fails on instanceIndex (11 -> 10, 12 -> 10), so a group of
these three instances forms -- but with group_instances 0 as well as 1, because the pool's test step takes a candidate's instance
from the triangle record whenever the derivation wrote one, whatever the launch option says.  (b) the instance step's "slot already
holds the group's ray" branch (traverse_pool.h) made to miss the root box: exactly the cells with kernel 3, group_instances 1 and
top_flat 1 fail, every cell with group_instances 0 (or top_flat 0, or kernel 2 / 1) passes: the option is exercised, and the
cells tell its two settings apart.

Family F (zero / NaN / inf / denormal rays) and why it may run on persistent kernels: every engine walks a finite tree whose
node, leaf and instance indices come from the acceleration structure only; a ray's floats decide nothing but WHICH children are
entered (slab and triangle tests: comparisons, all false on NaN), never whether a loop continues -- the per-lane walks
(kernels.hip traverse / traverse_wide) pop a stack that each visited node pushes to at most twice, the cooperative and pool
engines (traverse_coop.h, traverse_pool.h) drain integer-counted queues and carry an iteration bound that the host reports as
"a traversal wave exceeded its iteration bound".  So each walk ends after at most (nodes + triangles) steps per ray, as the
reference's does.  Family F lives in the last test functions of this file, in batches of 192 rays."""
import itertools
import os
import sys

import numpy as np
import pytest

import golden_cases as gc
import oracle_bind as ob
import ray_edge_cases as rec
import refgpu_bind as rg
from test_ray_edges_cpu import FIELDS, GOLD, load_cells, mismatches

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = {"kernel": 3, "cull": -1, "quad": 1, "group_instances": 1, "unified_tree": 1, "top_flat": 1, "inline_leaf_roots": 1}


def _matrix(**axes):
    keys = list(axes)
    return [dict(zip(keys, v)) for v in itertools.product(*axes.values())]


SMALL = _matrix(kernel=(3, 2, 1), cull=(0, 1))
FULL = _matrix(kernel=(3, 2, 1), cull=(0, 1), quad=(0, 1), group_instances=(0, 1))
FULL_INST = _matrix(kernel=(3, 2, 1), cull=(0, 1), quad=(0, 1), group_instances=(0, 1), unified_tree=(0, 1), top_flat=(0, 1),
                    inline_leaf_roots=(0, 1))


def matrix_of(cell):
    full = cell.family in "CD" or (cell.family == "A" and cell.name in rec.A_FULL_MATRIX)
    if not full:
        return SMALL
    return FULL_INST if cell.scene.startswith("edges_inst") else FULL


@pytest.fixture(scope="module")
def mods(gpu):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd, scenes
    return rd, scenes


@pytest.fixture(scope="module")
def ref(gpu):
    return rg.RefGpu("p") if rg.available("p") else None


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLD, "refgpu_rayedges.npz"))


class Ctx:
    """one scene on the device + its cells and the reference's answers"""

    def __init__(self, rd, scenes, G, ref, name):
        self.rd, self.name = rd, name
        self.dev = scenes.DeviceScene(rec.scene(scenes, name))
        blob = rd.ReadBuffer(self.dev.plt, self.dev.topAccelStruct, self.dev.topAccelStruct.size).tobytes()
        assert np.array_equal(gc.sha(blob), G[name + "/blob_sha256"]), "the TLAS blob of %s changed" % name
        self.cells, self.want = load_cells(scenes, G, name)
        self.ref, self.tl = ref, (rg.DevBuf.of(np.frombuffer(blob, np.uint8)) if ref is not None else None)


@pytest.fixture(scope="module")
def ctx(mods, fixture, ref):
    rd, scenes = mods
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Ctx(rd, scenes, fixture, ref, name)
        return cache[name]
    return get


def _fail(cell, n, rec_no, what, want, got, bad):
    i = int(np.flatnonzero(bad)[0])
    raise AssertionError("%s (%d rays) rec %d, %s: %d rays differ; first: ray %d o=%r d=%r tmin=%r tmax=%r want t=%r prim=%d inst=%d hit=%d, got t=%r prim=%d inst=%d hit=%d"
                         % (cell.key, n, rec_no, what, int(bad.sum()), i, cell.o[i].tolist(), cell.d[i].tolist(), cell.tmin, cell.tmax,
                            float(want["distance"][i]), int(want["primitiveIndex"][i]), int(want["instanceIndex"][i]), int(want["hit"][i]),
                            float(got["distance"][i]), int(got["primitiveIndex"][i]), int(got["instanceIndex"][i]), int(got["hit"][i])))


def check_cell(c, cell, w1, w2, configs, n=None):
    """the first n rays of a cell: fixture == live reference == reference-order kernel == every configuration"""
    rd = c.rd
    n = cell.n if n is None else n
    o, d = cell.o[:n], cell.d[:n]
    want2 = np.zeros(n, ob.HIT_DTYPE); want2["hit"] = w2[:n]
    for rec_no, want in ((1, w1[:n]), (2, want2)):
        closest = rec_no == 1
        if c.tl is not None and n == cell.n:          # (the ragged prefixes are the same launch's first rays)
            live = c.ref.trace(c.tl, o, d, cell.tmin, cell.tmax, rec_no)
            bad = mismatches(want, live, closest)
            if bad.any():
                _fail(cell, n, rec_no, "live reference against the fixture", want, live, bad)
        got = rd.TraceBatch(c.dev.topAccelStruct, o, d, cell.tmin, cell.tmax, rec_no, reference_order=True)
        bad = mismatches(want, got, closest)
        if bad.any():
            _fail(cell, n, rec_no, "reference-order kernel", want, got, bad)
        for cfg in configs:
            try:
                for k, v in cfg.items():
                    rd.SetOption(k, v)
                got = rd.TraceBatch(c.dev.topAccelStruct, o, d, cell.tmin, cell.tmax, rec_no)
            finally:
                for k in cfg:
                    rd.SetOption(k, DEFAULTS[k])
            assert got.shape[0] == n
            bad = mismatches(want, got, closest)
            if bad.any():
                _fail(cell, n, rec_no, " ".join("%s %d" % kv for kv in cfg.items()), want, got, bad)
    return n


def run_family(c, family, ragged=False):
    rays = 0
    for cell, (w1, w2) in zip(c.cells, c.want):
        if cell.family != family:
            continue
        rays += check_cell(c, cell, w1, w2, matrix_of(cell))
        if ragged:
            for n in rec.RAGGED:
                check_cell(c, cell, w1, w2, SMALL, n)
    return rays


NOT_PLANES = [n for n in rec.SCENES if n != "planes"]


@pytest.mark.parametrize("name", NOT_PLANES)
def test_family_a_golden_rays_under_every_interval(ctx, name):
    assert run_family(ctx(name), "A") == len(rec.INTERVALS) * rec.N_GOLDEN // (rec.N_GOLDEN // rec.N_A.get(name, 1024))


@pytest.mark.parametrize("name", [n for n in NOT_PLANES if n != "edges_inst_id"])
def test_family_b_scaled_directions(ctx, name):
    assert run_family(ctx(name), "B") > 0


@pytest.mark.parametrize("name", ["c0", "c1", "planes"])
def test_family_c_exact_ties_at_tmin_and_tmax(ctx, name):
    assert run_family(ctx(name), "C", ragged=True) == 20 * rec.N_C


@pytest.mark.parametrize("name", NOT_PLANES)
def test_family_d_second_surface(ctx, name):
    assert run_family(ctx(name), "D", ragged=True) == 2 * rec.N_GOLDEN


@pytest.mark.parametrize("name", rec.GOLDEN)
def test_family_e_far_and_large(ctx, name):
    assert run_family(ctx(name), "E") == 5 * rec.N_E


def _write_rays(rd, plt, buf, cell):
    head = np.array([cell.tmin, cell.tmax], np.float32)
    rays = np.concatenate([head, np.concatenate([cell.o, cell.d], 1).reshape(-1)]).astype(np.float32)
    rd.WriteBuffer(plt, buf, rays.nbytes, rays)


def test_user_program_traces_rays_with_its_own_interval(mods, fixture):
    """A user raygen that calls the product library's traceRay() with Tmin / Tmax read from a buffer (tests/golden/
    user_trace_interval.cl), compiled at run time against radiance-ray-tracing_amd/shader/: families A (all 13 intervals), C and D
    on c1, closest hit and any hit, against the reference's answers."""
    rd, scenes = mods
    s = rec.scene(scenes, "c1")
    text = open(os.path.join(GOLD, "user_trace_interval.cl")).read()
    rd.SetShaderIncludePath("")                       # nothing but the library's own directory
    dev = scenes.DeviceScene(s, shader_text=text)
    plt = dev.plt
    cells, want = load_cells(scenes, fixture, "c1")
    nmax = max(c.n for c in cells)
    bRays = rd.CreateBuffer(plt, (2 + nmax * 6) * 4)
    bOut = rd.CreateBuffer(plt, nmax * 28 * 4)
    done = 0
    for cell, (w1, w2) in zip(cells, want):
        if cell.family not in "ACD":
            continue
        n = cell.n
        _write_rays(rd, plt, bRays, cell)
        for rec_no in (1, 2):
            prop = np.zeros((), rd.RayTraceProperties)
            prop["batchSize"], prop["depth"] = n, rec_no
            rd.WriteBuffer(plt, dev.rdRTProp, 16, np.array(prop))
            rd.WriteBuffer(plt, bOut, n * 28 * 4, np.zeros(n * 28, np.uint32))
            rd.BindDescriptorSet(plt, rd.CreateDescriptorSet([dev.rdRTProp, bOut, dev.rdImage, dev.rdCamData, dev.rdSceneData, dev.meshInfoData, bRays,
                                                               dev.indexData, dev.uvData, dev.normalData, dev.materialData, None, None, dev.topAccelStruct]))
            rd.TraceRays(plt, 0, 0, 0, n, 1)
            got = rd.ReadBuffer(plt, bOut, n * 28 * 4).view(ob.HIT_DTYPE).reshape(-1)
            if rec_no == 1:
                bad = mismatches(w1, got)
            else:
                bad = w2 != got["hit"]
            if bad.any():
                wantr = w1 if rec_no == 1 else np.zeros(n, ob.HIT_DTYPE)
                _fail(cell, n, rec_no, "user program", wantr, got, bad)
        done += 1
    assert done == len(rec.INTERVALS) + 20 + 2


def test_fuzz_random_scenes_with_intervals_and_scales(mods):
    """12 random scenes of tools/fuzz_parity.py: every production kernel against the reference-order kernel under (0, FLT_MAX), an
    interval that cuts through the scene, a raised tmin, and directions scaled by 1e-22 and 3e7 (intervals scaled with them)"""
    rd, scenes = mods
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_parity as fz
    bad = fz.run(12, 4000, verbose=False, intervals=((0.0, rec.FLT_MAX), (0.001, 6.0), (5.0, 1000.0)), scales=(1e-22, 3e7))
    assert bad == 0


# ---------------------------------------------------------------------------------------------------------------------
# family F: degenerate rays (see the module docstring).  Keep these last.
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NOT_PLANES)
def test_family_f_degenerate_rays(ctx, name):
    c = ctx(name)
    assert run_family(c, "F") == 2 * len(rec.DEGENERATE_KINDS) <= 512


@pytest.mark.parametrize("name", ["edges_inst", "edges_inst_id"])
def test_family_f_degenerate_rays_every_option_on_the_instanced_scenes(ctx, name):
    """signed zeros, NaN and inf through the transform group, the identity group and the flat / walked top level"""
    c = ctx(name)
    n = 0
    for cell, (w1, w2) in zip(c.cells, c.want):
        if cell.family == "F":
            n += check_cell(c, cell, w1, w2, [m for m in FULL_INST if m["kernel"] == 3])
    assert n == 2 * len(rec.DEGENERATE_KINDS)
