#!/usr/bin/env python3
"""make_golden_gpu.py -- regenerates tests/golden/refgpu_*.npz by running the REAL reference device code on an MI355X.

The code object oracle/_ref/ref_shader_gfx950_p.co is the reference's own samples/shader.cl (+ radiance/shader/*.cl)
compiled where it lies by oracle/Makefile (ROCm clang, OpenCL C, gfx950, `-ffp-contract=off
-cl-fp32-correctly-rounded-divide-sqrt`, ROCm's own OpenCL builtin library) with the batch wrappers of
oracle/ref_gpu_dev.cl / ref_gpu_kern.cl.  It is built in the build container (where /root/reference exists) and
travels to the GPU box; run there:

    gpurun -- python tests/golden/make_golden_gpu.py        # writes gpurun_out/golden/refgpu_*.npz
    cp gpurun_out/golden/refgpu_*.npz tests/golden/

Every array in the fixtures is either an input (seeded numpy data, scene buffers from scenes.py) or an output of the
reference code object -- nothing here comes from the product or from the CPU oracle, except the TLAS blob, which the
product's host builder makes (the reference's builder needs assimp and cannot be built; its SHA-256 is stored so the
tests notice if the blob ever changes).

refgpu_kat.npz        intersectAABB, intersectTriangle, microfacetBRDF + sampleMicrofacetBRDF_transm on unit inputs
refgpu_<scene>.npz    per small scene (tests/golden_cases.py): primary rays of generateRay, HitData of a 4096-ray batch
                      (closest hit: sbt 1; any hit: sbt 2), `material` payloads on captured hits, imageScratch + RGBA8
                      after TraceRays call 1 and 2 (progressive mean)

Second entry point (leaves the files above alone):

    python tests/golden/make_golden_gpu.py rayedges [DIR]     # on the MI355X; writes DIR/refgpu_rayedges.npz
    cp DIR/refgpu_rayedges.npz tests/golden/                   # (DIR defaults to the folder the files above are written to, OUT)

Third entry point:

    python tests/golden/make_golden_gpu.py shadeedges [DIR]   # on the MI355X; writes DIR/refgpu_shade_edges.npz

Fourth entry point:

    python tests/golden/make_golden_gpu.py meshedges [DIR]    # on the MI355X; writes DIR/refgpu_meshedges.npz

refgpu_meshedges.npz  the reference's intersectTop on hostile geometry: every case of tests/mesh_edge_cases.py (NaN / infinite /
                      overflowing / denormal coordinates, degenerate and identical triangles, flat meshes, centroids on candidate
                      planes, signed zeros, lopsided deep trees, hostile instances), its rays at the stock interval and at
                      (0, FLT_MAX), closest hit (sbt 1: full HitData) and any hit (sbt 2: flags), and the blob's SHA-256.  Data only:
                      meshes and rays are rebuilt from mesh_edge_cases.py at test time.  Layout: as refgpu_rayedges.npz, per case.

refgpu_shade_edges.npz  the reference's `material`, microfacetBRDF, raygen (frames, the tone map alone at batchSize 0, the running
                      mean alone at depth 0) and generateRay on the edge inputs of tests/shade_edge_cases.py (layout: there).

refgpu_rayedges.npz   the reference's intersectTop beyond the stock ray interval and unit directions: every cell of
                      tests/ray_edge_cases.py (scene x family x interval), closest hit (sbt 1: full HitData) and any hit
                      (sbt 2: flags), plus the inputs that depend on the reference's own answers.  Layout: ray_edge_cases.py
                      "fixture layout".  The archive is written with fixed time stamps: a second run reproduces it byte for byte.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import golden_cases as gc          # noqa: E402
import refgpu_bind as rg           # noqa: E402
import rrt_amd                     # noqa: E402,F401
from radiance_ray_tracing_amd import rd, scenes    # noqa: E402

OUT = os.path.join(ROOT, "gpurun_out", "golden")


def main():
    os.makedirs(OUT, exist_ok=True)
    ref = rg.RefGpu("p")
    k = gc.kat_inputs()
    out = dict(k)
    out["aabb_hit"] = ref.aabb(k["aabb_o"], k["aabb_d"], k["aabb_lo"], k["aabb_hi"]).astype(np.uint8)
    hit, t, pt, bary = ref.triangle(k["tri_o"], k["tri_d"], k["tri_v0"], k["tri_v1"], k["tri_v2"])
    out.update(tri_hit=hit.astype(np.uint8), tri_t=t, tri_pt=pt, tri_bary=bary)
    out["brdf_out"] = ref.brdf(k["brdf_in"])
    np.savez_compressed(os.path.join(OUT, "refgpu_kat.npz"), **out)
    print("refgpu_kat.npz: aabb hits %d / %d, triangle hits %d / %d" % (out["aabb_hit"].sum(), out["aabb_hit"].size,
                                                                       out["tri_hit"].sum(), out["tri_hit"].size), flush=True)
    for name in gc.SCENES:
        s = gc.small_scene(scenes, name)
        blob = gc.scene_blob(rd, s)
        rs = rg.RefScene(ref, s, blob)
        out = {"blob_sha256": gc.sha(blob)}
        # primary rays: generateRay for every pixel
        npix = s.width * s.height
        rnd = gc.generate_inputs(npix, 3)
        go, gd = rs.generate(rnd)
        out.update(gen_rnd=rnd, gen_o=go, gen_d=gd)
        if name == "c1":                 # thin lens variant
            s2 = gc.small_scene(scenes, name, fstop=2.8)
            rs2 = rg.RefScene(ref, s2, blob)
            lo, ld = rs2.generate(rnd)
            out.update(lens_o=lo, lens_d=ld)
        # traversal batch
        sel = gc.spread(npix, gc.N_PRIMARY)
        po, pd = go[sel], gd[sel]
        ph = rs.trace(po, pd)
        o, d = gc.derived_rays(5, po, pd, ph["hit"], ph["distance"])
        h1 = rs.trace(o, d, 0.001, 1000.0, 1)
        h2 = rs.trace(o, d, 0.001, 1000.0, 2)
        out.update(ray_o=o, ray_d=d, hits=h1.view(np.uint8).reshape(h1.shape[0], -1), shadow_hit=h2["hit"].astype(np.uint8))
        # material on the closest hits of primary rays (item i is shaded as pixel i, the reference's RNG input)
        # (the hit of item i need not be pixel i's own: rays spread over the image)
        sel = gc.spread(npix, gc.N_MATERIAL)
        n = sel.shape[0]
        md = np.ascontiguousarray(gd[sel])
        mh = rs.trace(go[sel], md)
        frames, depths = gc.material_inputs(n)
        pay = rs.material_batch(mh, md, frames, depths)
        out.update(mat_hits=mh.view(np.uint8).reshape(n, -1), mat_dir=md, mat_payload=pay.view(np.uint8).reshape(n, -1))
        # two progressive frames
        for f in range(2):
            rs.frame()
            out["scratch%d" % f] = rs.read_scratch()
            out["image%d" % f] = rs.read_image()
        np.savez_compressed(os.path.join(OUT, "refgpu_%s.npz" % name), **out)
        print("refgpu_%s.npz: %d rays, %d closest hits, %d shadow hits, %d material hits" %
              (name, o.shape[0], int(h1["hit"].sum()), int(h2["hit"].sum()), int(mh["hit"].sum())), flush=True)


def save_npz_reproducibly(path, arrays):
    """np.savez_compressed with the archive's time stamps pinned (numpy stamps members with the wall clock)"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def rayedges(out_dir=OUT):
    import ray_edge_cases as rec
    os.makedirs(out_dir, exist_ok=True)
    ref = rg.RefGpu("p")
    out = {}
    for name in rec.SCENES:
        s = rec.scene(scenes, name)
        blob = gc.scene_blob(rd, s)
        rs = rg.RefScene(ref, s, blob)
        base = None
        if name in rec.GOLDEN:                  # the committed golden batch of the scene (itself the reference's output)
            G = np.load(os.path.join(HERE, "refgpu_%s.npz" % name))
            assert np.array_equal(G["blob_sha256"], gc.sha(blob))
            base = (G["ray_o"], G["ray_d"])
        cases = rec.Cases(scenes, name, base, None, rs.trace)
        cells = cases.cells()
        results = [(rs.trace(c.o, c.d, c.tmin, c.tmax, 1), rs.trace(c.o, c.d, c.tmin, c.tmax, 2)) for c in cells]
        out.update(rec.pack_scene(name, gc.sha(blob), cases.params, results))
        print("%s: %d cells, %d rays, %d closest hits, %d distinct records" % (name, len(cells), sum(c.n for c in cells),
              sum(int((r["hit"] == 1).sum()) for r, _ in results), out[name + "/recs"].shape[1]), flush=True)
    # rays of family F the live reference could not be run on: none -- every NaN comparison of its walk is false, it terminates
    out["notes"] = np.array([], dtype="U1")
    path = os.path.join(out_dir, "refgpu_rayedges.npz")
    save_npz_reproducibly(path, out)
    print("refgpu_rayedges.npz: %d bytes" % os.path.getsize(path), flush=True)


def meshedges(out_dir=OUT):
    import mesh_edge_cases as mec
    import ray_edge_cases as rec
    os.makedirs(out_dir, exist_ok=True)
    ref = rg.RefGpu("p")
    out = {}
    for c in mec.all_cases():
        blob = mec.product_blob(rd, c)[0]
        tl = rg.DevBuf.of(np.frombuffer(blob, np.uint8))
        cells = mec.cells(c)
        results = [(ref.trace(tl, x.o, x.d, x.tmin, x.tmax, 1), ref.trace(tl, x.o, x.d, x.tmin, x.tmax, 2)) for x in cells]
        out.update(rec.pack_scene(c.name, gc.sha(blob), {}, results))
        print("%s: %d cells, %d rays, %d closest hits, %d any hits" % (c.name, len(cells), sum(x.n for x in cells),
              sum(int((r["hit"] == 1).sum()) for r, _ in results), sum(int((r["hit"] == 1).sum()) for _, r in results)), flush=True)
    path = os.path.join(out_dir, "refgpu_meshedges.npz")
    save_npz_reproducibly(path, out)
    print("refgpu_meshedges.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)), flush=True)


def shadeedges(out_dir=OUT):
    import shade_edge_cases as se
    os.makedirs(out_dir, exist_ok=True)
    out = se.reference_recordings(rg.RefGpu("p"), rg, rd, scenes)
    path = os.path.join(out_dir, "refgpu_shade_edges.npz")
    save_npz_reproducibly(path, out)
    print("refgpu_shade_edges.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)), flush=True)


if __name__ == "__main__":
    if sys.argv[1:2] == ["rayedges"]:
        rayedges(*[os.path.abspath(a) for a in sys.argv[2:3]])
    elif sys.argv[1:2] == ["meshedges"]:
        meshedges(*[os.path.abspath(a) for a in sys.argv[2:3]])
    elif sys.argv[1:2] == ["shadeedges"]:
        shadeedges(*[os.path.abspath(a) for a in sys.argv[2:3]])
    else:
        main()
