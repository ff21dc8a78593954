#!/usr/bin/env python3
"""tlas_update_bench.py [--steps 24] [--rays 2097152] [--out profiles/tlas_update_bench.json]

What moving ONE instance costs, on the Sponza-class scene (25 instances, 262 144 triangles) and the 400-instance atrium: per step
one instance gets another translation, then `rays` rays are queried (rd.QueryRays, closest hit) against the scene.

  update   rd.UpdateAccelStruct + the first QueryRays after it           (wall clock, and the update alone)
  rebuild  rd.BuildAccelStruct of all instances + the first QueryRays    (the only route without the update: a new buffer, the
           whole blob uploaded, the traversal layout derived again; the old buffer stays allocated until shutdown)

Per scene and route: median, minimum and maximum over the steps, the update's path / bytes / owner words per step, and the
update's device time (ms_device: the owner-fill kernel) beside the kernel time of the query (rdx_trace_stats.ms_extend).
The rays are the same for both routes and every step: from one point outside the scene through a jittered cloud, fixed seed.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def stats(xs):
    a = np.array(xs, np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()), "n": int(a.shape[0])}


def main():
    args = dict(zip(sys.argv[1::2], sys.argv[2::2]))
    steps, nrays = int(args.get("--steps", 24)), int(args.get("--rays", 1 << 21))
    out_path = args.get("--out", os.path.join(ROOT, "profiles", "tlas_update_bench.json"))
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd, scenes
    plt = rd.Platform.GetPlatform()
    result = {"device": rd.Platform.device_name(), "steps": steps, "rays": nrays, "scenes": {}}
    for name, make in (("sponza_class", lambda: scenes.c2_atrium(64, 36, 1, 1)), ("atrium_400", lambda: scenes.c2_atrium_400(64, 36, 1, 1))):
        s = make()
        blases = rd.BuildAccelStructs(plt, [rd.Mesh(m[0], m[1]) for m in s.meshes])
        base = [np.array(tf, np.float32) for _, tf, _ in s.instances]

        def insts(step):
            """the scene after `step` steps: step t moves instance 1 + (t - 1) % 3 another 0.05 along x, nothing else"""
            tfs = [t.copy() for t in base]
            for j in (1, 2, 3):
                moved = max(0, (step - j + 3) // 3)
                if moved:
                    tfs[j] = (scenes.translate(0.05 * moved, 0, 0) @ base[j]).astype(np.float32)
            return [rd.Instance(tfs[i], 0, mat, blases[mi]) for i, (mi, _, mat) in enumerate(s.instances)]

        lo = np.min([np.asarray(m[0]).reshape(-1, 3).min(0) for m in s.meshes], 0).astype(np.float64)
        hi = np.max([np.asarray(m[0]).reshape(-1, 3).max(0) for m in s.meshes], 0).astype(np.float64)
        rng = np.random.default_rng(7)
        c, r = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
        eye = c + np.array([0.3, 0.45, 1.0]) / np.linalg.norm([0.3, 0.45, 1.0]) * 0.4 * r
        d = c + rng.uniform(-1, 1, (nrays, 3)) * (hi - lo) * 0.55 - eye
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays = np.zeros(nrays, rd.RAY_DTYPE)
        rays["origin"], rays["direction"], rays["tmin"], rays["tmax"] = eye.astype(np.float32), d.astype(np.float32), 0.001, 1000.0
        bRays = rd.CreateBuffer(plt, nrays * 32)
        rd.WriteBuffer(plt, bRays, nrays * 32, rays)
        bHits = rd.CreateBuffer(plt, nrays * 32)

        tlas = rd.BuildAccelStruct(plt, insts(0))
        rd.QueryRays(tlas, bRays, nrays, 1, bHits)          # the layout exists before the first update
        hits0 = int(rd.ReadBuffer(plt, bHits, nrays * 32).view(rd.RAY_HIT_DTYPE)["hit"].sum())
        upd, upd_only, upd_query, per_step, kernel_ms = [], [], [], [], []
        for step in range(1, steps + 1):
            ii = insts(step)
            t0 = time.perf_counter()
            rd.UpdateAccelStruct(plt, tlas, ii)
            t1 = time.perf_counter()
            rd.QueryRays(tlas, bRays, nrays, 1, bHits)
            t2 = time.perf_counter()
            st = rd.GetTlasUpdateStats()
            kernel_ms.append(float(rd.GetTraceStats().ms_extend))
            upd.append((t2 - t0) * 1e3); upd_only.append((t1 - t0) * 1e3); upd_query.append((t2 - t1) * 1e3)
            per_step.append({"path": int(st.path), "top_nodes": [int(st.top_nodes_before), int(st.top_nodes_after)], "bytes_h2d": int(st.bytes_h2d),
                             "bytes_d2d": int(st.bytes_d2d), "owner_words": int(st.tri_slots_rewritten), "ms_host": float(st.ms_host),
                             "ms_device": float(st.ms_device)})
        ref_hits = rd.ReadBuffer(plt, bHits, nrays * 32).copy()
        reb, reb_only, reb_query = [], [], []
        for step in range(1, steps + 1):
            ii = insts(step)
            t0 = time.perf_counter()
            fresh = rd.BuildAccelStruct(plt, ii)
            t1 = time.perf_counter()
            rd.QueryRays(fresh, bRays, nrays, 1, bHits)
            t2 = time.perf_counter()
            reb.append((t2 - t0) * 1e3); reb_only.append((t1 - t0) * 1e3); reb_query.append((t2 - t1) * 1e3)
        same = bool(np.array_equal(ref_hits, rd.ReadBuffer(plt, bHits, nrays * 32)))
        inc = [k for k, p in enumerate(per_step) if p["path"] == 1]
        result["scenes"][name] = {
            "instances": len(s.instances), "triangles": s.triangle_count(), "blob_bytes": int(tlas.size), "hits_of_first_query": hits0,
            "last_step_answers_equal_rebuild": same,
            "update_plus_first_query_ms": stats(upd), "update_ms": stats(upd_only), "query_after_update_ms": stats(upd_query),
            "update_plus_first_query_ms_incremental_steps": stats([upd[k] for k in inc]) if inc else None,
            "rebuild_plus_first_query_ms": stats(reb), "rebuild_ms": stats(reb_only), "query_after_rebuild_ms": stats(reb_query),
            "ratio_of_medians_rebuild_over_update": float(np.median(reb) / np.median(upd)),
            "query_kernel_ms": stats(kernel_ms), "update_ms_device": stats([p["ms_device"] for p in per_step]),
            "update_ms_host": stats([p["ms_host"] for p in per_step]), "per_step": per_step}
        print(name, json.dumps({k: v for k, v in result["scenes"][name].items() if k != "per_step"}), flush=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
