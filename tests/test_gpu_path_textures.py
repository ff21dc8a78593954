"""GPU suite (-m gpu): the three path calls on a TEXTURED scene -- rd.TraceLightPaths, rd.TracePunctualPaths, rd.TraceAreaPaths
(rdx_trace_paths_lights, rdx_trace_paths_punctual, rdx_trace_paths_area) with option "textures" 0 and 1.

The shade kernels of the path calls evaluate the material of a hit with the text of rd.ResolveMaterials (csrc/hit_material.h), whose
texture reads tests/test_gpu_materials.py `test_textures` holds to rd.ShadeHits.  Here the branch that reads texels is held inside
the path calls themselves: each call equals the README's loop over the public per-hit calls on the same scene buffers, image array
and sampler (light_paths_cases.public_loop, punctual_cases.public_loop_punctual, area_cases.public_loop_area), bit for bit.  The
scene is material_cases.textured_scene (48 x 27 = 1296 primary rays, every one of the four texture indices set on some material),
the depth is 3.  The punctual table holds one record of every kind the light loop branches on -- directional, point, spot and a
dark one (type 3) --, the area table a one-sided quad and a two-sided triangle.
"""
import numpy as np
import pytest

import area_cases as ar
import light_paths_cases as lp
import material_cases as mc
import punctual_cases as pu
import shade_cases as sh

pytestmark = pytest.mark.gpu
F = np.float32
DEPTH = 3
LO, HI = (-3.0, 0.0, -3.0), (3.0, 4.0, 3.0)        # the box of textured_scene: floor, wall and cube


@pytest.fixture(scope="module")
def mods(gpu):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd, scenes
    return rd, scenes


def punctual_table(rd):
    return pu.table(rd, [pu.light(rd, pu.DIRECTIONAL, direction=(0.35, -0.8, 0.45), color=(2.5, 2.25, 2.0)),
                         pu.light(rd, pu.POINT, (-1.5, 2.5, -1.0), range=5.5, color=(20.0, 18.0, 15.0)),
                         pu.light(rd, pu.SPOT, (1.8, 3.5, -1.5), (-0.3, -1.0, 0.4), color=(30.0, 36.0, 44.0),
                                  cone=rd.SpotCone(np.radians(20.0), np.radians(40.0))),
                         pu.light(rd, 3, (0.0, 2.0, 0.0), color=(50.0, 50.0, 50.0))])


def test_the_path_calls_read_textures_as_the_loop_does(mods):
    rd, scenes = mods
    s = mc.textured_scene(scenes)
    dev = scenes.DeviceScene(s)
    plt, tlas = dev.plt, dev.topAccelStruct
    tex = mc.textures()
    img = rd.CreateImageArray(plt, 16, 16, 3)
    for l in range(3):
        rd.WriteImage(plt, img, 16, 16, l, tex[l])
    px = np.arange(s.width * s.height, dtype=np.uint32)
    assert px.shape[0] == 1296
    o, d = rd.GenerateBatch(px, np.stack([np.zeros_like(px), np.zeros_like(px), px], 1))
    rays, frames = sh.rays_of(rd, o, d), (px % 5).astype(np.uint32)
    keys = sh.keys_of(frames, px, np.zeros_like(px))
    table = punctual_table(rd)
    named = ar.scene_lights(rd, LO, HI)
    area = ar.table(rd, [named["ceiling"], named["inner"]])
    assert sorted(int(t) for t in table["type"]) == [0, 1, 2, 3] and area.shape[0] == 2
    scene3 = lp.scene_buffer(rd, plt, mc.three_lights(rd))
    surf = dev.surface_buffers()
    got = {}
    try:
        for textures in (0, 1):
            rd.SetOption("textures", textures)
            sb = rd.ShadingBuffers(scene3, dev.meshInfoData, dev.indexData, dev.uvData, dev.normalData, dev.materialData, img,
                                   rd.CreateSampler(plt, rd.RD_ADDRESS_REPEAT, rd.RD_FILTER_LINEAR))
            # the depth-0 hits: all three materials, each of them textured, on more than 20 hits
            n = rays.shape[0]
            bR = sh.upload(rd, plt, rays)
            bM, invalid = rd.ResolveMaterials(tlas, bR, rd.QueryRays(tlas, bR, n, rd.QUERY_CLOSEST), n, sb)
            mat = sh.read(rd, plt, bM, n, mc.MATERIAL_RECORD_DTYPE)
            hit = mat["hit"] == 1
            per_material = [int((hit & (mat["materialIndex"] == m)).sum()) for m in range(3)]
            print("textures %d: depth-0 hits per material %s of %d rays" % (textures, per_material, n))
            assert invalid == 0 and set(np.unique(mat["materialIndex"][hit])) == {0, 1, 2} and min(per_material) > 20

            runs = (("area", lambda: ar.trace(rd, plt, tlas, sb, rays, keys, DEPTH, table, area),
                     lambda: ar.public_loop_area(rd, plt, tlas, sb, surf, table, area, rays, frames, px, DEPTH)),
                    ("punctual", lambda: pu.trace(rd, plt, tlas, sb, rays, keys, DEPTH, table),
                     lambda: pu.public_loop_punctual(rd, plt, tlas, sb, surf, table, rays, frames, px, DEPTH)),
                    ("lights", lambda: lp.trace(rd, plt, tlas, sb, rays, keys, DEPTH, 3),
                     lambda: lp.public_loop(rd, plt, tlas, sb, surf, 3, rays, frames, px, DEPTH)))
            for call, run, loop in runs:
                radiance, invalid = run()
                want = loop()
                color, lives, loop_invalid = want[0], want[1], want[2]
                tag = "%s, textures %d" % (call, textures)
                assert invalid == 0 and loop_invalid == 0, tag
                assert len(lives) == DEPTH and lives[0] == int(hit.sum()) and lives[-1] > 20, (tag, lives)
                assert np.isfinite(color).all(), tag
                eq = (sh.bits(radiance[:, :3]) == sh.bits(color)).all(1)
                assert eq.all(), "%s: radiance differs from the loop on %d of %d paths (first: %s)" % (tag, int((~eq).sum()), n, np.flatnonzero(~eq)[:8].tolist())
                assert not sh.bits(radiance[:, 3]).any(), tag
                if call != "lights":       # every uniform branch of the punctual loop is taken: a dark record, and three that light hits
                    dark0 = want[4]
                    assert dark0[3][1] == 0 and dark0[3][0] == lives[0] and all(lit > 20 for _, lit in dark0[:3]), (tag, dark0)
                if call == "area":
                    assert all(lit > 20 for _, lit in dark0[4:]), (tag, dark0)
                got[(call, textures)] = radiance
        for call in ("area", "punctual", "lights"):
            differ = (sh.bits(got[(call, 0)]) != sh.bits(got[(call, 1)])).any(1)
            print("%s: radiance differs between textures 0 and 1 on %d of %d paths" % (call, int(differ.sum()), differ.shape[0]))
            assert differ.any(), call
        # the three calls are three light sets, not one
        assert not mc.same(got[("area", 1)], got[("punctual", 1)]) and not mc.same(got[("punctual", 1)], got[("lights", 1)])
    finally:
        rd.SetOption("textures", 0)
