"""Shared pieces of the material-record tests (test_materials_cpu.py, test_gpu_materials.py): rd.ResolveMaterials / rd.LightHits
(rdx_resolve_materials, rdx_light_hits).

The comparand is rdx_shade_hits (tests/test_gpu_shade.py holds it to the reference's recorded payloads): the stock closest-hit
shader ends with

    direct  = (0, 0, 0) + microfacetBRDF(...) * lights[0].color          -- rdx_light_hits' `lit` for light 0
    ambient = albedo * 0.1f
    payload.color = direct + ambient            (the shadow ray is not occluded: rdx_shade.color)
    payload.color = (0, 0, 0) + ambient         (it is: rdx_shade.colorOccluded)

so the two colours of a shade record follow from a material record and a lit colour by two float32 operations, restated here in
numpy one IEEE operation per call (no contraction).  Every bar is equality of bits.
"""
import numpy as np

import shade_cases as sh

F = np.float32
MATERIAL_RECORD_DTYPE = np.dtype([("normal", "<f4", 3), ("hit", "<u4"), ("albedo", "<f4", 3), ("materialIndex", "<u4"), ("metallic", "<f4"),
                                  ("roughness", "<f4"), ("transmission", "<f4"), ("ior", "<f4"), ("above", "<f4", 3), ("_0", "<u4")])  # rdx_material_record
LIT_DTYPE = np.dtype([("rgb", "<f4", 3), ("w", "<f4")])
bits = sh.bits


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def ambient(albedo):
    """albedo * 0.1f (shader.cl:510): one float32 multiplication"""
    return (np.ascontiguousarray(albedo, F) * F(0.1)).astype(F)


def color_lit(lit_rgb, albedo):
    """payload.color with the light visible: direct + ambient"""
    return (np.ascontiguousarray(lit_rgb, F) + ambient(albedo)).astype(F)


def color_occluded(albedo):
    """payload.color with the light hidden: (0, 0, 0) + ambient"""
    return (np.zeros(3, F) + ambient(albedo)).astype(F)


def clamp(x, lo, hi):
    """clamp of finite values: max then min, each one IEEE operation (v_med3_f32 gives the same for finite x, lo <= hi)"""
    return np.minimum(np.maximum(np.ascontiguousarray(x, F), F(lo)), F(hi)).astype(F)


def table_props(materials, material_index):
    """what getAlbedo / getMaterialProp give for Material records whose texture index is -1: the table's values, clamped as the
    shader clamps them -> dict of albedo (n, 3), metallic, roughness, transmission, ior (n,) and `untextured` masks per field"""
    mt = np.ascontiguousarray(materials)[material_index]
    return dict(albedo=np.ascontiguousarray(mt["albedo"][:, :3], F), metallic=np.ascontiguousarray(mt["metallic"], F),
                roughness=clamp(mt["roughness"], 0.0, 1.0), transmission=clamp(mt["transmission"], 0.0, 1.0), ior=clamp(mt["ior"], 0.0, 10.0),
                plain=dict(albedo=mt["albedoTexIdx"] == -1, metallic=mt["metallicTexIdx"] == -1, roughness=mt["roughnessTexIdx"] == -1,
                           normal=mt["normalTexIdx"] == -1))


def all_finite(*arrays):
    return all(np.isfinite(np.ascontiguousarray(a, F)).all() for a in arrays)


# ---- the calls, on device buffers ----------------------------------------------------------------------------------------------------
def material_batch(rd, plt, tlas, sb, rays, scene=None, light=0, hits=None, want_shadow=True):
    """QueryRays (closest) -> ResolveMaterials -> LightHits(light) -> QueryRays (any) on its shadow rays -> dict: q (query records),
    mat (MATERIAL_RECORD_DTYPE), invalid, lit (LIT_DTYPE), shadow (rd.RAY_DTYPE), occluded (bool per ray), and the device buffers
    bR, bH, bM.  hits: records to resolve instead of the query's; scene: the SceneProperties buffer LightHits reads (sb.scene)"""
    n = rays.shape[0]
    bR = sh.upload(rd, plt, rays)
    bH = rd.QueryRays(tlas, bR, n, rd.QUERY_CLOSEST) if hits is None else sh.upload(rd, plt, hits)
    bM, invalid = rd.ResolveMaterials(tlas, bR, bH, n, sb)
    out = dict(q=sh.read(rd, plt, bH, n, rd.RAY_HIT_DTYPE), mat=sh.read(rd, plt, bM, n, MATERIAL_RECORD_DTYPE), invalid=invalid, bR=bR, bH=bH, bM=bM)
    out.update(light_batch(rd, plt, tlas, bR, bM, n, scene if scene is not None else sb.scene, light, want_shadow))
    return out


def light_batch(rd, plt, tlas, bR, bM, n, scene, light, want_shadow=True):
    bL, bSh = rd.LightHits(bR, bM, n, scene, light, shadow=True if want_shadow else None)
    occluded = np.zeros(n, bool)
    shadow = None
    if want_shadow:
        shadow = sh.read(rd, plt, bSh, n, rd.RAY_DTYPE)
        if n:
            occluded = sh.read(rd, plt, rd.QueryRays(tlas, bSh, n, rd.QUERY_ANY), n, rd.RAY_HIT_DTYPE)["hit"] == 1
    return dict(lit=sh.read(rd, plt, bL, n, LIT_DTYPE), shadow=shadow, occluded=occluded)


def check_against_shade(m, r, tag=""):
    """identity 1 of the issue between a material_batch `m` (light 0) and a not compacting shade_batch `r` of the same rays and
    records under the same settings"""
    mat, s = m["mat"], r["shade"]
    k = mat["hit"] == 1
    assert all_finite(mat["normal"], mat["albedo"], mat["metallic"], mat["roughness"], mat["transmission"], mat["ior"], mat["above"],
                      m["lit"]["rgb"], s["color"], s["colorOccluded"]), tag
    assert np.array_equal(mat["hit"], s["hit"]) and np.array_equal(mat["materialIndex"], s["materialIndex"]), tag
    assert not mat[~k].view(np.uint8).any() and not m["lit"][~k].view(np.uint8).any(), "%s: a miss is not zero bytes" % tag
    assert not mat["_0"].any() and not bits(m["lit"]["w"]).any(), tag
    for name, got, want in (("colorOccluded", color_occluded(mat["albedo"][k]), s["colorOccluded"][k]),
                            ("color", color_lit(m["lit"]["rgb"][k], mat["albedo"][k]), s["color"][k])):
        eq = (bits(got) == bits(want)).all(1)
        assert eq.all(), "%s: %s differs on %d of %d hits" % (tag, name, int((~eq).sum()), eq.shape[0])
    assert same(m["shadow"], r["shadow"]), "%s: shadow rays" % tag
    assert np.array_equal(m["occluded"], r["occluded"]), tag


def three_lights(rd):
    """a SceneProperties of lightCount 3: three lights of distinct directions and colours; light 1 shines upwards (below the
    horizon of every surface that faces up or sideways-and-up)"""
    sp = np.zeros((), rd.SceneProperties)
    sp["lightCount"][0] = 3
    for j, (d, c) in enumerate((((0.35, -0.8, 0.45), (5.0, 4.5, 4.0)), ((-0.2, 0.9, -0.3), (0.5, 2.0, 6.0)), ((-0.7, -0.25, -0.6), (3.0, 0.75, 1.5)))):
        sp["lights"][j]["direction"] = (d[0], d[1], d[2], 0.0)
        sp["lights"][j]["color"] = (c[0], c[1], c[2], 1.0)
    return sp


def with_first_light(rd, sp, j):
    """a SceneProperties whose lights[0] is light j of `sp`"""
    out = np.array(sp).copy()
    out["lights"][0] = np.array(sp)["lights"][j]
    return out


# ---- frames: compose_frames driven by ResolveMaterials + LightHits for the colour ------------------------------------------------------
def gpu_callables(rd, dev):
    """(generate, bounce) of sh.compose_frames: the colour of a hit comes from ResolveMaterials + LightHits(0) + an any-hit query of
    the shadow records + the ambient term, the next ray and factor from ShadeHits (not compacting); a miss has the miss colour"""
    plt, tlas, sb = dev.plt, dev.topAccelStruct, dev.shading_buffers()

    def bounce(o, d, frame, pixels, depth):
        n = o.shape[0]
        rays = sh.rays_of(rd, o, d)
        m = material_batch(rd, plt, tlas, sb, rays)
        bS, bN, _, _, live, invalid = rd.ShadeHits(tlas, m["bR"], m["bH"], sh.upload(rd, plt, sh.keys_of(frame, pixels, depth)), n, sb, shadow=None)
        assert invalid == 0 and m["invalid"] == 0
        s, nxt = sh.read(rd, plt, bS, n, rd.SHADE_DTYPE), sh.read(rd, plt, bN, n, rd.RAY_DTYPE)
        hit = m["mat"]["hit"] == 1
        assert np.array_equal(hit, s["hit"] == 1) and int(hit.sum()) == live
        albedo = m["mat"]["albedo"]
        pc = np.where(m["occluded"][:, None], color_occluded(albedo), color_lit(m["lit"]["rgb"], albedo)).astype(F)
        pc[~hit] = sh.ENVIRONMENT
        return hit, pc, s["nextFactor"], nxt["origin"], nxt["direction"]
    return rd.GenerateBatch, bounce


# ---- a textured scene: every one of the four texture indices is set on some material ---------------------------------------------------
def textured_scene(scenes, w=48, h=27):
    """two quads and a box: albedo map; albedo + roughness + metallic maps; albedo + normal map"""
    s = scenes.Scene("materials_textured")
    floor = s.add_mesh(scenes.quad([-3, 0, -3], [3, 0, -3], [3, 0, 3], [-3, 0, 3], [0, 1, 0]))
    wall = s.add_mesh(scenes.quad([-3, 0, 3], [3, 0, 3], [3, 4, 3], [-3, 4, 3], [0, 0, -1]))
    cube = s.add_mesh(scenes.box([-0.8, 0.0, -0.8], [0.8, 1.6, 0.8]))
    m0 = scenes.material((0.7, 0.7, 0.7), 0.0, 0.6); m0["albedoTexIdx"] = 0
    m1 = scenes.material((0.7, 0.7, 0.7), 0.0, 0.6); m1["albedoTexIdx"] = 1; m1["roughnessTexIdx"] = 2; m1["metallicTexIdx"] = 2
    m2 = scenes.material((0.9, 0.8, 0.5), 0.2, 0.4); m2["albedoTexIdx"] = 0; m2["normalTexIdx"] = 1
    s.materials = [m0, m1, m2]
    s.add_instance(floor, None, 0); s.add_instance(wall, None, 1); s.add_instance(cube, scenes.translate(0.3, 0.0, 0.2) @ scenes.rotate_y(25.0), 2)
    s.camera = scenes.blender_camera(w, h, 0.05, 0.036, 8.0, 0.0, (0.5, 9.0, 2.5), (-100.0, 180.0, 0.0))
    s.sceneProps = scenes.blender_dir_light(-45.0, 20.0, 6.0)
    s.rtprop = scenes._rtprop(0, 2, 3)
    return s


def textures(size=16):
    """three RGBA8 layers that vary in every channel the shader reads"""
    yy, xx = np.mgrid[0:size, 0:size]
    t = np.zeros((3, size, size, 4), np.uint8)
    t[0, ..., 0] = np.where(((xx // 2) + (yy // 2)) % 2, 230, 40); t[0, ..., 1] = 120; t[0, ..., 2] = (xx * 16) % 256; t[0, ..., 3] = 255
    t[1, ..., 0] = (xx * 13 + yy * 5) % 256; t[1, ..., 1] = (yy * 21) % 256; t[1, ..., 2] = 200; t[1, ..., 3] = 255
    t[2, ..., 0] = 17; t[2, ..., 1] = 60 + (xx % 4) * 32; t[2, ..., 2] = np.where(yy % 8 < 4, 0, 255); t[2, ..., 3] = 255
    return t


# ---- bounds: the construction of test_gpu_shade.py's test_records_that_point_outside_a_buffer_are_zeroed_and_counted ------------------
SLACK = 4096


def bounds_case(rd, c, q):
    """c: sh.Golden("c1"); q: the closest-hit records of c.mat_rays (all hits).  Every scene stream lives in an allocation 4 KiB
    larger than its content (the slack holds plausible values) and the library gets a view of the content alone; a two-layer
    image array is given, so with option "textures" 1 the uv stream and the texture indices count.  The streams are c1's with: one
    trap triangle (0, 1, the vertex one past the last mesh) appended to the indices; a Material with albedoTexIdx == layers
    appended, which instance T's MeshInfo points at; instance M's MeshInfo pointing past the Material table.
    -> (sb, ok, bad, poisoned, check): ok = q with the records that hit M or T re-pointed at instance 0 (no record breaks a rule),
    bad = ok with 64 records rewritten so that each breaks one rule by less than the slack, poisoned = their mask, check(hits,
    mask) = asserts through the host seam rd.DebugShadeInBounds that exactly the masked records are invalid"""
    plt, b = c.dev.plt, c.b
    M, T, LAYERS = 5, 6, 2
    mi, mt = b["meshInfo"].copy(), b["material"]
    ninst, nidx0, nfl, nmat = mi.shape[0], b["index"].shape[0], b["normal"].shape[0], b["material"].shape[0]
    A = int(np.flatnonzero(mi["normalOffset"] == mi["normalOffset"].max())[-1])
    assert A not in (M, T) and b["uv"].shape[0] == nfl
    nvA = (nfl - int(mi[A]["normalOffset"])) // 3
    index = np.concatenate([b["index"], np.array([0, 1, nvA], np.uint32)])
    bad_mat = mt[:1].copy()
    bad_mat["albedoTexIdx"] = LAYERS
    materials = np.concatenate([mt, bad_mat])
    mi[T]["materialIndex"] = nmat
    mi[M]["materialIndex"] = nmat + 1 + 20                     # 21 records past the table: 1008 bytes into the slack
    nidx = index.shape[0]
    trap = lambda inst, k: (nidx0 - int(mi[inst]["indexOffset"])) // 3 + k

    def view(content, slack_fill):
        content = np.ascontiguousarray(content)
        whole = np.concatenate([content.view(np.uint8).reshape(-1), np.resize(np.ascontiguousarray(slack_fill).view(np.uint8).reshape(-1), SLACK)])
        buf = sh.upload(rd, plt, whole)
        assert buf.size == content.nbytes + SLACK
        return rd.WrapDeviceMemory(plt, buf.device_ptr, content.nbytes, keepalive=buf)
    img = rd.CreateImageArray(plt, 4, 4, LAYERS)
    for l in range(LAYERS):
        rd.WriteImage(plt, img, 4, 4, l, np.full((4, 4, 4), 60 + 100 * l, np.uint8))
    sb = rd.ShadingBuffers(c.dev.rdSceneData, view(mi, mi[:1]), view(index, np.arange(3, dtype=np.uint32)), view(b["uv"], np.float32([0.25, 0.75, 0.0])),
                           view(b["normal"], np.float32([0.6, 0.0, 0.8])), view(materials, mt[:1]), img,
                           rd.CreateSampler(plt, rd.RD_ADDRESS_REPEAT, rd.RD_FILTER_NEAREST))
    assert (q["hit"] == 1).all()
    ok = q.copy()
    moved = np.isin(ok["instanceIndex"], (M, T))
    ok["instanceIndex"][moved], ok["primitiveIndex"][moved] = 0, 0
    rng = np.random.default_rng(9)
    rows = np.sort(rng.choice(q.shape[0], 64, replace=False))
    bad = ok.copy()
    for j, r in enumerate(rows):
        inst, k = int(bad["instanceIndex"][r]), j % 8
        if k == 0:      # instanceIndex: the first past the instance count (= the MeshInfo count), and further
            bad["instanceIndex"][r] = ninst + j // 8
        elif k == 1:    # ... and further ones whose MeshInfo would still be read from the slack (4096 / 32 = 128 records)
            bad["instanceIndex"][r] = ninst + 8 + 15 * (j // 8)
        elif k == 2:    # triangles past the index stream, by less than the slack
            bad["primitiveIndex"][r] = trap(inst, 1 + 37 * (j // 8))
        elif k == 3:    # 3 * primitiveIndex wraps in 32 bits to the triangle before the mesh / into the stream
            bad["primitiveIndex"][r] = (0xffffffff, 0x55555556, 0x7fffffff, 0xaaaaaaab)[(j // 8) % 4]
        elif k == 4:    # the trap triangle: a vertex whose normal and uv lie one vertex past their streams
            bad["instanceIndex"][r], bad["primitiveIndex"][r] = A, trap(A, 0)
        elif k == 5:    # materialIndex past the Material table
            bad["instanceIndex"][r], bad["primitiveIndex"][r] = M, (j // 8) % 2
        elif k == 6:    # a texture layer past the image array
            bad["instanceIndex"][r], bad["primitiveIndex"][r] = T, (j // 8) % 2
        else:           # a triangle far into the slack, its three indices still inside it
            bad["primitiveIndex"][r] = trap(inst, 300)
    assert 3 * 300 + 2 < SLACK // 4 and 8 + 15 * 7 < SLACK // 32 and (21 + 1) * 48 < SLACK
    poisoned = np.zeros(q.shape[0], bool)
    poisoned[rows] = True

    def check(hits, mask):
        for r in range(hits.shape[0]):
            inst, prim = int(hits["instanceIndex"][r]), int(hits["primitiveIndex"][r])
            first = int(mi[inst]["indexOffset"]) + 3 * prim if inst < ninst else -1
            idx3 = index[first:first + 3] if 0 <= first and first + 3 <= nidx else None
            got = rd.DebugShadeInBounds(mi, ninst, inst, prim, idx3, nidx, nfl, nfl, materials, textures=True, layers=LAYERS)
            assert got is (not mask[r]), (r, inst, prim)
    return sb, ok, bad, poisoned, check
