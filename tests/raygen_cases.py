"""Shared pieces of the tests of rd.GenerateRays / rd.Accumulate (test_raygen_cpu.py, test_gpu_raygen.py): the two ends of a frame
on the device.

running_mean is the numpy float32 restatement of what rdx_accumulate does to imageScratch, one operation at a time under the
contract of DESIGN.md section 2 (samples/shader.cl:262-270):

    imageScratch.rgb = color                                                              frameID == 0
    imageScratch.rgb = (float(frameID) * imageScratch.rgb + color) / float(frameID + 1)   otherwise; imageScratch.w stays

sample_colors is the per-sample half of shade_cases.compose_frames -- the reference's raygen loop up to the point where a sample
is finished -- so that the mean can be tested on its own; test_raygen_cpu.py pins the pair to the CPU oracle's own frames.
device_frames is the same loop over the public GPU calls alone, with GenerateRays at its start and Accumulate at its end.
"""
import numpy as np

import shade_cases as sh

F = np.float32
U4 = np.dtype("<u4")
RAYGEN_SEED_DTYPE = np.dtype([("in", "<u4", 3), ("_0", "<u4")])          # rdx_raygen_seed
SENTINEL = 0xA5


def running_mean(scratch, color, frame, pixels=None):
    """sample `frame` (colours (n, >= 3) float32) folded into scratch (npix, 4) float32, in place, for `pixels` (default: 0 .. n - 1)"""
    assert scratch.dtype == F and scratch.ndim == 2 and scratch.shape[1] == 4
    c = np.ascontiguousarray(color, F)[:, :3]
    px = np.arange(c.shape[0]) if pixels is None else np.asarray(pixels, np.int64)
    assert np.unique(px).shape[0] == px.shape[0], "the pixels of one call must be distinct"
    if frame == 0:
        scratch[px, :3] = c
    else:
        scaled = (F(frame) * scratch[px, :3]).astype(F)
        total = (scaled + c).astype(F)
        scratch[px, :3] = (total / F(frame + 1)).astype(F)
    return scratch


def debug_rgba8(mean):
    """RTProp.debug: (unsigned char)(int)(c * 255) per channel, alpha 255 -- for means in [0, 1)"""
    m = np.ascontiguousarray(mean, F)[:, :3]
    assert (m >= 0).all() and (m < 1).all()
    out = np.full((m.shape[0], 4), 255, np.uint8)
    out[:, :3] = (m * F(255)).astype(F).astype(np.int32).astype(np.uint8)
    return out


def sample_colors(npix, frame, total, max_depth, generate, bounce):
    """the colour of sample `frame` of every pixel, (npix, 3) float32: the reference's raygen loop (shader.cl:197-260) around the
    two callables of shade_cases.compose_frames"""
    px = np.arange(npix, dtype=np.uint32)
    rnd = np.stack([np.full(npix, frame, np.uint32), np.full(npix, total, np.uint32), px], 1)       # shader.cl:205
    o, d = generate(px, rnd)
    o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
    color = np.zeros((npix, 3), F)
    contribution = np.ones((npix, 3), F)
    alive = px.astype(np.int64)
    for depth in range(int(max_depth)):
        if not alive.size:
            break
        hit, pc, nf, no, nd = bounce(o, d, frame, alive.astype(np.uint32), depth)
        hit = np.asarray(hit, bool)
        pc, nf = np.ascontiguousarray(pc, F), np.ascontiguousarray(nf, F)
        h = alive[hit]
        color[h] = color[h] + contribution[h] * pc[hit]
        contribution[h] = contribution[h] * nf[hit]
        if depth == 0:
            color[alive[~hit]] = pc[~hit]
        alive = h
        o, d = np.ascontiguousarray(no, F)[hit], np.ascontiguousarray(nd, F)[hit]
    return color


def frames_of(npix, total_samples, batch_size, max_depth, nframes, generate, bounce):
    """shade_cases.compose_frames, taken apart: sample_colors, then running_mean"""
    scratch = np.zeros((npix, 4), F)
    out, total = [], int(total_samples)
    for _ in range(nframes):
        for it in range(int(batch_size)):
            running_mean(scratch, sample_colors(npix, total + it, total, max_depth, generate, bounce), total + it)
        total += int(batch_size)
        out.append(scratch.copy())
    return out


# ---- the public GPU calls -----------------------------------------------------------------------------------------------------------
def seeds_of(rnd):
    s = np.zeros(np.asarray(rnd).shape[0], RAYGEN_SEED_DTYPE)
    s["in"] = rnd
    return s


def filled(rd, plt, size, value=SENTINEL):
    buf = rd.CreateBuffer(plt, size)
    rd.WriteBuffer(plt, buf, size, np.full(size, value, np.uint8))
    return buf


def whole(rd, plt, buf):
    return rd.ReadBuffer(plt, buf, buf.size).copy()


def device_sample(rd, dev, sb, frame, total, max_depth):
    """one sample of every pixel from the public calls: GenerateRays -> per bounce (QueryRays closest -> ShadeHits, compacting ->
    QueryRays any on the shadow rays -> the fold, in numpy float32).  The rays, their keys of depth 0, the hit records, the shade
    records and the next rays never leave the device; the shade records and the shadow answers are read back for the fold.
    -> colours (npix, 4) float32 with a junk w"""
    plt, tlas = dev.plt, dev.topAccelStruct
    npix = dev.width * dev.height
    rays, keys = rd.GenerateRays(dev.frame_buffers()[0], npix, frame, total)
    color = np.zeros((npix, 3), F)
    contribution = np.ones((npix, 3), F)
    path = np.arange(npix, dtype=np.int64)          # the pixel of live ray k
    n = npix
    for depth in range(int(max_depth)):
        if not n:
            break
        if depth:
            keys = sh.upload(rd, plt, sh.keys_of(frame, path.astype(np.uint32), depth))
        hits = rd.QueryRays(tlas, rays, n, rd.QUERY_CLOSEST)
        bS, bN, bSh, bSrc, live, invalid = rd.ShadeHits(tlas, rays, hits, keys, n, sb, compact=True)
        assert invalid == 0
        s = sh.read(rd, plt, bS, n, rd.SHADE_DTYPE)
        hit = s["hit"] == 1
        assert int(hit.sum()) == live
        occluded = np.zeros(n, bool)
        if live:
            shadowed = sh.read(rd, plt, rd.QueryRays(tlas, bSh, live, rd.QUERY_ANY), live, rd.RAY_HIT_DTYPE)["hit"] == 1
            occluded[hit] = shadowed[s["slot"][hit]]
        pc = sh.chosen_color(s, occluded)
        h = path[hit]
        color[h] = color[h] + contribution[h] * pc[hit]
        contribution[h] = contribution[h] * s["nextFactor"][hit]
        if depth == 0:
            color[path[~hit]] = pc[~hit]
        path = path[sh.read(rd, plt, bSrc, live, U4).astype(np.int64)]      # next ray k continues input ray src[k]
        rays, n = bN, live
    out = np.full((npix, 4), 7.0, F)                # w is ignored by Accumulate
    out[:, :3] = color
    return out


def device_frames(rd, dev, scratch, image, total_samples, batch_size, max_depth, nframes):
    """`nframes` progressive frames into the device buffers scratch / image (image may be None), every sample ended by
    rd.Accumulate -> [(imageScratch (npix, 4) float32, image (npix, 4) uint8 or None) after each frame]"""
    plt, npix = dev.plt, dev.width * dev.height
    sb = dev.shading_buffers()
    out, total = [], int(total_samples)
    for _ in range(nframes):
        for it in range(int(batch_size)):
            colors = sh.upload(rd, plt, device_sample(rd, dev, sb, total + it, total, max_depth))
            assert rd.Accumulate(colors, npix, total + it, scratch, image) == 0
        total += int(batch_size)
        out.append((rd.ReadBuffer(plt, scratch, npix * 16).view(F).reshape(npix, 4).copy(),
                    rd.ReadBuffer(plt, image, npix * 4).reshape(npix, 4).copy() if image is not None else None))
    return out
