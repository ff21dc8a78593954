"""Helpers of the user-program texture tests (test_user_textures_cpu.py, test_gpu_user_textures.py): a numpy float32 restatement
of the texture array sampler (radiance-ray-tracing_amd/csrc/texture.h tex_read_ui, with the coordinate clamp of
csrc/user_texture.hip), in the same order of operations, and the compile-only seam of the run-time shader compiler."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LLVM = "/opt/rocm/lib/llvm/bin"
CLANG = os.path.join(LLVM, "clang")
F = np.float32

# texture.h TEX_ADDR_*
REPEAT, CLAMP_TO_EDGE, CLAMP, MIRRORED = 0, 1, 2, 3


def _addr(s, n, mode):
    nf = F(n)
    if mode == REPEAT:
        u = (s - np.floor(s)) * nf
        i = np.floor(u).astype(np.int64)
        return np.where(i > n - 1, i - n, i), u
    if mode == MIRRORED:
        sp = F(2.0) * np.rint(F(0.5) * s)
        sp = np.abs(s - sp)
        u = sp * nf
        i = np.floor(u).astype(np.int64)
        return np.where(i > n - 1, n - 1, i), u
    u = s * nf
    i = np.floor(u).astype(np.int64)
    if mode == CLAMP_TO_EDGE:
        return np.clip(i, 0, n - 1), u
    return np.where((i < 0) | (i > n - 1), -1, i), u


def _wrap(i, n, mode):
    if mode == REPEAT:
        return np.where(i < 0, i + n, np.where(i > n - 1, i - n, i))
    if mode in (MIRRORED, CLAMP_TO_EDGE):
        return np.clip(i, 0, n - 1)
    return np.where((i < 0) | (i > n - 1), -1, i)


def _texel(tex, layer, x, y):
    ok = (x >= 0) & (y >= 0)
    t = tex[layer, np.where(ok, y, 0), np.where(ok, x, 0)].astype(F)
    return np.where(ok[:, None], t, F(0.0))


def sample(tex, mode, linear, coords):
    """read_imageui(imageArray, sampler, coords) -> (N, 4) uint32; tex: (layers, h, w, 4) uint8, coords: (N, 4) float32"""
    layers, h, w, _ = tex.shape
    c = np.clip(np.asarray(coords, F), F(-16777216.0), F(16777216.0))          # user_texture.hip coord()
    u, v, lf = c[:, 0], c[:, 1], c[:, 2]
    layer = np.clip(np.rint(lf).astype(np.int64), 0, layers - 1)
    ix, uu = _addr(u, w, mode)
    iy, vv = _addr(v, h, mode)
    if not linear:
        return _texel(tex, layer, ix, iy).astype(np.uint32)
    fu, fv = uu - F(0.5), vv - F(0.5)
    i0, j0 = np.floor(fu).astype(np.int64), np.floor(fv).astype(np.int64)
    a, b = (fu - np.floor(fu))[:, None], (fv - np.floor(fv))[:, None]
    x0, x1 = _wrap(i0, w, mode), _wrap(i0 + 1, w, mode)
    y0, y1 = _wrap(j0, h, mode), _wrap(j0 + 1, h, mode)
    t00, t10, t01, t11 = _texel(tex, layer, x0, y0), _texel(tex, layer, x1, y0), _texel(tex, layer, x0, y1), _texel(tex, layer, x1, y1)
    one = F(1.0)
    r = (one - a) * (one - b) * t00 + a * (one - b) * t10 + (one - a) * b * t01 + a * b * t11 + F(0.5)
    assert r.dtype == F
    return r.astype(np.uint32)


def texel_read(tex, ic):
    """read_imageui(imageArray, (int4)(x, y, layer, 0)) -> (N, 4) uint32; out of range -> 0"""
    layers, h, w, _ = tex.shape
    x, y, z = ic[:, 0].astype(np.int64), ic[:, 1].astype(np.int64), ic[:, 2].astype(np.int64)
    ok = (x >= 0) & (y >= 0) & (z >= 0) & (x < w) & (y < h) & (z < layers)
    t = tex[np.where(ok, z, 0), np.where(ok, y, 0), np.where(ok, x, 0)].astype(np.uint32)
    return np.where(ok[:, None], t, 0).astype(np.uint32)


def test_image(w=48, h=32, layers=3, seed=5):
    """a non-square RGBA8 image array whose texels all differ from their neighbours"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(layers, h, w, 4), dtype=np.uint8)


def probe_program():
    return open(os.path.join(GOLD, "user_texture_probe.cl")).read()


def stage_program(read=True, query=False):
    """tests/golden/user_texture_stages.cl; read=False: the same program with the texel read replaced by a constant, query=True:
    with the stock shadow query in its closest-hit shader"""
    t = open(os.path.join(GOLD, "user_texture_stages.cl")).read()
    if not read:
        t2 = t.replace("read_imageui(imageArray, sampler, c)", "(uint4)((uint)c.x, 1u, 2u, 3u)")
        assert t2 != t
        t = t2
    if query:
        t2 = t.replace("    payload->hit = true;\n    const float4 c",
                       "    payload->hit = true;\n    struct Payload query;\n"
                       "    traceRay(sceneData->topLevel, 2, 4, payload->nextRayOrigin, (float3)(0.0f, 1.0f, 0.0f), 0.001f, 1000, &query, sceneData, imageArray, sampler);\n"
                       "    const float4 c")
        assert t2 != t
        t = t2
    return t


def jit_lib(path=None):
    L = ctypes.CDLL(path or os.path.join(ROOT, "radiance-ray-tracing_amd", "librdx.so"))
    L.rdx_last_error.restype = ctypes.c_char_p
    L.rdx_debug_jit_compiles.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_int]
    L.rdx_debug_jit_compile_to.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p]
    L.rdx_debug_jit_key.restype = ctypes.c_ulonglong
    L.rdx_debug_jit_key.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]
    L.rdx_debug_stage_reduced_hash.restype = ctypes.c_ulonglong
    L.rdx_debug_stage_reduced_hash.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    return L


def compile_to(lib, text, stages):
    """the code object the run-time compiler makes of `text` -> (disassembly, kernel notes); raises with the log if it fails"""
    t = text.encode() if isinstance(text, str) else text
    with tempfile.TemporaryDirectory() as d:
        co = os.path.join(d, "user.co")
        if lib.rdx_debug_jit_compile_to(t, len(t), b"gfx950", int(stages), co.encode()) != 0:
            raise RuntimeError(lib.rdx_last_error().decode())
        dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", co]).decode()
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co]).decode()
    return dis, notes


def image_instructions(dis):
    """hardware image instructions of a disassembly (mnemonics only, not symbol names)"""
    return [l.strip() for l in dis.splitlines() if re.match(r"\s+image_\w+", l)]


def _kernel_block(notes, kernel):
    for b in re.split(r"\n  - (?=\.)", notes):
        if re.search(r"\n    \.name:\s+%s\s*\n" % re.escape(kernel), "\n    " + b):
            return "\n    " + b
    raise KeyError(kernel)


def kernel_resources(notes, kernel):
    """{'.private_segment_fixed_size': .., '.vgpr_count': .., ...} of `kernel` from `llvm-readelf --notes`"""
    return {k: int(v) for k, v in re.findall(r"\n    (\.[a-z_]+):\s+(\d+)\s*(?=\n)", _kernel_block(notes, kernel))}


def kernel_args(notes, kernel):
    """[(offset, size, value_kind)] of the explicit arguments of `kernel`"""
    out = []
    block = _kernel_block(notes, kernel)
    args = re.search(r"\n    \.args:(.*?)(?=\n    \.|$)", block, re.S).group(1)
    for e in args.split("\n      - ")[1:]:
        kind = re.search(r"\.value_kind:\s+(\w+)", e).group(1)
        if not kind.startswith("hidden_"):
            out.append((int(re.search(r"\.offset:\s+(\d+)", e).group(1)), int(re.search(r"\.size:\s+(\d+)", e).group(1)), kind))
    return out


def assert_no_image_code(lib, text, stages):
    """the CPU-side check the GPU tests make before they launch a program: it compiles to a code object without hardware
    image instructions (an older library emits image_sample for read_imageui and fails here, before any launch)"""
    dis, notes = compile_to(lib, text, stages)
    kernel = "rdx_stage_entry" if stages else "rdx_user_entry"
    assert kernel in notes, notes[:2000]
    assert not image_instructions(dis), image_instructions(dis)[:5]
    return dis, notes
