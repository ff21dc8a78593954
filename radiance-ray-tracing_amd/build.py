"""build.py -- compiles the HIP ray-tracing core into radiance-ray-tracing_amd/librdx.so (in-tree), and the texture
functions of user shader programs (csrc/user_texture.hip) into device bitcode next to it (user_texture.bc), which the
run-time shader compiler links into every user program.

hipcc cross-compiles for gfx950 without a GPU.  -ffp-contract=off is part of the numerical
contract: traversal / intersection results must be the IEEE values of the
expressions as written.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "librdx.so")
# experiment builds: RDX_DEFINES="-DFOO -DBAR" RDX_LIB_NAME=librdx_foo.so python build.py --force
EXTRA = os.environ.get("RDX_DEFINES", "").split()
if os.environ.get("RDX_LIB_NAME"):
    LIB = os.path.join(HERE, os.environ["RDX_LIB_NAME"])
SOURCES = ["kernels.hip", "tlas_update.hip", "surface.hip", "shade.hip", "material.hip", "scatter.hip", "light_paths.hip", "punctual.hip", "area.hip", "env.hip", "env_mis.hip", "denoise.hip", "temporal.hip", "svgf.hip", "raygen.hip", "paths.hip", "rdx_runtime.cpp", "accel_layout.cpp", "bvh_build.cpp", "scene_obj.cpp", "user_shader.cpp"]
HEADERS = ["kernels.h", "accel_layout.h", "stages.h", "texture.h", "device_math.h", "rdx_types.h", "surface.h", "shade.h", "material_eval.h", "hit_material.h", "light_emit.h", "path_shade.h", "scatter.h", "light_paths.h", "punctual.h", "area.h", "env.h", "env_mis.h", "denoise.h", "temporal.h", "svgf.h", "raygen.h", "raygen_device.h", "paths.h", "bvh_build.h", "sbt_generated.h", "traverse_coop.h", "traverse_pool.h", "user_shader.h",
           os.path.join("..", "..", "include", "rdx.h")]
# device bitcode for user programs: one file for every library name (it depends on texture.h only)
TEX_BC = os.path.join(HERE, "user_texture.bc")
TEX_SOURCES = ["user_texture.hip", "texture.h"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
         "-fno-fast-math", "-Wall", "-Wno-unused-function", "-x", "hip"]


TEX_FLAGS = ["--offload-arch=gfx950", "--cuda-device-only", "-fgpu-rdc", "-emit-llvm", "-c", "-O3", "-std=c++17", "-ffp-contract=off",
             "-fno-fast-math", "-Wall", "-x", "hip"]


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps + [os.path.abspath(__file__)])


def _lib_stale():
    return _stale(LIB, [os.path.join(CSRC, f) for f in SOURCES + HEADERS])


def _tex_stale():
    return _stale(TEX_BC, [os.path.join(CSRC, f) for f in TEX_SOURCES])


def needs_build():
    return _lib_stale() or _tex_stale()


def build_texture_bitcode(verbose=True):
    """written to a temporary name and renamed: a process compiling a user program meanwhile reads the old file or the new one"""
    tmp = "%s.%d.tmp" % (TEX_BC, os.getpid())
    cmd = [HIPCC] + TEX_FLAGS + [os.path.join(CSRC, "user_texture.hip"), "-o", tmp]
    if verbose:
        print(" ".join(cmd), flush=True)
    try:
        subprocess.check_call(cmd)
        os.replace(tmp, TEX_BC)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return TEX_BC


def build(force=False, verbose=True):
    if force or _tex_stale():
        build_texture_bitcode(verbose)
    if not force and not _lib_stale():
        return LIB
    # regenerate the SBT tables from samples/sbt.json -- or, for a library with another shader binding table
    # (RDX_SBT_JSON=<file> RDX_LIB_NAME=<name>.so), into a header next to that library, selected with -DRDX_SBT_HEADER
    gen = os.path.join(HERE, "..", "tools", "genSBT.py")
    sbt = []
    if os.environ.get("RDX_SBT_JSON"):
        hdr = LIB[:-3] + "_sbt.h"
        subprocess.check_call([sys.executable, gen, os.environ["RDX_SBT_JSON"], hdr], stdout=subprocess.DEVNULL)
        sbt = ['-DRDX_SBT_HEADER="%s"' % hdr]
    else:
        subprocess.check_call([sys.executable, gen], stdout=subprocess.DEVNULL)
    cmd = [HIPCC] + FLAGS + EXTRA + sbt + [os.path.join(CSRC, s) for s in SOURCES] + ["-o", LIB]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print("built", LIB)
