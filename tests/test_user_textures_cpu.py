"""CPU suite: texture reads in user shader programs (csrc/user_shader.cpp prelude + entry unit, csrc/user_texture.hip) up to the
point where a GPU is needed -- what the run-time compiler makes of programs that sample the bound texture array (code objects
without hardware image instructions), which programs it refuses, and its cache key.  No compute."""
import os
import re
import shutil

import pytest

import user_texture_ref as tr

REF_SHADER = "/root/reference/samples/shader.cl"
pytestmark = pytest.mark.skipif(not os.path.exists(tr.CLANG), reason="ROCm clang is not installed")


@pytest.fixture(scope="module")
def lib(built):
    return tr.jit_lib()


def test_probe_program_compiles_without_image_instructions(lib):
    """tests/golden/user_texture_probe.cl (read_imageui with a sampler and with int4 coordinates, get_image_width / height /
    array_size / dim) compiles as a megakernel whose code object holds no hardware image instruction: the reads go to the
    library's sampler, linked in as bitcode"""
    dis, notes = tr.assert_no_image_code(lib, tr.probe_program(), 0)
    assert "rdx_tex_read_sampled" in dis or "global_load" in dis
    # the entry point takes the two views after the 12 buffers: 14 pointers, then npixels (user_shader.cpp launch_user_shader)
    args = tr.kernel_args(notes, "rdx_user_entry")
    assert [a[:2] for a in args] == [(8 * k, 8) for k in range(14)] + [(112, 4)], args


_READ = "    imageScratch[i] = read_imageui(imageArray, sampler, coords[i]);\n"


@pytest.mark.parametrize("edit,name", [
    (lambda t: t + "\n__kernel void clear(write_only image2d_array_t img) { write_imageui(img, (int4)(0), (uint4)(1u)); }\n", "write_imageui"),
    (lambda t: t.replace(_READ, "    imageScratch[i] = as_uint4(read_imagef(imageArray, sampler, coords[i]));\n"), "read_imagef"),
    (lambda t: t.replace(_READ, "    imageScratch[i] = as_uint4(read_imagei(imageArray, sampler, coords[i]));\n"), "read_imagei"),
    (lambda t: t.replace(_READ, "    const sampler_t s = CLK_NORMALIZED_COORDS_TRUE | CLK_ADDRESS_REPEAT | CLK_FILTER_NEAREST;\n"
                                "    imageScratch[i] = read_imageui(imageArray, s, coords[i]);\n"), "inline sampler constant"),
])
def test_builtins_that_need_a_hardware_descriptor_are_refused(lib, edit, name):
    """write_image*, read_imagef / read_imagei and inline sampler constants compile to image instructions that read a hardware
    descriptor the program does not have (a GPU memory fault at run time): the run-time compiler refuses such a program and
    names the builtin"""
    text = edit(tr.probe_program())
    assert text != tr.probe_program()
    t = text.encode()
    assert lib.rdx_debug_jit_compiles(t, len(t), b"gfx950", 0) != 0
    err = lib.rdx_last_error().decode()
    assert name in err and "hardware image descriptor" in err, err[:2000]
    assert "compilation failed" not in err


def test_compiler_errors_keep_the_users_line_numbers(lib):
    """a program that does not compile still fails with the compiler's log, and its line numbers are the user's (the prelude
    is followed by #line 1)"""
    probe = tr.probe_program()
    text = probe.replace("const uint n = RTProp[1];", "const uint n = RTProp[1] this is not OpenCL C;")
    t = text.encode()
    assert lib.rdx_debug_jit_compiles(t, len(t), b"gfx950", 0) != 0
    err = lib.rdx_last_error().decode()
    line = 1 + [k for k, l in enumerate(probe.split("\n")) if "const uint n = RTProp[1];" in l][0]
    assert "compilation failed" in err and ("user.cl:%d:" % line) in err, err[:2000]


def test_textured_closest_hit_compiles_as_stage_kernel(lib):
    """tests/golden/user_texture_stages.cl: a closest-hit shader that samples the texture array compiles as the wavefront
    pipeline's shade stage, with no image instructions, and needs no more private (scratch) memory than the same program
    without the read"""
    _, with_read = tr.assert_no_image_code(lib, tr.stage_program(read=True), 1)
    _, without = tr.assert_no_image_code(lib, tr.stage_program(read=False), 1)
    r1, r0 = tr.kernel_resources(with_read, "rdx_stage_entry"), tr.kernel_resources(without, "rdx_stage_entry")
    assert r1[".private_segment_fixed_size"] <= r0[".private_segment_fixed_size"], (r1, r0)
    # the stage entry point takes the two views after its 31 pointers: 6 scalars, then 33 pointers (launch_user_stage)
    args = tr.kernel_args(with_read, "rdx_stage_entry")
    assert [a[:2] for a in args] == [(4 * k, 4) for k in range(6)] + [(24 + 8 * k, 8) for k in range(33)], args
    print("stage kernel with the read: %s, without: %s" % (r1, r0))


def test_cache_key_covers_abi_and_texture_bitcode(lib, tmp_path):
    """the run-time compiler's cache key changes with RDX_JIT_ABI and with the texture bitcode's bytes, so that a code object
    cached on disk by a library with another argument layout or sampler is never loaded"""
    t = tr.probe_program().encode()
    key = lambda abi=-1, bc=None, stages=0: lib.rdx_debug_jit_key(t, len(t), b"gfx950", stages, abi, bc)
    base = key()
    assert base != 0 and key() == base
    assert key(abi=base % 1000 + 1000) != base and key(abi=1000) != key(abi=1001)
    own = os.path.join(tr.ROOT, "radiance-ray-tracing_amd", "user_texture.bc")
    same = tmp_path / "same.bc"
    shutil.copyfile(own, same)
    assert key(bc=str(same).encode()) == base
    data = bytearray(open(own, "rb").read())
    data[len(data) // 2] ^= 0x40
    changed = tmp_path / "changed.bc"
    changed.write_bytes(bytes(data))
    assert key(bc=str(changed).encode()) != base
    assert key(stages=1) != base


@pytest.mark.skipif(not os.path.exists(REF_SHADER), reason="/root/reference is absent")
def test_reference_shader_with_its_texture_reads_uncommented(lib):
    """The reference's stock shader.cl with its four commented-out read_imageui calls made live compiles as a megakernel with
    no image instructions; a read placed inside `material` keeps the reduced stage hash (the program stays eligible for the
    wavefront pipeline).  (Reads the reference's file as data, here only.)"""
    stock = open(REF_SHADER).read()
    live = stock.replace("uint4 tex = 0.0f;//read_imageui(imageArray, sampler, coord);", "uint4 tex = read_imageui(imageArray, sampler, coord);")
    assert live.count("= read_imageui(imageArray, sampler, coord);") == 4
    tr.assert_no_image_code(lib, live, 0)
    want = lib.rdx_debug_stage_reduced_hash(None, 0)
    h = lambda s: lib.rdx_debug_stage_reduced_hash(s.encode(), len(s.encode()))
    assert h(stock) == want
    edited = stock.replace("color += albedo * 0.1f;", "color += albedo * 0.1f + (float)read_imageui(imageArray, sampler, (float4)(0.5f)).x;")
    assert edited != stock and h(edited) == want
    tr.assert_no_image_code(lib, edited, 1)
