#!/usr/bin/env python3
"""kernel_text_diff.py OLD.co NEW.co -- are the kernels of two device code objects the same machine code?  (no GPU needed)

Both files are gfx950 code objects of csrc/kernels.hip (ELF, or the bundle hipcc -c writes), e.g. from
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -x hip --cuda-device-only -c kernels.hip -o X.co
For every function symbol of OLD the bytes of its .text range and its 64-byte kernel descriptor in .rodata (`<name>.kd`: register
counts, LDS, scratch; without the code's offset, which moves with the layout) are compared with NEW's symbol of the same name.  Prints one summary line per class and every symbol that
differs or is missing; symbols only NEW has are listed as added.  Exit status 1 if an OLD symbol differs or is missing."""
import struct
import subprocess
import sys


def symbols(path):
    data = open(path, "rb").read()
    if data[:24] == b"__CLANG_OFFLOAD_BUNDLE__":       # hipcc -c: an (uncompressed) bundle; take the device entry
        n, = struct.unpack_from("<Q", data, 24)
        at = 32
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", data, at)
            ident = data[at + 24:at + 24 + idlen].decode()
            at += 24 + idlen
            if ident.startswith("hip") and size:
                data = data[off:off + size]
                break
    assert data[:4] == b"\x7fELF" and data[4] == 2, "%s: not a 64-bit ELF file" % path
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for name, typ, flags, addr, off, size, link, info, align, entsize in sec:
        if typ != 2:            # SHT_SYMTAB
            continue
        stroff = sec[link][4]
        for k in range(size // 24):
            st_name, st_info, st_other, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", data, off + k * 24)
            if st_shndx == 0 or st_shndx >= shnum or st_size == 0 or (st_info & 15) not in (1, 2):      # objects (.kd) and functions
                continue
            end = data.index(b"\0", stroff + st_name)
            if data[stroff + st_name:end].startswith(b"__hip_cuid_"):      # the compilation unit's id, derived from the command line
                continue
            s = sec[st_shndx]
            start = s[4] + (st_value - s[3])
            out[data[stroff + st_name:end].decode()] = ((st_info & 15), data[start:start + st_size])
    return out


def strip(kind, blob):
    """a kernel descriptor without its bytes 16-23, the offset from the descriptor to the kernel's code: that one moves with the layout"""
    return blob if kind == 2 or len(blob) != 64 else blob[:16] + blob[24:]


def main():
    old, new = symbols(sys.argv[1]), symbols(sys.argv[2])
    names = sorted(old)
    dem = dict(zip(names + sorted(set(new) - set(old)),
                   subprocess.run(["c++filt"], input="\n".join(names + sorted(set(new) - set(old))), capture_output=True, text=True).stdout.split("\n")))
    bad = 0
    for kind, label in ((2, "functions (.text)"), (1, "objects (kernel descriptors)")):
        same = nbytes = 0
        for n in names:
            if old[n][0] != kind:
                continue
            if n not in new:
                print("MISSING  %s" % dem[n]); bad += 1
            elif strip(kind, new[n][1]) != strip(kind, old[n][1]):
                print("DIFFERS  %s (%d -> %d bytes)" % (dem[n], len(old[n][1]), len(new[n][1]))); bad += 1
            else:
                same += 1; nbytes += len(old[n][1])
        print("%s: %d of %d symbols of %s byte-identical in %s (%d bytes)"
              % (label, same, sum(1 for n in names if old[n][0] == kind), sys.argv[1], sys.argv[2], nbytes))
    added = sorted(n for n in new if n not in old and new[n][0] == 2)
    print("added functions: %d (%d bytes)" % (len(added), sum(len(new[n][1]) for n in added)))
    for n in added:
        print("  + %s (%d bytes)" % (dem[n][:150], len(new[n][1])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
