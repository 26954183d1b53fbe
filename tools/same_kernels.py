#!/usr/bin/env python3
"""same_kernels.py A B -- do two object files or libraries hold the same gfx950 device code?  Dumps .hip_fatbin of each
(llvm-objcopy), unbundles the gfx950 code object of every bundle in it (clang-offload-bundler) and compares, by name, the bytes
of every FUNC symbol and of every kernel descriptor (*.kd; but for its offset to the code).  Prints the counts; exit status 1 on any difference.  No GPU."""
import collections
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
MAGICS = (b"__CLANG_OFFLOAD_BUNDLE__", b"CCOB")      # plain and compressed bundles


def code_objects(path, tmp):
    fat = os.path.join(tmp, "fatbin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, path, os.path.join(tmp, "copy")])
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(b"|".join(MAGICS), data)]
    for n, (a, b) in enumerate(zip(starts, starts[1:] + [len(data)])):
        part, out = os.path.join(tmp, "bundle%d" % n), os.path.join(tmp, "co%d" % n)
        open(part, "wb").write(data[a:b])
        bundler = [os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--input=" + part]
        targets = [t for t in subprocess.check_output(bundler + ["--list"], text=True).split() if t.endswith("gfx950")]
        for t in targets:
            subprocess.check_call(bundler + ["--unbundle", "--targets=" + t, "--output=" + out])
            yield open(out, "rb").read()


def symbols(elf):
    """name -> bytes of every FUNC symbol and every *.kd object of an ELF64 little-endian code object"""
    shoff, shentsize, shnum = struct.unpack_from("<Q", elf, 0x28)[0], *struct.unpack_from("<HH", elf, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    for s in sec:
        if s[1] != 2:                   # SHT_SYMTAB
            continue
        strtab = sec[s[6]]
        for off in range(s[4], s[4] + s[5], 24):
            name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, off)
            text = elf[strtab[4] + name:elf.index(b"\0", strtab[4] + name)].decode()
            if 0 < shndx < shnum and size and ((info & 15) == 2 or text.endswith(".kd")):
                at = sec[shndx][4] + value - sec[shndx][3]
                blob = elf[at:at + size]
                # a descriptor's kernel_code_entry_byte_offset (bytes 16-23) is the distance to its code: where the kernel sits
                # in .text, not what it is
                yield text, blob[:16] + blob[24:] if text.endswith(".kd") else blob


def table(path):
    out = collections.defaultdict(list)
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(path, tmp):
            for name, blob in symbols(co):
                out[name].append(blob)
    return {k: sorted(v) for k, v in out.items()}


def main():
    a, b = table(sys.argv[1]), table(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    kd = sum(1 for k in a if k.endswith(".kd"))
    print(f"A: {len(a) - kd} functions, {kd} kernel descriptors; B: {len(b) - sum(1 for k in b if k.endswith('.kd'))} functions, "
          f"{sum(1 for k in b if k.endswith('.kd'))} kernel descriptors")
    print(f"only in A: {len(only_a)}; only in B: {len(only_b)}; same name, different bytes: {len(differ)}; identical: {len(set(a) & set(b)) - len(differ)}")
    for k in only_a + only_b + differ:
        print(("A only  " if k in only_a else "B only  " if k in only_b else "differs ") + k)
    return 1 if only_a or only_b or differ else 0


if __name__ == "__main__":
    sys.exit(main())
