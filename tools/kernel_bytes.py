#!/usr/bin/env python
"""usage: tools/kernel_bytes.py A.o B.o — compare the gfx950 kernels of two builds of one translation unit by the sha1 of each kernel's .text bytes.

Prints the kernel counts and the symbols removed / added / surviving with different bytes.  A refactor of the host-side routing must show
"added 0, different 0".  Only byte ranges are hashed: nothing is disassembled.  Needs llvm-objcopy, clang-offload-bundler and llvm-readelf
(ROCM_LLVM_BIN, default /opt/rocm/llvm/bin).
"""
import hashlib
import os
import subprocess
import sys
import tempfile

BIN = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")


def kernels(obj):
    """{kernel symbol: sha1 of its bytes} of the gfx950 code object embedded in `obj`."""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "x.fat"), os.path.join(d, "x.co")
        subprocess.run([f"{BIN}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj], check=True)
        subprocess.run([f"{BIN}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        out = subprocess.run([f"{BIN}/llvm-readelf", "-sW", "-SW", co], check=True, capture_output=True, text=True).stdout
        data = open(co, "rb").read()
    text, syms, kd = None, {}, set()
    for line in out.splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) >= 6 and f[1] == ".text" and f[2] == "PROGBITS":
            text = (f[0], int(f[3], 16), int(f[4], 16))            # section index, address, file offset
        elif len(f) == 8 and f[3] == "FUNC" and f[6] != "UND" and int(f[2]) > 0:
            syms[f[7]] = (int(f[1], 16), int(f[2]), f[6])
        elif len(f) == 8 and f[3] == "OBJECT" and f[7].endswith(".kd"):
            kd.add(f[7][:-3])                                       # a kernel = a function with a kernel descriptor
    assert text, "no .text section in the gfx950 code object of " + obj
    return {n: data[a - text[1] + text[2]: a - text[1] + text[2] + sz] for n, (a, sz, ndx) in syms.items() if ndx == text[0] and n in kd}


def how(x, y):
    """what differs between two byte strings of one kernel: the 32-bit words, and whether all of them moved by one constant (the literal of a pc-relative address
    of a device variable moves by what was removed between the kernel and the variable; the instructions are the same)"""
    if len(x) != len(y):
        return f"{len(x)} against {len(y)} bytes"
    w = [i for i in range(0, len(x), 4) if x[i:i + 4] != y[i:i + 4]]
    deltas = {(int.from_bytes(x[i:i + 4], "little") - int.from_bytes(y[i:i + 4], "little")) & 0xffffffff for i in w}
    return f"{len(w)} of {len(x) // 4} words" + (f", every one shifted by {deltas.pop():#x}" if len(deltas) == 1 else "")


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    sha = lambda d: hashlib.sha1(d).hexdigest()
    removed, added = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(n for n in set(a) & set(b) if sha(a[n]) != sha(b[n]))
    print(f"{sys.argv[1]}: {len(a)} kernels; {sys.argv[2]}: {len(b)} kernels; removed {len(removed)}, added {len(added)}, surviving with different bytes {len(differ)}")
    for title, names in (("removed", removed), ("added", added)):
        for n in names:
            print(f"  {title}: {n}")
    for n in differ:
        print(f"  different: {n} ({how(a[n], b[n])})")
    return 1 if added or differ else 0


if __name__ == "__main__":
    sys.exit(main())
