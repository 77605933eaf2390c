"""Scan the gfx950 code objects inside a built HIP shared library for
packed-FP32 VALU instructions (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 /
v_pk_mov_b32), which the library must not contain (DESIGN.md section 8:
their lanes 48-63 came out wrong beside another workgroup's LDS-DMA on the
same CU).  The .hip_fatbin section holds one offload bundle per object;
each is unbundled with clang-offload-bundler and disassembled with
llvm-objdump.
    python tools/pk_scan.py [lib.so]   -> prints {kernel: count}"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
PK = re.compile(r"\bv_pk_(fma|mul|add)_f32\b")


def tools_available():
    return all(os.path.exists(os.path.join(LLVM, t)) for t in ("clang-offload-bundler", "llvm-objdump")) \
        and subprocess.run(["which", "objcopy"], capture_output=True).returncode == 0


def scan(lib):
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fatbin")
        # with an output file of its own: without one objcopy rewrites `lib` in
        # place, and a process that has the library loaded (mapped) dies of a
        # bus error the next time it touches one of its pages
        subprocess.run(["objcopy", "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(d, "copy.so")],
                       check=True, capture_output=True)
        data = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
        found = {}
        n_objs = 0
        for i, s in enumerate(starts):
            e = starts[i + 1] if i + 1 < len(starts) else len(data)
            b = os.path.join(d, "b%d" % i)
            open(b, "wb").write(data[s:e])
            co = os.path.join(d, "c%d.co" % i)
            r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                                "--input=" + b, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                "--output=" + co], capture_output=True, text=True)
            if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            n_objs += 1
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], capture_output=True,
                                 text=True, check=True).stdout
            fn = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
                if m:
                    fn = m.group(1)
                elif PK.search(line):
                    found[fn] = found.get(fn, 0) + 1
        return n_objs, found


if __name__ == "__main__":
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "smer_music_generation_amd", "libsmer_hip.so")
    n, f = scan(lib)
    print("%d gfx950 code objects, %d kernels with packed-FP32 instructions" % (n, len(f)))
    for k, v in sorted(f.items(), key=lambda x: -x[1])[:20]:
        print("  %6d  %s" % (v, k))
