"""The device code of one compiled translation unit, kernel by kernel (developer tool):
    python dev/kernel_bytes.py any4_amd/lib/obj/tg_gemv.o [--sections]
Extracts the gfx950 code object of the host object (llvm-objcopy --dump-section .hip_fatbin, clang-offload-bundler --unbundle
--targets=hipv4-amdgcn-amd-amdhsa--gfx950), reads its FUNC symbols (llvm-readelf -sW), cuts .text by symbol value and size and prints
`name size sha256` sorted by name: two builds of a unit hold the same kernels, whatever their order, when the two outputs are equal.
--sections: print the sha256 of the whole .text and .rodata instead (the per-unit hashes of profiles/*_checks.txt)."""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROCM_LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def tool(name):
    path = os.path.join(ROCM_LLVM, name)
    return path if os.path.exists(path) else (shutil.which(name) or name)


def code_object(obj, tmp):
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "gfx950.co")
    subprocess.check_call([tool("llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", obj, os.path.join(tmp, "unused.o")])
    subprocess.check_call([tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           f"--input={fat}", f"--output={co}"])
    return co


def section(co, name, tmp):
    out = os.path.join(tmp, name.strip(".") + ".bin")
    subprocess.check_call([tool("llvm-objcopy"), "-O", "binary", f"--only-section={name}", co, out])
    with open(out, "rb") as f:
        return f.read()


def main():
    args = [a for a in sys.argv[1:] if a != "--sections"]
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(args[0], tmp)
        text = section(co, ".text", tmp)
        if "--sections" in sys.argv:
            print(".text  ", hashlib.sha256(text).hexdigest())
            print(".rodata", hashlib.sha256(section(co, ".rodata", tmp)).hexdigest())
            return
        hdr = subprocess.run([tool("llvm-readelf"), "-SW", co], capture_output=True, text=True, check=True).stdout
        m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)", hdr)
        base = int(m.group(1), 16)
        syms = subprocess.run([tool("llvm-readelf"), "-sW", co], capture_output=True, text=True, check=True).stdout
        rows = set()  # (.symtab and .dynsym list the same kernels)
        for line in syms.splitlines():
            f = line.split()
            if len(f) >= 8 and f[3] == "FUNC" and f[6] != "UND":
                value, size = int(f[1], 16), int(f[2], 0)
                rows.add((f[7], size, hashlib.sha256(text[value - base:value - base + size]).hexdigest()))
        rows = sorted(rows)
        names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.splitlines()
        for name, (_, size, digest) in sorted(zip(names, rows)):
            print(re.sub(r"\(anonymous namespace\)::", "", name), size, digest)


if __name__ == "__main__":
    main()
