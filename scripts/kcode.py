"""Device code of a built object, per kernel: python scripts/kcode.py [--by-name] OBJ [OBJ2]

One object: for every kernel its size, the sha256 of its bytes in .text and the resources from the
code object's metadata (VGPRs, AGPRs, SGPRs, scratch and LDS bytes), then the unit's .text and
.rodata hashes.  Two objects (parent, child): the kernels whose bytes differ, with both resource
lines, and whether the unit's sections are the same.  --by-name pairs the kernels of two objects by
name and template arguments without the parameter list (a change of a kernel's parameters changes
its mangled name) and prints both resource lines of every kernel.  The code object is taken out of the host
object with llvm-objcopy --dump-section .hip_fatbin and clang-offload-bundler --unbundle
(profiles/engine_plan_refactor.md).
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
ARCH = os.environ.get("SDR_OFFLOAD_ARCH", "gfx950")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    with open(obj, "rb") as f:
        head = f.read(24)
    if head[:4] == b"\x7fELF" and head[18:20] == b"\xe0\x00":  # EM_AMDGPU: a code object itself
        return obj
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    if head == b"__CLANG_OFFLOAD_BUNDLE__":  # hipcc --cuda-device-only -c
        fat = obj
    else:
        run(f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj)
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets=hipv4-amdgcn-amd-amdhsa--{ARCH}",
        f"--input={fat}", f"--output={co}")
    return co


def unit(obj):
    """{'.text': sha, '.rodata': sha, 'kernels': {name: (size, sha, resources)}}"""
    with tempfile.TemporaryDirectory() as tmp:
        try:
            co = code_object(obj, tmp)
        except subprocess.CalledProcessError:
            return {"size": 0, "kernels": {}}  # a unit without device code
        data = open(co, "rb").read()
        secs = {}  # name -> (index, address, file offset, size)
        for m in re.finditer(r"\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)",
                             run(f"{LLVM}/llvm-readelf", "-S", "--wide", co)):
            secs[m.group(2)] = (int(m.group(1)), int(m.group(3), 16), int(m.group(4), 16), int(m.group(5), 16))
        out = {"size": len(data), "kernels": {}}
        for s in (".text", ".rodata"):
            if s in secs:
                _, _, off, size = secs[s]
                out[s] = hashlib.sha256(data[off:off + size]).hexdigest()[:16]
        meta = {}
        notes = run(f"{LLVM}/llvm-readelf", "--notes", co)
        for blk in re.split(r"\n\s+- \.", notes[notes.find("amdhsa.kernels"):])[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            g = lambda k: (re.search(r"\." + k + r":\s+(\d+)", blk) or [None, "?"])[1]
            if name:
                meta[name.group(1)] = (f"vgpr={g('vgpr_count')} agpr={g('agpr_count')} sgpr={g('sgpr_count')} "
                                       f"scratch={g('private_segment_fixed_size')} lds={g('group_segment_fixed_size')} "
                                       f"spills={g('vgpr_spill_count')}v/{g('sgpr_spill_count')}s")
        ti, taddr, toff, _ = secs[".text"]
        for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+(\d+)\s+(\S+)$",
                             run(f"{LLVM}/llvm-readelf", "-s", "--wide", co), re.M):
            addr, size, shndx, name = int(m.group(1), 16), int(m.group(2)), int(m.group(3)), m.group(4)
            if shndx == ti and name in meta:
                o = toff + addr - taddr
                out["kernels"][name] = (size, hashlib.sha256(data[o:o + size]).hexdigest()[:16], meta[name])
        return out


def demangle(names):
    filt = next((f for f in (f"{LLVM}/llvm-cxxfilt", shutil.which("c++filt")) if f and os.path.exists(f)), None)
    return dict(zip(names, run(filt, *names).splitlines() if filt and names else names))


def bare(demangled):
    """A demangled kernel name without its parameter list: `void ns::k<float, 1>(...)` -> `ns::k<float, 1>`."""
    depth, end = 0, len(demangled)
    for i in range(len(demangled) - 1, -1, -1):  # the parenthesis that matches the last one
        depth += {")": 1, "(": -1}.get(demangled[i], 0)
        if depth == 0 and demangled[i] == "(":
            end = i
            break
    return demangled[:end].split(" ", 1)[-1] if demangled.startswith("void ") else demangled[:end]


def by_name(a, b):
    dm = demangle(sorted(set(a["kernels"]) | set(b["kernels"])))
    ka = {bare(dm[n]): v for n, v in a["kernels"].items()}
    kb = {bare(dm[n]): v for n, v in b["kernels"].items()}
    same = 0
    for n in sorted(set(ka) | set(kb)):
        x, y = ka.get(n), kb.get(n)
        same += bool(x and y and x[:2] == y[:2])
        print(n + ("  (identical)" if x and y and x[:2] == y[:2] else ""))
        for tag, k in (("parent", x), ("child", y)):
            print(f"    {tag:6s} " + (f"{k[0]:7d} bytes {k[1]} {k[2]}" if k else "absent"))
    print(f"{same} of {len(set(ka) | set(kb))} kernels identical; code object {a['size']} -> {b['size']} bytes")


def main():
    if sys.argv[1] == "--by-name":
        return by_name(unit(sys.argv[2]), unit(sys.argv[3]))
    a = unit(sys.argv[1])
    if len(sys.argv) == 2:
        dm = demangle(list(a["kernels"]))
        for n, (size, sha, res) in sorted(a["kernels"].items()):
            print(f"{dm[n][:90]:90s} {size:7d} {sha} {res}")
        print(f"code object {a['size']} bytes  .text {a.get('.text')}  .rodata {a.get('.rodata')}")
        return
    b = unit(sys.argv[2])
    dm = demangle(sorted(set(a["kernels"]) | set(b["kernels"])))
    same = 0
    for n in sorted(set(a["kernels"]) | set(b["kernels"])):
        ka, kb = a["kernels"].get(n), b["kernels"].get(n)
        if ka and kb and ka[:2] == kb[:2]:
            same += 1
            continue
        print(dm[n])
        for tag, k in (("parent", ka), ("child", kb)):
            print(f"    {tag:6s} " + (f"{k[0]:7d} bytes {k[1]} {k[2]}" if k else "absent"))
    print(f"{same} kernels identical; code object {a['size']} -> {b['size']} bytes; "
          f".text {'same' if a.get('.text') == b.get('.text') else 'differs'} "
          f"({a.get('.text')} {b.get('.text')}); "
          f".rodata {'same' if a.get('.rodata') == b.get('.rodata') else 'differs'} "
          f"({a.get('.rodata')} {b.get('.rodata')})")


if __name__ == "__main__":
    main()
