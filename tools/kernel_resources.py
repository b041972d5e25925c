"""Code-object resources of every kernel in two builds of `_fks_hip`, side by side.

    python tools/kernel_resources.py OLD/_fks_hip.so NEW/_fks_hip.so

Reads each extension's `.hip_fatbin` section, unbundles the gfx950 code
objects and prints, per kernel symbol, the VGPRs, SGPRs, scratch bytes and
static LDS bytes of its `amdhsa.kernels` metadata (what the loader allocates),
and a SHA-1 of the kernel's machine code.  A kernel of both builds is marked
`same` or `DIFFERS`; kernels of one build only are listed after them.  Exit
status 1 when a shared kernel's resources differ (a changed code hash alone
is reported, not counted).
"""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("scratch", ".private_segment_fixed_size"),
          ("lds", ".group_segment_fixed_size"))


def code_objects(so, tmp):
    """The device ELF files bundled in an extension (one per translation unit)."""
    fat = os.path.join(tmp, "fatbin")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", so, os.devnull], check=True)
    data = open(fat, "rb").read()
    out, pos = [], data.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", data, pos + len(MAGIC))
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if triple.startswith("hip") and size:
                path = os.path.join(tmp, f"co{len(out)}.elf")
                with open(path, "wb") as f:
                    f.write(data[pos + off:pos + off + size])
                out.append(path)
        pos = data.find(MAGIC, pos + len(MAGIC))
    return out


def kernels(so):
    """{kernel symbol: {vgpr, sgpr, scratch, lds, code}}; a name that several
    units define (a kernel that is no template, compiled once per unit) gets
    its unit's position in the bundle appended."""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for ui, co in enumerate(code_objects(so, tmp)):
            unit = {}
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True,
                                   text=True).stdout
            cur = {}
            for line in notes.splitlines():
                # the keys of a kernel's own entry (its arguments' keys sit deeper)
                m = re.match(r"(?:  - |    )(\.[a-z_]+):\s+(\S+)", line)
                if not m:
                    continue
                if line.startswith("  - "):
                    cur = {}
                cur[m.group(1)] = m.group(2).strip("'")
                if m.group(1) == ".wavefront_size" and ".name" in cur:   # the last key of a kernel's entry
                    unit[cur[".name"]] = {k: int(cur.get(f, -1)) for k, f in FIELDS}
            syms = subprocess.run([f"{LLVM}/llvm-readelf", "-sW", co], check=True, capture_output=True, text=True).stdout
            secs = subprocess.run([f"{LLVM}/llvm-readelf", "-SW", co], check=True, capture_output=True, text=True).stdout
            m = re.search(r"\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", secs)
            addr, off = int(m.group(1), 16), int(m.group(2), 16)
            blob = open(co, "rb").read()
            for line in syms.splitlines():
                f = line.split()
                if len(f) >= 8 and f[3] == "FUNC" and f[7] in unit:
                    a, size = int(f[1], 16), int(f[2])
                    unit[f[7]]["code"] = hashlib.sha1(blob[off + a - addr:off + a - addr + size]).hexdigest()[:10]
            for k, v in unit.items():
                res[k if k not in res else f"{k} [unit {ui}]"] = v
    return res


def main(old_so, new_so):
    old, new = kernels(old_so), kernels(new_so)
    names = sorted(set(old) | set(new))
    try:
        demangle = subprocess.run(["c++filt"], input="\n".join(names), text=True, capture_output=True).stdout.splitlines()
    except OSError:
        demangle = []
    pretty = dict(zip(names, demangle if len(demangle) == len(names) else names))
    fmt = lambda r: f"vgpr {r['vgpr']:>3} sgpr {r['sgpr']:>3} scratch {r['scratch']:>5} lds {r['lds']:>5}"
    differ = 0
    print(f"# {len(old)} kernels in the old build, {len(new)} in the new one")
    print("# kernels of both builds: resources old | new | verdict (machine code)")
    for k in sorted(set(old) & set(new)):
        same = all(old[k][f] == new[k][f] for f, _ in FIELDS)
        differ += not same
        code = "code same" if old[k].get("code") == new[k].get("code") else "code differs"
        print(f"{fmt(old[k])} | {fmt(new[k])} | {'same' if same else 'DIFFERS'} ({code}) | {pretty[k]}")
    for title, only, tab in (("old", set(old) - set(new), old), ("new", set(new) - set(old), new)):
        print(f"# kernels of the {title} build only")
        for k in sorted(only):
            print(f"{fmt(tab[k])} | {pretty[k]}")
    print(f"# shared kernels whose resources differ: {differ}")
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
