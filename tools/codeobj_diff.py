"""Compare the gfx950 code objects of two builds of a library, symbol by symbol (no GPU).

  python tools/codeobj_diff.py parent/libbls381.so consensus-specs_amd/lib/libbls381.so

For a change that must leave the device code as it was.  The code objects themselves are never
byte-identical: hipcc names a symbol after the compilation unit's id (__hip_cuid_<hash>), which
follows the source's path and text -- build_native.py compiles a snapshot under a temporary
directory, so even two builds of one tree differ, and so does a tree with one comment edited -- and
the symbol tables and the order of the constants in .rodata move with it.  So the comparison is
per symbol: every function's instruction sequence with addresses, branch and call
targets and pc-relative literals stripped, and every kernel's metadata (registers, spills, private
segment, LDS, kernarg size).  Prints the sha256 of both code objects, the symbols only one side
has, the symbols whose instructions differ and the kernels whose metadata differs; exit status 1
if anything but the hashes differs.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from extract_co import OBJDUMP, extract  # noqa: E402

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def functions(co):
    """{symbol: [instruction, ...]} with everything that moves with the layout stripped."""
    dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        s = re.sub(r"\s*//.*$", "", line.strip())   # the address comment
        if cur is None or not s:
            continue
        s = re.sub(r"<[^>]*>", "<>", s)
        if re.match(r"^s_(cbranch|branch|call)", s):
            s = s.split()[0]
        # the literal of the address arithmetic after s_getpc_b64 (a constant's or a callee's offset)
        if re.match(r"^s_addc?_u32 ", s) and any(p.startswith("s_getpc_b64") for p in cur[-2:]):
            s = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "<pcrel>", s)
        cur.append(s)
    for insts in out.values():   # alignment padding after the last instruction
        while insts and insts[-1].startswith("s_nop"):
            insts.pop()
    return out


def kernels(co):
    """{kernel symbol: {field: value}} from the AMDGPU metadata note, without the argument lists."""
    txt = subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout
    res, cur, base, on = [], None, None, False
    for line in txt.splitlines():
        if "amdhsa.kernels:" in line:
            on = True
            continue
        if not on:
            continue
        if re.match(r"^\s*amdhsa\.", line):
            break
        m = re.match(r"^(\s*)- ", line)
        if m and (base is None or len(m.group(1)) == base):
            base = len(m.group(1))
            cur = {}
            res.append(cur)
        m = re.match(r"^[\s-]*\.(\w+):\s*(.*)$", line)
        if m and cur is not None and len(line) - len(line.lstrip(" -")) == base + 2 and m.group(1) != "args":
            cur[m.group(1)] = m.group(2).strip()
    return {k["symbol"]: k for k in res if "symbol" in k}


def main(lib_a, lib_b):
    with tempfile.TemporaryDirectory() as d:
        cos = []
        for name, lib in (("a", lib_a), ("b", lib_b)):
            co = os.path.join(d, name + ".co")
            extract(lib, co)
            print("sha256 %s  %s (%d bytes)" % (hashlib.sha256(open(co, "rb").read()).hexdigest(), lib,
                                                os.path.getsize(co)))
            cos.append(co)
        fa, fb = functions(cos[0]), functions(cos[1])
        ka, kb = kernels(cos[0]), kernels(cos[1])
    only_a, only_b = sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa))
    moved = [s for s in sorted(set(fa) & set(fb)) if fa[s] != fb[s]]
    meta = [k for k in sorted(set(ka) | set(kb)) if ka.get(k) != kb.get(k)]
    print("symbols: %d / %d, kernels: %d / %d" % (len(fa), len(fb), len(ka), len(kb)))
    for title, names in (("only in the first", only_a), ("only in the second", only_b),
                         ("instructions differ", moved), ("kernel metadata differs", meta)):
        print("%s: %d" % (title, len(names)))
        for s in names:
            print("  " + s)
    return 1 if only_a or only_b or moved or meta else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
