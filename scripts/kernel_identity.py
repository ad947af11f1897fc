"""Is the device code of csrc/pipeline.hip the same in two builds (a host-side refactor must not move a kernel)?
    python scripts/kernel_identity.py <tree A> <tree B> > profiles/<name>.txt
Both trees are built with the same flags (__graft_entry__.build).  The gfx950 code object of each csrc/build/pipeline.o is disassembled
(llvm-objdump -d) and compared per symbol - mnemonics, operands and encodings; only the absolute address column is dropped - and the
rows of scripts/kernel_resources.py (registers, spills, scratch, LDS, threads of every kernel of libazmi.so) of both trees are diffed."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

import kernel_resources as kr

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

def disasm(obj):
    blob = open(obj, "rb").read()
    cos = list(kr.code_objects(blob))
    assert len(cos) == 1, len(cos)
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(cos[0]); f.flush()
        txt = subprocess.run([OBJDUMP, "-d", f.name], capture_output=True, text=True, check=True).stdout
    syms, cur = {}, None
    for line in txt.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1); syms[cur] = []
            continue
        if cur and line.strip():
            syms[cur].append(re.sub(r"//\s*[0-9A-Fa-f]+:", "//", line).strip())      # drop the absolute address, keep mnemonic + encoding
    return syms

def rows(tree):
    out = subprocess.run([sys.executable, os.path.join(tree, "scripts", "kernel_resources.py")], capture_output=True, text=True, check=True).stdout
    return out.split("\n")

a_tree, b_tree = sys.argv[1], sys.argv[2]
A = disasm(os.path.join(a_tree, "alphazero-pybind11_amd/csrc/build/pipeline.o"))
B = disasm(os.path.join(b_tree, "alphazero-pybind11_amd/csrc/build/pipeline.o"))
dem = lambda names: dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")))
d = dem(sorted(set(A) | set(B)))
print("device symbols of pipeline.o: A %d, B %d" % (len(A), len(B)))
for s in sorted(set(A) - set(B)): print("  only in A:", d[s])
for s in sorted(set(B) - set(A)): print("  only in B:", d[s])
diff = [s for s in sorted(set(A) & set(B)) if A[s] != B[s]]
for s in sorted(set(A) & set(B)):
    print("  %-9s %6d instructions  %s" % ("DIFFERS" if A[s] != B[s] else "identical", len(A[s]), d[s][:150]))
print("differing symbols:", [d[s] for s in diff] if diff else "none")
ra, rb = rows(a_tree), rows(b_tree)
dl = [l for l in difflib.unified_diff(ra, rb, "A", "B", lineterm="", n=0)]
print("kernel_resources.py rows: A %d lines, B %d lines; diff:" % (len(ra), len(rb)))
print("\n".join(dl) if dl else "  (none)")
