"""Is the device code of libazmi.so the same in two builds (a host-side refactor must not change a kernel)?
    python scripts/kernel_identity.py <tree A> <tree B> > profiles/<name>.txt
Both trees are built with the same flags (__graft_entry__.build).  The gfx950 code object of every csrc/build/*.o is disassembled
(llvm-objdump -d) and the union of their symbols is compared by name, whichever object a symbol sits in - mnemonics, operands and
encodings; only the absolute address column is dropped.  A kernel that several translation units instantiate must be the same in all
of them; copies that are not get a line of their own.  The rows of scripts/kernel_resources.py (registers, spills, scratch, LDS, threads of every kernel of libazmi.so) of both
trees are diffed, a kernel counted once however many objects carry a copy.  Last, the exported azmi_* names of the two libraries are
compared and the objects that define k_assign are named."""
import difflib
import glob
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
    assert len(cos) <= 1, len(cos)
    syms, cur = {}, None
    if not cos:
        return syms                     # a translation unit without device code
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(cos[0]); f.flush()
        txt = subprocess.run([OBJDUMP, "-d", f.name], capture_output=True, text=True, check=True).stdout
    for line in txt.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1); syms[cur] = []
            continue
        if cur and line.strip() and line.strip() != "...":      # ("...": zero padding behind the last symbol of a section, no code)
            syms[cur].append(re.sub(r"//\s*[0-9A-Fa-f]+:", "//", line).strip())      # drop the absolute address, keep mnemonic + encoding
    return syms

def tree_symbols(tree):
    """symbol -> instructions over every object of the tree.  Keyed by mangled name: a template kernel that several translation units
    instantiate is one symbol, and so are two DIFFERENT anonymous-namespace kernels that share a name in two files - either way copies
    that differ are listed (`conflicts`) and the first copy stands in the comparison."""
    syms, conflicts = {}, []
    for obj in sorted(glob.glob(os.path.join(tree, "alphazero-pybind11_amd/csrc/build/*.o"))):
        for name, ins in disasm(obj).items():
            if syms.setdefault(name, ins) != ins:
                conflicts.append((os.path.basename(obj), name))
    return syms, conflicts

def rows(tree):
    out = subprocess.run([sys.executable, os.path.join(tree, "scripts", "kernel_resources.py")], capture_output=True, text=True, check=True).stdout
    lines = out.split("\n")
    # kernel_resources.py sorts by kernel name, so the copies of one kernel are neighbours; equal neighbours count once
    return [l for i, l in enumerate(lines) if i == 0 or l != lines[i - 1]]

a_tree, b_tree = sys.argv[1], sys.argv[2]
(A, ca), (B, cb) = tree_symbols(a_tree), tree_symbols(b_tree)
dem = lambda names: dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")))
d = dem(sorted(set(A) | set(B)))
print("device symbols of csrc/build/*.o: A %d, B %d" % (len(A), len(B)))
for t, c in (("A", ca), ("B", cb)):
    for obj, s in c: print("  %s: the copy in %s differs from another object's: %s" % (t, obj, d[s]))
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

# the C ABI of the two libraries, and the one kernel that is not a template: a second definition would be a link error waiting to happen
def abi(tree):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(tree, "alphazero-pybind11_amd/libazmi.so")], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("azmi_"))
aa, ab = abi(a_tree), abi(b_tree)
print("exported azmi_* names (nm -D --defined-only libazmi.so): A %d, B %d; %s" % (len(aa), len(ab), "the same list" if aa == ab else
      "DIFFERENT: only in A %s, only in B %s" % (sorted(set(aa) - set(ab)), sorted(set(ab) - set(aa)))))
for t, tree in (("A", a_tree), ("B", b_tree)):
    owners = []
    for obj in sorted(glob.glob(os.path.join(tree, "alphazero-pybind11_amd/csrc/build/*.o"))):
        out = subprocess.run(["nm", "-C", "--defined-only", obj], capture_output=True, text=True, check=True).stdout
        if any("__device_stub__k_assign(" in l for l in out.splitlines()): owners.append(os.path.basename(obj))
    print("k_assign is defined in: %s %s" % (t, owners))
