"""Same-box A/B of two builds of libazmi.so: the build in --base (a libazmi.so of the same ABI, handed to the package through AZMI_LIB)
against the current one, alternating base, new, base, new, ... for --pairs pairs; --tests first, on the current build.
    python scripts/ab.py --base OTHER/libazmi.so --limit 240 --pick 'block 3: ([0-9.]+)' [--pairs 3] [--tests "tests/test_gpu_pipeline.py -x -q"
        --tests-limit 600] [--out FILE] -- python scripts/pipe_bench.py
Every run is a fresh child `timeout -k 10 <limit> <command>`, one at a time; AZMI_LIB is set (base) or absent (new) in the child's
environment only.  --pick is a regular expression with one group: the number to take from a run's output (stdout and stderr), the last
match wins.  The first step that ends with a non-zero status (124 / 137 = the time limit, 134 = an abort, 139 = a segmentation fault)
ends the tool with that status: nothing more is started, nothing is tried again, the table so far is still printed.  Printed (and written
to --out): every run's value in run order, per side the median, min, max and spread = (max - min) / median, and new / base of the medians."""
import argparse
import os
import re
import shlex
import statistics
import subprocess
import sys


def child(cmd, limit, azmi_lib):
    env = dict(os.environ)
    env.pop("AZMI_LIB", None)
    if azmi_lib:
        env["AZMI_LIB"] = azmi_lib
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, errors="replace")
    return (p.returncode if p.returncode >= 0 else 128 - p.returncode), p.stdout       # a child killed by signal n counts as 128 + n, as in a shell


def table(header, runs):
    lines = [header] + ["run %d %-4s %s" % (i + 1, side, "%.6g" % v) for i, (side, v) in enumerate(runs)]
    med = {}
    for side in ("base", "new"):
        v = [x for s, x in runs if s == side]
        if v:
            med[side] = statistics.median(v)
            lines.append("%-4s median %.6g  min %.6g  max %.6g  spread %.2f %%  (%d runs)" % (side, med[side], min(v), max(v), 100 * (max(v) - min(v)) / med[side], len(v)))
    if len(med) == 2:
        lines.append("new / base of the medians: %.4f" % (med["new"] / med["base"]))
    return "\n".join(lines) + "\n"


def main(argv):
    if "--" not in argv:
        sys.exit("ab.py: the command to run goes after `--`")
    cut = argv.index("--")
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--base", required=True, help="the other libazmi.so (same ABI)")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--limit", type=int, required=True, help="seconds per run")
    ap.add_argument("--pick", required=True, help="regular expression with one group: the number of a run")
    ap.add_argument("--tests", help="pytest arguments: run once on the current build before the first pair")
    ap.add_argument("--tests-limit", type=int, help="seconds for --tests")
    ap.add_argument("--out", help="also write the table to this file")
    a = ap.parse_args(argv[:cut])
    cmd, pick = argv[cut + 1:], re.compile(a.pick)
    if not cmd or pick.groups != 1 or not os.path.isfile(a.base) or (a.tests and not a.tests_limit):
        ap.error("needs a command after `--`, one group in --pick, an existing --base and --tests-limit with --tests")
    if a.tests:
        rc, text = child([sys.executable, "-m", "pytest"] + shlex.split(a.tests), a.tests_limit, None)
        print("\n".join(text.splitlines()[-3:]), flush=True)
        if rc:
            print("ab.py: the tests ended with status %d: no run started" % rc)
            return rc
    header = "# scripts/ab.py: base = %s, %d pairs, %d s per run: %s" % (a.base, a.pairs, a.limit, " ".join(map(shlex.quote, cmd)))
    runs, rc = [], 0
    for n in range(2 * a.pairs):
        side = ("base", "new")[n % 2]
        rc, text = child(cmd, a.limit, os.path.abspath(a.base) if side == "base" else None)
        found = pick.findall(text)
        try:
            value = float(found[-1])
        except (IndexError, ValueError):
            value = None
        if rc or value is None:
            print("\n".join(text.splitlines()[-10:]))
            print("ab.py: run %d (%s, pair %d) %s" % (n + 1, side, n // 2 + 1, "ended with status %d" % rc if rc else "printed no number that --pick matches"))
            rc = rc or 1
            break
        runs.append((side, value))
        print("ab.py: run %d of %d (%s): %s" % (n + 1, 2 * a.pairs, side, found[-1]), file=sys.stderr, flush=True)      # progress; the table goes to stdout
    text = table(header, runs)
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
