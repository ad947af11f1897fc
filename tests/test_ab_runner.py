"""CPU tests of scripts/ab.py, the same-box A/B runner: run order, where AZMI_LIB goes, the statistics it prints and that the first
failing step ends it.  The command under measurement is a stub: a small `python -c` program that counts its starts in a file, logs
the AZMI_LIB it was given and prints the next value of its side (base = AZMI_LIB set, new = absent)."""
import importlib.util
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB = os.path.join(ROOT, "scripts", "ab.py")

STUB = r"""
import os, sys, time
d = os.environ["AB_DIR"]
starts = os.path.join(d, "starts")
n = (int(open(starts).read()) if os.path.exists(starts) else 0) + 1
open(starts, "w").write(str(n))
lib = os.environ.get("AZMI_LIB")
open(os.path.join(d, "log"), "a").write((lib or "-") + "\n")
if os.environ.get("AB_EXIT3_AT") == str(n): sys.exit(3)
if os.environ.get("AB_SLEEP_AT") == str(n): time.sleep(30)
values = os.environ["AB_BASE" if lib else "AB_NEW"].split()
print("rate 1.0 M/s (warm-up)")
print("rate %s M/s" % values[(n - 1) // 2])
"""
# by hand: base 100 104 102 -> median 102, spread (104 - 100) / 102 = 3.92 %; new 110 99 121 -> median 110, spread (121 - 99) / 110 = 20.00 %;
# 110 / 102 = 1.0784
BASE, NEW = "100 104 102", "110 99 121"


def _ab(tmp_path, *args, cmd=(sys.executable, "-c", STUB), pick=r"rate ([0-9.]+) M/s", limit="20", **env):
    base = tmp_path / "libazmi_base.so"
    base.write_bytes(b"")
    e = dict(os.environ, AB_DIR=str(tmp_path), AB_BASE=BASE, AB_NEW=NEW, **env)
    r = subprocess.run([sys.executable, AB, "--base", str(base), "--limit", limit, "--pick", pick, *args, "--", *cmd], capture_output=True, text=True, timeout=60, env=e)
    log = (tmp_path / "log").read_text().split() if (tmp_path / "log").exists() else []
    return r, log, str(base)


def _starts(tmp_path):
    return int((tmp_path / "starts").read_text()) if (tmp_path / "starts").exists() else 0


def test_order_library_and_statistics(tmp_path):
    out = tmp_path / "table.txt"
    r, log, base = _ab(tmp_path, "--pairs", "3", "--out", str(out), AZMI_LIB="/stale/libazmi.so")
    assert r.returncode == 0, r.stdout + r.stderr
    # base, new, base, new, base, new; AZMI_LIB reaches the base runs only, also when the caller's environment carries one
    assert log == [base, "-", base, "-", base, "-"]
    table = out.read_text()
    assert r.stdout.endswith(table)
    assert re.findall(r"^run (\d) (base|new) +(\S+)$", table, re.M) == [("1", "base", "100"), ("2", "new", "110"), ("3", "base", "104"), ("4", "new", "99"),
                                                                         ("5", "base", "102"), ("6", "new", "121")]
    side = {m[0]: tuple(map(float, m[1:])) for m in re.findall(r"^(base|new) +median (\S+) +min (\S+) +max (\S+) +spread (\S+) %", table, re.M)}
    assert side == {"base": (102.0, 100.0, 104.0, 3.92), "new": (110.0, 99.0, 121.0, 20.0)}
    assert re.search(r"^new / base of the medians: 1\.0784$", table, re.M)


def test_default_is_three_pairs_and_the_callers_environment_is_left_alone(tmp_path, monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location("ab_under_test", AB)
    ab = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ab)
    base = tmp_path / "libazmi_base.so"
    base.write_bytes(b"")
    for k, v in (("AB_DIR", str(tmp_path)), ("AB_BASE", BASE), ("AB_NEW", NEW)):
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("AZMI_LIB", raising=False)
    assert ab.main(["--base", str(base), "--limit", "20", "--pick", r"rate ([0-9.]+) M/s", "--", sys.executable, "-c", STUB]) == 0
    assert "AZMI_LIB" not in os.environ
    assert _starts(tmp_path) == 6 and "new / base of the medians: 1.0784" in capsys.readouterr().out


def test_first_failing_run_ends_the_tool_with_its_status(tmp_path):
    r, log, base = _ab(tmp_path, "--pairs", "3", AB_EXIT3_AT="2")
    assert r.returncode == 3, r.stdout + r.stderr
    assert _starts(tmp_path) == 2 and log == [base, "-"]                      # no third start
    assert "run 2 (new, pair 1) ended with status 3" in r.stdout
    assert re.search(r"^run 1 base +100$", r.stdout, re.M) and re.search(r"^base +median 100 ", r.stdout, re.M)      # the partial table
    assert "new / base" not in r.stdout


def test_time_limit_ends_the_tool_with_124(tmp_path):
    r, log, base = _ab(tmp_path, "--pairs", "2", limit="1", AB_SLEEP_AT="2")
    assert r.returncode == 124, r.stdout + r.stderr
    assert _starts(tmp_path) == 2
    assert "run 2 (new, pair 1) ended with status 124" in r.stdout


def _pytest_file(tmp_path, ok):
    f = tmp_path / "test_step.py"
    f.write_text("import os\ndef test_step():\n    open(os.path.join(os.environ['AB_DIR'], 'log'), 'a').write('tests:' + os.environ.get('AZMI_LIB', '-') + '\\n')\n"
                 "    assert %s\n" % ok)
    # rootdir and confcutdir: this pytest looks at nothing above its own file (a directory above it need not be listable)
    return "%s -q -p no:cacheprovider --rootdir=%s --confcutdir=%s" % (f, tmp_path, tmp_path)


def test_tests_run_first_on_the_new_build(tmp_path):
    r, log, base = _ab(tmp_path, "--pairs", "1", "--tests", _pytest_file(tmp_path, True), "--tests-limit", "60", AZMI_LIB="/stale/libazmi.so")
    assert r.returncode == 0, r.stdout + r.stderr
    assert log == ["tests:-", base, "-"]


def test_failing_tests_stop_before_any_run(tmp_path):
    r, log, base = _ab(tmp_path, "--pairs", "2", "--tests", _pytest_file(tmp_path, False), "--tests-limit", "60")
    assert r.returncode == 1, r.stdout + r.stderr
    assert log == ["tests:-"] and _starts(tmp_path) == 0
    assert "no run started" in r.stdout


def test_pick_that_matches_nothing_is_an_error_that_names_the_run(tmp_path):
    r, log, base = _ab(tmp_path, "--pairs", "2", pick=r"games/s ([0-9.]+)")
    assert r.returncode == 1, r.stdout + r.stderr
    assert _starts(tmp_path) == 1
    assert "run 1 (base, pair 1) printed no number that --pick matches" in r.stdout
    assert not re.search(r"median|^run 1 base", r.stdout, re.M)               # no value was made up for it
