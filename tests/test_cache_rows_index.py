"""csrc/cache_rows_index.h - the ordered compaction of the cache's miss list and the chunk / row_count cut of its row-list insert -
checked on the CPU: tests/cache_rows_index_check.cpp is compiled with g++ -fsanitize=address,undefined and run.  It runs the
arithmetic the way the kernels do at n = 0, 1, 63, 64, 65, 255, 257, 4001, 8192, 8193, 16385 and compares with a plain loop."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cache_rows_index_arithmetic(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    if not cxx:
        pytest.fail("no g++ to build tests/cache_rows_index_check.cpp with")
    exe = str(tmp_path / "cache_rows_index_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "cache_rows_index_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "cache_rows_index_check: ok (11 sizes)" in run.stdout
