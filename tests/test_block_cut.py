"""csrc/block_cut.h and every device-block layout written with it (search_batch_types.h, samples_layout.h), checked on the CPU:
tests/block_cut_check.cpp is compiled with g++ -fsanitize=address,undefined and run.  It asserts, for every layout, that the
sizing pass equals the cutting pass, that every array is aligned, in order, disjoint and inside the block (writing each array's
last byte), and that the sizes are the byte formulas the layouts replaced."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_cut_layouts(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    if not cxx:
        pytest.fail("no g++ to build tests/block_cut_check.cpp with")
    exe = str(tmp_path / "block_cut_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "block_cut_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "block_cut_check: ok" in run.stdout
    # the sizes at N = 3, M = 7, V = 3: computed by hand from the expressions of the code before the cutter
    assert "sweep cap 2: 752 bytes (clear 612), frontier per-tree 560, records cap 5: 195, sweep metrics 1134" in run.stdout
