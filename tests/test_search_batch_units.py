"""CPU: the batched search keeps its device module and its host code apart.  search_batch.hip is the one unit that includes the
search_*_kernels.h and launches; it defines every sb_launch_* of search_batch_host.h and no entry point.  Every other
search_batch_*.hip is host code over that header.  File reading only: neither the GPU nor the library is touched."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "alphazero-pybind11_amd", "csrc")
MODULE = os.path.join(CSRC, "search_batch.hip")
HOST_UNITS = sorted(p for p in glob.glob(os.path.join(CSRC, "search_batch_*.hip")) if p != MODULE)


def _read(path):
    return open(path).read()


def test_host_units_launch_nothing_and_include_no_kernel_header():
    assert len(HOST_UNITS) >= 4, HOST_UNITS      # sweep, pool, frontier and at least one unit of the core
    for path in HOST_UNITS:
        text = _read(path)
        assert "<<<" not in text, f"{os.path.basename(path)} launches a kernel"
        kernel_headers = [h for h in re.findall(r'#\s*include\s*[<"]([^>"]+)[>"]', text) if h.endswith("_kernels.h")]
        assert not kernel_headers, f"{os.path.basename(path)} includes {kernel_headers}"


def test_device_module_has_no_entry_points():
    assert 'extern "C"' not in _read(MODULE)


def test_every_launch_function_is_defined_in_the_device_module_alone():
    declared = set(re.findall(r"^void\s+(sb_launch_\w+)\s*\(", _read(os.path.join(CSRC, "search_batch_host.h")), re.M))
    assert len(declared) >= 29, sorted(declared)      # the 27 before the split, sb_launch_seed and sb_launch_gather
    definition = r"^(?:static\s+|inline\s+)*void\s+(sb_launch_\w+)\s*\([^;{]*\)\s*\{"
    defined_in_module = set(re.findall(definition, _read(MODULE), re.M))
    assert declared <= defined_in_module, f"declared, not defined in search_batch.hip: {sorted(declared - defined_in_module)}"
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        if path == MODULE:
            continue
        elsewhere = set(re.findall(definition, _read(path), re.M)) & declared
        assert not elsewhere, f"{os.path.basename(path)} defines {sorted(elsewhere)}"
