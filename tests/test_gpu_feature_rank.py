"""feature_rank on the device (azmi_samples_feature_rank, csrc/feature_rank_kernels.h) against numpy float64 through the SVD
(tests/feature_rank_ref.py): the exact cases the reference states, random features across every block edge of the kernels (the
64-column tile, the 32-row step, the row slabs of both passes), the two-pass centring under a large column offset, and bitwise
repeatability.

MARGIN is ten times the largest relative deviation from the numpy reference measured over the cases below on an MI355X
(DESIGN.md 8.5.3 has both figures); every test prints what it measures before it asserts.
"""
import numpy as np
import pytest
import torch

import feature_rank_ref as fr
from test_gpu_search_batch import az  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEASURED = 1.61e-15      # the largest relative deviation over RANDOM_CASES, any field: frob2 at (600, 512); the offset case: 5.87e-15
MARGIN = 10 * MEASURED

# (n, C): the issue's six, then the kernels' own sizes - 64-column tile, 32-row step and slab, 128-row slab of the column sums - each
# with its neighbours, then the widths and heights the entry point promises (C = 512, n = 65536)
RANDOM_CASES = [(2, 1), (5, 3), (17, 16), (64, 17), (300, 64), (1025, 130),
                (31, 63), (32, 64), (33, 65), (127, 5), (128, 127), (129, 129), (600, 512), (65536, 8)]


def _random(n, c, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, c)) * rng.uniform(0.2, 3.0, size=c) + rng.uniform(-1.0, 1.0, size=c)).astype(np.float32)


def _deviation(got, want):
    """the largest relative deviation over the five figures"""
    devs = {k: abs(got[k] - want[k]) / abs(want[k]) if want[k] else abs(got[k]) for k in ("trace", "frob2", "rank")}
    devs["mean"] = fr.rel(got["mean"], want["mean"])
    devs["gram"] = fr.rel(got["gram"], want["gram"])
    return devs


@pytest.mark.parametrize("n,c", RANDOM_CASES)
def test_random_features_match_numpy_float64(az, n, c):     # noqa: F811
    f = _random(n, c, 1000 * n + c)
    want = fr.feature_rank_ref(f)
    got = az.feature_rank(f, return_gram=True, return_mean=True)
    devs = _deviation(got, want)
    print(f"feature_rank ({n}, {c}): rank {got['rank']:.12g} (numpy {want['rank']:.12g}) deviations " + " ".join(f"{k} {v:.3g}" for k, v in devs.items()))
    assert got["n"] == n and got["channels"] == c and got["gram"].shape == (c, c) and got["mean"].shape == (c,)
    assert np.array_equal(got["gram"], got["gram"].T), "both triangles hold the same bits"
    assert 1.0 - MARGIN <= got["rank"] <= min(n - 1, c) * (1 + MARGIN) if n > 1 else got["rank"] == 1.0
    assert max(devs.values()) <= MARGIN, devs


def test_a_large_column_offset_stays_inside_the_margin(az):     # noqa: F811
    """unit-variance columns around 1e4: S2 - S1 S1^T / n would keep no digit of the variance in float32 and eight in float64;
    centring before the products keeps them all"""
    rng = np.random.default_rng(77)
    f = (rng.standard_normal((300, 64)) + 1.0e4).astype(np.float32)
    want = fr.feature_rank_ref(f)
    got = az.feature_rank(f, return_gram=True, return_mean=True)
    devs = _deviation(got, want)
    print("feature_rank offset 1e4 (300, 64): deviations " + " ".join(f"{k} {v:.3g}" for k, v in devs.items()))
    assert max(devs.values()) <= MARGIN, devs


def test_exact_cases(az):     # noqa: F811
    c = 24
    eye = np.concatenate([np.eye(c), -np.eye(c)]).astype(np.float32) * np.float32(3.0)
    got = az.feature_rank(eye, return_gram=True, return_mean=True)
    assert got["rank"] == float(c) and got["trace"] == 18.0 * c and got["frob2"] == 324.0 * c
    assert np.array_equal(got["gram"], 18.0 * np.eye(c)) and not got["mean"].any()
    row = _random(1, 37, 5)
    same = az.feature_rank(np.repeat(row, 4, axis=0), return_gram=True)
    assert same["rank"] == 1.0 and same["frob2"] == 0.0 and same["trace"] == 0.0 and not same["gram"].any()
    one = az.feature_rank(row)
    assert one["rank"] == 1.0 and one["frob2"] == 0.0 and one["n"] == 1
    empty = az.feature_rank(np.zeros((0, 37), np.float32), return_gram=True, return_mean=True)
    assert np.isnan(empty["rank"]) and empty["n"] == 0 and empty["channels"] == 37 and empty["gram"].shape == (37, 37)
    # rank one, exactly so in float32: small integers, u centred (201 rows: its mean is an integer)
    rng = np.random.default_rng(9)
    u = np.arange(201, dtype=np.float64) - 100.0
    outer = np.outer(u, rng.integers(-9, 10, size=70).astype(np.float64)).astype(np.float32)
    r1 = az.feature_rank(outer)["rank"]
    print(f"feature_rank rank-one (201, 70): rank - 1 = {r1 - 1.0:.3g}")
    assert abs(r1 - 1.0) <= MARGIN


def test_two_calls_return_the_same_bits_and_cuda_tensors_are_used_in_place(az):     # noqa: F811
    f = _random(1025, 130, 3)
    a = az.feature_rank(f, return_gram=True, return_mean=True)
    b = az.feature_rank(f, return_gram=True, return_mean=True)
    for k in ("rank", "trace", "frob2"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k
    assert a["gram"].tobytes() == b["gram"].tobytes() and a["mean"].tobytes() == b["mean"].tobytes()
    t = torch.from_numpy(f).to(DEV)
    d = az.feature_rank(t, return_gram=True, return_mean=True)
    assert d["gram"].is_cuda and d["gram"].dtype == torch.float64 and d["mean"].is_cuda
    assert np.float64(d["rank"]).tobytes() == np.float64(a["rank"]).tobytes()
    assert d["gram"].cpu().numpy().tobytes() == a["gram"].tobytes() and d["mean"].cpu().numpy().tobytes() == a["mean"].tobytes()
    plain = az.feature_rank(t)
    assert sorted(plain) == ["channels", "frob2", "n", "rank", "trace"] and np.float64(plain["rank"]).tobytes() == np.float64(a["rank"]).tobytes()


def test_the_library_refuses_what_it_cannot_take(az):     # noqa: F811
    with pytest.raises(RuntimeError, match=r"C must be in \[1, 2048\]"):
        az.feature_rank(np.zeros((4, 2049), np.float32))
    import ctypes as C
    from alphazero import _capi
    rec = _capi.FeatureRankRecordC()
    t = torch.zeros((4, 8), dtype=torch.float32, device=DEV)
    assert az.lib.azmi_samples_feature_rank(t.data_ptr(), 4, 0, None, None, C.byref(rec), 0, None) == -1
    assert "1 to 2048 channels" in az.lib.azmi_samples_last_error().decode()
    assert az.lib.azmi_samples_feature_rank(None, 4, 8, None, None, C.byref(rec), 0, None) == -1
    assert az.lib.azmi_samples_feature_rank(None, 0, 8, None, None, C.byref(rec), 0, None) == 0 and np.isnan(rec.rank) and rec.channels == 8
