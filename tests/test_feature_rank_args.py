"""CPU: feature_rank, effective_rank and selfplay.window_effective_rank: the entry points exist with the declared signatures, every
refusal is a RuntimeError raised by name before the library or the net is touched, empty calls need no device, and the float64
reference of tests/feature_rank_ref.py agrees with itself on the cases the reference states."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import feature_rank_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = {
    "azmi_net_trunk_channels": "azmi_net* net, uint32_t* cf",
    "azmi_net_trunk_features": "azmi_net* net, const float* dev_canonical, float* dev_features, uint32_t batch, void* stream",
    "azmi_samples_feature_rank": "const float* dev_features, uint32_t n, uint32_t C, double* dev_mean_out, double* dev_gram_out, "
                                 "azmi_feature_rank_record* host_record_out, int device, void* stream",
}


@pytest.fixture(scope="module")
def az():
    import __graft_entry__ as g
    g.build()
    import alphazero
    return alphazero


class _Net:
    """stands in for a HipLeafNet: touching it is a device call the argument checks must come before"""
    def __getattr__(self, name):
        raise AssertionError(f"net.{name} was read before the arguments were checked")


def test_the_entry_points_exist_with_the_declared_signatures(az):
    from alphazero import _capi, samples, selfplay
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "azmi.h")).read(), flags=re.S)
    raw = C.CDLL(_capi.LIB_PATH)
    for name, params in ENTRY_POINTS.items():
        assert hasattr(raw, name), f"{name} is not exported by libazmi.so"
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
        assert m and " ".join(m.group(1).split()) == params, name
        assert len(_capi.SYMBOLS[name][1]) == params.count(",") + 1, name
    assert C.sizeof(_capi.FeatureRankRecordC) == 32 and _capi.FeatureRankRecordC.rank.offset == 16 and _capi.FeatureRankRecordC.channels.offset == 28
    assert int(re.search(r"#define\s+AZMI_FEATURE_RANK_MAX_CHANNELS\s+(\d+)", header).group(1)) == _capi.FEATURE_RANK_MAX_CHANNELS
    assert az.feature_rank is samples.feature_rank and az.effective_rank is samples.effective_rank
    assert callable(selfplay.window_effective_rank)


@pytest.mark.parametrize("features,fragment", [
    (np.zeros((4, 3), np.float64), "features must be contiguous float32, got contiguous float64"),
    (np.zeros((4, 3), np.int32), "features must be contiguous float32, got contiguous int32"),
    (np.zeros(4, np.float32), r"features must be an \[n, C\] array, got shape \(4,\)"),
    (np.zeros((4, 3, 2), np.float32), r"features must be an \[n, C\] array"),
    (np.zeros((4, 6), np.float32)[:, ::2], "features must be contiguous float32, got non-contiguous float32"),
    (np.zeros((4, 0), np.float32), r"C must be in \[1, 2048\], got 0"),
    (np.zeros((1, 2049), np.float32), r"C must be in \[1, 2048\], got 2049"),
    ([[1.0, 2.0]], "features must be a numpy array or a CUDA tensor, got list"),
])
def test_feature_rank_refuses_by_name(az, features, fragment):
    with pytest.raises(RuntimeError, match="feature_rank: " + fragment):
        az.feature_rank(features)


def test_feature_rank_refuses_a_bad_device_and_a_cpu_tensor(az):
    import torch
    with pytest.raises(RuntimeError, match="feature_rank: device must be a device index"):
        az.feature_rank(np.zeros((4, 3), np.float32), device=-1)
    with pytest.raises(RuntimeError, match="feature_rank: features must be a CUDA tensor"):
        az.feature_rank(torch.zeros((4, 3)))


def test_empty_calls_need_no_device(az):
    out = az.feature_rank(np.zeros((0, 5), np.float32), return_gram=True, return_mean=True)
    assert np.isnan(out["rank"]) and out["n"] == 0 and out["channels"] == 5 and out["trace"] == 0.0 and out["frob2"] == 0.0
    assert out["gram"].shape == (5, 5) and out["mean"].shape == (5,) and np.isnan(out["gram"]).all()
    assert sorted(az.feature_rank(np.zeros((0, 5), np.float32))) == ["channels", "frob2", "n", "rank", "trace"]
    assert np.isnan(az.effective_rank(None, _Net()))


@pytest.mark.parametrize("canonical,kw,fragment", [
    (np.zeros((4, 2, 3, 3), np.float32), dict(batch_rows=0), "batch_rows must be an integer >= 1, got 0"),
    (np.zeros((4, 2, 3, 3), np.float32), dict(batch_rows=-5), "batch_rows must be an integer >= 1, got -5"),
    (np.zeros((4, 2, 3, 3), np.float32), dict(batch_rows=2.0), "batch_rows must be an integer >= 1, got 2.0"),
    (None, dict(batch_rows=0), "batch_rows must be an integer >= 1, got 0"),
    (np.zeros((4, 2, 3, 3), np.float64), {}, "canonical must be contiguous float32, got contiguous float64"),
    (np.zeros((4, 2, 9), np.float32), {}, r"canonical must be an \[n, C, H, W\] array, got shape \(4, 2, 9\)"),
    (np.zeros((4, 2, 3, 6), np.float32)[..., ::2], {}, "canonical must be contiguous float32, got non-contiguous float32"),
    ("boards", {}, "canonical must be a numpy array or a CUDA tensor, got str"),
])
def test_effective_rank_refuses_by_name_before_the_net_is_touched(az, canonical, kw, fragment):
    with pytest.raises(RuntimeError, match="effective_rank: " + fragment):
        az.effective_rank(canonical, _Net(), **kw)


def test_effective_rank_refuses_what_is_no_leaf_net(az):
    with pytest.raises(RuntimeError, match="effective_rank: net must be a HipLeafNet, got object"):
        az.effective_rank(np.zeros((4, 2, 3, 3), np.float32), object())


@pytest.mark.parametrize("rows", [0, -1, 1.5, True, (1 << 30) + 1])
def test_window_effective_rank_refuses_by_name(az, rows):
    from alphazero import selfplay
    window = az.SampleWindow(2, 0, 1.0, 0)
    with pytest.raises(RuntimeError, match=r"window_effective_rank: rows must be an integer in \[1, 2\^30\], got"):
        selfplay.window_effective_rank(window, _Net(), rows=rows)
    with pytest.raises(RuntimeError, match="window_effective_rank: window must be a SampleWindow, got list"):
        selfplay.window_effective_rank([], _Net())
    with pytest.raises(RuntimeError, match="window_effective_rank: seed must be an integer"):
        selfplay.window_effective_rank(window, _Net(), seed=-1)
    assert np.isnan(selfplay.window_effective_rank(window, _Net()))      # an empty window: the reference's nan, no device


def test_the_reference_states_its_own_edge_cases():
    c = 6
    eye = np.concatenate([np.eye(c), -np.eye(c)]) * 3.0
    assert abs(fr.feature_rank_ref(eye)["rank"] - c) < 1e-12
    assert fr.feature_rank_ref(np.ones((4, 3)))["rank"] == 1.0 and fr.feature_rank_ref(np.ones((1, 3)))["rank"] == 1.0
    assert np.isnan(fr.feature_rank_ref(np.zeros((0, 3)))["rank"])
    f = np.random.default_rng(1).standard_normal((40, 7))
    r = fr.feature_rank_ref(f)
    assert abs(np.trace(r["gram"]) - r["trace"]) <= 1e-12 * r["trace"] and abs((r["gram"] ** 2).sum() - r["frob2"]) <= 1e-12 * r["frob2"]
