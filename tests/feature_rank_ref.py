"""Shared by the tests of feature_rank / trunk_features / effective_rank: the float64 references.

`feature_rank_ref` is the tail of the reference's NNWrapper.effective_rank (neural_net.py:867-873) in numpy float64: centre the
columns, take the singular values, (sum s^2)^2 / sum s^4 - so a comparison against it tests the Gram identity the kernel rests on,
not only its sums.  `trunk_features_ref` is the head of that function on the package's LeafNet in float64: a forward hook on
`conv_layers`, then the mean over the cells.
"""
import copy

import numpy as np
import torch


def feature_rank_ref(features):
    """-> {"rank", "trace", "frob2", "n", "channels", "mean" [C], "gram" [C, C]} of an [n, C] array, in float64 through the SVD"""
    f = np.asarray(features, dtype=np.float64)
    n, c = f.shape
    if n == 0:
        return {"rank": float("nan"), "trace": 0.0, "frob2": 0.0, "n": 0, "channels": c, "mean": np.full(c, np.nan), "gram": np.full((c, c), np.nan)}
    mean = f.mean(axis=0)
    fc = f - mean
    s2 = np.linalg.svd(fc, compute_uv=False) ** 2
    trace, frob2 = float(s2.sum()), float((s2 * s2).sum())
    return {"rank": 1.0 if frob2 == 0 else trace * trace / frob2, "trace": trace, "frob2": frob2, "n": n, "channels": c, "mean": mean,
            "gram": fc.T @ fc}


@torch.no_grad()
def trunk_features_ref(net, x):
    """float64 [n, CF]: the output of `net.conv_layers` on the CPU in float64, averaged over the cells"""
    ref = copy.deepcopy(net).cpu().double().eval()
    seen = []
    handle = ref.conv_layers.register_forward_hook(lambda m, i, o: seen.append(o.detach()))
    try:
        ref(x.detach().cpu().double())
    finally:
        handle.remove()
    return seen[0].mean(dim=(2, 3))


def rel(a, b):
    """the largest |a - b| over the largest |b| (0 for two all-zero arrays)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = float(np.abs(b).max()) if b.size else 0.0
    diff = float(np.abs(a - b).max()) if b.size else 0.0
    return diff / scale if scale else diff
