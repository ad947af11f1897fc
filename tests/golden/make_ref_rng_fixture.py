"""Generates tests/golden/ref_rng_libstdcxx.npz: the real-reference RNG streams that
tests/test_oracle_pinned.py::test_rng_against_real_libstdcxx compares the oracle with, recorded once so that the test
needs nothing outside the repository.

The streams come from oracle/_ref/librngref.so (the reference's vendored pcg header + libstdc++, built by
`make -C oracle ref` where the reference tree is present).  Stored:
  sha.<name>          SHA-256 of each reference stream (the integer and uniform streams are bit-exact: the digest is the check)
  idx.<name>, val.<name>  gamma / Gumbel streams: the draws where the reference differs from the oracle, index and value; the
                      test patches them into the oracle's stream and checks the result against sha.<name>, so the stream it
                      compares with is the reference's, bit for bit
Run:  python tests/golden/make_ref_rng_fixture.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_api as orc  # noqa: E402

# the draws test_rng_against_real_libstdcxx makes (names shared with the test)
SHUFFLE_N = (1, 2, 3, 4, 5, 6, 7, 8, 33, 112, 113, 250, 1000)
GAMMA_ALPHA = (10.83 / 7, 10.83 / 2, 0.3, 0.77, 5.0)


def streams(which=None):
    """name -> array of one stream; exact = True for the streams the reference and the oracle must agree on bit for bit"""
    out = {"pcg32": (orc.pcg32_outputs(7, 100000, which=which), True),
           "uniform01": (orc.uniform01(5, 500000, which=which), True),
           "gumbel": (orc.gumbel(77, 100000, which=which), False)}
    for n in SHUFFLE_N:
        out[f"shuffle_{n}"] = (orc.shuffle_iota(99 + n, n, 100, which=which), True)
    for k, alpha in enumerate(GAMMA_ALPHA):
        for fresh in (False, True):
            out[f"gamma_{k}_{int(fresh)}"] = (orc.gamma(77, alpha, 100000, fresh, which=which), False)
    return out


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def main():
    ref = orc.ref_rng()
    if ref is None:
        sys.exit("oracle/_ref/librngref.so is not built: run `make -C oracle ref` with the reference tree present")
    mine = streams()
    fx = {}
    for name, (b, exact) in streams(ref).items():
        fx["sha." + name] = digest(b)
        if not exact:
            a = mine[name][0]
            idx = np.flatnonzero(a != b).astype(np.int64)
            fx["idx." + name], fx["val." + name] = idx, b[idx]
    np.savez_compressed(os.path.join(HERE, "ref_rng_libstdcxx.npz"), **fx)


if __name__ == "__main__":
    main()
