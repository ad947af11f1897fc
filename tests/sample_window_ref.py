"""The numpy restatement of csrc/samples_window_kernels.h: mix64, the key formula of reservoir_keys, the stable
argsort selection of select_top and the Feistel permutation of window_gather.  Written from the formulas, array at a time."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
ROUNDS = 6


def mix64(x):
    """mix64 of csrc/dev_rng.h on a uint64 array (arithmetic mod 2^64)"""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=np.uint64) + GOLDEN
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def uniform_bits(seed, ids):
    """m_i = ((mix64(seed + GOLDEN * (id_i + 1)) >> 12) << 1) | 1: an odd integer below 2^53"""
    with np.errstate(over="ignore"):
        ids = np.asarray(ids).astype(np.uint64)
        x = mix64(np.uint64(seed) + GOLDEN * (ids + np.uint64(1)))
    return ((x >> np.uint64(12)) << np.uint64(1)) | np.uint64(1)


def reservoir_keys(iters, iteration, decay, seed, row_ids=None):
    """key_i = log(u_i) / decay ** max(0, iteration - iters[i]), u_i = m_i * 2^-53, in float64"""
    ids = np.arange(len(iters), dtype=np.uint64) if row_ids is None else row_ids
    u = uniform_bits(seed, ids).astype(np.float64) * 2.0 ** -53
    age = np.maximum(0.0, float(iteration) - np.asarray(iters, dtype=np.float64))
    with np.errstate(divide="ignore"):
        return np.log(u) / np.power(float(decay), age)


def select_top(keys, k):
    """the rows of the k largest keys, ascending; ties to the lower row (a stable sort of the negated keys; -0.0 == +0.0 there)"""
    keys = np.asarray(keys, dtype=np.float64)
    if np.isnan(keys).any():
        raise ValueError(f"NaN at row {int(np.flatnonzero(np.isnan(keys))[0])}")
    return np.sort(np.argsort(-keys, kind="stable")[:k]).astype(np.int64)


def perm_bits(total):
    bits = 2
    while (1 << bits) < total:
        bits += 1
    return bits


def round_keys(seed, pass_index):
    """key_r = mix64(k0 + GOLDEN * (r + 1)), k0 = mix64(seed + GOLDEN * (pass_index + 1))"""
    with np.errstate(over="ignore"):
        k0 = mix64(np.uint64(seed) + GOLDEN * np.uint64(pass_index + 1))
        return [mix64(k0 + GOLDEN * np.uint64(r + 1)) for r in range(ROUNDS)]


def _feistel(x, bits, keys):
    wl, wr = bits // 2, bits - bits // 2
    with np.errstate(over="ignore"):
        for r in range(ROUNDS):
            L, R = x >> np.uint64(wr), x & np.uint64((1 << wr) - 1)
            x = (R << np.uint64(wl)) | (L ^ (mix64(R + keys[r]) & np.uint64((1 << wl) - 1)))
            wl, wr = wr, wl
    return x


def permutation(total, seed, pass_index):
    """perm(0), ..., perm(total - 1): the Feistel network over perm_bits(total) bits, walked until the value is below total"""
    x = np.arange(total, dtype=np.uint64)
    if total == 0:
        return x.astype(np.int64)
    bits, keys = perm_bits(total), round_keys(seed, pass_index)
    x = _feistel(x, bits, keys)
    while True:
        out = x >= np.uint64(total)
        if not out.any():
            return x.astype(np.int64)
        x[out] = _feistel(x[out], bits, keys)
