"""The 64-bit mixer and the seed derivations of csrc/dev_rng.h, in pure Python: what the device computes, for callers that name a
tree's or a rollout's stand-alone twin."""
MASK64 = 0xFFFFFFFFFFFFFFFF
ROLL_SALT = 0x9E3779B97F4A7C15      # kRollSalt, csrc/dev_rng.h


def mix64(x):                       # mix64, csrc/dev_rng.h
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def rollout_seed(rollout_seed_i, j):
    """The seed of the j-th rollout (j from 0) of a tree whose rollout seed is `rollout_seed_i`: playout_eval(leaf,
    seed=MCTSBatch.rollout_seed(rs, j)) is that rollout.  Pure Python, no device."""
    j = int(j)
    if j < 0:
        raise RuntimeError(f"rollout_seed: j counts from 0, got {j}")
    return mix64(((int(rollout_seed_i) & MASK64) + ROLL_SALT * (j + 1)) & MASK64)
