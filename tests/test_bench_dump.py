"""bench.py --dump-outputs without a GPU: the row sample that keeps a large output within its share of the 64 MB."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_an_array_within_budget_is_kept_whole():
    a = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
    assert bench.sample_rows(a, a.nbytes) is a


def test_a_large_array_keeps_a_fixed_sample_of_whole_rows():
    rng = np.random.default_rng(5)
    a = rng.standard_normal((32, 40, 2, 8, 16)).astype(np.float32)  # [layers, nq, 2, Hkv, D]
    budget = a.nbytes // 3 + 100
    s = bench.sample_rows(a, budget)
    rows = a.reshape(32 * 40, 2, 8, 16)
    assert s.shape == (budget // rows[0].nbytes, 2, 8, 16) and s.nbytes <= budget
    # every kept row is a whole row of the input, in order and without repeats
    idx = [int(np.flatnonzero((rows == r).all(axis=(1, 2, 3)))[0]) for r in s]
    assert idx == sorted(set(idx))
    # the same shape keeps the same rows, whatever the values
    s2 = bench.sample_rows(a + 1.0, budget)
    assert np.array_equal(s2, s + 1.0)


def test_two_halves_stay_within_the_cap():
    per_file = bench.DUMP_BYTES // 2 - bench.DUMP_HEADER_ALLOWANCE
    assert 2 * (per_file + bench.DUMP_HEADER_ALLOWANCE) <= 64_000_000
