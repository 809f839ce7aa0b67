"""The inputs of tests/test_gpu_cutoff.py are in the regime that file is about - asserted on the CPU with the oracle alone, so that a seed
or shape changed later cannot quietly turn those tests back into aligned, constant-dimension ones: this test fails first.

Conditions of every case that is not deliberately degenerate (kept dimension = what the oracle keeps at a bond update):
    distinct                      at least 5 distinct kept dimensions
    quarter_unaligned             at least a quarter of the bonds keep a dimension that is no multiple of 4
    below_cap_in_each_half_sweep  every half-sweep has a bond strictly below both chi_max and the full rank (the cutoff decided)
    shrinks                       a bond of a later sweep keeps fewer states than that bond held at the end of the sweep before
A case lists in ``unmet`` the conditions its shape cannot meet (reasons next to the case); those are asserted NOT to hold, so the list
cannot go stale.  Float64 / complex128: the smallest decision margin (tests/helpers.py truncation_margin) is at least 1e-5 - eight decades
above the Gram route's error -, which is why the GPU test allows no flip there.  float32 / complex64: the bonds the flip excuse could
cover are at most a quarter.  The collapse case: the second sweep takes every bond down to 1, the third runs on the all-ones chain."""
import numpy as np
import pytest

from tests.helpers import truncation_margin
from tests.test_gpu_cutoff import ALL_CASES, excusable, oracle_run

CONDITIONS = ("distinct", "quarter_unaligned", "below_cap_in_each_half_sweep", "shrinks")


def test_truncation_margin_follows_the_rule_it_measures():
    S = np.sqrt(np.array([0.9, 0.09, 0.009, 0.0009, 0.0001]))          # discarded weights 1e-4, 1e-3, 1e-2, 1e-1 from the tail
    m, n = truncation_margin(S, 32, 5e-4)                               # keeps 4: D(4) = 1e-4 <= 5e-4 < D(3) = 1e-3
    assert n == 4 and abs(m - min(4e-4, 5e-4) / 5e-4) < 1e-9
    m, n = truncation_margin(S, 3, 5e-4)                                # the cap stopped the rule: only D(2) > cutoff was decided
    assert n == 3 and abs(m - (1e-2 - 5e-4) / 5e-4) < 1e-9
    m, n = truncation_margin(S, 32, 0.5)                                # mindim: only D(1) <= cutoff was decided
    assert n == 1 and abs(m - (0.5 - 0.1) / 0.5) < 1e-9
    assert truncation_margin(S[:1], 32, 1e-3) == (np.inf, 1)


@pytest.mark.parametrize("case", ALL_CASES, ids=[c.id for c in ALL_CASES])
def test_case_is_in_the_cutoff_limited_regime(case):
    ds, recs, W_end = oracle_run(case)
    nb = case.T - 1
    dims = [r["tr"]["chi"] for r in recs]
    profiles = [[t.shape[2] for t in recs[s * 2 * nb]["W"][:-1]] for s in range(1, case.sweeps)] + [[t.shape[2] for t in W_end[:-1]]]
    margin = min(r["margin"] for r in recs)
    could_excuse = sum(1 for r in recs if excusable(r, case.cutoff))
    unaligned = sum(1 for n in dims if n % 4)
    below = [sum(1 for r in recs[h * nb:(h + 1) * nb] if r["tr"]["chi"] < min(case.chi, r["full_rank"])) for h in range(2 * case.sweeps)]
    shrinks = sum(1 for r in recs[2 * nb:] if r["tr"]["chi"] < profiles[r["sweep"] - 1][r["lid"]])
    print(f"{case.id}: {len(set(dims))} distinct kept dimensions, {unaligned} of {len(dims)} no multiple of 4, cutoff-decided bonds per half-sweep {below}, "
          f"{shrinks} shrinking, smallest margin {margin:.2e}, excusable {could_excuse}, profiles after each sweep {profiles}")
    if case.collapse:
        assert profiles[1] == [1] * nb and profiles[-1] == [1] * nb, profiles
        assert all(r["tr"]["chi"] == 1 for r in recs[4 * nb:])                  # the third sweep runs on the all-ones chain
        assert min(profiles[0]) >= 2 and max(profiles[0]) >= 4                  # the second sweep takes the chain from these down to 1
    else:
        holds = dict(distinct=len(set(dims)) >= 5, quarter_unaligned=4 * unaligned >= len(dims), below_cap_in_each_half_sweep=min(below) >= 1,
                     shrinks=shrinks >= 1)
        assert case.unmet <= set(CONDITIONS)
        for k in CONDITIONS:
            assert holds[k] == (k not in case.unmet), (case.id, k, holds)
    if case.dtype in ("float64", "complex128"):
        assert margin >= 1e-5, margin
    else:
        assert 4 * could_excuse <= len(recs), could_excuse
