"""The float64 reference of the filtered sampler (tests/sampling_filters_ref.py) checked against itself and the oracle, and the
margins of the shared cases: every threshold lies at least 4x the kernel's derived error bound away from every token, and every
winner beats its runner-up by far more than fp32 can move p / q - so the GPU test may ask for the reference's kept set and winner
exactly."""
import math

import numpy as np
import pytest
import torch

import sampling_filters_ref as R
from oracle import csm_oracle as O


@pytest.mark.parametrize("V", R.VS)
def test_filters_off_is_the_oracle(V):
    sets, q = R.inputs(V)
    for name, x in sets.items():
        for r in range(R.ROWS):
            ref = R.reference(x[r], R.TOPK[r], R.TEMP[r], 1.0, 0.0, q[r])
            assert ref["winner"] == int(O.sample_topk(x[r], R.TOPK[r], R.TEMP[r], q[r])), (name, r)
            assert (ref["N"] == ref["K"]).all() and math.isinf(ref["topp_margin"]) and math.isinf(ref["minp_margin"])


def _sorted_formulation(v, topk, top_p, min_p):
    """Tie-free inputs only: sort, cumulative sum - the textbook nucleus that keeps the token crossing top_p."""
    order = np.argsort(-v)[:topk]
    e = np.exp(v[order] - v[order[0]])
    order, e = order[e >= min_p], e[e >= min_p]
    before = (np.cumsum(e) - e) / e.sum()
    keep = np.zeros(v.shape[0], bool)
    keep[order[before < top_p]] = True
    return keep


def test_agrees_with_sort_and_cumsum_on_tie_free_inputs():
    sets, q = R.inputs(2051)
    x = sets["drawn"]
    for r in range(R.ROWS):
        v = R.scaled(x[r], R.TEMP[r])
        assert len(np.unique(v)) == v.shape[0]
        for topk, top_p, min_p in ((2051, 0.9, 0.0), (2051, 1.0, 0.02), (50, 0.5, 0.0), (200, 0.95, 0.001), (2051, 0.3, 0.1)):
            ref = R.reference(x[r], topk, R.TEMP[r], top_p, min_p, q[r])
            want = _sorted_formulation(v, topk, float(np.float32(top_p)), float(np.float32(min_p)))
            assert (ref["N"] == want).all(), (r, topk, top_p, min_p)


@pytest.mark.parametrize("name", R.SETS)
def test_kept_sets_are_nested(name):
    sets, q = R.inputs(2051)
    x = sets[name]
    for r in (0, 3, 9):
        last = None
        for top_p in (1.0, 0.99, 0.9, 0.5, 0.1, 1e-3, 1e-6):
            N = R.reference(x[r], 2051, R.TEMP[r], top_p, 0.0, q[r])["N"]
            assert last is None or not (N & ~last).any()
            last = N
        last = None
        for min_p in (0.0, 1e-6, 1e-3, 0.05, 0.5, 1.0):
            N = R.reference(x[r], 2051, R.TEMP[r], 1.0, min_p, q[r])["N"]
            assert last is None or not (N & ~last).any()
            last = N


@pytest.mark.parametrize("name", R.SETS)
def test_extreme_thresholds_keep_the_top_group(name):
    sets, q = R.inputs(2051)
    x = sets[name]
    for r in range(R.ROWS):
        top1 = R.reference(x[r], 1, R.TEMP[r], 1.0, 0.0, q[r])
        for topk in (50, 2051):
            assert (R.reference(x[r], topk, R.TEMP[r], 1.0, 1.0, q[r])["N"] == top1["N"]).all()
            assert (R.reference(x[r], topk, R.TEMP[r], 1e-6, 0.0, q[r])["N"] == top1["N"]).all()
            assert R.reference(x[r], topk, R.TEMP[r], 1e-6, 1.0, q[r])["winner"] == top1["winner"]


@pytest.mark.parametrize("V", R.VS)
def test_case_margins_clear_the_derived_bounds(V):
    worst = {}
    for (name, kind), c in R.cases(V).items():
        for r, ref in enumerate(c["ref"]):
            where = (V, name, kind, r)
            assert 0.0 < c["top_p"][r] <= 1.0 and 0.0 <= c["min_p"][r] <= 1.0, where
            assert ref["topp_margin"] >= R.HEADROOM * ref["topp_bound"], (where, ref["topp_margin"], ref["topp_bound"])
            assert ref["minp_margin"] >= R.HEADROOM * ref["minp_bound"], (where, ref["minp_margin"], ref["minp_bound"])
            # fp32 moves p / q by well under 1e-4 relative (two expf and a logf of arguments below 2^7, two divisions)
            assert ref["runner_up"] >= 1.001, (where, ref["runner_up"])
            # the boundary probes of the GPU test are decisive: with q = 1e-30 the last kept token beats every other p / q
            last = ref["last_kept"][0]
            others = np.delete(ref["p"] / c["q"][r].double().numpy(), last).max()
            assert ref["p"][last] / 1e-30 >= 1e3 * others and ref["p"][last] >= 1e-30, where
            w = worst.setdefault(name, [math.inf, math.inf, math.inf])
            w[0], w[1], w[2] = min(w[0], ref["topp_margin"]), min(w[1], ref["minp_margin"]), min(w[2], ref["runner_up"])
        if kind != "min_p":                      # the filter did something, and both finishes are met
            kept = [int(ref["N"].sum()) for ref in c["ref"]]
            assert any(k_ < int(ref["K"].sum()) for k_, ref in zip(kept, c["ref"]))
            if name == "drawn":
                assert min(kept) <= 64 < max(kept)
    print(V, {k_: ["%.2e" % a for a in v_] for k_, v_ in worst.items()})
