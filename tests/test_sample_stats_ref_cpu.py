"""tests/sample_stats_ref.py proves itself: the reference against torch's float64 ``log_softmax``, a correct fp32 restatement
inside the bound on every case, three wrong restatements outside it."""
import math

import pytest
import torch

import sample_stats_ref as R


def test_reference_is_torch_float64_log_softmax():
    for c in R.CASES:
        m = c.made
        ls = torch.log_softmax(m["x"].double(), 1)
        p = ls.exp()
        lp, _ = m["ref"]["logprob"]
        ent, _ = m["ref"]["entropy"]
        pm, _ = m["ref"]["pmax"]
        codes = m["codes"].long()
        inside = (codes >= 0) & (codes < c.V)
        want = ls.gather(1, codes.clamp(0, c.V - 1).view(-1, 1)).view(-1)
        assert torch.allclose(lp[inside], want[inside], rtol=1e-12, atol=1e-12), c
        assert bool((lp[~inside] == -math.inf).all()), c
        h = -(torch.where(p > 0, p * ls, torch.zeros_like(p))).sum(1)
        assert torch.allclose(ent, h, rtol=1e-10, atol=1e-12), c
        assert torch.allclose(pm, p.max(1).values, rtol=1e-12, atol=0), c


def test_cases_cover_what_they_claim():
    assert {c.V for c in R.CASES} == {1, 2, 63, 64, 65, 2051, 2304, 2305, 4096} and {c.rows for c in R.CASES} == {1, 3, 512}
    assert R.CASE["V2051_ldl2112_rows512"].ldl == 2112 and any(c.ldl == c.V for c in R.CASES)
    big = R.CASE["V2051_ldl2112_rows512"].made
    assert {(k, ck) for k, ck in zip(big["kinds"], big["ckinds"])} == {(k, ck) for k in R.KINDS for ck in R.CODES}
    x, codes = big["x"], big["codes"]
    assert float(x.max()) > 88.0 and float(x.min()) < -88.0                # exp overflows / underflows without the max
    assert {int(v) for v in codes.unique()} >= {-1, 0, 2050, 2051}
    # every element outside the window is NaN: padding columns and guard rows
    buf = big["logits"].clone()
    R.logits_window(buf, R.CASE["V2051_ldl2112_rows512"]).fill_(0.0)
    assert int(torch.isnan(buf).sum()) == buf.numel() - 512 * 2051


def test_special_rows_have_their_values():
    m = R.CASE["V2051_ldl2112_rows512"].made
    for r, (k, ck) in enumerate(zip(m["kinds"], m["ckinds"])):
        lp, ent, pm = (m["ref"][n][0][r] for n in R.OUTPUTS)
        if k == "onehot":
            assert abs(float(ent)) < 1e-30 and abs(float(pm) - 1.0) < 1e-30
            if ck == "random":
                assert abs(float(lp)) < 1e-30
        if k == "const":
            assert abs(float(ent) - math.log(2051)) < 1e-12 and abs(float(pm) - 1 / 2051) < 1e-15
            if ck in ("first", "last", "random"):
                assert abs(float(lp) + math.log(2051)) < 1e-12


def test_bounds_are_small_and_positive():
    for c in R.CASES:
        for n in R.OUTPUTS:
            val, bound = c.made["ref"][n]
            fin = torch.isfinite(val)
            assert bool((bound[fin] > 0).all()) and bool((bound[~fin] == 0).all()), (c, n)
            # (V + 2) U on S dominates: a few 1e-4 at V = 4096, never a loose bound
            assert float(bound.max()) < 4e-3 * max(1.0, float(val[fin].abs().max()) if fin.any() else 1.0), (c, n, float(bound.max()))


@pytest.mark.parametrize("c", R.CASES, ids=repr)
def test_fp32_restatement_fits(c):
    worst = R.judge_outputs(c, R.restate(c))
    assert all(w <= 1.0 for w in worst.values())


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_wrong_restatements_do_not_fit(mut):
    caught = 0
    for c in R.CASES:
        if mut == "reads_padding" and c.ldl == c.V:
            continue                                                    # (no padding to read)
        if c.V == 1:
            continue                                                    # (one value: entropy 0 either way, exp(x) alone may not overflow)
        names = ("entropy",) if mut == "entropy_of_code" else R.OUTPUTS
        try:
            R.judge_outputs(c, R.restate(c, mut), names)
        except AssertionError:
            caught += 1
            continue
        # a case the mutant survives must be one where it cannot show: small rows of one kind
        assert c.rows < 512, (mut, c)
    assert caught >= 6, (mut, caught)
    with pytest.raises(AssertionError):
        R.judge_outputs(R.CASE["V2051_ldl2112_rows512"], R.restate(R.CASE["V2051_ldl2112_rows512"], mut),
                        ("entropy",) if mut == "entropy_of_code" else R.OUTPUTS)


def test_guard_rows_are_judged():
    c = R.CASE["V65_ldl67_rows3"]
    got = R.restate(c)
    got["pmax"][0] = 0.0                                               # a store below the window
    with pytest.raises(AssertionError):
        R.judge_outputs(c, got)
    got = R.restate(c)
    R.window(got["logprob"], c)[:] = 0.0                               # -inf rows overwritten
    if any(ck in ("minus1", "V") for ck in c.made["ckinds"]):
        with pytest.raises(AssertionError):
            R.judge_outputs(c, got)
