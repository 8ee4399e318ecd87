"""The yardstick of the typical rows sampler (tests/sampling_typical_ref.py) proved on the CPU: the rule on an example a reader can
do by hand, the same kept sets as the ``TypicalLogitsWarper`` of the installed ``transformers``, every case row's margins clear of
the derived bounds by ``HEADROOM`` with no row left out, every path of the kernel reached, the argmax dropped in a good share of the
rows, and ``typical_p = 1`` the processors reference - so the GPU test may ask for the reference's winner and kept set exactly."""
import math

import numpy as np
import pytest
import torch

import sampling_filters_ref as R
import sampling_processors_ref as P
import sampling_typical_ref as T

LN2 = math.log(2.0)


def _all_rows():
    for V in R.VS:
        for (name, kind), c in T.cases(V).items():
            for r, ref in enumerate(c["ref"]):
                yield (V, name, kind, r), c, r, ref


def test_the_rule_on_the_hand_example():
    x = torch.log(torch.tensor([0.5, 0.25, 0.125, 0.125], dtype=torch.float64)).float()
    q = torch.ones(4)
    v = R.scaled(x, 1.0)
    delta, dvals, inv, gmass, D, D2, dmax = T._groups(v, np.ones(4, dtype=bool))
    assert np.allclose(delta / LN2, [0.75, 0.25, 1.25, 1.25], atol=1e-6) and abs(D / LN2 - 0.75) < 1e-6   # H = 1.75 ln 2 = ln 2 + D
    assert len(dvals) == 3 and np.allclose(gmass, [0.25, 0.5, 0.25], atol=1e-6)
    want = {0.2: [1], 0.5: [0, 1], 0.8: [0, 1, 2, 3], 1.0: [0, 1, 2, 3], 0.24: [1], 0.26: [0, 1], 0.74: [0, 1], 0.76: [0, 1, 2, 3]}
    for tp, kept in want.items():
        ref = T.reference(x, 4, 1.0, 1.0, 0.0, tp, q)
        assert np.nonzero(ref["T"])[0].tolist() == kept, tp
        assert ref["drops_argmax"] == (0 not in kept)
    ref = T.reference(x, 4, 1.0, 1.0, 0.0, 0.2, q)
    assert ref["winner"] == 1 and ref["last_kept"] == [1] and ref["first_dropped"] == [0] and ref["single"]
    assert abs(ref["mass_margin"] - 0.05) < 1e-6 and abs(ref["order_margin"] - 0.5 * LN2) < 1e-6
    ref = T.reference(x, 4, 1.0, 1.0, 0.0, 0.5, q)                       # the tied pair is one delta group: it goes together
    assert ref["last_kept"] == [0] and ref["first_dropped"] == [2, 3]


def test_same_sets_as_the_transformers_warper_on_rows_of_distinct_values():
    tf = pytest.importorskip("transformers")
    rows = 0
    for V in R.VS:
        for kind in T.KINDS:
            c = T.cases(V)[("drawn", kind)]
            for r, ref in enumerate(c["ref"]):
                v = R.scaled(c["xp"][r], c["temperature"][r])
                N = ref["N"]
                if len(np.unique(v[N])) != int(N.sum()) or int(N.sum()) < 2:
                    continue
                scores = torch.from_numpy(np.where(N, v, -np.inf)).unsqueeze(0)
                warper = tf.TypicalLogitsWarper(mass=float(np.float32(c["typical_p"][r])), min_tokens_to_keep=1)
                kept = torch.isfinite(warper(torch.zeros(1, 1, dtype=torch.long), scores))[0].numpy()
                assert (kept == ref["T"]).all(), (V, kind, r, int(kept.sum()), int(ref["T"].sum()))
                rows += 1
    assert rows >= 56, rows


def test_every_case_row_clears_the_derived_bounds_and_none_is_left_out():
    worst = [math.inf, math.inf, math.inf]
    rows = single_group = 0
    for where, c, r, ref in _all_rows():
        rows += 1
        tp = c["typical_p"][r]
        assert 0.0 < tp < 1.0 and tp == float(np.float32(tp)), where
        assert ref["topp_margin"] >= R.HEADROOM * ref["topp_bound"] and ref["minp_margin"] >= R.HEADROOM * ref["minp_bound"], where
        assert ref["mass_margin"] >= T.HEADROOM * ref["mass_bound"], (where, ref["mass_margin"], ref["mass_bound"])
        assert ref["order_margin"] >= T.HEADROOM * ref["delta_bound"], (where, ref["order_margin"], ref["delta_bound"])
        assert ref["single"] and ref["runner_up"] >= T.RUNNER_UP, (where, ref["runner_up"])
        n = min(R.GROUPS[r], R.QUANT_CAP) if where[1] == "quant" else R.GROUPS[r]
        v = R.scaled(c["xp"][r], c["temperature"][r])
        G = len(T._groups(v, ref["N"])[1])
        if G < 2:
            single_group += 1
            assert tp == 0.5 and ref["groups"] == 1 and (ref["T"] == ref["N"]).all(), where
        else:
            assert abs(ref["groups"] - max(1, min(n, G - 1))) <= T.SEARCH and not (ref["T"] == ref["N"]).all(), where
        # the boundary probes of the GPU test are decisive: q = 1e-30 on a member of the last kept group beats everything else
        last = ref["last_kept"][0]
        others = np.delete(ref["p"] / c["q"][r].double().numpy(), last)
        assert ref["p"][last] >= 1e-30 and ref["p"][last] / 1e-30 >= 1e3 * others.max(), where
        assert all(ref["T"][i] for i in ref["last_kept"]) and not any(ref["T"][i] for i in ref["first_dropped"]), where
        worst = [min(worst[0], ref["mass_margin"] / ref["mass_bound"]), min(worst[1], ref["order_margin"] / ref["delta_bound"]),
                 min(worst[2], ref["runner_up"])]
    print("rows %d (one delta group: %d); margins / bound: mass %.1fx, order %.1fx; runner-up %.4f"
          % (rows, single_group, worst[0], worst[1], worst[2]))
    assert rows == 2 * len(R.SETS) * len(T.KINDS) * R.ROWS == 192
    # the stand-in the cases were first tried with is looser than the derived bound
    for where, c, r, ref in _all_rows():
        v = R.scaled(c["xp"][r], c["temperature"][r])
        d = (v.max() - v)[ref["N"]]
        assert ref["delta_bound"] <= 64 * T.EPS24 * max(1.0, float(d.max())), where


def test_the_cases_reach_every_path_of_the_kernel():
    paths = dict(wave=0, wide_to_wave=0, wide=0, wide_nucleus_then_wide_typical=0, wave_nucleus_then_wave_typical=0,
                 wide_nucleus_then_wave_typical=0)
    drops = rows = 0
    for where, c, r, ref in _all_rows():
        rows += 1
        nK, nN, nT = int(ref["K"].sum()), int(ref["N"].sum()), int(ref["T"].sum())
        filters = c["top_p"][r] < 1.0 or c["min_p"][r] > 0.0
        paths["wave"] += nN <= 64
        paths["wide_to_wave"] += nN > 64 and nT <= 64
        paths["wide"] += nT > 64
        paths["wide_nucleus_then_wide_typical"] += filters and c["top_p"][r] < 1.0 and nK > 64 and nN > 64
        paths["wave_nucleus_then_wave_typical"] += filters and nK <= 64
        paths["wide_nucleus_then_wave_typical"] += filters and nK > 64 and nN <= 64
        drops += ref["drops_argmax"]
    print(paths, "argmax dropped in %d of %d rows" % (drops, rows))
    assert all(n >= 4 for n in paths.values()), paths
    assert 3 * drops >= rows, (drops, rows)


def test_typical_p_one_is_the_processors_reference():
    for V in R.VS:
        for name in R.SETS:
            c = P.cases(V)[(name, "both")]
            for r, want in enumerate(c["ref"]):
                ref = T.reference(c["xp"][r], c["topk"][r], R.TEMP[r], c["top_p"][r], c["min_p"][r], 1.0, c["q"][r])
                assert ref["winner"] == want["winner"] and (ref["T"] == want["N"]).all() and (ref["p"] == want["p"]).all(), (V, name, r)
                assert ref["mass_margin"] == math.inf and not ref["drops_argmax"]
        for (name, kind), c in T.cases(V).items():
            for r, (ref, proc) in enumerate(zip(c["ref"], c["proc"])):
                assert (proc["T"] == ref["N"]).all() and (proc["N"] == ref["N"]).all(), (V, name, kind, r)
