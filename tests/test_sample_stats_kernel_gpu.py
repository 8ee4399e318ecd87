"""``csm_sample_stats_rows`` against the float64 reference of tests/sample_stats_ref.py: every case held to the reference's
bound with the whole output buffers judged (guard rows) and the logits framed in NaN (padding columns, guard rows); equal bits
from two launches; a row's bits alone and inside a 512-row launch; each output NULL in turn; refusals launch nothing."""
import pytest
import torch

import sample_stats_ref as R

pytestmark = pytest.mark.gpu
WORST = {n: 0.0 for n in R.OUTPUTS}


def _launch(c, logits, codes, names=R.OUTPUTS):
    """One launch into fresh sentinel buffers: {name: the whole buffer}; an output not in ``names`` gets NULL."""
    from csm.hip import ops
    bufs = R.output_buffers(c, logits.device)
    ops.sample_stats_rows(R.logits_window(logits, c), codes, *[R.window(bufs[n], c) if n in names else None for n in R.OUTPUTS],
                          V=c.V)
    return bufs


@pytest.fixture(scope="module")
def on_device(dev):
    """Per case: the NaN-framed logits and the codes on the device, made once and never written."""
    return {c.name: (c.made["logits"].to(dev), c.made["codes"].to(dev)) for c in R.CASES}


@pytest.mark.parametrize("c", R.CASES, ids=repr)
def test_case_is_within_the_bound_and_deterministic(on_device, c):
    logits, codes = on_device[c.name]
    got = _launch(c, logits, codes)
    worst = R.judge_outputs(c, got)
    for n, w in worst.items():
        WORST[n] = max(WORST[n], w)
    print("RATIO sample_stats", c, " ".join(f"{n} {w:.4f}" for n, w in worst.items()))
    again = _launch(c, logits, codes)
    for n in R.OUTPUTS:
        assert torch.equal(got[n].view(torch.int32), again[n].view(torch.int32)), (c, n)


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"V{s[0]}")
def test_a_row_alone_has_the_bits_it_has_among_512(on_device, shape):
    from csm.hip import ops
    V, ldl = shape
    c = R.CASE[f"V{V}_ldl{ldl}_rows512"]
    logits, codes = on_device[c.name]
    full = _launch(c, logits, codes)
    for r in (0, 1, 255, 511, 300, 77):
        out = torch.zeros(3, 1, dtype=torch.float32, device=logits.device)
        ops.sample_stats_rows(R.logits_window(logits, c)[r:r + 1], codes[r:r + 1], out[0], out[1], out[2], V=V)
        for j, n in enumerate(R.OUTPUTS):
            assert torch.equal(out[j].view(torch.int32), R.window(full[n], c)[r:r + 1].view(torch.int32)), (c, r, n)


@pytest.mark.parametrize("missing", R.OUTPUTS)
def test_each_output_may_be_null(on_device, missing):
    for name in ("V2051_ldl2112_rows3", "V4096_ldl4100_rows3", "V1_ldl4_rows3"):
        c = R.CASE[name]
        logits, codes = on_device[name]
        names = tuple(n for n in R.OUTPUTS if n != missing)
        got = _launch(c, logits, codes, names)
        R.judge_outputs(c, got, names, f" without {missing}")
        full = _launch(c, logits, codes)
        for n in names:
            assert torch.equal(got[n].view(torch.int32), full[n].view(torch.int32)), (c, n, missing)


def test_worst_ratios_are_printed():
    print("WORST sample_stats", " ".join(f"{n} {w:.4f}" for n, w in WORST.items()))
    assert all(0.0 <= w <= 1.0 for w in WORST.values())


def test_entry_point_refusals_launch_nothing(dev, on_device):
    from csm import hip
    c = R.CASE["V2051_ldl2112_rows3"]
    logits, codes = on_device[c.name]
    lg = R.logits_window(logits, c)
    bufs = R.output_buffers(c, dev)
    before = {n: b.clone() for n, b in bufs.items()}
    stream = torch.cuda.current_stream().cuda_stream
    names = ("logits", "codes", "logprob", "entropy", "pmax", "rows", "V", "ldl")
    a0 = dict(logits=lg.data_ptr(), codes=codes.data_ptr(), rows=c.rows, V=c.V, ldl=c.ldl,
              **{n: R.window(bufs[n], c).data_ptr() for n in R.OUTPUTS})
    bad = [dict(logits=None), dict(codes=None), dict(logprob=None, entropy=None, pmax=None), dict(rows=0), dict(rows=-3),
           dict(V=0), dict(V=-1), dict(V=4097, ldl=4097), dict(ldl=c.V - 1), dict(ldl=0),
           dict(logits=lg.data_ptr() + 2), dict(codes=codes.data_ptr() + 1), dict(logprob=a0["logprob"] + 2),
           dict(entropy=a0["entropy"] + 1), dict(pmax=a0["pmax"] + 3)]
    for change in bad:
        a = {**a0, **change}
        rc = hip.lib.csm_sample_stats_rows(*[a[n] for n in names], stream)
        assert rc == 1, change
        assert b"csm_sample_stats_rows" in hip.lib.csm_last_error(), change
    torch.cuda.synchronize()
    for n in R.OUTPUTS:
        assert torch.equal(bufs[n].view(torch.int32), before[n].view(torch.int32)), n
    assert hip.lib.csm_sample_stats_rows(*[a0[n] for n in names], stream) == 0
    R.judge_outputs(c, bufs)
