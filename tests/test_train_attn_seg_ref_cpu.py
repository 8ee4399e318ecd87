"""CPU proof of tests/train_attn_seg_ref.py, the float64 reference and bounds the segment-masked attention kernels are judged by
(tests/test_train_attn_seg_kernels_gpu.py).  No GPU.

  * the per-segment composition equals a dense float64 softmax under the explicit block-diagonal causal mask, and torch autograd
    through it, on every case;
  * a restatement of the kernels' scheme (fp32, exp2, bf16 P, key blocks of 64 aligned to the row, the finite floor of the
    exponent's maximum) fits EVERY bound on EVERY case;
  * each deliberately wrong restatement exceeds a bound (or gives a NaN, which the judge reports) on at least one case;
  * the case list holds the layouts it is meant to hold."""
import math

import pytest
import torch

import train_attn_ref as A
import train_attn_seg_ref as G

F64 = torch.float64
_memo = {}


def _ref(c):
    if c.name not in _memo:
        i = G.inputs(c)
        f = G.ref_forward(i["qkv"], c)
        out, lse = f.out.to(A.BF16), f.lse.float()
        _memo[c.name] = (i, f, out, lse, G.ref_backward(i["qkv"], out, lse, i["dout"], c))
    return _memo[c.name]


def _err(a, b):
    return float((a.detach() - b.detach()).abs().max())


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("c", G.CASES, ids=[c.name for c in G.CASES])
def test_reference_is_the_dense_masked_softmax_and_its_autograd(c):
    i = G.inputs(c)
    W, rep = c.H + 2 * c.KV, c.H // c.KV
    leaf = i["qkv"].double().reshape(c.B, c.S, W, c.HD).requires_grad_(True)
    q, k, v = leaf[:, :, :c.H].transpose(1, 2), leaf[:, :, c.H:c.H + c.KV].transpose(1, 2), leaf[:, :, c.H + c.KV:].transpose(1, 2)
    s = (q @ k.repeat_interleave(rep, 1).transpose(2, 3)) / math.sqrt(c.HD)
    s = s.masked_fill(~G.visible(c)[:, None], float("-inf"))
    out = (torch.softmax(s, -1) @ v.repeat_interleave(rep, 1)).transpose(1, 2).reshape(c.B * c.S, c.H * c.HD)
    f = G.ref_forward(i["qkv"], c)
    assert out.dtype == F64 and _err(out, f.out) < 1e-12 and _err(torch.logsumexp(s, -1), f.lse) < 1e-12
    assert bool(torch.isfinite(f.lse).all())                      # padding included: every query sees itself
    out.backward(i["dout"].double())
    b = G.ref_backward(i["qkv"], f.out, f.lse, i["dout"], c)
    g = leaf.grad.reshape(c.B * c.S, W * c.HD)
    assert _err(g, b.dqkv) < 1e-12 * max(1.0, float(g.abs().max()))
    assert _err(b.delta, (i["dout"].double() * f.out).reshape(c.B, c.S, c.H, c.HD).sum(-1).transpose(1, 2)) < 1e-12


@pytest.mark.parametrize("c", G.SINGLE, ids=[c.name for c in G.SINGLE])
def test_one_segment_is_the_unsegmented_reference_with_one_more_block(c):
    i, f = _ref(c)[:2]
    u = A.ref_forward(i["qkv"], c.B, c.S, c.H, c.KV, c.HD)
    assert torch.equal(u.out, f.out) and torch.equal(u.lse, f.lse)
    assert bool((f.out_slack >= u.out_slack).all()) and bool((f.lse_slack >= u.lse_slack).all())


@pytest.mark.parametrize("c", G.CASES, ids=[c.name for c in G.CASES])
def test_correct_restatement_fits_every_bound(c):
    i, f, out, lse, b = _ref(c)
    o, l = G.restate_forward(i["qkv"], c)
    A.judge_forward("cpu.seg_fwd", o, l, f, c.name)
    dqkv, delta = G.restate_backward(i["qkv"], out, lse, i["dout"], c)
    A.judge_backward("cpu.seg_bwd", dqkv, delta, b, c, c.name)


@pytest.mark.parametrize("mut", G.FWD_MUTANTS)
def test_wrong_forward_is_rejected(mut):
    hit = []
    for c in G.CASES:
        i, f = _ref(c)[:2]
        o, l = G.restate_forward(i["qkv"], c, mut=mut)
        if _rejected(lambda: A.judge_forward(f"mutant.{mut}", o, l, f)):
            hit.append(c.name)
    print(f"MUTANT seg fwd {mut}: rejected on {len(hit)} cases, e.g. {hit[:3]}")
    assert hit, f"{mut}: no case rejects it"


@pytest.mark.parametrize("mut", G.BWD_MUTANTS)
def test_wrong_backward_is_rejected(mut):
    hit = []
    for c in G.CASES:
        i, f, out, lse, b = _ref(c)
        dqkv, delta = G.restate_backward(i["qkv"], out, lse, i["dout"], c, mut=mut)
        if _rejected(lambda: A.judge_backward(f"mutant.{mut}", dqkv, delta, b, c)):
            hit.append(c.name)
    print(f"MUTANT seg bwd {mut}: rejected on {len(hit)} cases, e.g. {hit[:3]}")
    assert hit, f"{mut}: no case rejects it"


def test_no_floor_gives_a_nan_on_the_dead_tile_case():
    c = next(c for c in G.CASES if "_dead_" in c.name)
    o, l = G.restate_forward(G.inputs(c)["qkv"], c, mut="no_floor")
    assert bool(torch.isnan(o.float()[100:128]).any()), "queries 100..127 walk three wholly masked tiles"
    assert _rejected(lambda: A.judge_forward("mutant.no_floor", o, l, _ref(c)[1]))


def test_spike_premise():
    """Every query of the second segment matches the keys at 128 and 129 equally; only 129 is visible, and it takes the row."""
    c = next(c for c in G.CASES if c.kind == "spike")
    i = G.inputs(c)
    q, k, _ = A.split_heads(i["qkv"], c.B, c.S, c.H, c.KV, c.HD)
    s = (q[0] @ k[0].repeat_interleave(c.H // c.KV, 0).transpose(1, 2)) / 8
    assert bool((s[:, 129:, 128] == s[:, 129:, 129]).all()) and float(s[:, 129:, 128].min()) == 128.0
    assert not bool(G.visible(c)[0, 129:, 128].any()) and bool(G.visible(c)[0, 129:, 129].all())
    no = G.restate_forward(i["qkv"], c, mut="no_mask")[0].float()
    assert _err(no[129:].double(), _ref(c)[1].out[129:]) > 0.1    # a leak halves the weight of key 129


def test_case_list_holds_what_it_is_meant_to():
    by = {c.name.split("_")[1]: c for c in G.CASES}
    assert {tuple(c.layouts[0]) for c in G.CASES} >= {(128, 128, 128), (64, 64, 64, 192), (63, 65, 127, 129), (65, 63, 129, 127), (31, 33, 1, 319),
                                                     (1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 57), (10, 90, 28, 128), (90, 61), (128, 1), (64, 1), (5, 12)}
    assert sorted(c.S for c in G.SINGLE) == [129, 200, 256]
    for tag, walked in (("ring5", 5), ("ring4", 4), ("ring3", 3)):   # the last workgroup's walked key blocks
        c = by[tag]
        ss = G.arrays(c)[0]
        assert (c.S - 1) // 64 - int(ss[(c.S - 1) & ~127]) // 64 + 1 == walked
    assert by["pad"].S - sum(by["pad"].layouts[0]) == 49 and len(G.segments(by["pad"], 0)) == 3
    assert by["rows"].B == 3 and len(set(by["rows"].layouts)) == 3
    sc = by["sched"]
    assert sc.KV * sc.B == 16 and (sc.H, sc.KV) == (8, 2) and all(v[1] > 0 for v in A.schedule(A.Case("s", sc.B, sc.S, sc.H, sc.KV, 64, "rand"), A.DEFAULT_WORD | 1 << 10).values())
    sp = by["spike"]
    assert (sp.S, sp.H, sp.KV, sp.layouts) == (320, 4, 1, ((129, 191),))
    for c in G.CASES:                                             # heads of the listed cases cycle over HEADS64
        assert (c.H, c.KV) in A.HEADS64 and c.HD == 64
        ss, se, pos = G.arrays(c)
        assert bool((ss.reshape(c.B, c.S).diff(dim=1) >= 0).all()) and bool((se.reshape(c.B, c.S).diff(dim=1) >= 0).all())
        assert bool((pos >= 0).all()) and bool((ss <= torch.arange(c.S, dtype=torch.int32).repeat(c.B)).all())
