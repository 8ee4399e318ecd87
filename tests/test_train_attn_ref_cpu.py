"""CPU proof of tests/train_attn_ref.py, the float64 reference and bounds the training attention kernels are judged by
(tests/test_train_attn_kernels_gpu.py).  No GPU.

  * every reference against torch's own float64 machinery (scaled_dot_product_attention, the oracle, autograd), to 1e-12;
  * restatements of the kernels' numeric schemes in fp32 / bf16 fit EVERY bound on EVERY case;
  * deliberately wrong restatements each exceed a bound on at least one case;
  * the premise of the spike cases; that the case list holds the grids and dispatch conditions it is meant to hold;
  * the kernels' work orders, restated: each hands out every work item exactly once, and the scheduling cases make them reorder."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_attn_ref as A
from oracle import csm_oracle as O

F64 = torch.float64
_memo = {}


def _ref(c):
    """(inputs, Fwd, bf16 out, fp32 lse, Bwd without and with the table) of a case, computed once and left unchanged."""
    if c.name not in _memo:
        i = A.inputs(c)
        f = A.ref_forward(i["qkv"], c.B, c.S, c.H, c.KV, c.HD)
        out, lse = f.out.to(A.BF16), f.lse.float()
        tab = A.rope_table(c)
        b = A.ref_backward_both(i["qkv"], out, lse, i["dout"], c.B, c.S, c.H, c.KV, c.HD, tab)
        _memo[c.name] = (i, f, out, lse, b, tab)
    return _memo[c.name]


def _err(a, b):
    return float((a - b).abs().max())


SMALL = [A.CASE[n] for n in ("hd64_S17_h2_2_B1", "hd64_S65_h8_1_B1", "hd64_S129_h8_2_B3", "hd128_S33_h8_2_B3", "hd128_S100_h2_1_B3",
                             "hd64_spike_S320_h4_2_B1", "hd64_big_S200_h8_2_B1")]


@pytest.mark.parametrize("c", SMALL, ids=[c.name for c in SMALL])
def test_ref_forward_is_sdpa_and_the_oracle(c):
    qkv = A.inputs(c)["qkv"]
    f = A.ref_forward(qkv, c.B, c.S, c.H, c.KV, c.HD)
    x = qkv.double().reshape(c.B, c.S, c.H + 2 * c.KV, c.HD)
    q, k, v = x[:, :, :c.H], x[:, :, c.H:c.H + c.KV], x[:, :, c.H + c.KV:]
    rep = c.H // c.KV
    sd = F.scaled_dot_product_attention(q.transpose(1, 2), k.repeat_interleave(rep, 2).transpose(1, 2), v.repeat_interleave(rep, 2).transpose(1, 2),
                                        attn_mask=torch.tril(torch.ones(c.S, c.S, dtype=torch.bool)))
    assert sd.dtype == F64 and _err(sd.transpose(1, 2).reshape(c.B * c.S, -1), f.out) < 1e-12
    orc = O.attention(q, k, v)
    assert orc.dtype == F64 and _err(orc.reshape(c.B * c.S, -1), f.out) < 1e-12
    s = (q.transpose(1, 2) @ k.repeat_interleave(rep, 2).transpose(1, 2).transpose(2, 3)) / math.sqrt(c.HD)
    s = s.masked_fill(~torch.tril(torch.ones(c.S, c.S, dtype=torch.bool)), float("-inf"))
    assert _err(torch.logsumexp(s, -1), f.lse) < 1e-12
    assert _err(torch.softmax(s, -1), f.p) < 1e-12 and _err(f.p.sum(-1), torch.ones(())) < 1e-12
    assert _err((f.p @ v.repeat_interleave(rep, 2).transpose(1, 2).abs()).transpose(1, 2).reshape(c.B * c.S, -1), f.absv) < 1e-12


@pytest.mark.parametrize("rope", (False, True), ids=("plain", "rope"))
@pytest.mark.parametrize("c", SMALL, ids=[c.name for c in SMALL])
def test_ref_backward_is_autograd(c, rope):
    """Fed the float64 forward's own out and lse, the kernels' contract IS the gradient."""
    i = A.inputs(c)
    tab = A.rope_table(c)
    W, a, e = c.H + 2 * c.KV, c.H * c.HD, (c.H + c.KV) * c.HD
    pos = torch.arange(c.S)[None].expand(c.B, c.S)
    leaf = i["qkv"].double().reshape(c.B, c.S, W, c.HD).requires_grad_(True)
    # with the table the leaf is the un-rotated projection output; the kernels see its rotation (float64 here, through the oracle)
    x = torch.cat([O.rope(leaf[:, :, :c.H + c.KV], tab, pos), leaf[:, :, c.H + c.KV:]], 2) if rope else leaf
    assert x.dtype == F64
    qkv = x.detach().reshape(c.B * c.S, W * c.HD)
    f = A.ref_forward(qkv, c.B, c.S, c.H, c.KV, c.HD)
    b = A.ref_backward(qkv, f.out, f.lse, i["dout"], c.B, c.S, c.H, c.KV, c.HD, tab if rope else None)
    O.attention(x[:, :, :c.H], x[:, :, c.H:c.H + c.KV], x[:, :, c.H + c.KV:]).backward(i["dout"].double().reshape(c.B, c.S, c.H, c.HD))
    g = leaf.grad.reshape(c.B * c.S, W * c.HD)
    tol = 1e-12 * max(1.0, float(g.abs().max()))
    assert _err(g[:, :a], b.dqkv[:, :a]) < tol and _err(g[:, a:e], b.dqkv[:, a:e]) < tol and _err(g[:, e:], b.dqkv[:, e:]) < tol
    assert _err(b.delta, (i["dout"].double() * f.out).reshape(c.B, c.S, c.H, c.HD).sum(-1).transpose(1, 2)) < 1e-12


@pytest.mark.parametrize("H,KV,pos0,n", [(4, 1, 0, 17), (4, 2, 63, 65), (2, 2, 130, 16), (4, 1, 64, 1)])
def test_ref_append_is_the_forward_of_the_concatenated_sequence(H, KV, pos0, n):
    g = torch.Generator().manual_seed(pos0 + n)
    S, S_max, HD = pos0 + n, 256, 64
    qkv = torch.randn(S, (H + 2 * KV) * HD, generator=g).to(A.BF16)
    x = qkv.reshape(S, H + 2 * KV, HD)
    guard = torch.full((KV, S_max, HD), 7.0, dtype=A.BF16)
    kc, vc = guard.clone(), guard.clone()
    kc[:, :pos0], vc[:, :pos0] = x[:pos0, H:H + KV].transpose(0, 1), x[:pos0, H + KV:].transpose(0, 1)
    a = A.ref_append(qkv[pos0:], kc, vc, pos0, n, H, KV)
    f = A.ref_forward(qkv, 1, S, H, KV, HD)
    assert _err(a.out, f.out[pos0:]) < 1e-12
    assert torch.equal(a.kcache[:, :S], x[:, H:H + KV].transpose(0, 1)) and torch.equal(a.vcache[:, :S], x[:, H + KV:].transpose(0, 1))
    assert bool((a.kcache[:, S:] == 7.0).all()) and bool((a.vcache[:, S:] == 7.0).all())
    # the bound is the forward's with two more rescales: never below it
    assert bool((a.out_slack >= f.out_slack[pos0:]).all())


# ------------------------------------------------------------------------------------------------------------- restatements
SCHEMES = {"fwd_l_fp32_kb64": dict(l_bf16=False, kb=64), "fwd_l_bf16_kb32": dict(l_bf16=True, kb=32)}


@pytest.mark.parametrize("c", A.CASES, ids=[c.name for c in A.CASES])
def test_correct_restatements_fit_every_bound(c):
    i, f, out, lse, b, tab = _ref(c)
    for name, kw in SCHEMES.items():
        o, l = A.restate_forward(i["qkv"], c.B, c.S, c.H, c.KV, c.HD, **kw)
        A.judge_forward(f"cpu.{name}", o, l, f, c.name)
    for rope in (False, True):
        dqkv, delta = A.restate_backward(i["qkv"], out, lse, i["dout"], c.B, c.S, c.H, c.KV, c.HD, tab if rope else None)
        A.judge_backward("cpu.bwd_bf16_p_ds" + ("_rope" if rope else ""), dqkv, delta, b[rope], c, c.name)
        if c.kind == "rand" and c.S >= 3:                         # the all-zero dout row: an exactly zero dQ row is what the bound asks
            assert bool((b[rope].dqkv_slack[c.S // 2, :c.H * c.HD] == 0).all()) and bool((dqkv[c.S // 2, :c.H * c.HD] == 0).all())
    if c.kind == "rand" and c.S >= 3:                             # the all-zero query row: uniform probabilities
        assert _err(f.p[0, 0, c.S // 3, :c.S // 3 + 1], torch.full((), 1.0 / (c.S // 3 + 1), dtype=F64)) < 1e-15


MUTANT_CASES = [c for c in A.CASES if c not in A.SCHED]           # the scheduling cases add grids, not numerics: left out for time


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mut", A.FWD_MUTANTS)
def test_wrong_forward_is_rejected(mut):
    hit = []
    for c in MUTANT_CASES:
        i, f = _ref(c)[:2]
        for kw in SCHEMES.values():
            o, l = A.restate_forward(i["qkv"], c.B, c.S, c.H, c.KV, c.HD, mut=mut, **kw)
            if _rejected(lambda: A.judge_forward(f"mutant.{mut}", o, l, f)):
                hit.append(c.name)
    print(f"MUTANT fwd {mut}: rejected on {len(hit)} judgements, e.g. {hit[:3]}")
    assert hit, f"{mut}: no case rejects it"


@pytest.mark.parametrize("mut", A.BWD_MUTANTS)
def test_wrong_backward_is_rejected(mut):
    hit = []
    for c in MUTANT_CASES:
        i, f, out, lse, b, tab = _ref(c)
        rope = mut.startswith("rope")
        dqkv, delta = A.restate_backward(i["qkv"], out, lse, i["dout"], c.B, c.S, c.H, c.KV, c.HD, tab if rope else None, mut=mut)
        if _rejected(lambda: A.judge_backward(f"mutant.{mut}", dqkv, delta, b[rope], c)):
            hit.append(c.name)
    print(f"MUTANT bwd {mut}: rejected on {len(hit)} cases, e.g. {hit[:3]}")
    assert hit, f"{mut}: no case rejects it"


def test_a_tile_edge_mask_mistake_is_rejected_at_every_edge():
    """An off-by-one of the mask confined to ONE query row at a 16 / 32 / 64 / 128 tile edge (row r sees key r + 1) must be
    rejected by the bounds of that row alone: that is the mistake the old whole-tensor tolerance could not see."""
    c = A.CASE["hd64_S384_h8_2_B1"]
    i, f = _ref(c)[:2]
    good, lse = A.restate_forward(i["qkv"], c.B, c.S, c.H, c.KV, c.HD)
    bad, lse_bad = A.restate_forward(i["qkv"], c.B, c.S, c.H, c.KV, c.HD, mut="mask_plus1")
    for r in (15, 31, 63, 127, 255, 319):
        o, l = good.clone(), lse.clone()
        o[r], l[:, :, r] = bad[r], lse_bad[:, :, r]
        assert _rejected(lambda: A.judge_forward("mutant.edge", o, l, f)), f"row {r}"


def test_spike_premise():
    """In a spike case the marked key scores at least 64 above every other visible key, so the float64 softmax leaves less than
    2^-13 elsewhere (exp(-64) n << 2^-13)."""
    for c in A.CASES:
        if c.kind != "spike":
            continue
        i, f = _ref(c)[:2]
        q, k, _ = A.split_heads(i["qkv"], c.B, c.S, c.H, c.KV, c.HD)
        s = (q @ k.repeat_interleave(c.H // c.KV, 1).transpose(2, 3)) / math.sqrt(c.HD)
        for (qi, kj) in A.SPIKES[c.S]:
            row = s[:, :, qi, :qi + 1].clone()
            top = row[..., kj].clone()
            row[..., kj] = float("-inf")
            assert float((top - row.amax(-1)).min()) >= 64.0, (c.name, qi, kj)
            assert float((1 - f.p[:, :, qi, kj]).max()) < 2.0 ** -13


def test_case_list_holds_what_it_is_meant_to():
    hd64 = [c for c in A.CASES if c.HD == 64 and c not in A.SCHED]
    assert {c.S for c in hd64} >= set(A.S64) and {(c.H, c.KV) for c in hd64} == set(A.HEADS64) and {c.B for c in hd64} == {1, 2, 3}
    for kern in ("fwd", "dkv"):                                   # the XCD remap: grids that are and are not multiples of 8
        assert {A.grids(c)[kern] % 8 == 0 for c in hd64} == {True, False}
    assert {A.expected_kernels(c) for c in hd64} == {0, 1}
    word = A.DEFAULT_WORD | 1 << 12
    assert {A.expected_kernels(c, word) for c in hd64} == {0, 1, 3}
    hd128 = [c for c in A.CASES if c.HD == 128 and c not in A.SCHED]
    assert {c.S for c in hd128 if (c.H, c.KV) == (8, 2)} >= {1, 16, 17, 31, 32, 33, 64, 129}
    assert {(c.H, c.KV) for c in hd128 if c.S == 32} == {(8, 2), (4, 2), (2, 1)} and {c.S for c in hd128} >= {64, 65, 100, 129}


# ------------------------------------------------------------------------------------------------------------- work orders
LENGTHS = (1, 16, 33, 63, 64, 65, 127, 128, 129, 192, 200, 256, 257, 320, 384, 512, 1000, 2048)
PAIRS = sorted({B * KV for B in range(1, 33) for KV in (1, 2, 4, 8)})


def test_every_work_order_hands_out_every_item_once():
    """The restated index arithmetic of attn_dkv_kernel (work orders 0..3, 64- and 128-key tiles), attn64_dkv_kernel, attn_q_kernel
    with lpt (64 and 128 queries per block) and work_item is a bijection of the grid onto the work items for B 1..32,
    KV 1 / 2 / 4 / 8, rep 1 / 2 / 4 / 8 and 18 lengths.  (Work order 2 was not, until it took the parity from the work item.)"""
    nblks = sorted({-(-S // t) for S in LENGTHS for t in (64, 128)})
    for P in PAIRS:
        for nblk in nblks:
            for order in range(4):
                items, _ = A.dkv_work_order(P, nblk, order)
                assert A.is_bijection(items, P, nblk), ("dkv", P, nblk, order)
            for rep in (1, 2, 4, 8):
                items, _ = A.q_work_order(P, nblk, rep, True)
                assert A.is_bijection(items, P, rep, nblk), ("q", P, nblk, rep)
    items, moved = A.q_work_order(16, 3, 4, False)                # without lpt: the work items in the order of the runs
    assert A.is_bijection(items, 16, 4, 3) and moved == 0


def test_work_order_2_as_it_was_is_seen():
    """is_bijection sees the mistake work order 2 had: the parity of the place in the run for the parity of the key block, at
    S = 384, 2 kv heads, B = 1 (12 workgroups)."""
    nid, within, _, _ = A.xcd_runs(12)
    kblk = nid % 6
    kblk = np.where((within & 1) == 1, 6 - 1 - (kblk ^ 1), kblk)
    assert not A.is_bijection(np.stack([nid // 6, kblk], 1), 2, 6)
    assert A.is_bijection(A.dkv_work_order(2, 6, 2)[0], 2, 6)


def test_scheduling_cases_make_every_work_order_reorder():
    """Without them no case has a run of whole (batch, kv head) pairs: every reordering branch is skipped or moves nothing."""
    G1 = A.DEFAULT_WORD | 3 << 8
    others = [c for c in A.CASES if c not in A.SCHED]
    for word in (0, G1, (G1 & ~(3 << 4)) | 1 << 4, G1 & ~(1 << 6)):
        assert not any(v[1] for c in others for v in A.schedule(c, word).values())
    for c in A.SCHED:
        assert c.KV * c.B == 16
        for word in (0, G1, G1 & ~(1 << 6), (G1 & ~(3 << 4)) | 1 << 4, (G1 & ~(3 << 4) & ~(1 << 6)) | 1 << 4):
            sc = A.schedule(c, word)
            assert set(sc) == {"fwd", "dq", "dkv"} and all(v[1] > 0 and A.is_bijection(v[0], *v[2]) for v in sc.values()), (c.name, hex(word))
        assert not any(v[1] for k, v in A.schedule(c, G1 & ~(1 << 7)).items() if k != "dkv")          # bit 7 clear: the plain order
        assert A.schedule(c, G1 & ~(3 << 4))["dkv"][1] == 0                                          # work order 0: the plain order
