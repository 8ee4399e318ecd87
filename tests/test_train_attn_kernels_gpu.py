"""The training attention kernels - csm_attn_fwd, csm_attn_bwd, csm_attn_bwd_rope in all three generations (csrc/attention.hip,
attention64.hip, attention64_asm.hip) and every code-selecting switch of csm_set_attn_variant, csm_attn_append and
csm_attn_append_rows - against the float64 reference of tests/train_attn_ref.py (proved by tests/test_train_attn_ref_cpu.py).
Kernel level only: no model is built.

Every output buffer starts as NaN and EVERY element is judged by ``train_ops_ref.judge`` against a bound derived there from the
roundings the kernels perform - never from what the kernels give.  Each judgement prints ``RATIO <kernel> <worst |err| / bound>``;
a ratio above 1 fails.  Each case asserts which kernel took it where csm_attn_last_dkv_kernel() answers that."""
import ctypes

import numpy as np
import pytest
import torch

import train_attn_ref as A

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
D = A.DEFAULT_WORD
_memo = {}


def _s():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape, dtype=BF16):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _lib():
    from csm.hip import check, lib
    return check, lib


def _ref(c):
    """Inputs and references of a case, computed once, shared by the tests and left unchanged."""
    if c.name not in _memo:
        i = A.inputs(c)
        f = A.ref_forward(i["qkv"], c.B, c.S, c.H, c.KV, c.HD)
        _memo[c.name] = dict(i=i, f=f, out=f.out.to(BF16), lse=f.lse.float(), tab=A.rope_table(c), b={})
    return _memo[c.name]


def _ref_bwd(c, rope):
    """The backward of the reference's own out (rounded to bf16) and lse (rounded to fp32)."""
    r = _ref(c)
    if not r["b"]:
        r["b"] = A.ref_backward_both(r["i"]["qkv"], r["out"], r["lse"], r["i"]["dout"], c.B, c.S, c.H, c.KV, c.HD, r["tab"])
    return r["b"][rope]


def _fwd(c, qkv):
    check, lib = _lib()
    out, lse = _nan(c.B * c.S, c.H * c.HD), _nan(c.B, c.H, c.S, dtype=F32)
    check(lib.csm_attn_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), c.B, c.S, c.H, c.KV, c.HD, _s()), "csm_attn_fwd")
    return out, lse


def _bwd(c, qkv, out, lse, dout, table):
    check, lib = _lib()
    dqkv, ws = _nan(*qkv.shape), _nan(2, c.B, c.H, c.S, dtype=F32)
    assert ws.numel() * 4 == lib.csm_attn_bwd_workspace_bytes(c.B, c.S, c.H)
    if table is None:
        check(lib.csm_attn_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), ws.data_ptr(), c.B, c.S, c.H, c.KV,
                               c.HD, _s()), "csm_attn_bwd")
    else:
        check(lib.csm_attn_bwd_rope(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), ws.data_ptr(),
                                    table.data_ptr(), c.B, c.S, c.H, c.KV, c.HD, _s()), "csm_attn_bwd_rope")
    return dqkv, ws.cpu(), lib.csm_attn_last_dkv_kernel()


def _kernel_names(c, word):
    """(forward, backward) names for the records: which generation the word selects for this case."""
    w = word or D
    if c.HD == 128:
        g = "grouped" if (c.S <= 32 and c.H == 4 * c.KV and not (w >> 14) & 1) else "per_head"
        return f"hd128_{g}", f"hd128_{g}"
    fwd = "gen1_fwd" if (w >> 8) & 1 else "gen2_fwd"
    if (w >> 8) & 2:
        return fwd, "gen1_bwd"
    k = A.expected_kernels(c, w)
    return fwd, ("asm" if k & 2 else "gen2") + "_dq+" + ("asm" if k & 1 else "gen2") + "_dkv"


def _judge_bwd(name, c, word, dqkv, ws, b, lse_given, what):
    """dQ, dK, dV and what the dQ pass published: delta (first generation, head_dim 128) or -delta and -lse log2(e) (second
    generation and asm, the form their dK/dV pass consumes); the first generation leaves the second half of the scratch alone."""
    gen2 = c.HD == 64 and not ((word or D) >> 8) & 2
    A.judge_backward(name, dqkv, -ws[0] if gen2 else ws[0], b, c, what)
    if gen2:
        ref = -lse_given.double() * float(np.float32(A.LOG2E32))
        A.judge(f"{name}.nlse2", ws[1], ref, 2 * A.U * ref.abs())
    else:
        assert bool(torch.isnan(ws[1]).all()), "the first generation writes only delta"


def _check_case(c, word, rope_modes=(False, True), chain=True, fwd=True, bwd=True):
    check, lib = _lib()
    r = _ref(c)
    qkv, dout = r["i"]["qkv"].cuda(), r["i"]["dout"].cuda()
    kf, kb = _kernel_names(c, word)
    chained = None
    try:
        lib.csm_set_attn_variant(word)
        out, lse = _fwd(c, qkv) if fwd or chain else (None, None)
        if fwd:
            A.judge_forward(f"attn.{kf}", out, lse, r["f"], f"{c.name} word={word:#x}")
        if not bwd:
            return
        for rope in rope_modes:
            tab = r["tab"].cuda() if rope else None
            tag = f"attn.{kb}" + (".rope" if rope else "")
            # in isolation: the reference's own out and lse as inputs
            dqkv, ws, took = _bwd(c, qkv, r["out"].cuda(), r["lse"].cuda(), dout, tab)
            assert took == A.expected_kernels(c, word), f"{c.name} word={word:#x}: kernels {took}, the dispatch promises {A.expected_kernels(c, word)}"
            _judge_bwd(tag, c, word, dqkv, ws, _ref_bwd(c, rope), r["lse"], f"{c.name} word={word:#x} isolated")
            if c.kind == "rand" and c.S >= 3:
                assert bool((dqkv[c.S // 2, :c.H * c.HD] == 0).all()), "a zero dout row must give an exactly zero dQ row"
            if chain:                                             # in a chain: the kernel's own out and lse, against ref_backward of those
                dqkv, ws, _ = _bwd(c, qkv, out, lse, dout, tab)
                chained = chained or A.ref_backward_both(r["i"]["qkv"], out.cpu(), lse.cpu(), r["i"]["dout"], c.B, c.S, c.H, c.KV, c.HD, r["tab"])
                _judge_bwd(tag + ".chain", c, word, dqkv, ws, chained[rope], lse.cpu(), f"{c.name} word={word:#x} chained")
    finally:
        lib.csm_set_attn_variant(0)


@pytest.mark.parametrize("c", A.CASES, ids=[c.name for c in A.CASES])
def test_default_dispatch(dev, c):
    """Every case through the default kernels: forward (out, lse), backward isolated and chained, with and without the table.
    On the scheduling cases every default kernel that has a work order reorders by it (the restated arithmetic says so)."""
    if c in A.SCHED:
        sc = A.schedule(c, 0)
        assert set(sc) == {"fwd", "dq", "dkv"} and all(v[1] > 0 for v in sc.values()), {k: v[1] for k, v in sc.items()}
    _check_case(c, 0)


# every code-selecting switch of csm_set_attn_variant (a non-zero word replaces ALL the defaults, so each starts from DEFAULT_WORD)
G1F, G1B, G1 = D | 1 << 8, D | 2 << 8, D | 3 << 8
VARIANTS = {
    "bit10_gen2_dkv": D | 1 << 10, "bit11_asm_dkv_pairs": D | 1 << 11, "bit12_asm_dq": D | 1 << 12, "bit12_13_asm_dq_one_block": D | 1 << 12 | 1 << 13,
    "bit12_11_asm_both_pairs": D | 1 << 12 | 1 << 11, "bits8_9_gen1_fwd": G1F, "bits8_9_gen1_bwd": G1B, "bits8_9_gen1_both": G1,
    "fwd_one_tile_per_wave": (G1 & ~3) | 1, "dq_two_tiles_per_wave": (G1 & ~(3 << 2)) | 2 << 2, "dq_one_tile_per_wave": (G1 & ~(3 << 2)) | 1 << 2,
    "dkv_order0": (G1B & ~(3 << 4)) | 0 << 4, "dkv_order1": (G1B & ~(3 << 4)) | 1 << 4, "dkv_order2": (G1B & ~(3 << 4)) | 2 << 4,
    "dkv_order3": (G1B & ~(3 << 4)) | 3 << 4, "bit6_clear_128_key_tile": G1B & ~(1 << 6), "bit7_clear_plain_q_order": G1 & ~(1 << 7),
}
V64 = ("hd64_S65_h8_1_B1", "hd64_S129_h4_1_B2", "hd64_S192_h8_2_B1", "hd64_S256_h4_1_B3", "hd64_S384_h8_2_B1", "hd64_spike_S320_h4_1_B2")
V128 = ("hd128_S17_h8_2_B3", "hd128_S32_h8_2_B2", "hd128_S33_h8_2_B3", "hd128_S32_h2_1_B3", "hd128_S129_h8_2_B1", "hd128_spike_S100_h8_2_B1")


@pytest.mark.parametrize("c", [A.CASE[n] for n in V64], ids=V64)
@pytest.mark.parametrize("v", list(VARIANTS), ids=list(VARIANTS))
def test_variant_switch_head_dim_64(dev, v, c):
    word = VARIANTS[v]
    touches_fwd = bool((word >> 8) & 1)                           # the other words leave the forward at the default, judged above
    _check_case(c, word, chain=False, fwd=touches_fwd, bwd=True)


@pytest.mark.parametrize("c", [A.CASE[n] for n in V128], ids=V128)
@pytest.mark.parametrize("v", ("bit14_per_head", "bit7_clear_plain_q_order"))
def test_variant_switch_head_dim_128(dev, v, c):
    _check_case(c, {"bit14_per_head": D | 1 << 14, "bit7_clear_plain_q_order": D & ~(1 << 7)}[v], chain=False)


# The scheduling switches on the scheduling cases (KV B = 16: two whole pairs in every XCD's run), where the code they select
# reorders.  name: (word, kernels whose order must move workgroups, kernels whose order must move none, cases)
def _order(o, key_tile_64=True, word=G1):
    return ((word & ~(3 << 4)) | o << 4) & ~(0 if key_tile_64 else 1 << 6)


ALL3, S64_SCHED = {"fwd", "dq", "dkv"}, tuple(c.name for c in A.SCHED if c.HD == 64)
SCHED_VARIANTS = {
    "gen1_bit7_set_order3_key_tile_64": (G1, ALL3, set(), S64_SCHED),
    "gen1_bit7_set_order3_key_tile_128": (_order(3, False), ALL3, set(), S64_SCHED),
    "gen1_bit7_clear_order3": (G1 & ~(1 << 7), {"dkv"}, {"fwd", "dq"}, S64_SCHED),
    "gen1_order1_key_tile_64": (_order(1), ALL3, set(), S64_SCHED),
    "gen1_order1_key_tile_128": (_order(1, False), ALL3, set(), S64_SCHED),
    "gen1_order2_key_tile_64": (_order(2), ALL3, set(), ("hd64_sched_S200_h4_1_B16",)),               # four key blocks: 2 pairs even ones
    "gen1_order0_bit7_clear": (_order(0) & ~(1 << 7), set(), ALL3, S64_SCHED),
    "gen1_fwd_one_tile_dq_two_tiles_per_wave": ((G1 & ~15) | 1 | 2 << 2, ALL3, set(), S64_SCHED),
    "hd128_bit7_clear_order3": (D & ~(1 << 7), {"dkv"}, {"fwd", "dq"}, ("hd128_sched_S129_h8_2_B8",)),
    "hd128_bit7_set_order1": (_order(1, word=D), ALL3, set(), ("hd128_sched_S129_h8_2_B8",)),
    "hd128_per_head_order0": (_order(0, word=D | 1 << 14), {"fwd", "dq"}, {"dkv"}, ("hd128_sched_S129_h8_2_B8",)),
}
SCHED_RUNS = [(v, n) for v, t in SCHED_VARIANTS.items() for n in t[3]]


@pytest.mark.parametrize("v,n", SCHED_RUNS, ids=[f"{v}-{n}" for v, n in SCHED_RUNS])
def test_scheduling_switch_where_it_reorders(dev, v, n):
    """First the host: by the restated index arithmetic (A.schedule; the CPU file proves it a bijection) the switch's branch is
    taken and moves workgroups on this case - or, for the plain orders, moves none.  Then every element against the reference."""
    word, moves, stays, _ = SCHED_VARIANTS[v]
    c = A.CASE[n]
    sc = A.schedule(c, word)
    assert set(sc) == ALL3 and all(A.is_bijection(it, *ext) for it, _, ext in sc.values())
    assert all(sc[k][1] > 0 for k in moves) and all(sc[k][1] == 0 for k in stays), {k: x[1] for k, x in sc.items()}
    print(f"SCHED {v} {n} moved " + " ".join(f"{k}={x[1]}/{len(x[0])}" for k, x in sc.items()))
    _check_case(c, word, chain=False, fwd=c.HD == 128 or bool((word >> 8) & 1))


def test_asm_dq_workgroup_walks_more_than_one_query_block(dev):
    """csm_attn64_dq_asm_launch: P = KV B pairs, nq = S / 128 query blocks, levels = min(nq, ceil(256 / P)) workgroups per pair; a
    workgroup walks more than one block iff nq > levels.  P = 128 (levels 2) with nq = 3 - B = 16, KV = 8, H = 32, S = 384: round 0
    gives level 0 block 2 and level 1 block 1; round 1, an odd round, walks the levels in reversed order - level 1 takes block 0
    and level 0 falls off the end (jb < 0: it skips the round).  (P = 256, nq = 2 also has nq > levels, but levels = 1 there: the
    reversed order is the same order and no workgroup skips.)  With and without the table: the rotation is the last step of the
    reference, so one float64 backward per batch row serves both.  The reference is computed batch row by batch row."""
    check, lib = _lib()
    B, S, H, KV, HD = 16, 384, 32, 8, 64
    P, nq = KV * B, S // 128
    levels = min(nq, -(-256 // P))
    assert nq > levels >= 1
    for level, blocks in ((0, [2]), (1, [1, 0])):                    # the walk of the kernel's loop, restated
        jbs = [nq - 1 - (r * levels + (levels - 1 - level if r & 1 else level)) for r in range(-(-nq // levels))]
        assert [j for j in jbs if j >= 0] == blocks
    g = A.seeded(16, 384, 32, 8)
    qkv = torch.randn(B * S, (H + 2 * KV) * HD, generator=g).to(BF16)
    dout = torch.randn(B * S, H * HD, generator=g).to(BF16)
    c1 = A.Case("asm_dq_persistent", 1, S, H, KV, HD, "plain")
    tab = A.rope_table(c1)
    refs = []
    for b in range(B):
        rows = slice(b * S, (b + 1) * S)
        f = A.ref_forward(qkv[rows], 1, S, H, KV, HD)
        refs.append((f.out.to(BF16), f.lse.float()))
    out, lse = torch.cat([r[0] for r in refs]), torch.cat([r[1] for r in refs])
    cB = c1._replace(B=B)
    try:
        lib.csm_set_attn_variant(D | 1 << 12)
        got = {}
        for rope in (False, True):
            dqkv, ws, took = _bwd(cB, qkv.cuda(), out.cuda(), lse.cuda(), dout.cuda(), tab.cuda() if rope else None)
            assert took == 3, "the asm dQ and dK/dV kernels take this shape"
            got[rope] = (dqkv.cpu(), ws)
        for b in range(B):
            rows = slice(b * S, (b + 1) * S)
            bw = A.ref_backward_both(qkv[rows], refs[b][0], refs[b][1], dout[rows], 1, S, H, KV, HD, tab)
            for rope in (False, True):
                dqkv, ws = got[rope]
                _judge_bwd("attn.asm_dq_persistent+asm_dkv" + (".rope" if rope else ""), c1, D | 1 << 12, dqkv[rows], ws[:, b:b + 1], bw[rope], refs[b][1],
                           f"row {b}")
    finally:
        lib.csm_set_attn_variant(0)


# ------------------------------------------------------------------------------------------------------------- append
KS = 2                                                            # attn_append_kernel<REP, 2>: key blocks of 64 dealt to two splits
S_MAX, GUARD = 256, 3.0                                           # the guard value is exact in bf16


def _append_problem(H, KV, pos0, n, seed):
    g = A.seeded(seed, H, KV, pos0, n)
    qkv = torch.randn(n, (H + 2 * KV) * 64, generator=g).to(BF16)
    kc, vc = torch.full((KV, S_MAX, 64), GUARD, dtype=BF16), torch.full((KV, S_MAX, 64), GUARD, dtype=BF16)
    kc[:, :pos0], vc[:, :pos0] = torch.randn(KV, pos0, 64, generator=g).to(BF16), torch.randn(KV, pos0, 64, generator=g).to(BF16)
    return qkv, kc, vc


APPEND_N, APPEND_HEADS = (1, 15, 16, 17, 64, 65), ((4, 1), (4, 2), (2, 2))


@pytest.mark.parametrize("H,KV", APPEND_HEADS)
@pytest.mark.parametrize("n", APPEND_N)
def test_append(dev, n, H, KV):
    """csm_attn_append: n new positions from pos0 in 0, 1, 63, 64, 65 and S_max - n, in batch row 1 of three; the output by the
    forward bound, the cache rows bit for bit, the guard beyond them and the other batch rows untouched.  pos0 + n > 64 KS / 2
    reaches the second key split (every pos0 >= 63 here; S_max - n walks four blocks)."""
    check, lib = _lib()
    for pos0 in (0, 1, 63, 64, 65, S_MAX - n):
        qkv, kc, vc = _append_problem(H, KV, pos0, n, 1)
        ref = A.ref_append(qkv, kc, vc, pos0, n, H, KV)
        kd, vd = torch.full((3, KV, S_MAX, 64), GUARD, dtype=BF16).cuda(), torch.full((3, KV, S_MAX, 64), GUARD, dtype=BF16).cuda()
        kd[1], vd[1] = kc.cuda(), vc.cuda()
        out = _nan(n, H * 64)
        check(lib.csm_attn_append(qkv.cuda().data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), 1, pos0, n, H, KV, 64, S_MAX, 0.125, _s()),
              "csm_attn_append")
        w = A.judge("attn.append.out", out, ref.out, ref.out_slack)
        print(f"RATIO attn.append {w:.4f} H={H} KV={KV} pos0={pos0} n={n} blocks={(pos0 + n - 1) // 64 + 1} splits={KS}")
        kd, vd = kd.cpu(), vd.cpu()
        assert torch.equal(kd[1], ref.kcache) and torch.equal(vd[1], ref.vcache), "cache rows: bit for bit, nothing else touched"
        assert bool((kd[0] == GUARD).all() and (kd[2] == GUARD).all() and (vd[0] == GUARD).all() and (vd[2] == GUARD).all())


def _append_rows_plan(R):
    """The launches of R segments each, as (n, pos0) per segment.  R = 1 and 2: six and three launches that walk the six pos0 edges
    0, 1, 63, 64, 65, S_max - n in turn, n one or two places ahead; R = 16: one launch, n cycling and pos0 advancing one edge
    further every six segments - sixteen different pairs.  Every edge occurs for every R, S_max - n in multi-segment launches too."""
    edge = lambda k, n: (0, 1, 63, 64, 65, S_MAX - n)[k]          # noqa: E731
    if R == 16:
        idx = [(r % 6, (r + r // 6) % 6) for r in range(R)]
        return [[(APPEND_N[a], edge(k, APPEND_N[a])) for a, k in idx]]
    return [[(APPEND_N[(g + R) % 6], edge(g, APPEND_N[(g + R) % 6])) for g in range(L * R, L * R + R)] for L in range(6 // R)]


def test_append_rows_plan_holds_every_edge():
    for R in (1, 2, 16):
        plan = _append_rows_plan(R)
        assert all(len(launch) == R for launch in plan)
        segs = [s for launch in plan for s in launch]
        assert {n for n, _ in segs} == set(APPEND_N) and {p for _, p in segs} >= {0, 1, 63, 64, 65}
        assert any(p + n == S_MAX for n, p in segs) and len(set(segs)) == len(segs)
        assert all(p + n <= S_MAX for n, p in segs)               # nothing is written past the cache


@pytest.mark.parametrize("H,KV", APPEND_HEADS)
@pytest.mark.parametrize("R", (1, 2, 16))
def test_append_rows(dev, R, H, KV):
    """csm_attn_append_rows: launches of R segments, each segment against its own cache row (rows in a scrambled order), over all
    six pos0 edges of test_append and every n (_append_rows_plan); the end of the cache (pos0 + n = S_max) is reached for every R."""
    check, lib = _lib()
    worst, seen = 0.0, []
    for L, launch in enumerate(_append_rows_plan(R)):
        ns, pos0s = [n for n, _ in launch], [p for _, p in launch]
        rows = [(5 * r + 3 + L) % 17 for r in range(R)]           # distinct rows of 17
        probs = [_append_problem(H, KV, pos0s[r], ns[r], 2 + r + 16 * L) for r in range(R)]
        kd, vd = torch.full((17, KV, S_MAX, 64), GUARD, dtype=BF16), torch.full((17, KV, S_MAX, 64), GUARD, dtype=BF16)
        for r in range(R):
            kd[rows[r]], vd[rows[r]] = probs[r][1], probs[r][2]
        want_k, want_v = kd.clone(), vd.clone()
        kd, vd = kd.cuda(), vd.cuda()
        qkv = torch.cat([p[0] for p in probs]).cuda()
        out = _nan(sum(ns), H * 64)
        arr = ctypes.c_int * R
        check(lib.csm_attn_append_rows(qkv.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), arr(*rows), arr(*pos0s), arr(*ns), R, H, KV, 64,
                                       S_MAX, 0.125, _s()), "csm_attn_append_rows")
        out, off = out.cpu(), 0
        for r in range(R):
            ref = A.ref_append(*probs[r], pos0s[r], ns[r], H, KV)
            worst = max(worst, A.judge("attn.append_rows.out", out[off:off + ns[r]], ref.out, ref.out_slack))
            want_k[rows[r]], want_v[rows[r]] = ref.kcache, ref.vcache
            off += ns[r]
        seen += launch
        assert torch.equal(kd.cpu(), want_k) and torch.equal(vd.cpu(), want_v), "cache rows: bit for bit, nothing else touched"
    print(f"RATIO attn.append_rows {worst:.4f} H={H} KV={KV} R={R} (n, pos0)={seen}")


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(dev):
    """Every CSM_REQUIRE of check_attn, csm_attn_fwd, csm_attn_bwd and csm_attn_bwd_rope returns 1 with its message; none launches."""
    _, lib = _lib()
    B, S, H, KV, HD = 1, 16, 4, 2, 64
    qkv, out, lse = _nan(B * S, (H + 2 * KV) * HD), _nan(B * S, H * HD), _nan(B, H, S, dtype=F32)
    dout, dqkv, ws, tab = _nan(B * S, H * HD), _nan(B * S, (H + 2 * KV) * HD), _nan(2, B, H, S, dtype=F32), _nan(S, HD // 2, 2, dtype=F32)
    P = dict(qkv=qkv.data_ptr(), out=out.data_ptr(), lse=lse.data_ptr(), dout=dout.data_ptr(), dqkv=dqkv.data_ptr(), ws=ws.data_ptr(), tab=tab.data_ptr())

    def fwd(B=B, S=S, H=H, KV=KV, HD=HD, **p):
        a = {**P, **p}
        return lib.csm_attn_fwd(a["qkv"], a["out"], a["lse"], B, S, H, KV, HD, _s())

    def bwd(B=B, S=S, H=H, KV=KV, HD=HD, rope=False, **p):
        a = {**P, **p}
        if rope:
            return lib.csm_attn_bwd_rope(a["qkv"], a["out"], a["dout"], a["lse"], a["dqkv"], a["ws"], a["tab"], B, S, H, KV, HD, _s())
        return lib.csm_attn_bwd(a["qkv"], a["out"], a["dout"], a["lse"], a["dqkv"], a["ws"], B, S, H, KV, HD, _s())

    def refused(rc, text):
        assert rc == 1 and text in lib.csm_last_error(), (rc, lib.csm_last_error())

    for name, f in ((b"csm_attn_fwd", fwd), (b"csm_attn_bwd", bwd), (b"csm_attn_bwd", lambda **k: bwd(rope=True, **k))):
        for bad in (dict(B=0), dict(B=-1), dict(S=0), dict(H=0), dict(KV=0), dict(H=4, KV=3)):
            refused(f(**bad), name + b": bad shape")
        for hd in (32, 96, 256):
            refused(f(HD=hd), name + b": head_dim " + str(hd).encode() + b" unsupported (64 or 128)")
    for k in ("qkv", "out", "lse"):
        refused(fwd(**{k: None}), b"csm_attn_fwd: null pointer")
    for k in ("qkv", "out", "dout", "lse", "dqkv", "ws"):
        refused(bwd(**{k: None}), b"csm_attn_bwd: null pointer")
        refused(bwd(rope=True, **{k: None}), b"csm_attn_bwd: null pointer")
    refused(bwd(rope=True, tab=None), b"csm_attn_bwd_rope: null table")
    torch.cuda.synchronize()
    for t in (out, lse, dqkv, ws):
        assert bool(torch.isnan(t).all()), "a refused call launched something"
