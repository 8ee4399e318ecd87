"""A float64 reference of the training attention kernels (csrc/attention.hip, attention64.hip, attention64_asm.hip: csm_attn_fwd,
csm_attn_bwd, csm_attn_bwd_rope, csm_attn_append, csm_attn_append_rows), a rounding-error bound for every output element and the
seeded cases the two train-attention tests share.  test_train_attn_ref_cpu.py proves this module against torch's own float64
machinery, proves that correct fp32 / bf16 restatements of the kernels' numeric schemes fit the bounds and that wrong ones do
not; test_train_attn_kernels_gpu.py judges the kernels by it.

Everything is plain torch on the CPU in float64, seeded, the same on every machine.  The inputs are the kernels' own operands
(the bf16 fused rows [B*S, (H + 2 KV) HD], the bf16 out / dout, the fp32 lse, the fp32 RoPE table) cast to float64.  q head h uses
kv head h // (H / KV); key j is visible to query i iff j <= i; scale = 1 / sqrt(HD).

The backward is written to the kernels' contract, not to autograd's: from a GIVEN out and lse,
    p_ij = exp(s_ij scale - lse_i), delta_i = sum_d dO_id out_id, dS = p (dP - delta), dP = dO V^T,
    dQ = scale dS K, dK = scale sum_{heads of the group} dS^T Q, dV = sum_{heads of the group} P^T dO,
and with a table the transposed interleaved-pair rotation (g0 c + g1 s, g1 c - g0 s) on dQ and dK before rounding; dV is left.

The judge is ``train_ops_ref.judge``: EVERY element, |got - ref| <= bound, the worst element reported as (index, got, reference,
bound, ratio); a NaN or an infinity anywhere fails.  For a bf16 output bound = hulp(|ref| + slack) + slack, hulp(v) = half a bf16
ulp at v <= 2^-8 v (the output's own rounding); for an fp32 output bound = slack.  The functions below return ``slack``.

Bounds.  U = 2^-24 (fp32), B8 = 2^-8 (bf16: |round(x) - x| <= half an ulp <= 2^-8 |x|).  None is fitted to a kernel's output.
(The bf16 rounding of P and dS is B8 = 2^-8 per term, the unit roundoff of an 8-bit significand, not 2^-9: 2^-9 is only the mean
over a binade.  The worst case is a value just above a power of two - p = 0.53 rounds with an error of up to 2^-9 / 0.53 - and a
correct kernel reaches it on a row of two keys.)
  score         s~_ij = sum_d q_id k_jd by fp32 MFMA: the products of two bf16 are exact, HD additions:
                |s~ - s| <= (HD + 2) U sum_d |q_id k_jd| =: es_ij (unscaled).
  exponential   forward  p~_ij = exp2(fma(s~, c2, -m c2)), c2 = fl(scale log2 e), m the running max of the row;
                backward p~_ij = exp2(fma(s~, c2, -fl(lse log2 e))).
                Error of the exponent in natural units: scale es_ij (score; in the forward twice, m is a score as well)
                + U (2 |s_ij| scale + 3 |c_i| + |x_ij|), c = m scale (forward: <= max_j |s_ij| scale, any running max) or lse
                (backward), x = the exponent: the roundings of c2, of the product c log2 e and of the fma.
                + raw v_exp_f32: documented accuracy 1 ulp (CDNA ISA: V_EXP_F32), taken with a 4x margin: 4 ulp = 8 U of the value.
                This whole term sits about 2^13 below the bf16 terms (8 U = 2^-21 against 2^-8), so the margin cannot hide anything.
                A result below 2^-126 is flushed to 0 (no denormal fix-up): TINY = 2^-126 absolute per key.
                Together: eps_ij (relative) and TINY (absolute).
  rescale       each key block whose maximum moves multiplies l and O by alpha = exp2((m_old - m_new) c2): 8 U + 6 U max|s| scale
                per block, nkb_i = i / 64 + 1 blocks at most (+ 2 for the append kernel's combination of its key splits): er_i.
  chain         L fp32 additions over terms t err by at most (L + 2) U sum |t|.  Forward / dQ: the visible keys of the row,
                i + 1 (masked keys add exact zeros), + 2 per key block (the MFMA's own partial sums and the join of the lanes).
                dK / dV of key j: rep (S - j) queries, + 8 (the join of the waves / parities / heads through LDS).
  out_id        = sum_j e_ij v_jd / l_i, e = exp((s - m) scale), l = sum_j e_ij.
                  numerator: e_ij rounded to bf16 before the PV MFMA (frag_from_acc / pack8f), relative to the running max of its
                  block and rescaled afterwards, which only shrinks the error: <= B8 e_ij |v_jd|            -> B8 AV_id
                  (AV_id = sum_j p_ij |v_jd|: the absolute sum ref_forward returns);
                  denominator: the second generation sums l from the bf16-ROUNDED P through an all-ones MFMA operand: relative
                  B8; the first generation sums the fp32 P: relative el_i = sum_j p_ij eps_ij + chain.  The bound carries both:
                  |out| (B8 + el_i) - the B8 there is the term that covers the difference between the generations;
                  fp32: sum_j p_ij eps_ij |v_jd| + (er_i + chain_i U) (AV_id + |out_id|) + TINY sum_{j<=i} |v_jd|.
  lse_i         = m scale + logf(l):  -log(1 - B8) (l of the second generation from bf16 P: the same covering term; the first
                generation does not need it) + el_i + er_i + A_log 2 U |log l| (logf: ``codec_ref.allowance``) + 2 U (|m scale| +
                |log l| + |lse|) (the product, logf's argument, the sum) + (i + 1) TINY.  Invariant to WHICH maximum the kernel holds.
  delta_i       sum of HD exact products, HD + 6 additions (lanes joined by permlane swaps): (HD + 8) U sum_d |dO_id out_id|.
  dS_ij         what enters the second MFMA is bf16(p~ (dP~ - delta~)):
                  G_ij = B8 |dS_ij| + p_ij ((HD + 4) U (sum_d |dO_id v_jd| + sum_d |dO_id out_id|) + 2 U (|dP_ij| + |delta_i|))
                         + eps_ij |dS_ij| + TINY (|dP_ij| + |delta_i|).
                ABSOLUTE, through the absolute sums: dP - delta cancels, so dS - and a whole dQ row - may be near zero while its
                inputs are not.  Where dO_i = 0 every term is 0: the dQ row must be exactly zero.
  dQ_id         scale sum_j G_ij |k_jd| + (chain_i + 2) U scale sum_j |dS_ij| |k_jd| + 2 U |dQ_id|.
  dK_jd         the same over the queries i >= j and the heads of the group, chain rep (S - j) + 8.
  dV_jd         P rounded to bf16: sum (B8 + eps_ij) p_ij |dO_id| + TINY sum |dO_id| + (chain + 2) U sum p_ij |dO_id|.
  RoPE^T        on the fp32 values before the rounding: (g0 c + g1 s, g1 c - g0 s): |c| b0 + |s| b1 + 3 U (|g0 c| + |g1 s|) and
                likewise, b the bounds of the two members of the pair.
  append        the first generation's scheme (bf16 P, fp32 l) per key split, the splits combined in fp32: the forward bound with
                two more rescales.  The cache rows are copies: bit for bit, and nothing else in the caches may change."""
import math
from collections import namedtuple

import numpy as np
import torch

from codec_ref import allowance
from train_ops_ref import TINY, U, hulp, judge, utilisation      # noqa: F401  (re-exported for the two tests)

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
B8 = 2.0 ** -8
EXP_ALLOW = 8 * U                                                 # v_exp_f32: 1 ulp documented, 4x margin
LOG2E32 = 1.4426950408889634
DEFAULT_WORD = 2 | (1 << 2) | (3 << 4) | (1 << 6) | (1 << 7)      # what csm_set_attn_variant(0) stands for

Fwd = namedtuple("Fwd", "out lse p absv out_slack lse_slack")
Bwd = namedtuple("Bwd", "dqkv delta dqkv_slack delta_slack")
App = namedtuple("App", "out out_slack kcache vcache")


def split_heads(qkv, B, S, H, KV, HD):
    """The fused rows -> q [B, H, S, HD], k and v [B, KV, S, HD] in float64."""
    x = qkv.double().reshape(B, S, H + 2 * KV, HD).permute(0, 2, 1, 3)
    return x[:, :H], x[:, H:H + KV], x[:, H + KV:]


def _rows(x):                                                     # [B, heads, S, HD] -> [B*S, heads*HD]
    B, Hh, S, HD = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * S, Hh * HD)


def _attend(q, k, v, qpos, extra_rescales=0):
    """One sequence.  q [H, n, HD] at positions ``qpos`` [n] against k / v [KV, T, HD] (key j at position j).
    -> out [H, n, HD], lse [H, n], p [H, n, T], absv, out_slack, lse_slack."""
    H, n, HD = q.shape
    KV, T, _ = k.shape
    rep, scale = H // KV, 1.0 / math.sqrt(HD)
    kx, vx = k.repeat_interleave(rep, 0), v.repeat_interleave(rep, 0)
    vis = torch.arange(T)[None, :] <= qpos[:, None]               # [n, T]
    s = (q @ kx.transpose(1, 2)) * scale
    sm = s.masked_fill(~vis, float("-inf"))
    m = sm.amax(-1)
    e = torch.exp(sm - m[..., None])
    l = e.sum(-1)
    p = e / l[..., None]
    out, absv = p @ vx, p @ vx.abs()
    logl = torch.log(l)
    lse = m + logl
    # fp32 terms
    es = (HD + 2) * U * (q.abs() @ kx.abs().transpose(1, 2)) * scale
    smax = s.abs().masked_fill(~vis, 0.0).amax(-1)
    x = (sm - m[..., None]).masked_fill(~vis, 0.0).abs()
    eps = (es + es.masked_fill(~vis, 0.0).amax(-1, keepdim=True) + U * (2 * s.abs() + 3 * smax[..., None] + x) + EXP_ALLOW).masked_fill(~vis, 0.0)
    nvis = (qpos + 1).double()[None, :]
    nkb = (qpos // 64 + 1 + extra_rescales).double()[None, :]
    er = nkb * (8 * U + 6 * U * smax)
    chain = (nvis + 2 * nkb + 2) * U
    w = p * eps
    el = w.sum(-1) + chain
    vcum = (vx.abs().cumsum(1))[:, qpos.clamp(max=T - 1)]        # sum_{j <= pos_i} |v_jd|
    out_slack = B8 * absv + out.abs() * (B8 + el)[..., None] + w @ vx.abs() + (er + chain)[..., None] * (absv + out.abs()) + TINY * vcum
    a_log = allowance("logf", l.float())
    lse_slack = -math.log1p(-B8) + el + er + a_log * 2 * U * logl.abs() + 2 * U * (m.abs() + logl.abs() + lse.abs()) + nvis * TINY
    return out, lse, p, absv, out_slack, lse_slack


def ref_forward(qkv, B, S, H, KV, HD):
    """-> Fwd: out / absv / out_slack [B*S, H*HD], lse / lse_slack [B, H, S], p [B, H, S, S] (float64)."""
    q, k, v = split_heads(qkv, B, S, H, KV, HD)
    pos = torch.arange(S)
    r = [_attend(q[b], k[b], v[b], pos) for b in range(B)]
    st = lambda i: torch.stack([x[i] for x in r])                 # noqa: E731
    return Fwd(_rows(st(0)), st(1), st(2), _rows(st(3)), _rows(st(4)), st(5))


def _unrope(val, slack, table, S, HD):
    """The transposed rotation on [..., S, HD] float64 values and their bounds."""
    t = table.double()[:S]
    c, s = t[:, :, 0], t[:, :, 1]                                 # [S, HD/2]
    g, b = val.reshape(*val.shape[:-1], HD // 2, 2), slack.reshape(*slack.shape[:-1], HD // 2, 2)
    g0, g1, b0, b1 = g[..., 0], g[..., 1], b[..., 0], b[..., 1]
    o = torch.stack([g0 * c + g1 * s, g1 * c - g0 * s], -1)
    ob = torch.stack([c.abs() * b0 + s.abs() * b1 + 3 * U * ((g0 * c).abs() + (g1 * s).abs()),
                      c.abs() * b1 + s.abs() * b0 + 3 * U * ((g1 * c).abs() + (g0 * s).abs())], -1)
    return o.reshape(val.shape), ob.reshape(val.shape)


def _backward(qkv, out_given, lse_given, dout, B, S, H, KV, HD):
    """The backward before the rotation, in the [B, heads, S, HD] layout: values and slacks of dQ, dK, dV, then delta's."""
    q, k, v = split_heads(qkv, B, S, H, KV, HD)
    rep, scale = H // KV, 1.0 / math.sqrt(HD)
    dO = dout.double().reshape(B, S, H, HD).permute(0, 2, 1, 3)
    og = out_given.double().reshape(B, S, H, HD).permute(0, 2, 1, 3)
    lse = lse_given.double()
    kx, vx = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)
    vis = torch.tril(torch.ones(S, S, dtype=torch.bool))
    s = (q @ kx.transpose(2, 3)) * scale
    x = (s - lse[..., None]).masked_fill(~vis, float("-inf"))
    p = torch.exp(x)
    delta, dabs = (dO * og).sum(-1), (dO * og).abs().sum(-1)
    dP, dPabs = dO @ vx.transpose(2, 3), dO.abs() @ vx.abs().transpose(2, 3)
    dS = p * (dP - delta[..., None])
    eps = ((HD + 2) * U * scale * (q.abs() @ kx.abs().transpose(2, 3)) + U * (2 * s.abs() + 3 * lse.abs()[..., None] + x.masked_fill(~vis, 0.0).abs())
           + EXP_ALLOW).masked_fill(~vis, 0.0)
    span = (dP.abs() + delta.abs()[..., None]).masked_fill(~vis, 0.0)
    G = B8 * dS.abs() + p * ((HD + 4) * U * (dPabs + dabs[..., None]) + 2 * U * span) + eps * dS.abs() + TINY * span
    Gp = (B8 + eps) * p
    qi = torch.arange(S).double()
    chain_q = ((qi + 1) + 2 * (torch.arange(S) // 64 + 1) + 4) * U                   # [S] queries
    chain_k = (rep * (S - qi) + 8 + 2) * U                                          # [S] keys
    grp = lambda t: t.reshape(B, KV, rep, S, HD).sum(2)                              # noqa: E731
    dQ = scale * (dS @ kx)
    dQs = scale * (G @ kx.abs()) + chain_q[:, None] * scale * (dS.abs() @ kx.abs()) + 2 * U * dQ.abs()
    dK = scale * grp(dS.transpose(2, 3) @ q)
    dKs = scale * grp(G.transpose(2, 3) @ q.abs()) + chain_k[:, None] * scale * grp(dS.abs().transpose(2, 3) @ q.abs()) + 2 * U * dK.abs()
    dV = grp(p.transpose(2, 3) @ dO)
    dVs = grp(Gp.transpose(2, 3) @ dO.abs()) + chain_k[:, None] * grp(p.transpose(2, 3) @ dO.abs()) + TINY * grp(vis.double().t() @ dO.abs())
    return dQ, dQs, dK, dKs, dV, dVs, delta, (HD + 8) * U * dabs


def _finish(t, rope_table, S, HD):
    dQ, dQs, dK, dKs, dV, dVs, delta, delta_slack = t
    if rope_table is not None:
        dQ, dQs = _unrope(dQ, dQs, rope_table, S, HD)
        dK, dKs = _unrope(dK, dKs, rope_table, S, HD)
    return Bwd(torch.cat([_rows(dQ), _rows(dK), _rows(dV)], 1), delta, torch.cat([_rows(dQs), _rows(dKs), _rows(dVs)], 1), delta_slack)


def ref_backward(qkv, out_given, lse_given, dout, B, S, H, KV, HD, rope_table=None):
    """-> Bwd: dqkv / dqkv_slack [B*S, (H + 2 KV) HD] (dQ | dK | dV), delta / delta_slack [B, H, S]."""
    return _finish(_backward(qkv, out_given, lse_given, dout, B, S, H, KV, HD), rope_table, S, HD)


def ref_backward_both(qkv, out_given, lse_given, dout, B, S, H, KV, HD, rope_table):
    """-> {False: the Bwd without the table, True: the Bwd with it}: the rotation is the last step, so one backward serves both."""
    t = _backward(qkv, out_given, lse_given, dout, B, S, H, KV, HD)
    return {False: _finish(t, None, S, HD), True: _finish(t, rope_table, S, HD)}


def ref_append(qkv_new, kcache, vcache, pos0, n, H, KV, HD=64):
    """By the contract above attn_append_kernel: the n rows of ``qkv_new`` are positions pos0 .. pos0+n-1 of ONE sequence whose
    earlier keys / values are rows 0 .. pos0-1 of kcache / vcache [KV, S_max, HD] (bf16).  -> App: out / out_slack [n, H*HD] and
    the caches as they must stand afterwards (rows pos0 .. pos0+n-1 replaced by the new rows' bits, nothing else touched)."""
    x = qkv_new.reshape(n, H + 2 * KV, HD).permute(1, 0, 2)
    kc, vc = kcache.clone(), vcache.clone()
    kc[:, pos0:pos0 + n], vc[:, pos0:pos0 + n] = x[H:H + KV], x[H + KV:]
    r = _attend(x[:H].double(), kc[:, :pos0 + n].double(), vc[:, :pos0 + n].double(), pos0 + torch.arange(n), extra_rescales=2)
    flat = lambda t: t.permute(1, 0, 2).reshape(n, H * HD)          # noqa: E731
    return App(flat(r[0]), flat(r[4]), kc, vc)


# ------------------------------------------------------------------------------------------------------------- cases
Case = namedtuple("Case", "name B S H KV HD kind")
S64 = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 200, 256, 257, 320, 384)
HEADS64 = ((4, 1), (8, 2), (4, 2), (2, 2), (8, 1))
# (query, key) of the spike cases: the dominant key in the first key block, in the last one, on the diagonal, at a block's first
# and last row, and late in the sequence (the running maximum moves in the last block: the rescale path)
SPIKES = {320: ((300, 5), (310, 290), (200, 200), (128, 128), (127, 127), (255, 192), (256, 255), (319, 318), (64, 63), (63, 0), (191, 129)),
          100: ((90, 3), (99, 98), (70, 70), (64, 64), (63, 63), (80, 65), (31, 16))}


def _cases():
    cs = []
    for i, S in enumerate(S64):                                   # every length, heads and batch cycling against it
        H, KV = HEADS64[i % 5]
        cs.append(Case(f"hd64_S{S}_h{H}_{KV}_B{1 + i % 3}", 1 + i % 3, S, H, KV, 64, "rand"))
    for j, (H, KV) in enumerate(HEADS64):                         # every head layout at a ragged and at an asm-eligible length
        cs.append(Case(f"hd64_S129_h{H}_{KV}_B{1 + (j + 1) % 3}", 1 + (j + 1) % 3, 129, H, KV, 64, "rand"))
        cs.append(Case(f"hd64_S192_h{H}_{KV}_B{1 + (j + 2) % 3}", 1 + (j + 2) % 3, 192, H, KV, 64, "rand"))
    cs = list(dict.fromkeys(cs))                                  # (4,2) at S = 129, B = 1 is in both loops: once
    cs += [Case("hd64_S256_h4_1_B3", 3, 256, 4, 1, 64, "rand"), Case("hd64_S384_h8_2_B1", 1, 384, 8, 2, 64, "rand"),
           Case("hd64_S64_h4_1_B1", 1, 64, 4, 1, 64, "rand"), Case("hd64_S128_h8_2_B2", 2, 128, 8, 2, 64, "rand")]
    cs += [Case(f"hd128_S{S}_h8_2_B{1 + i % 3}", 1 + i % 3, S, 8, 2, 128, "rand") for i, S in enumerate((1, 16, 17, 31, 32, 33))]
    cs += [Case("hd128_S32_h4_2_B2", 2, 32, 4, 2, 128, "rand"), Case("hd128_S32_h2_1_B3", 3, 32, 2, 1, 128, "rand")]
    cs += [Case(f"hd128_S{S}_h{H}_{KV}_B{B}", B, S, H, KV, 128, "rand") for S, H, KV, B in ((64, 8, 2, 1), (65, 4, 2, 2), (100, 2, 1, 3), (129, 8, 2, 1))]
    cs += [Case("hd64_spike_S320_h4_1_B2", 2, 320, 4, 1, 64, "spike"), Case("hd64_spike_S320_h4_2_B1", 1, 320, 4, 2, 64, "spike"),
           Case("hd128_spike_S100_h8_2_B1", 1, 100, 8, 2, 128, "spike"),
           Case("hd64_big_S200_h8_2_B1", 1, 200, 8, 2, 64, "big"), Case("hd64_big_S256_h4_1_B1", 1, 256, 4, 1, 64, "big"),
           Case("hd128_big_S33_h8_2_B2", 2, 33, 8, 2, 128, "big")]
    return cs + list(SCHED)


# KV B = 16 (batch, kv head) pairs: every XCD's run of workgroups holds two whole pairs, which is what the work orders' own
# conditions ask before they reorder anything (``schedule`` below; training runs KV B = 32).  With fewer pairs than 16 every
# reordering branch of attn_q_kernel, attn_dkv_kernel, work_item and attn64_dkv_kernel is skipped or moves nothing.  Key blocks
# per pair of the 64- / 128-key dK/dV tile: 3 / 2 (ragged), 4 / 2 (ragged, even: order 2 pairs blocks), 5 / 3 (both odd).
SCHED = (Case("hd64_sched_S129_h8_2_B8", 8, 129, 8, 2, 64, "rand"), Case("hd64_sched_S200_h4_1_B16", 16, 200, 4, 1, 64, "rand"),
         Case("hd64_sched_S320_h2_2_B8", 8, 320, 2, 2, 64, "rand"), Case("hd128_sched_S129_h8_2_B8", 8, 129, 8, 2, 128, "rand"))


CASES = _cases()
CASE = {c.name: c for c in CASES}


def seeded(*xs):
    """A generator seeded by the given integers alone."""
    s = 4242
    for x in xs:
        s = (s * 1000003 + int(x)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def inputs(c):
    """-> dict(qkv, dout) bf16, different data in every batch row.  Every 'rand' case with S >= 3 carries one all-zero dout row
    (batch row 0, position S // 2, every head: its dQ row must be exactly zero) and one all-zero query row (batch row 0, position
    S // 3, head 0: uniform probabilities)."""
    g = seeded(c.B, c.S, c.H, c.KV, c.HD, len(c.kind))
    W = (c.H + 2 * c.KV) * c.HD
    amp = {"rand": 1.0, "spike": 0.5, "big": 4.0}[c.kind]        # 'big': scores with a standard deviation of 16
    qkv = torch.randn(c.B * c.S, W, generator=g) * amp
    if c.kind == "big":
        qkv[:, (c.H + c.KV) * c.HD:] /= amp
    dout = torch.randn(c.B * c.S, c.H * c.HD, generator=g)
    if c.kind == "spike":
        for b in range(c.B):
            for (i, j) in SPIKES[c.S]:
                for h in range(c.H):                              # every head of the group looks at the same key, with the key's signs
                    kvh = h // (c.H // c.KV)
                    sg = torch.where(torch.rand(c.HD, generator=seeded(7, i, j, kvh)) < 0.5, -4.0, 4.0)
                    qkv[b * c.S + i, h * c.HD:(h + 1) * c.HD] = sg
                    qkv[b * c.S + j, (c.H + kvh) * c.HD:(c.H + kvh + 1) * c.HD] = sg
    elif c.kind == "rand" and c.S >= 3:
        dout[c.S // 2] = 0
        qkv[c.S // 3, :c.HD] = 0
    return dict(qkv=qkv.to(BF16), dout=dout.to(BF16))


def rope_table(c):
    from oracle.csm_oracle import rope_table as rt
    return rt(c.S, c.HD).contiguous()


def grids(c):
    """Workgroup counts of the default kernels of a case (the XCD remap and its lpt condition depend on them modulo 8)."""
    if c.HD == 64:
        return {"fwd": -(-c.S // 128) * c.H * c.B, "dkv": -(-c.S // 64) * c.KV * c.B}
    grp = c.S <= 32 and c.H == 4 * c.KV
    return {"fwd": c.KV * c.B if grp else -(-c.S // 64) * c.H * c.B, "dkv": -(-c.S // 64) * c.KV * c.B}


def expected_kernels(c, word=0):
    """What csm_attn_last_dkv_kernel() must answer after a backward of this case under the variant word (bit 0: asm dK/dV,
    bit 1: asm dQ), from the dispatch of attn_bwd_impl and the two asm launchers."""
    if word == 0:
        word = DEFAULT_WORD
    if c.HD != 64 or (word >> 8) & 2 or c.H != 4 * c.KV:
        return 0
    dkv = int(not (word >> 10) & 1 and c.S % 64 == 0 and c.S >= 64)
    dq = int((word >> 12) & 1 and c.S % 128 == 0 and c.S >= 128)
    return dkv | dq << 1


# ------------------------------------------------------------------------------------------------------------- work orders
def xcd_runs(T):
    """Workgroup ids are dealt round-robin over the 8 XCDs; the kernels hand XCD x the contiguous run of work items
    base .. base + run - 1.  -> per workgroup: its work item nid, its place ``within`` the run, the run's length and base."""
    wg = np.arange(T)
    xcd, within = wg & 7, wg >> 3
    q8, r8 = T >> 3, T & 7
    nid = np.where(xcd < r8, xcd * (q8 + 1), r8 * (q8 + 1) + (xcd - r8) * q8) + within
    return nid, within, np.where(xcd < r8, q8 + 1, q8), nid - within


def q_work_order(P, nblk, rep, lpt=True):
    """The index arithmetic of attn_q_kernel (attention.hip) and work_item (attention64.hip; lpt always) for P (batch, kv head)
    pairs, rep query heads per pair and nblk query blocks per head, restated.  -> (pair, head of the group, query block) per
    workgroup [T, 3] and the number of workgroups that took the longest-first branch AND got another item by it."""
    per_pair = rep * nblk
    nid, within, run, base = xcd_runs(P * per_pair)
    pair, local = nid // per_pair, nid % per_pair
    take = (run % per_pair == 0) & (base % per_pair == 0) & bool(lpt)
    ncomb = np.maximum(run // per_pair, 1) * rep
    comb = within % ncomb
    pair2, local2 = base // per_pair + comb // rep, (comb % rep) * nblk + within // ncomb
    moved = int((take & ((pair2 != pair) | (local2 != local))).sum())
    pair, local = np.where(take, pair2, pair), np.where(take, local2, local)
    return np.stack([pair, local // nblk, nblk - 1 - local % nblk], 1), moved


def dkv_work_order(P, nkblk, order):
    """The index arithmetic of attn_dkv_kernel (attention.hip; work orders 0..3) and of attn64_dkv_kernel (attention64.hip:
    order 3) for P pairs of nkblk key blocks, restated.  -> (pair, key block) per workgroup [T, 2] and the number of workgroups
    that took the order's branch AND got another item by it."""
    nid, within, run, base = xcd_runs(P * nkblk)
    pair, kblk = nid // nkblk, nid % nkblk
    pair2, kblk2 = pair, kblk
    take = np.zeros(len(nid), dtype=bool)
    if order == 1:
        half = run >> 1
        take = ((run & 1) == 0) & (half % nkblk == 0) & (within >= half)
        kblk2 = nkblk - 1 - kblk
    elif order == 2:
        take = ((nkblk & 1) == 0) & ((nid & 1) == 1)
        kblk2 = nkblk - 1 - (kblk ^ 1)
    elif order == 3:
        take = (run % nkblk == 0) & (base % nkblk == 0)
        npairs = np.maximum(run // nkblk, 1)
        kblk2, pair2 = within // npairs, base // nkblk + within % npairs
    moved = int((take & ((pair2 != pair) | (kblk2 != kblk))).sum())
    return np.stack([np.where(take, pair2, pair), np.where(take, kblk2, kblk)], 1), moved


def is_bijection(items, *extents):
    """Every work item of the grid exactly once."""
    flat = np.ravel_multi_index(tuple(items.T), extents)
    return len(flat) == int(np.prod(extents)) and len(np.unique(flat)) == len(flat)


def schedule(c, word=0):
    """Which work order each kernel of a case walks under the variant word, from the launchers of attention.hip and
    attention64.hip: {"fwd" | "dq" | "dkv": (items, moved, extents)}.  A kernel that has no such order - the grouped head_dim-128
    mapping (one workgroup per pair) and the asm kernels (their own schedules) - is left out."""
    w = word or DEFAULT_WORD
    P, rep, lpt, k = c.KV * c.B, c.H // c.KV, (w >> 7) & 1, expected_kernels(c, word)
    blocks = lambda n: -(-c.S // n)                               # noqa: E731
    out = {}

    def q(name, nblk, lpt):
        items, moved = q_work_order(P, nblk, rep, lpt)
        out[name] = (items, moved, (P, rep, nblk))

    def dkv(nkblk, order):
        items, moved = dkv_work_order(P, nkblk, order)
        out["dkv"] = (items, moved, (P, nkblk))

    if c.HD == 128:
        if not (c.S <= 32 and c.H == 4 * c.KV and not (w >> 14) & 1):
            q("fwd", blocks(64), lpt)
            q("dq", blocks(64), lpt)
        dkv(blocks(64), (w >> 4) & 3)
        return out
    tiles = lambda f: 2 if c.S > 64 and f == 2 else 1             # noqa: E731  query tiles per wave of the first generation
    if (w >> 8) & 1:
        q("fwd", blocks(64 * tiles(w & 3)), lpt)
    else:
        q("fwd", blocks(128), True)
    if (w >> 8) & 2:
        q("dq", blocks(64 * tiles((w >> 2) & 3)), lpt)
        dkv(blocks(64 if (w >> 6) & 1 else 128), (w >> 4) & 3)
    else:
        if not k & 2:
            q("dq", blocks(128), True)
        if not k & 1:
            dkv(blocks(64), 3)
    return out


# ------------------------------------------------------------------------------------------------------------- restatements
def _bf(t):
    return t.to(BF16).float()


def _split32(qkv, B, S, H, KV, HD, kv_mod=False):
    x = qkv.float().reshape(B, S, H + 2 * KV, HD).permute(0, 2, 1, 3)
    q, k, v = x[:, :H], x[:, H:H + KV], x[:, H + KV:]
    idx = torch.arange(H) % KV if kv_mod else torch.arange(H) // (H // KV)
    return q, k[:, idx], v[:, idx]


def _mask(S, T, mut):
    i, j = torch.arange(S)[:, None], torch.arange(T)[None, :]
    if mut == "mask_plus1":
        return j <= i + 1
    if mut == "mask_lt":
        return j < i
    if mut == "mask_tile16":
        return j <= (i | 15)
    return j <= i


FWD_MUTANTS = ("mask_plus1", "mask_lt", "mask_tile16", "kv_mod", "clamp_dup", "lse_no_m", "skip_last_block", "stale_max")
BWD_MUTANTS = ("mask_plus1", "mask_lt", "mask_tile16", "kv_mod", "clamp_dup", "no_scale_dq", "no_scale_dk", "no_delta", "dv_from_ds",
               "rope_fwd", "rope_dv", "drop_head")


def restate_forward(qkv, B, S, H, KV, HD, l_bf16=False, kb=64, mut=None):
    """The kernels' forward in fp32 / bf16: key blocks of ``kb``, online softmax by exp2, P rounded to bf16 for the PV product, l
    summed from the fp32 P (first generation, append) or from the bf16 P (second generation).  -> out bf16, lse fp32."""
    q, k, v = _split32(qkv, B, S, H, KV, HD, mut == "kv_mod")
    T = S
    if mut == "clamp_dup" and S % 16:                             # the clamped copy of row S - 1 leaks into the ragged tail
        k, v, T = torch.cat([k, k[:, :, -1:]], 2), torch.cat([v, v[:, :, -1:]], 2), S + 1
    vis = _mask(S, T, mut)
    if T > S:
        vis[:, S] = False
        vis[S - 1, S] = True
    scale = torch.tensor(1.0 / math.sqrt(HD), dtype=F32)
    c2 = scale * torch.tensor(LOG2E32, dtype=F32)
    s = (q @ k.transpose(2, 3)).masked_fill(~vis, float("-inf"))
    m = torch.full((B, H, S), float("-inf"))
    l, o = torch.zeros(B, H, S), torch.zeros(B, H, S, HD)
    blocks = list(range(0, T, kb))
    if mut == "skip_last_block" and len(blocks) > 1:
        blocks = blocks[:-1]
    for k0 in blocks:
        sb = s[..., k0:k0 + kb]
        m_new = torch.maximum(m, sb.amax(-1))
        m_use = torch.where(torch.isinf(m_new), torch.zeros(()), m_new)
        alpha = torch.exp2((m - m_use) * c2)
        if mut == "stale_max":
            alpha = torch.where(torch.isinf(m), alpha, torch.ones(()))
        p = torch.exp2(sb * c2 - (m_use * c2)[..., None])
        pb = _bf(p)
        l = l * alpha + (pb if l_bf16 else p).sum(-1)
        o = o * alpha[..., None] + pb @ v[:, :, k0:k0 + kb]
        m = m_new
    lse = (0.0 if mut == "lse_no_m" else m * scale) + torch.log(l)
    return _rows((o / l[..., None])).to(BF16), lse


def _rot32(g, table, S, HD, forward):
    t = table[:S]
    c, s = t[:, :, 0], t[:, :, 1] * (-1.0 if forward else 1.0)
    x = g.reshape(*g.shape[:-1], HD // 2, 2)
    return torch.stack([x[..., 0] * c + x[..., 1] * s, x[..., 1] * c - x[..., 0] * s], -1).reshape(g.shape)


def restate_backward(qkv, out_bf16, lse32, dout, B, S, H, KV, HD, rope_table=None, mut=None):
    """The kernels' backward in fp32 / bf16: p by exp2 from the given lse, delta in fp32 from the bf16 out, P and dS rounded to
    bf16 for the second products.  -> dqkv bf16, delta fp32."""
    q, k, v = _split32(qkv, B, S, H, KV, HD, mut == "kv_mod")
    rep = H // KV
    T = S
    if mut == "clamp_dup" and S % 16:
        k, v, T = torch.cat([k, k[:, :, -1:]], 2), torch.cat([v, v[:, :, -1:]], 2), S + 1
    vis = _mask(S, T, mut)
    if T > S:
        vis[:, S] = False
        vis[S - 1, S] = True
    dO = dout.float().reshape(B, S, H, HD).permute(0, 2, 1, 3)
    og = out_bf16.float().reshape(B, S, H, HD).permute(0, 2, 1, 3)
    scale = torch.tensor(1.0 / math.sqrt(HD), dtype=F32)
    c2 = scale * torch.tensor(LOG2E32, dtype=F32)
    nl = -lse32.float() * torch.tensor(LOG2E32, dtype=F32)
    p = torch.exp2((q @ k.transpose(2, 3)) * c2 + nl[..., None]).masked_fill(~vis, 0.0)
    delta = (dO * og).sum(-1)
    dS = p * ((dO @ v.transpose(2, 3)) - (0.0 if mut == "no_delta" else delta[..., None]))
    pb, dsb = _bf(p), _bf(dS)
    dQ = (dsb @ k) * (1.0 if mut == "no_scale_dq" else scale)
    dKh = (dsb.transpose(2, 3) @ q) * (1.0 if mut == "no_scale_dk" else scale)
    dVh = (dsb if mut == "dv_from_ds" else pb).transpose(2, 3) @ dO
    if T > S:                                                     # the leaked copy's gradient lands on row S - 1
        dKh = torch.cat([dKh[:, :, :S - 1], dKh[:, :, S - 1:S] + dKh[:, :, S:]], 2)
        dVh = torch.cat([dVh[:, :, :S - 1], dVh[:, :, S - 1:S] + dVh[:, :, S:]], 2)
    if mut == "drop_head" and rep > 1:
        dKh[:, rep - 1::rep] = 0
        dVh[:, rep - 1::rep] = 0
    if mut == "kv_mod":
        grp = lambda t: torch.stack([t[:, kvh::KV].sum(1) for kvh in range(KV)], 1)          # noqa: E731
    else:
        grp = lambda t: t.reshape(B, KV, rep, S, HD).sum(2)                                  # noqa: E731
    dK, dV = grp(dKh), grp(dVh)
    if rope_table is not None:
        dQ, dK = _rot32(dQ, rope_table, S, HD, mut == "rope_fwd"), _rot32(dK, rope_table, S, HD, mut == "rope_fwd")
        if mut == "rope_dv":
            dV = _rot32(dV, rope_table, S, HD, False)
    return torch.cat([_rows(dQ), _rows(dK), _rows(dV)], 1).to(BF16), delta


def judge_forward(name, out, lse, f, what=""):
    w = max(judge(f"{name}.out", out, f.out, f.out_slack), judge(f"{name}.lse", lse, f.lse, f.lse_slack))
    print(f"RATIO {name} fwd {w:.4f} {what}")
    return w


def judge_backward(name, dqkv, delta, b, c, what=""):
    a, e = c.H * c.HD, (c.H + c.KV) * c.HD
    got = dqkv.detach().cpu()
    w = max(judge(f"{name}.dq", got[:, :a], b.dqkv[:, :a], b.dqkv_slack[:, :a]), judge(f"{name}.dk", got[:, a:e], b.dqkv[:, a:e], b.dqkv_slack[:, a:e]),
            judge(f"{name}.dv", got[:, e:], b.dqkv[:, e:], b.dqkv_slack[:, e:]), judge(f"{name}.delta", delta, b.delta, b.delta_slack))
    print(f"RATIO {name} bwd {w:.4f} {what}")
    return w
