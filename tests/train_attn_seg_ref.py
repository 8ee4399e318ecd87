"""A float64 reference of the segment-masked (packed-row) training attention kernels - csm_attn_fwd_seg and csm_attn_bwd_seg, the SEG
instantiations of attn64_fwd_kernel, attn64_dq_kernel and attn64_dkv_kernel in csrc/attention64.hip - with a rounding-error bound
for every output element, and the seeded cases the two tests share.  test_train_attn_seg_ref_cpu.py proves this module;
test_train_attn_seg_kernels_gpu.py judges the kernels by it.

A packed row holds several segments one after the other; key j is visible to query i iff seg_start[i] <= j <= i.  What is left of
a row after its listed segments is padding and forms one more segment, so the descriptor is total.  Mathematically a packed row IS
its segments run as sequences of their own, so the float64 values and the slacks are those of ``train_attn_ref._attend`` and
``train_attn_ref._backward`` per segment (B = 1, S = the segment's length, positions 0 .. n-1), scattered back into place.  Nothing
else is new, and no bound is fitted to a kernel's output.  The judge is ``train_ops_ref.judge`` (through train_attn_ref's
judge_forward / judge_backward).

One term differs from a sequence run alone: the number of key blocks a query's row is summed over.  The kernels' key blocks of 64
are aligned to the ROW, not to the segment.  A query at local position i of a segment that starts at row position o has its
visible keys at row positions o .. o + i, which lie in the blocks floor(o / 64) .. floor((o + i) / 64): that is
floor((o + i) / 64) - floor(o / 64) + 1 <= floor(i / 64) + 2 blocks, ONE more than the floor(i / 64) + 1 of the segment run alone
(o = 0), and the bound is reached whenever o is no multiple of 64.  Every block count of the bounds therefore takes one more:
  forward   ``extra_rescales = 1`` in _attend: nkb_i = i // 64 + 2 enters the rescale term er_i and the chain (2 per block);
  dQ        chain_q of _backward is (i + 1) + 2 (i // 64 + 1) + 4; one more block adds 2 U scale sum_j |dS_ij| |k_jd| to the slack;
  dK / dV   their chain counts queries and heads (rep (n - j) + 8), not key blocks: unchanged.
Leading tiles that a workgroup walks but that are wholly masked for a row (the row's segment starts later than the workgroup's
first one) add nothing: the row's running maximum stays -inf, the exponent's maximum is held at 0, every exp2 gives an exact 0 and
the rescale multiplies zeros.  So they enter no bound."""
import math
from collections import namedtuple

import torch

import train_attn_ref as A
from train_attn_ref import BF16, F32, HEADS64, U, _rows, seeded    # noqa: F401

SegCase = namedtuple("SegCase", "name B S H KV HD kind layouts")   # layouts: per batch row the lengths of its segments, in order
SPIKE_KEYS = (128, 129)                                            # spike case: last key of segment 0 (hidden), first of segment 1 (seen)


def _mk(tag, S, *layouts, heads, kind="rand"):
    H, KV = heads
    name = f"seg_{tag}_S{S}_h{H}_{KV}_B{len(layouts)}_" + "_".join("x".join(map(str, l)) for l in layouts[:3])
    return SegCase(name, len(layouts), S, H, KV, 64, kind, tuple(tuple(l) for l in layouts))


def _cases():
    raw = [("single", 129, [[129]]), ("single", 200, [[200]]), ("single", 256, [[256]]),
           ("aligned", 384, [[128, 128, 128]]), ("aligned", 384, [[64, 64, 64, 192]]),
           ("off1", 384, [[63, 65, 127, 129]]), ("off1", 384, [[65, 63, 129, 127]]), ("off1", 384, [[31, 33, 1, 319]]),
           ("tiny", 200, [[1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 57]]),
           ("dead", 256, [[10, 90, 28, 128]]),
           ("ring5", 384, [[70, 314]]), ("ring4", 384, [[134, 250]]), ("ring3", 384, [[198, 186]]),
           ("pad", 200, [[90, 61]]), ("ragged", 129, [[128, 1]]), ("ragged", 65, [[64, 1]]), ("ragged", 17, [[5, 12]]),
           ("rows", 256, [[256], [100, 156], [37, 219]])]
    cs = [_mk(tag, S, *lay, heads=HEADS64[i % 5]) for i, (tag, S, lay) in enumerate(raw)]
    cyc = ([128, 1], [129], [5, 12, 112], [64, 65], [63, 1, 65], [1, 128], [33, 31, 64], [100, 20])   # the last one: 9 of padding
    cs.append(_mk("sched", 129, *cyc, heads=(8, 2)))
    cs.append(_mk("spike", 320, [129, 191], heads=(4, 1), kind="spike"))
    return cs


CASES = _cases()
CASE = {c.name: c for c in CASES}
SINGLE = [c for c in CASES if all(l == (c.S,) for l in c.layouts)]
assert len(CASE) == len(CASES)


def segments(c, b):
    """[(start, length)] of batch row b, the padding tail as the last segment."""
    out, o = [], 0
    for n in c.layouts[b]:
        assert n >= 1
        out.append((o, n))
        o += n
    assert o <= c.S
    if o < c.S:
        out.append((o, c.S - o))
    return out


def arrays(c):
    """-> seg_start, seg_end, pos: int32 [B*S] (row-local)."""
    ss, se = torch.empty(c.B, c.S, dtype=torch.int32), torch.empty(c.B, c.S, dtype=torch.int32)
    for b in range(c.B):
        for o, n in segments(c, b):
            ss[b, o:o + n], se[b, o:o + n] = o, o + n - 1
    pos = torch.arange(c.S, dtype=torch.int32)[None] - ss
    return ss.reshape(-1), se.reshape(-1), pos.reshape(-1).contiguous()


def visible(c):
    """[B, S, S] bool: the explicit block-diagonal causal mask."""
    ss, _, _ = arrays(c)
    i, j = torch.arange(c.S)[None, :, None], torch.arange(c.S)[None, None, :]
    return (j <= i) & (j >= ss.reshape(c.B, c.S, 1))


def inputs(c):
    """-> dict(qkv, dout) bf16.  'spike': every query of the second segment, on every head, carries the +-4 sign pattern of the keys
    at SPIKE_KEYS - position 128 is the last key of the FIRST segment and must stay invisible, position 129 is the second
    segment's first key and must be seen."""
    g = seeded(len(c.name), c.B, c.S, c.H, c.KV, sum(map(sum, c.layouts)), len(c.layouts[0]))
    W = (c.H + 2 * c.KV) * c.HD
    qkv = torch.randn(c.B * c.S, W, generator=g) * (0.5 if c.kind == "spike" else 1.0)
    dout = torch.randn(c.B * c.S, c.H * c.HD, generator=g)
    if c.kind == "spike":
        (o0, n0), (o1, n1) = segments(c, 0)[:2]
        assert SPIKE_KEYS == (o1 - 1, o1)
        for kvh in range(c.KV):
            sg = torch.where(torch.rand(c.HD, generator=seeded(7, kvh)) < 0.5, -4.0, 4.0)
            for j in SPIKE_KEYS:
                qkv[j, (c.H + kvh) * c.HD:(c.H + kvh + 1) * c.HD] = sg
            for h in range(kvh * (c.H // c.KV), (kvh + 1) * (c.H // c.KV)):
                qkv[o1:o1 + n1, h * c.HD:(h + 1) * c.HD] = sg
    return dict(qkv=qkv.to(BF16), dout=dout.to(BF16))


# ------------------------------------------------------------------------------------------------------------- reference
def ref_forward(qkv, c):
    """-> train_attn_ref.Fwd (p = None): per segment ``_attend`` with one more key block, scattered."""
    q, k, v = A.split_heads(qkv, c.B, c.S, c.H, c.KV, c.HD)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)             # noqa: E731
    out, absv, osl = z(c.B, c.H, c.S, c.HD), z(c.B, c.H, c.S, c.HD), z(c.B, c.H, c.S, c.HD)
    lse, lsl = z(c.B, c.H, c.S), z(c.B, c.H, c.S)
    for b in range(c.B):
        for o, n in segments(c, b):
            r = A._attend(q[b][:, o:o + n], k[b][:, o:o + n], v[b][:, o:o + n], torch.arange(n), extra_rescales=1)
            out[b, :, o:o + n], lse[b, :, o:o + n], absv[b, :, o:o + n], osl[b, :, o:o + n], lsl[b, :, o:o + n] = r[0], r[1], r[3], r[4], r[5]
    return A.Fwd(_rows(out), lse, None, _rows(absv), _rows(osl), lsl)


def ref_backward(qkv, out_given, lse_given, dout, c):
    """-> train_attn_ref.Bwd (no rotation): per segment ``_backward`` from the given out and lse, dQ's chain with one more block."""
    W, rep, scale = (c.H + 2 * c.KV) * c.HD, c.H // c.KV, 1.0 / math.sqrt(c.HD)
    a = c.H * c.HD
    dqkv, sl = torch.zeros(c.B * c.S, W, dtype=torch.float64), torch.zeros(c.B * c.S, W, dtype=torch.float64)
    delta, dsl = torch.zeros(c.B, c.H, c.S, dtype=torch.float64), torch.zeros(c.B, c.H, c.S, dtype=torch.float64)
    lse_given = lse_given.reshape(c.B, c.H, c.S)
    for b in range(c.B):
        for o, n in segments(c, b):
            rows = slice(b * c.S + o, b * c.S + o + n)
            lg = lse_given[b:b + 1, :, o:o + n]
            dQ, dQs, dK, dKs, dV, dVs, dl, dls = A._backward(qkv[rows], out_given[rows], lg, dout[rows], 1, n, c.H, c.KV, c.HD)
            # one more key block in chain_q: 2 U scale sum_j |dS_ij| |k_jd|
            q, k, v = A.split_heads(qkv[rows], 1, n, c.H, c.KV, c.HD)
            kx, vx = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)
            dO = dout[rows].double().reshape(1, n, c.H, c.HD).permute(0, 2, 1, 3)
            vis = torch.tril(torch.ones(n, n, dtype=torch.bool))
            p = torch.exp(((q @ kx.transpose(2, 3)) * scale - lg.double()[..., None]).masked_fill(~vis, float("-inf")))
            dS = p * (dO @ vx.transpose(2, 3) - dl[..., None])
            dQs = dQs + 2 * U * scale * (dS.abs() @ kx.abs())
            dqkv[rows] = torch.cat([_rows(dQ), _rows(dK), _rows(dV)], 1)
            sl[rows] = torch.cat([_rows(dQs), _rows(dKs), _rows(dVs)], 1)
            delta[b, :, o:o + n], dsl[b, :, o:o + n] = dl[0], dls[0]
    assert dqkv.shape[1] == a + 2 * c.KV * c.HD
    return A.Bwd(dqkv, delta, sl, dsl)


# ------------------------------------------------------------------------------------------------------------- restatements
FWD_MUTANTS = ("no_mask", "start_plus1", "start_minus1", "start_per_tile16", "skip_by_largest_start", "no_floor")
BWD_MUTANTS = ("no_mask", "start_plus1", "start_minus1", "start_per_tile16", "skip_by_largest_start", "dkv_to_block_end")


def _starts(c, mut):
    """The per-query segment start [B, S] a (wrong) kernel would use, and the first key block [B, S] its workgroup walks."""
    ss = arrays(c)[0].reshape(c.B, c.S).long()
    i = torch.arange(c.S)[None].expand(c.B, c.S)
    if mut == "no_mask":
        use = torch.zeros_like(ss)
    elif mut == "start_plus1":
        use = torch.minimum(ss + 1, i)                            # (a query still sees itself)
    elif mut == "start_minus1":
        use = (ss - 1).clamp(min=0)
    elif mut == "start_per_tile16":
        use = ss.gather(1, i & ~15)                               # the tile's first query's start for all 16
    else:
        use = ss
    first = ss.gather(1, i & ~127)                                # smallest start of the workgroup's 128 queries
    if mut == "no_mask":
        first = torch.zeros_like(ss)
    if mut == "skip_by_largest_start":
        first = ss.gather(1, (i | 127).clamp(max=c.S - 1))
    return use, first // 64


def restate_forward(qkv, c, mut=None):
    """The SEG forward in fp32 / bf16: per workgroup of 128 queries the key blocks of 64 (aligned to the row) from the workgroup's
    first one to its last query's, online softmax by exp2 with the exponent's maximum held at 0 while a row has seen no key,
    P rounded to bf16 for the PV product and for l.  -> out bf16, lse fp32."""
    q, k, v = A._split32(qkv, c.B, c.S, c.H, c.KV, c.HD)
    S = c.S
    use, kb0 = _starts(c, mut)
    i, j = torch.arange(S)[None, :, None], torch.arange(S)[None, None, :]
    vis = ((j <= i) & (j >= use[..., None]))[:, None]             # [B, 1, S, S]
    last = ((torch.arange(S) | 127).clamp(max=S - 1) // 64)[None].expand(c.B, S)
    scale = torch.tensor(1.0 / math.sqrt(c.HD), dtype=F32)
    c2 = scale * torch.tensor(A.LOG2E32, dtype=F32)
    s = (q @ k.transpose(2, 3)).masked_fill(~vis, float("-inf"))
    m = torch.full((c.B, c.H, S), float("-inf"))
    l, o = torch.zeros(c.B, c.H, S), torch.zeros(c.B, c.H, S, c.HD)
    for k0 in range(0, S, 64):
        walk = ((kb0 <= k0 // 64) & (k0 // 64 <= last))[:, None]  # [B, 1, S]: the rows whose workgroup walks this block
        sb = s[..., k0:k0 + 64]
        m_new = torch.maximum(m, sb.amax(-1))
        m_use = m_new if mut == "no_floor" else torch.where(torch.isinf(m_new), torch.zeros(()), m_new)
        alpha = torch.exp2((m - m_use) * c2)
        pb = A._bf(torch.exp2(sb * c2 - (m_use * c2)[..., None]))
        l = torch.where(walk, l * alpha + pb.sum(-1), l)
        o = torch.where(walk[..., None], o * alpha[..., None] + pb @ v[:, :, k0:k0 + 64], o)
        m = torch.where(walk, m_new, m)
    return _rows(o / l[..., None]).to(BF16), m * scale + torch.log(l)


def restate_backward(qkv, out_bf16, lse32, dout, c, mut=None):
    """The SEG backward in fp32 / bf16 (train_attn_ref.restate_backward under the segment mask): the dQ pass masks by the query's
    seg_start and walks from its workgroup's first block, the dK/dV pass masks by the key's seg_end.  -> dqkv bf16, delta fp32."""
    q, k, v = A._split32(qkv, c.B, c.S, c.H, c.KV, c.HD)
    S, rep = c.S, c.H // c.KV
    use, kb0 = _starts(c, mut)
    se = arrays(c)[1].reshape(c.B, S).long()
    if mut == "dkv_to_block_end":
        se = (se | 63).clamp(max=S - 1)
    if mut == "no_mask":
        se = torch.full_like(se, S - 1)
    i, j = torch.arange(S)[None, :, None], torch.arange(S)[None, None, :]
    vis_q = ((j <= i) & (j >= use[..., None]) & (j // 64 >= kb0[..., None]))[:, None]
    vis_k = ((j <= i) & (i <= se[:, None, :]))[:, None]           # query i, key j: i <= seg_end[j] (that pass has no seg_start)
    dO = dout.float().reshape(c.B, S, c.H, c.HD).permute(0, 2, 1, 3)
    og = out_bf16.float().reshape(c.B, S, c.H, c.HD).permute(0, 2, 1, 3)
    scale = torch.tensor(1.0 / math.sqrt(c.HD), dtype=F32)
    c2 = scale * torch.tensor(A.LOG2E32, dtype=F32)
    nl = -lse32.float().reshape(c.B, c.H, S) * torch.tensor(A.LOG2E32, dtype=F32)
    pfull = torch.exp2((q @ k.transpose(2, 3)) * c2 + nl[..., None])
    delta = (dO * og).sum(-1)
    dSfull = pfull * ((dO @ v.transpose(2, 3)) - delta[..., None])
    dQ = (A._bf(dSfull.masked_fill(~vis_q, 0.0)) @ k) * scale
    pk, dsk = A._bf(pfull.masked_fill(~vis_k, 0.0)), A._bf(dSfull.masked_fill(~vis_k, 0.0))
    grp = lambda t: t.reshape(c.B, c.KV, rep, S, c.HD).sum(2)     # noqa: E731
    dK, dV = grp((dsk.transpose(2, 3) @ q) * scale), grp(pk.transpose(2, 3) @ dO)
    return torch.cat([_rows(dQ), _rows(dK), _rows(dV)], 1).to(BF16), delta
