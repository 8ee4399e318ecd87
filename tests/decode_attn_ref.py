"""A float64 reference of the decode-step cache attention and the cases the decode-attention tests run (test_decode_attn_cpu.py
proves this module against the oracle; test_decode_attn_gpu.py judges the kernels of csrc/generate.hip by it).

Everything here is plain torch on the CPU, seeded, and identical on every machine.

One-hot cases.  The q heads of one kv group get disjoint supports (rotation pair i belongs to the head with i % rep == h % rep;
the rotation keeps pairs apart, so the rotated heads are disjoint too).  Their sum times a power of two c is therefore
bf16-exact, and as key s* it gives every head of the group the score c |q_h|^2 / sqrt(HD) - chosen >= 64 - while every other key
is randn (|score| of a few units).  The float64 softmax then leaves less than 2^-13 outside s*, the values lie in [1, 2), and
the expected output is v[s*] bit for bit.  For s* == pos the NEW key (before rotation) is c times the sum of the unrotated
heads: a rotation commutes exactly with a power of two."""
import functools
import math
from collections import namedtuple

import torch

BF = torch.bfloat16

GEOMS = {"backbone": (32, 8, 64), "decoder": (8, 2, 128), "tiny64": (4, 2, 64), "tiny128": (2, 1, 128)}      # H, KV, HD
SWEEP = {
    2048: (0, 1, 2, 7, 8, 15, 16, 31, 32, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 2046, 2047),
    96: (0, 94, 95),
    8192: (4095, 8191),
}
SWEEP_CASES = [(s_max, pos) for s_max, ps in SWEEP.items() for pos in ps]
RANGE_POS = (0, 300)                                   # the softmax-range cases
RANGE_S_MAX = 512
ONEHOT_SCORE = 64.0                                    # the least score a one-hot case gives its target key
GUARD = 0.1005859375                                   # bf16-exact guard value for the cache-write checks

Ref = namedtuple("Ref", "out kc vc absv probs scores")
Case = namedtuple("Case", "qkv kc vc pos H KV HD table want")


def oracle():
    from oracle import csm_oracle as O
    return O


@functools.lru_cache(maxsize=None)
def rope_table(s_max, hd):
    return oracle().rope_table(s_max, hd).contiguous()


def onehot_targets(pos):
    """The target keys of the one-hot cases at ``pos``: 0, pos // 2, 255, 256, pos - 1, pos, where these exist."""
    return sorted({s for s in (0, pos // 2, 255, 256, pos - 1, pos) if 0 <= s <= pos})


def split_row(qkv, H, KV, HD):
    """q [B,H,HD], k [B,KV,HD], v [B,KV,HD] of the (possibly padded) fused rows."""
    B = qkv.shape[0]
    q = qkv[:, :H * HD].reshape(B, H, HD)
    k = qkv[:, H * HD:(H + KV) * HD].reshape(B, KV, HD)
    v = qkv[:, (H + KV) * HD:(H + 2 * KV) * HD].reshape(B, KV, HD)
    return q, k, v


def rotate(x, table, pos):
    """oracle.csm_oracle.rope of bf16 heads x [B,h,HD] at pos [B]: fp32 products, one rounding to bf16 - the library's promise."""
    pl = torch.as_tensor(pos).long().view(-1, 1)
    return oracle().rope(x.unsqueeze(1), table, pl)[:, 0]


def ref_decode_attention(qkv, kc, vc, pos, H, KV, HD, table=None):
    """One query position per batch row against the caches, in float64.

    qkv [B, >= (H + 2 KV) HD] bf16 (q | k | v, padding ignored), kc / vc [B, KV, S_max, HD] bf16, pos [B].  With ``table`` the new q
    and k are rotated first (oracle rope on the bf16 inputs, rounded to bf16 as the kernels round); without, they are taken as
    they are.  Keys and values 0 .. pos-1 come from the caches, key and value pos from the qkv row; cache rows >= pos are never
    read.  Returns Ref(out [B, H HD] float64, the expected caches (row pos of every (b, kv head) replaced, nothing else),
    absv = sum_s p_s |v_s| per output element, probs[b] [H, pos+1], scores[b] [H, pos+1])."""
    assert qkv.dtype == BF and kc.dtype == BF and vc.dtype == BF and kc.shape == vc.shape
    B, rep = qkv.shape[0], H // KV
    pos = [int(p) for p in torch.as_tensor(pos).flatten().tolist()]
    assert len(pos) == B and all(0 <= p < kc.shape[2] for p in pos)
    q, k, v = split_row(qkv, H, KV, HD)
    if table is not None:
        q, k = rotate(q, table, pos), rotate(k, table, pos)
    kc_e, vc_e = kc.clone(), vc.clone()
    out = torch.zeros(B, H, HD, dtype=torch.float64)
    absv = torch.zeros(B, H, HD, dtype=torch.float64)
    probs, scores = [], []
    for b, p in enumerate(pos):
        kc_e[b, :, p], vc_e[b, :, p] = k[b], v[b]
        pb, sb = [], []
        for g in range(KV):
            K = torch.cat([kc[b, g, :p], k[b, g][None]]).double()               # [p + 1, HD]
            V = torch.cat([vc[b, g, :p], v[b, g][None]]).double()
            s = q[b, g * rep:(g + 1) * rep].double() @ K.t() / math.sqrt(HD)    # [rep, p + 1]
            pr = torch.softmax(s, dim=-1)
            out[b, g * rep:(g + 1) * rep] = pr @ V
            absv[b, g * rep:(g + 1) * rep] = pr @ V.abs()
            pb.append(pr)
            sb.append(s)
        probs.append(torch.cat(pb))
        scores.append(torch.cat(sb))
    return Ref(out.reshape(B, H * HD), kc_e, vc_e, absv.reshape(B, H * HD), probs, scores)


def ref_product(attn_out, W, residual=None):
    """The fused product kernels: the attention result rounded to bf16, then W [N, H HD] and the residual in float64."""
    y = attn_out.float().to(BF).double() @ W.double().t()
    return y if residual is None else y + residual.double()


def error_bound(ref, score_scaled=False):
    """|got - ref| <= 2^-8 |ref| + 2^-16 sum_s p_s |v_s| per element.  First term: the rounding of the result to bf16 - half an
    ulp of an 8-bit significand is up to 2^-8 of a value just above a power of two, and a result whose fp32 error straddles a
    rounding boundary still lands within half an ulp plus that error.  Second term: fp32 accumulation and __expf (argument
    error about |x| 2^-24 for |x| up to a few tens), about 4x margin.  ``score_scaled`` (the softmax-range cases only):
    the second term times max(1, max_s |score_s| / 8), the fp32 error of a score growing with its magnitude."""
    second = 2.0 ** -16 * ref.absv
    if score_scaled:
        B = ref.out.shape[0]
        H = ref.scores[0].shape[0]
        mult = torch.stack([s.abs().amax(dim=-1).div(8).clamp(min=1.0) for s in ref.scores])       # [B, H]
        second = (second.reshape(B, H, -1) * mult[:, :, None]).reshape(B, -1)
    return 2.0 ** -8 * ref.out.abs() + second


def worst_ratio(got, ref, score_scaled=False):
    """max over elements of |got - ref| / bound (inf for a non-finite result)."""
    got = got.detach().cpu().double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err, bound = (got - ref.out).abs(), error_bound(ref, score_scaled)
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------------------- random cases
def _seed(*xs):
    s = 12345
    for x in xs:
        s = (s * 1000003 + int(x)) % (2 ** 31 - 1)
    return s


def random_case(H, KV, HD, s_max, pos, rope=True, pad=0, seed=0, fill=0.0):
    """randn everywhere the reference reads: the fused rows and cache rows < pos[b]; ``fill`` in every other cache element and
    NaN in the ``pad`` extra columns of a qkv row."""
    pos = [int(p) for p in pos]
    B, width = len(pos), (H + 2 * KV) * HD
    g = torch.Generator().manual_seed(_seed(H, KV, HD, s_max, seed, *pos))
    qkv = torch.full((B, width + pad), float("nan"), dtype=BF)
    qkv[:, :width] = torch.randn(B, width, generator=g).to(BF)
    kc = torch.full((B, KV, s_max, HD), fill, dtype=BF)
    vc = torch.full((B, KV, s_max, HD), fill, dtype=BF)
    for b, p in enumerate(pos):
        kc[b, :, :p] = torch.randn(KV, p, HD, generator=g).to(BF)
        vc[b, :, :p] = torch.randn(KV, p, HD, generator=g).to(BF)
    table = rope_table(s_max, HD) if rope else None
    return Case(qkv, kc, vc, torch.tensor(pos, dtype=torch.int32), H, KV, HD, table, None)


# ------------------------------------------------------------------------------------------------------------- one-hot cases
def value_pattern(KV, s_max, HD):
    """v[g, s, d] = 1 + m / 128 in [1, 2), bf16-exact, m = (s + d (1 + (s >> 7)) + 41 g) mod 128: neighbouring slots differ in
    column 0, slots 128 k apart differ in column 1, the kv heads differ everywhere - no two (head, slot) rows are equal."""
    s = torch.arange(s_max).view(1, -1, 1)
    d = torch.arange(HD).view(1, 1, -1)
    g = torch.arange(KV).view(-1, 1, 1)
    m = (s + d * (1 + (s >> 7)) + 41 * g) % 128
    return (1.0 + m.double() / 128.0).to(BF)


@functools.lru_cache(maxsize=4)
def _base_keys(KV, s_max, HD):
    g = torch.Generator().manual_seed(_seed(KV, s_max, HD, 99))
    return torch.randn(KV, s_max, HD, generator=g).to(BF)


@functools.lru_cache(maxsize=4)
def _base_values(KV, s_max, HD):
    return value_pattern(KV, s_max, HD)


def _disjoint_queries(H, KV, HD, gen):
    rep = H // KV
    q = torch.randn(H, HD // 2, 2, generator=gen)
    keep = (torch.arange(HD // 2).view(1, -1) % rep) == (torch.arange(H).view(-1, 1) % rep)
    q = q * keep[:, :, None]
    # keep every kept component away from zero, so that |q_h|^2 is never small by chance
    q = torch.where(keep[:, :, None] & (q.abs() < 0.25), torch.full_like(q, 0.5), q).reshape(H, HD)
    q = q * (HD / rep / q.pow(2).sum(-1, keepdim=True)).sqrt()                  # |q_h|^2 = HD / rep for every head (up to rounding)
    return q.to(BF)


def onehot_case(H, KV, HD, s_max, pos, s_star, rope=True, score=ONEHOT_SCORE, snap=math.ceil):
    """A B = 1 case whose softmax sits on key ``s_star`` for every q head (its score is ``score`` rounded up - ``snap`` - to a power of two
    times |q_h|^2 / sqrt(HD)); want = v[s_star] of each head's kv head, [1, H HD]."""
    assert 0 <= s_star <= pos < s_max
    rep, width = H // KV, (H + 2 * KV) * HD
    gen = torch.Generator().manual_seed(_seed(H, KV, HD, s_max, pos, s_star))
    table = rope_table(s_max, HD) if rope else None
    q = _disjoint_queries(H, KV, HD, gen)
    qr = rotate(q[None], table, [pos])[0] if rope else q
    norm2 = qr.double().pow(2).sum(-1).min().item()
    key_scale = 2.0 ** snap(math.log2(score * math.sqrt(HD) / norm2))
    kc = _base_keys(KV, s_max, HD).clone()[None]
    vc = _base_values(KV, s_max, HD).clone()[None]
    kc[:, :, pos:], vc[:, :, pos:] = 0.0, 0.0
    k_new = torch.randn(KV, HD, generator=gen).to(BF)
    v_new = _base_values(KV, s_max, HD)[:, pos].clone()
    if s_star == pos:
        k_new = (key_scale * q.float().reshape(KV, rep, HD).sum(1)).to(BF)
    else:
        kc[0, :, s_star] = (key_scale * qr.float().reshape(KV, rep, HD).sum(1)).to(BF)
    qkv = torch.cat([q.reshape(-1), k_new.reshape(-1), v_new.reshape(-1)])[None].contiguous()
    assert qkv.shape[1] == width
    want = _base_values(KV, s_max, HD)[:, s_star].repeat_interleave(rep, 0).reshape(1, H * HD).clone()
    return Case(qkv, kc, vc, torch.tensor([pos], dtype=torch.int32), H, KV, HD, table, want)


def onehot_margin(case, ref, s_star):
    """max over output elements of  sum_{s != s*} p_s |v[s, d]| / |v[s*, d]|  in the float64 reference: must be <= 2^-12.
    Summed from the probabilities with column s* taken out (the difference absv - p* |v*| would cancel to nothing)."""
    H, KV, HD = case.H, case.KV, case.HD
    rep, pos = H // KV, int(case.pos[0])
    want = case.want.double().reshape(H, HD)
    v_new = split_row(case.qkv, H, KV, HD)[2][0]                                # [KV, HD]
    p_off = ref.probs[0].clone()                                                # [H, pos + 1]
    p_off[:, s_star] = 0.0
    worst = 0.0
    for g in range(KV):
        V = torch.cat([case.vc[0, g, :pos], v_new[g][None]]).double().abs()     # [pos + 1, HD]
        rest = p_off[g * rep:(g + 1) * rep] @ V
        worst = max(worst, float((rest / want[g * rep:(g + 1) * rep].abs()).max()))
    return worst


# ------------------------------------------------------------------------------------------------------------- softmax range
def mean_exact_values(KV, n, HD):
    """n value rows whose mean is 1.5 in every column exactly: rows 2i, 2i+1 are 1.5 +- a (a a multiple of 1/64 below 1/2,
    varying with i, column and head), an odd last row is 1.5.  Every partial sum is a small multiple of 1/64: exact in fp32."""
    i = torch.arange(n // 2).view(1, -1, 1)
    d = torch.arange(HD).view(1, 1, -1)
    g = torch.arange(KV).view(-1, 1, 1)
    a = ((7 * i + d + 3 * g) % 31 + 1).double() / 64.0
    v = torch.full((KV, n, HD), 1.5, dtype=torch.float64)
    v[:, 0:2 * (n // 2):2] += a
    v[:, 1:2 * (n // 2):2] -= a
    return v.to(BF)


def range_case(kind, H, KV, HD, pos, s_max=RANGE_S_MAX):
    """kind: 'spike' (key pos // 2 scores about 200 above the rest; want = its value row), 'equal' (every key is the same vector,
    the new one included; want = the mean of the values = 1.5), 'low' (every score about -300), 'zero_q' (q = 0; want = 1.5)."""
    rep, n = H // KV, pos + 1
    table = rope_table(s_max, HD)
    gen = torch.Generator().manual_seed(_seed(H, KV, HD, pos, len(kind), ord(kind[0])))
    if kind == "spike":
        return onehot_case(H, KV, HD, s_max, pos, pos // 2, score=200.0, snap=round)
    q = _disjoint_queries(H, KV, HD, gen)
    qr = rotate(q[None], table, [pos])[0]
    kc = torch.zeros(1, KV, s_max, HD, dtype=BF)
    vc = torch.zeros(1, KV, s_max, HD, dtype=BF)
    k_new = torch.randn(KV, HD, generator=gen).to(BF)
    want = None
    if kind in ("equal", "zero_q"):
        vals = mean_exact_values(KV, n, HD)
        want = torch.full((1, H * HD), 1.5, dtype=BF)
        if kind == "zero_q":
            q = torch.zeros_like(q)
            kc[0, :, :pos] = torch.randn(KV, pos, HD, generator=gen).to(BF)
        else:
            kc[0, :, :pos] = rotate(k_new[None], table, [pos])[0][:, None, :]    # the cached keys ARE the rotated new key
    else:
        assert kind == "low"
        vals = _base_values(KV, s_max, HD)[:, :n].clone()
        norm2 = qr.double().pow(2).sum(-1).min().item()
        c = 2.0 ** round(math.log2(300.0 * math.sqrt(HD) / norm2))
        anti = -(c * qr.float().reshape(KV, rep, HD).sum(1))                     # [KV, HD]: score -c |q_h|^2 / sqrt(HD)
        kc[0, :, :pos] = (anti[:, None, :] + torch.randn(KV, pos, HD, generator=gen)).to(BF)
        k_new = (-(c * q.float().reshape(KV, rep, HD).sum(1))).to(BF)
    vc[0, :, :pos] = vals[:, :pos]
    qkv = torch.cat([q.reshape(-1), k_new.reshape(-1), vals[:, pos].reshape(-1)])[None].contiguous()
    return Case(qkv, kc, vc, torch.tensor([pos], dtype=torch.int32), H, KV, HD, table, want)


def reads_are_finite(case):
    """No non-finite value where the reference reads: the q | k | v columns of the rows and cache rows < pos."""
    width = (case.H + 2 * case.KV) * case.HD
    ok = bool(torch.isfinite(case.qkv[:, :width].float()).all())
    for b, p in enumerate(case.pos.tolist()):
        ok = ok and bool(torch.isfinite(case.kc[b, :, :p].float()).all()) and bool(torch.isfinite(case.vc[b, :, :p].float()).all())
    return ok
