"""A float64 reference of the KV-cache context shift (csm_kv_shift, csrc/generate.hip) and the cases its tests run:
test_kv_shift_ref_cpu.py proves this module, test_kv_shift_gpu.py judges the kernel by it.

The operation, from the index formula of include/csm_hip.h.  src is bf16 [layers][2][KV][len][HD] (K plane, then V plane),
dst is bf16 [layers][2][KV][len - drop][HD].  For every layer and kv head:

    p <  keep:       dst K, V [p] = src K, V [p]                                  bit for bit   (the head)
    p >= keep, V:    dst V [p]    = src V [p + drop]                              bit for bit
    p >= keep, K:    dst K [p]    = pairs (x0, x1) of src K [p + drop] rotated by -drop positions:
                                    y0 = x0 c + x1 s,   y1 = x1 c - x0 s,   (c, s) = table[drop][pair]

The reference works on the kernel's own operands: the bf16 src and the fp32 table row, both cast to float64, so it has no
rounding of its own worth naming (two float64 products and one sum of values of order 1: < 2^-51 relative).

The bound, derived and not fitted.  The kernel computes in fp32 with contraction off (``rope_rot``):
y0 = fl(fl(x0 c) - fl(x1 (-s))), y1 = fl(fl(x1 c) + fl(x0 (-s))), then ONE rounding to bf16.  With U = 2^-24 the unit
roundoff of fp32, each product is off by at most U |product|, and the sum by at most U |sum| <= U (|x0 c| + |x1 s|) (1 + U).
Together |fp32 result - exact| <= 2U (1 + U)(|x0 c| + |x1 s|) < 3U (|x0 c| + |x1 s|) =: slack (the same two magnitudes serve
y1 with x0 and x1 swapped).  Rounding an fp32 value that lies within slack of ref to bf16 (nearest even) lands within half a
bf16 ulp, taken at |ref| + slack, of that value: |got - ref| <= hulp(|ref| + slack) + slack - which is what
``train_ops_ref.judge`` computes from (ref, slack) for a bf16 result.  ``slack = None`` asks bit equality: the head, every V
and every guard element around dst.
"""
import functools

import torch

from train_ops_ref import BF16, F32, F64, U, judge, trunc_bf16                      # noqa: F401

GUARD = 0.1005859375                                    # bf16-exact guard value around dst (tests/decode_attn_ref.py's)
PAD = 64                                                # guard elements before and after dst (128 bytes: dst stays 16-byte aligned)


def oracle():
    from oracle import csm_oracle as O
    return O


@functools.lru_cache(maxsize=None)
def rope_table(rows, hd):
    return oracle().rope_table(rows, hd).contiguous()


def _seed(*xs):
    s = 424243
    for x in xs:
        s = (s * 1000003 + int(x)) % (2 ** 31 - 1)
    return s


def random_src(layers, KV, HD, length, seed=0):
    """bf16 randn [layers, 2, KV, length, HD]; K and V differ, so does every (layer, head, position)."""
    g = torch.Generator().manual_seed(_seed(layers, KV, HD, length, seed))
    return torch.randn(layers, 2, KV, length, HD, generator=g).to(BF16)


def rotated_keys(k_raw, table, pos0):
    """What the library's rope leaves in a cache: bf16 keys k_raw [..., n, HD] at positions pos0 .. pos0+n-1, rotated in fp32 and
    rounded to bf16 (oracle.rope on the bf16 input)."""
    n, hd = k_raw.shape[-2], k_raw.shape[-1]
    flat = k_raw.reshape(-1, n, 1, hd)
    pos = torch.arange(pos0, pos0 + n).view(1, n).expand(flat.shape[0], n)
    return oracle().rope(flat, table, pos).reshape(k_raw.shape)


def rotate_back64(k, trow, sign=-1.0, half_split=False):
    """float64: every interleaved pair of k [..., HD] rotated by ``sign`` x the angle of the table row ``trow`` [HD/2, 2]
    (sign = -1: the shift).  ``half_split``: pairs (i, i + HD/2) instead - a mutant's pairing."""
    k, c, s = k.double(), trow[:, 0].double(), sign * trow[:, 1].double()
    if half_split:
        h = k.shape[-1] // 2
        x0, x1 = k[..., :h], k[..., h:]
        return torch.cat([x0 * c - x1 * s, x1 * c + x0 * s], -1)
    x = k.reshape(*k.shape[:-1], k.shape[-1] // 2, 2)
    return torch.stack([x[..., 0] * c - x[..., 1] * s, x[..., 1] * c + x[..., 0] * s], -1).flatten(-2)


def kv_shift_ref(src, table, keep, drop):
    """-> {"head": (bf16, None), "v_tail": (bf16, None), "k_tail": (float64, slack)} - the three parts of dst
    [layers, 2, KV, len - drop, HD] as ``split`` cuts them, each with its slack for ``judge``."""
    assert src.dtype == BF16 and src.dim() == 5 and src.shape[1] == 2 and table.dtype == F32
    length = src.shape[3]
    assert drop >= 1 and keep >= 0 and keep + drop <= length and length - drop >= 1 and drop < table.shape[0]
    trow = table[drop]
    x = src[:, 0, :, keep + drop:].double()                                       # [layers, KV, tail, HD]
    ref = rotate_back64(x, trow)
    pairs = x.reshape(*x.shape[:-1], x.shape[-1] // 2, 2).abs()
    c, s = trow[:, 0].double().abs(), trow[:, 1].double().abs()
    m0 = pairs[..., 0] * c + pairs[..., 1] * s                                    # |x0 c| + |x1 s|   (y0)
    m1 = pairs[..., 1] * c + pairs[..., 0] * s                                    # |x1 c| + |x0 s|   (y1)
    slack = 3 * U * torch.stack([m0, m1], -1).flatten(-2)
    return {"head": (src[:, :, :, :keep].clone(), None), "v_tail": (src[:, 1, :, keep + drop:].clone(), None), "k_tail": (ref, slack)}


def split(dst, keep):
    """dst [layers, 2, KV, len - drop, HD] cut into the parts of ``kv_shift_ref``: together they are every element of dst."""
    return {"head": dst[:, :, :, :keep], "v_tail": dst[:, 1, :, keep:], "k_tail": dst[:, 0, :, keep:]}


def judge_shift(name, dst, src, table, keep, drop):
    """Every element of ``dst`` against the reference; -> worst |err| / bound (0 where only bit equality is asked)."""
    ref, got = kv_shift_ref(src, table, keep, drop), split(dst.detach().cpu(), keep)
    assert dst.shape == (src.shape[0], 2, src.shape[2], src.shape[3] - drop, src.shape[4]) and dst.dtype == BF16
    assert sum(g.numel() for g in got.values()) == dst.numel()
    return max(judge(f"{name}.{part}", got[part], val, slack) for part, (val, slack) in ref.items())


def restate_fp32(src, table, keep, drop, mutant=None):
    """The kernel's arithmetic restated in fp32 torch ops in its own order (separate products, one sum, one rounding to bf16 by
    nearest even) -> dst.  ``mutant`` names one wrong restatement the reference must reject."""
    assert mutant in (None, "plus_d", "no_rotation", "half_split", "v_rotated", "head_rotated", "src_row_minus_1", "table_row_plus_1",
                      "truncate")
    length = src.shape[3]
    off = drop - 1 if mutant == "src_row_minus_1" else drop
    trow = table[drop + 1 if mutant == "table_row_plus_1" else drop]
    c, s = trow[:, 0], (trow[:, 1] if mutant == "plus_d" else -trow[:, 1])

    def rot(x):
        x = x.float()
        if mutant == "no_rotation":
            return x
        if mutant == "half_split":
            h = x.shape[-1] // 2
            x0, x1 = x[..., :h], x[..., h:]
            return torch.cat([x0 * c - x1 * s, x1 * c + x0 * s], -1)
        p = x.reshape(*x.shape[:-1], x.shape[-1] // 2, 2)
        return torch.stack([p[..., 0] * c - p[..., 1] * s, p[..., 1] * c + p[..., 0] * s], -1).flatten(-2)

    def down(x32):
        return trunc_bf16(x32) if mutant == "truncate" else x32.to(BF16)

    dst = torch.cat([src[:, :, :, :keep], src[:, :, :, keep + off:keep + off + length - drop - keep]], 3).clone()
    dst[:, 0, :, keep:] = down(rot(dst[:, 0, :, keep:]))
    if mutant == "v_rotated":
        dst[:, 1, :, keep:] = down(rot(dst[:, 1, :, keep:]))
    if mutant == "head_rotated":
        dst[:, 0, :, :keep] = down(rot(dst[:, 0, :, :keep]))
    return dst


# the kernel-level cases: (layers, KV, HD, len, keep, drop).  len 2 / 9 / 64 / 65 / 200, keep 0 / 1 / 7, drop 1 / 8 / 63 / 64 and
# len - keep - 1 (one tail position left, = keep + drop == len - 1), both head dims, 1 / 2 layers and kv heads
CASES = [
    (1, 1, 64, 2, 0, 1), (1, 1, 128, 2, 0, 1), (2, 2, 64, 2, 1, 1),
    (1, 2, 64, 9, 0, 1), (2, 1, 128, 9, 1, 7), (2, 2, 64, 9, 7, 1), (1, 1, 64, 9, 0, 8),
    (2, 2, 64, 64, 0, 63), (1, 2, 128, 64, 7, 8), (2, 1, 64, 64, 1, 62),
    (2, 2, 128, 65, 0, 64), (1, 1, 64, 65, 1, 63), (2, 2, 64, 65, 7, 57),
    (2, 2, 64, 200, 7, 64), (1, 2, 128, 200, 1, 63), (2, 1, 64, 200, 0, 199), (2, 2, 128, 200, 7, 192), (1, 1, 64, 200, 1, 8),
]
LATE = (1, 1, 64, 2047, 1, 1500)                         # a late table row
TABLE_ROWS = 2048


def drift_ratio(keys, k_raw, table, shifts):
    """Information, not a check of one launch: how far keys [..., n, HD] that went through ``shifts`` context shifts are from
    rope(k_raw, the position they now hold) in float64, over the bound.  The bound per element: every rounding to bf16 - the
    cache's own and one per shift - moves a component of a pair by at most half an ulp at the pair's magnitude |k| (a component
    was never larger), i.e. the pair's error vector by sqrt(2) of that, and the later rotations keep the length of that vector:
    (shifts + 1) sqrt(2) hulp(|k|); plus the table term 2^-13 |k|: the fp32 rounding of an angle below 2048 rad moves it by up
    to 2^-13 rad, and the rotations applied (forward once, back once per shift) are by table rows whose angles add up only
    to that accuracy."""
    import math
    from train_ops_ref import hulp
    n, hd = keys.shape[-2], keys.shape[-1]
    pairs = k_raw.double().reshape(*k_raw.shape[:-1], hd // 2, 2)
    t = table[torch.arange(n)].double()                                           # [n, HD/2, 2]
    want = torch.stack([pairs[..., 0] * t[..., 0] - pairs[..., 1] * t[..., 1], pairs[..., 1] * t[..., 0] + pairs[..., 0] * t[..., 1]], -1).flatten(-2)
    norm = pairs.pow(2).sum(-1).sqrt().repeat_interleave(2, -1)                   # |k| of the element's pair
    bound = (shifts + 1) * math.sqrt(2.0) * hulp(norm) + 2.0 ** -13 * norm
    return float(((keys.double() - want).abs() / bound.clamp(min=1e-300)).max())


# ------------------------------------------------------------------------------------- relative-position invariance (attention)
INVARIANCE = [("tiny64", 9, 1), ("tiny64", 65, 8), ("tiny64", 200, 64), ("tiny64", 200, 137), ("tiny128", 64, 63), ("tiny128", 200, 8),
              ("tiny128", 129, 64)]                               # (geometry of decode_attn_ref, pos, d): keys d .. pos-1 are kept
INV_S_MAX = 256


def key_bound(src, table, keep, drop):
    """The error the shift may leave in each element of a shifted key, [layers, KV, tail, HD]: the bound ``judge`` applies to the
    ``k_tail`` part, hulp(|ref| + slack) + slack."""
    from train_ops_ref import hulp
    ref, slack = kv_shift_ref(src, table, keep, drop)["k_tail"]
    return hulp(ref.abs() + slack) + slack


def invariance_problem(geom, pos, d):
    """-> (case, src): a B = 1 random decode-attention case of tests/decode_attn_ref.py at ``pos`` and its cache rows 0 .. pos-1 as
    the one-layer parked history [1, 2, KV, pos, HD] that csm_kv_shift takes (keep 0, drop d)."""
    import decode_attn_ref as D
    H, KV, HD = D.GEOMS[geom]
    c = D.random_case(H, KV, HD, INV_S_MAX, [pos], seed=d)
    src = torch.stack([c.kc[0, :, :pos], c.vc[0, :, :pos]])[None].contiguous()
    return c, src


def invariance_reference(c, src, d):
    """-> (Ref of decode_attn_ref on the ORIGINAL cache restricted to keys d .. pos-1 at their original positions - q and the new
    k rotated at ``pos`` -, tolerance per output element).

    Tolerance = decode_attn_ref.error_bound + the shift's slack carried through the scores.  A shifted key element may be off by
    b[s, j] (``key_bound``), so the score of key s against the query q' the kernel holds (the row's q rotated at pos - d, rounded
    to bf16) moves by at most  Delta_s = scale x sum_j |q'_j| b[s, j];  the new key is not shifted.  With every |delta_s| <=
    Delta = max_s Delta_s each softmax weight changes by a factor within e^(+-2 Delta) (numerator e^(+-Delta), denominator
    e^(-+Delta)), so an output element sum_s p_s v_s moves by at most (e^(2 Delta) - 1) sum_s p_s |v_s| = (e^(2 Delta) - 1)
    absv.  The rounding of q' and of the new key at pos - d instead of pos is given no term of its own."""
    import math
    import decode_attn_ref as D
    H, KV, HD, pos = c.H, c.KV, c.HD, int(c.pos[0])
    q, k, v = D.split_row(c.qkv, H, KV, HD)
    qkv_rot = torch.cat([D.rotate(q, c.table, [pos]).reshape(1, -1), D.rotate(k, c.table, [pos]).reshape(1, -1), v.reshape(1, -1)], 1)
    kc = torch.zeros_like(c.kc)
    vc = torch.zeros_like(c.vc)
    kc[0, :, :pos - d], vc[0, :, :pos - d] = c.kc[0, :, d:pos], c.vc[0, :, d:pos]
    ref = D.ref_decode_attention(qkv_rot.contiguous(), kc, vc, [pos - d], H, KV, HD, table=None)
    b = key_bound(src, c.table, 0, d)[0]                                          # [KV, pos - d, HD]
    qk = D.rotate(q, c.table, [pos - d])[0].double().abs()                         # [H, HD]: the kernel's own query
    rep = H // KV
    delta = torch.stack([(qk[h][None, :] * b[h // rep]).sum(-1).max() if pos - d > 0 else torch.zeros((), dtype=F64)
                         for h in range(H)]) / math.sqrt(HD)                       # [H]
    extra = (torch.exp(2 * delta) - 1)[:, None] * ref.absv.reshape(H, HD)
    return ref, D.error_bound(ref) + extra.reshape(1, H * HD)


def shifted_caches(c, dst, d):
    """The case's caches with rows 0 .. pos-d-1 taken from a shifted history ``dst`` [1, 2, KV, pos - d, HD]; zeros elsewhere."""
    pos = int(c.pos[0])
    kc, vc = torch.zeros_like(c.kc), torch.zeros_like(c.vc)
    kc[0, :, :pos - d], vc[0, :, :pos - d] = dst[0, 0], dst[0, 1]
    return kc, vc


def invariance_ratio(out, ref, tol):
    """max |out - ref| / tolerance over the output elements (inf for a non-finite result)."""
    got = out.detach().cpu().double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref.out).abs() / tol.clamp(min=1e-300)).max())
