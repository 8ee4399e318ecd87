"""The float64 decode-attention reference and its case generators (tests/decode_attn_ref.py), checked on the CPU before any kernel
is judged by them (tests/test_decode_attn_gpu.py): the reference against the oracle's own causal attention, the one-hot
condition for every case the GPU file runs, and the finiteness of everything the reference reads."""
import pytest
import torch

import decode_attn_ref as R
from decode_attn_ref import BF, GEOMS


def _oracle_row(q, k, v, table):
    """Row S-1 of oracle.attention over S positions (fp32): q [S,H,HD] / k, v [S,KV,HD] bf16, rotated by the oracle as the
    library rotates (rounded to bf16)."""
    O = R.oracle()
    S = q.shape[0]
    if table is not None:
        pos = torch.arange(S).view(1, S)
        q, k = O.rope(q[None], table, pos)[0], O.rope(k[None], table, pos)[0]
    return O.attention(q[None].float(), k[None].float(), v[None].float(), causal=True)[0, S - 1].reshape(-1), k


@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("rope", [False, True])
def test_reference_is_a_row_of_the_oracles_causal_attention(geom, rope):
    H, KV, HD = GEOMS[geom]
    s_max = 80
    table = R.rope_table(s_max, HD) if rope else None
    g = torch.Generator().manual_seed(3)
    for p in (0, 1, 17, 64, 79):
        S = p + 1
        q = torch.randn(S, H, HD, generator=g).to(BF)
        k = torch.randn(S, KV, HD, generator=g).to(BF)
        v = torch.randn(S, KV, HD, generator=g).to(BF)
        want, k_rot = _oracle_row(q, k, v, table)
        # the decode view of the same problem: rotated keys 0 .. p-1 in the cache, position p in the fused row (unrotated)
        kc = torch.full((1, KV, s_max, HD), float("nan"), dtype=BF)
        vc = torch.full((1, KV, s_max, HD), float("nan"), dtype=BF)
        kc[0, :, :p], vc[0, :, :p] = k_rot[:p].transpose(0, 1), v[:p].transpose(0, 1)
        qkv = torch.cat([q[p].reshape(-1), k[p].reshape(-1), v[p].reshape(-1)])[None]
        ref = R.ref_decode_attention(qkv, kc, vc, [p], H, KV, HD, table)
        err = (ref.out[0] - want.double()).abs().max().item()
        assert err <= 2e-6 * max(1.0, want.abs().max().item()), (geom, rope, p, err)     # fp32 accuracy of the oracle
        # expected caches: row p of every kv head replaced by the (rotated) key and the value, NaN everywhere from p + 1 on
        assert torch.equal(ref.kc[0, :, p], k_rot[p]) and torch.equal(ref.vc[0, :, p], v[p])
        assert torch.equal(ref.kc[0, :, :p], kc[0, :, :p]) and bool(ref.kc[0, :, p + 1:].isnan().all())
        assert torch.equal(ref.vc[0, :, :p], vc[0, :, :p]) and bool(ref.vc[0, :, p + 1:].isnan().all())
        assert abs(float(ref.probs[0].sum(-1).min()) - 1.0) < 1e-12
        assert bool((ref.absv >= ref.out.abs() - 1e-12).all())


@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("rope", [False, True])
def test_onehot_condition_holds_for_every_swept_case(geom, rope):
    H, KV, HD = GEOMS[geom]
    worst, count = 0.0, 0
    for s_max, pos in R.SWEEP_CASES:
        for s_star in R.onehot_targets(pos):
            c = R.onehot_case(H, KV, HD, s_max, pos, s_star, rope=rope)
            assert R.reads_are_finite(c)
            assert bool((c.vc[0, :, :pos] != 0).all()) and bool((R.split_row(c.qkv, H, KV, HD)[2] != 0).all())
            ref = R.ref_decode_attention(c.qkv, c.kc, c.vc, c.pos, H, KV, HD, c.table)
            m = R.onehot_margin(c, ref, s_star)
            assert m <= 2.0 ** -12, (geom, rope, s_max, pos, s_star, m)
            assert float(ref.scores[0][:, s_star].min()) >= R.ONEHOT_SCORE * 0.999
            assert torch.equal(ref.out.float().to(BF), c.want), (geom, rope, s_max, pos, s_star)
            assert torch.equal(c.want.double().to(BF), c.want)                           # bf16-exact by construction
            worst, count = max(worst, m), count + 1
    print(f"one-hot {geom} rope={rope}: {count} cases, worst off-target share {worst:.3e} (limit {2.0 ** -12:.3e})")


def test_value_pattern_rows_are_distinct():
    for KV, s_max, HD in ((8, 8192, 64), (2, 2048, 128), (1, 96, 128)):
        v = R.value_pattern(KV, s_max, HD)
        assert bool((v >= 1).all()) and bool((v < 2).all()) and torch.equal(v.double().to(BF), v)
        for g in range(KV):                                                              # every slot of a head has its own row
            assert torch.unique(v[g].view(torch.int16), dim=0).shape[0] == s_max
        for g in range(1, KV):                                                           # and the heads differ at every slot
            assert bool((v[g] != v[0]).any(dim=-1).all())
        assert bool((v[:, 1:, 0] != v[:, :-1, 0]).all())                                 # a slot off by one shows in column 0


@pytest.mark.parametrize("geom", ["backbone", "decoder"])
def test_softmax_range_cases(geom):
    H, KV, HD = GEOMS[geom]
    for pos in R.RANGE_POS:
        c = R.range_case("spike", H, KV, HD, pos)
        ref = R.ref_decode_attention(c.qkv, c.kc, c.vc, c.pos, H, KV, HD, c.table)
        assert R.reads_are_finite(c) and torch.equal(ref.out.float().to(BF), c.want)
        top = ref.scores[0][:, pos // 2]
        if pos:
            rest = torch.cat([ref.scores[0][:, :pos // 2], ref.scores[0][:, pos // 2 + 1:]], 1).amax(-1)
            assert 130.0 <= float((top - rest).min()) and float((top - rest).max()) <= 300.0          # 'about 200 above the rest'
            assert R.onehot_margin(c, ref, pos // 2) <= 2.0 ** -12
        for kind in ("equal", "zero_q"):
            c = R.range_case(kind, H, KV, HD, pos)
            ref = R.ref_decode_attention(c.qkv, c.kc, c.vc, c.pos, H, KV, HD, c.table)
            assert R.reads_are_finite(c)
            s = ref.scores[0]
            assert float((s - s[:, :1]).abs().max()) <= 1e-12, (kind, pos)
            assert float((ref.out - 1.5).abs().max()) <= 1e-12 and bool((c.want == 1.5).all())
        c = R.range_case("low", H, KV, HD, pos)
        ref = R.ref_decode_attention(c.qkv, c.kc, c.vc, c.pos, H, KV, HD, c.table)
        assert R.reads_are_finite(c) and bool(torch.isfinite(ref.out).all())
        assert float(ref.scores[0].max()) <= -200.0, float(ref.scores[0].max())


def test_random_cases_are_seeded_and_finite():
    H, KV, HD = GEOMS["tiny64"]
    a = R.random_case(H, KV, HD, 96, [70, 0, 95], pad=64, fill=R.GUARD)
    b = R.random_case(H, KV, HD, 96, [70, 0, 95], pad=64, fill=R.GUARD)
    assert torch.equal(a.qkv.view(torch.int16), b.qkv.view(torch.int16)) and torch.equal(a.kc, b.kc) and torch.equal(a.vc, b.vc)
    assert R.reads_are_finite(a) and bool(a.qkv[:, -64:].isnan().all())
    assert bool((a.kc[1] == R.GUARD).all()) and bool((a.kc[0, :, 70:] == R.GUARD).all())
    dense = R.random_case(H, KV, HD, 96, [70, 0, 95])
    assert torch.equal(dense.qkv, a.qkv[:, :-64])
    ra = R.ref_decode_attention(a.qkv, a.kc, a.vc, a.pos, H, KV, HD, a.table)
    rd = R.ref_decode_attention(dense.qkv, dense.kc, dense.vc, dense.pos, H, KV, HD, dense.table)
    assert torch.equal(ra.out, rd.out)                                                   # padding and unused rows are never read
    # a batch row of the reference is the one-row reference
    one = R.ref_decode_attention(a.qkv[2:3], a.kc[2:3], a.vc[2:3], a.pos[2:3], H, KV, HD, a.table)
    assert torch.equal(one.out[0], ra.out[2]) and torch.equal(one.kc[0], ra.kc[2])


def test_error_bound_and_product_reference():
    H, KV, HD = GEOMS["tiny128"]
    c = R.random_case(H, KV, HD, 64, [40])
    ref = R.ref_decode_attention(c.qkv, c.kc, c.vc, c.pos, H, KV, HD, c.table)
    exact = ref.out.float().to(BF)
    # one correct rounding to bf16 (8-bit significand) errs up to 2^-8 of a value just above a power of two: the first term alone
    assert 0.25 < R.worst_ratio(exact, ref) <= 1.0
    assert R.worst_ratio(exact * 1.02, ref) > 1.0 and R.worst_ratio(exact * float("nan"), ref) == float("inf")
    W = torch.randn(24, H * HD, generator=torch.Generator().manual_seed(1)).to(BF)
    res = torch.randn(1, 24, generator=torch.Generator().manual_seed(2)).to(BF)
    y = R.ref_product(ref.out, W, res)
    assert torch.allclose(y, exact.double() @ W.double().t() + res.double(), rtol=0, atol=1e-12)
