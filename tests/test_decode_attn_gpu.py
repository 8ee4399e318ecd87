"""The decode-step cache-attention kernels of csrc/generate.hip - csm_kv_append, csm_attn_decode, csm_attn_decode_rope,
csm_attn_decode_rope_at, csm_gemv_attn_bf16, csm_gemv_attn_at_bf16 - against the float64 reference of tests/decode_attn_ref.py
(proved against the oracle by tests/test_decode_attn_cpu.py).  Kernel level only: no model is built.

Bound on random data, per output element, derived from the kernels' rounding points and not from what they measure:
|got - ref| <= 2^-8 |ref| + 2^-16 sum_s p_s |v_s|  (decode_attn_ref.error_bound).  One-hot cases are exact: the output is the
value row of the target key, bit for bit.  Caches are compared with the reference's expected caches bit for bit everywhere.

"decode" below is csm_kv_append + csm_attn_decode on rows that are taken as already rotated (reference without a table);
"rope" is csm_attn_decode_rope on unrotated rows.  A rope case can be handed to "decode" after rotating its q and k with the
oracle (``_prerotated``)."""
import pytest
import torch

import decode_attn_ref as R
from decode_attn_ref import BF, GEOMS, Case

pytestmark = pytest.mark.gpu

_TABLES = {}
_IDENTITY = {}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _table(c, dev):
    key = tuple(c.table.shape)
    if key not in _TABLES:
        _TABLES[key] = c.table.to(dev).contiguous()
    return _TABLES[key]


def _prerotated(c):
    """The same attention problem with q and k rotated up front (by the oracle, rounded to bf16) and no table."""
    q, k, v = R.split_row(c.qkv, c.H, c.KV, c.HD)
    q, k = R.rotate(q, c.table, c.pos), R.rotate(k, c.table, c.pos)
    B = c.qkv.shape[0]
    qkv = torch.cat([q.reshape(B, -1), k.reshape(B, -1), v.reshape(B, -1)], 1).contiguous()
    return Case(qkv, c.kc, c.vc, c.pos, c.H, c.KV, c.HD, None, c.want)


def _row(c, b):
    return Case(c.qkv[b:b + 1].contiguous(), c.kc[b:b + 1].contiguous(), c.vc[b:b + 1].contiguous(), c.pos[b:b + 1].contiguous(),
                c.H, c.KV, c.HD, c.table, None if c.want is None else c.want[b:b + 1])


def _run(name, c, dev, W=None, res=None):
    """Launch kernel ``name`` on fresh device copies of the case; -> (out or y, kcache, vcache) on the device."""
    from csm.hip import check, lib, ops
    H, KV, HD = c.H, c.KV, c.HD
    B, s_max = c.qkv.shape[0], c.kc.shape[2]
    qkv, kc, vc, pos = c.qkv.to(dev), c.kc.to(dev), c.vc.to(dev), c.pos.to(dev)
    out = torch.full((B, H * HD), 7.0, dtype=BF, device=dev)
    if name == "append":
        ops.kv_append(qkv, kc, vc, pos, H, KV, HD)
    elif name == "decode_only":
        ops.attn_decode(qkv, kc, vc, out, pos, H, KV, HD)
    elif name == "decode":
        ops.kv_append(qkv, kc, vc, pos, H, KV, HD)
        ops.attn_decode(qkv, kc, vc, out, pos, H, KV, HD)
    elif name == "rope":
        ops.attn_decode_rope(qkv, kc, vc, out, pos, _table(c, dev), H, KV, HD)
    elif name == "rope_at":
        p = int(c.pos[0])
        assert all(int(x) == p for x in c.pos)
        check(lib.csm_attn_decode_rope_at(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), p, _table(c, dev).data_ptr(),
                                          B, H, KV, HD, s_max, qkv.stride(0), _stream()), "csm_attn_decode_rope_at")
    elif name in ("gemv_attn", "gemv_attn_at", "rope+gemv"):
        N = W.shape[0]
        y = torch.full((B, N), 7.0, dtype=BF, device=dev)
        if name == "gemv_attn":
            check(lib.csm_gemv_attn_bf16(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), pos.data_ptr(), _table(c, dev).data_ptr(),
                                         W.data_ptr(), y.data_ptr(), None if res is None else res.data_ptr(), B, N, H, KV, HD, s_max,
                                         qkv.stride(0), W.stride(0), y.stride(0), _stream()), "csm_gemv_attn_bf16")
        elif name == "gemv_attn_at":
            assert B == 1 and qkv.is_contiguous()
            check(lib.csm_gemv_attn_at_bf16(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), int(c.pos[0]), _table(c, dev).data_ptr(),
                                            W.data_ptr(), y.data_ptr(), None if res is None else res.data_ptr(), N, H, KV, HD, s_max,
                                            W.stride(0), _stream()), "csm_gemv_attn_at_bf16")
        else:
            ops.attn_decode_rope(qkv, kc, vc, out, pos, _table(c, dev), H, KV, HD)
            ops.gemv(out, W, y, residual=res)
        out = y
    else:
        raise KeyError(name)
    torch.cuda.synchronize()
    return out, kc, vc


def _ref(c):
    return R.ref_decode_attention(c.qkv, c.kc, c.vc, c.pos, c.H, c.KV, c.HD, c.table)


def _caches_ok(kc, vc, ref):
    return _same(kc, ref.kc) and _same(vc, ref.vc)


def _weights(H, HD, N, B, dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, H * HD, generator=g) * 0.05).to(BF)
    res = torch.randn(B, N, generator=g).to(BF)
    return W, res, W.to(dev), res.to(dev)


def _report(title, worst, failures):
    for k, v in worst.items():
        print(f"{title} {k}: worst |err| / bound {v:.3f}")
    assert not failures, failures[:8]


# --------------------------------------------------------------------------------------------------------- a. position sweep
@pytest.mark.parametrize("geom", list(GEOMS))
def test_position_sweep_random_vs_float64(dev, geom):
    """Every swept (S_max, position), randn data, both forms, against float64 within the derived bound; caches bit-equal to the
    expected ones.  Measured on one MI355X, worst |err| / bound over the 27 positions: csm_attn_decode 0.985 / 0.981 / 0.960 /
    0.979 and csm_attn_decode_rope 0.983 / 0.984 / 0.986 / 0.986 (backbone / decoder / tiny 64 / tiny 128).  That is the rounding
    of the result to bf16: the float64 result rounded exactly gives the same figures to three digits (tests/test_decode_attn_cpu.py
    ::test_error_bound_and_product_reference shows a value just above a power of two erring 2^-8 of itself)."""
    H, KV, HD = GEOMS[geom]
    worst, failures = {"decode": 0.0, "rope": 0.0}, []
    for s_max, pos in R.SWEEP_CASES:
        c = R.random_case(H, KV, HD, s_max, [pos])
        for name, case in (("decode", Case(*c[:7], None, None)), ("rope", c)):
            ref = _ref(case)
            out, kc, vc = _run(name, case, dev)
            r = R.worst_ratio(out, ref)
            worst[name] = max(worst[name], r)
            if not r <= 1.0:
                failures.append((name, s_max, pos, "ratio", r))
            if not _caches_ok(kc, vc, ref):
                failures.append((name, s_max, pos, "caches"))
    _report(f"sweep {geom}", worst, failures)


@pytest.mark.parametrize("geom", list(GEOMS))
def test_position_sweep_onehot_is_exact(dev, geom):
    """The softmax sits on one key s* (0, pos // 2, 255, 256, pos - 1, pos): every q head must return the value row of s* of its
    own kv head bit for bit - a dropped, duplicated or shifted key, or a wrong head, is a wrong row."""
    H, KV, HD = GEOMS[geom]
    failures, count = [], 0
    for s_max, pos in R.SWEEP_CASES:
        for s_star in R.onehot_targets(pos):
            for name, rope in (("decode", False), ("rope", True)):
                c = R.onehot_case(H, KV, HD, s_max, pos, s_star, rope=rope)
                out, kc, vc = _run(name, c, dev)
                count += 1
                if not _same(out, c.want):
                    got, want = out.cpu().float().view(H, HD), c.want.float().view(H, HD)
                    bad = [h for h in range(H) if not torch.equal(got[h], want[h])]
                    failures.append((name, s_max, pos, s_star, "heads", bad[:8], got[bad[0], :3].tolist(), want[bad[0], :3].tolist()))
                if not _caches_ok(kc, vc, _ref(c)):
                    failures.append((name, s_max, pos, s_star, "caches"))
    print(f"one-hot {geom}: {count} launches, {len(failures)} wrong")
    assert not failures, failures[:8]


# --------------------------------------------------------------------------------------------------------- b. batch rows
BATCH_POS = {1: [1024], 3: [2047, 0, 256], 4: [255, 2046, 1, 513],
             16: [0, 1, 7, 16, 31, 63, 64, 255, 256, 257, 511, 512, 1023, 1024, 2046, 2047]}


@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("B", [1, 3, 4, 16])
def test_batch_rows_equal_single_row_launches(dev, geom, B):
    H, KV, HD = GEOMS[geom]
    c = R.random_case(H, KV, HD, 2048, BATCH_POS[B], seed=B)
    worst, failures = {"decode": 0.0, "rope": 0.0}, []
    for name, case in (("decode", Case(*c[:7], None, None)), ("rope", c)):
        ref = _ref(case)
        out, kc, vc = _run(name, case, dev)
        worst[name] = R.worst_ratio(out, ref)
        if not worst[name] <= 1.0:
            failures.append((name, "ratio", worst[name]))
        if not _caches_ok(kc, vc, ref):
            failures.append((name, "caches"))
        for b in range(B):
            o1, k1, v1 = _run(name, _row(case, b), dev)
            if not (_same(o1[0], out[b]) and _same(k1[0], kc[b]) and _same(v1[0], vc[b])):
                failures.append((name, "row", b, BATCH_POS[B][b]))
    _report(f"batch {geom} B={B}", worst, failures)


# --------------------------------------------------------------------------------------------------------- c. stale slots
def _poison(t):
    pat = torch.tensor([float("nan"), float("inf"), float("-inf"), 3e38, -3e38], dtype=BF)
    return pat[torch.arange(t.numel()) % 5].view(t.shape)


def _poisoned(c, include_pos):
    kc, vc = c.kc.clone(), c.vc.clone()
    for b, p in enumerate(c.pos.tolist()):
        lo = p if include_pos else p + 1
        kc[b, :, lo:] = _poison(kc[b, :, lo:])
        vc[b, :, lo:] = _poison(vc[b, :, lo:])
    return c._replace(kc=kc, vc=vc)


STALE = [("decode", "backbone", 2048, [300, 0]), ("rope", "backbone", 2048, [300, 0]), ("decode", "decoder", 2048, [17, 2046]),
         ("rope", "decoder", 2048, [17, 2046]), ("rope", "tiny64", 96, [94, 1]), ("rope", "tiny128", 96, [0, 64]),
         ("rope_at", "decoder", 32, [9, 9]), ("rope_at", "decoder", 17, [0, 0]), ("gemv_attn", "decoder", 32, [30, 3, 0]),
         ("gemv_attn", "tiny128", 64, [40, 63]), ("gemv_attn_at", "decoder", 32, [12]), ("gemv_attn_at", "decoder", 8, [0])]


@pytest.mark.parametrize("name,geom,s_max,posv", STALE)
def test_stale_slots_are_never_read(dev, name, geom, s_max, posv):
    """What a truncated conversation or a scripted EOS leaves above pos: NaN, +-Inf and 3e38 there (for the fused kernels in row pos
    too: it is overwritten, not read) give the bits of the run with zeros there; rows < pos are never poisoned."""
    H, KV, HD = GEOMS[geom]
    c = R.random_case(H, KV, HD, s_max, posv, seed=11)
    if name == "decode":
        c = Case(*c[:7], None, None)
    W = res = None
    if name.startswith("gemv_attn"):
        _, _, W, res = _weights(H, HD, 264, len(posv), dev)
    assert R.reads_are_finite(c)
    clean = _run(name, c, dev, W, res)
    bad = _poisoned(c, include_pos=(name != "decode"))
    assert R.reads_are_finite(bad)
    dirty = _run(name, bad, dev, W, res)
    assert bool(torch.isfinite(dirty[0].float()).all()) and _same(dirty[0], clean[0]), (name, geom, posv)
    for b, p in enumerate(posv):
        for i in (1, 2):
            assert _same(dirty[i][b, :, :p + 1], clean[i][b, :, :p + 1]), (name, "rows <= pos", b)
            assert _same(dirty[i][b, :, p + 1:], (bad.kc, bad.vc)[i - 1][b, :, p + 1:]), (name, "rows > pos keep their bits", b)


# --------------------------------------------------------------------------------------------------------- d. cache writes
WRITES = [("append", "backbone", 96, [95, 5, 0]), ("append", "decoder", 2048, [2047, 0, 700]), ("append", "tiny64", 96, [40, 95, 95]),
          ("rope", "backbone", 96, [95, 5, 0]), ("rope", "decoder", 2048, [2047, 0, 700]), ("rope", "tiny64", 96, [0, 95, 94]),
          ("rope", "tiny128", 8192, [8191, 4095, 1]), ("rope_at", "decoder", 32, [31, 31, 31]), ("rope_at", "decoder", 17, [16, 16, 16]),
          ("rope_at", "decoder", 8, [3, 3, 3]), ("gemv_attn", "decoder", 32, [31, 0, 7]), ("gemv_attn", "tiny128", 64, [63, 62, 0]),
          ("gemv_attn_at", "decoder", 32, [31]), ("gemv_attn_at", "decoder", 17, [16]), ("gemv_attn_at", "decoder", 32, [5]),
          ("decode_only", "backbone", 96, [95, 5, 0]), ("decode_only", "decoder", 2048, [2047, 0, 700])]


@pytest.mark.parametrize("name,geom,s_max,posv", WRITES)
def test_cache_write_discipline(dev, name, geom, s_max, posv):
    """Guard pattern in every cache element the history does not own: afterwards the caches are the expected ones bit for bit -
    row pos of each (b, kv head) and nothing else, the head that follows in memory at pos = S_max - 1 and the other batch rows
    included.  csm_attn_decode alone writes nothing."""
    H, KV, HD = GEOMS[geom]
    c = R.random_case(H, KV, HD, s_max, posv, seed=21, fill=R.GUARD)
    if name in ("append", "decode_only"):
        c = Case(*c[:7], None, None)
    W = res = None
    if name.startswith("gemv_attn"):
        _, _, W, res = _weights(H, HD, 264, len(posv), dev)
    ref = _ref(c)
    _, kc, vc = _run(name, c, dev, W, res)
    if name == "decode_only":
        assert _same(kc, c.kc) and _same(vc, c.vc)
        return
    assert not _same(ref.kc, c.kc)
    changed = (_bits(kc) != _bits(c.kc)).any(-1)                                  # [B, KV, S_max]: rows that changed at all
    for b, p in enumerate(posv):
        rows = changed[b].nonzero()[:, 1].unique().tolist()
        assert rows == [p], (name, geom, b, p, rows[:8])
    assert _caches_ok(kc, vc, ref), (name, geom, posv)


# --------------------------------------------------------------------------------------------------------- e. softmax range
@pytest.mark.parametrize("geom", ["backbone", "decoder"])
def test_softmax_range(dev, geom):
    """One score about 200 above the rest, all scores equal, all scores about -300, q = 0: finite and within the bound (its second
    term times max(1, max|score| / 8): the fp32 error of a score grows with its magnitude); the spike, equal-score and q = 0 cases
    are exact by construction (the spiked key's value row; 1.5, the mean of the values)."""
    H, KV, HD = GEOMS[geom]
    worst, failures = {"decode": 0.0, "rope": 0.0}, []
    for pos in R.RANGE_POS:
        for kind in ("spike", "equal", "low", "zero_q"):
            c = R.range_case(kind, H, KV, HD, pos)
            for name, case in (("decode", _prerotated(c)), ("rope", c)):
                ref = _ref(case)
                out, kc, vc = _run(name, case, dev)
                r = R.worst_ratio(out, ref, score_scaled=True)
                print(f"range {geom} {name} pos={pos} {kind}: |err| / bound {r:.3f}, max |score| {max(float(s.abs().max()) for s in ref.scores):.1f}")
                worst[name] = max(worst[name], r)
                if not (bool(torch.isfinite(out.float()).all()) and r <= 1.0):
                    failures.append((name, pos, kind, "ratio", r))
                if c.want is not None and not _same(out, c.want):
                    failures.append((name, pos, kind, "not exact", out.float().flatten()[:4].tolist()))
                if not _caches_ok(kc, vc, ref):
                    failures.append((name, pos, kind, "caches"))
    _report(f"range {geom}", worst, failures)


# --------------------------------------------------------------------------------------------------------- f. padded rows
PADDED = [("decode", g, 96, [70, 0, 95]) for g in GEOMS] + [("rope", g, 96, [70, 0, 95]) for g in GEOMS] + \
         [("rope_at", "decoder", 32, [13] * 4), ("gemv_attn", "decoder", 32, [31, 2, 16]), ("gemv_attn", "tiny128", 64, [50, 7])]


@pytest.mark.parametrize("name,geom,s_max,posv", PADDED)
def test_padded_qkv_rows(dev, name, geom, s_max, posv):
    """Row stride (H + 2 KV) HD + 64 with NaN in the padding: the bits of the dense layout."""
    H, KV, HD = GEOMS[geom]
    padded = R.random_case(H, KV, HD, s_max, posv, pad=64, seed=31)
    dense = R.random_case(H, KV, HD, s_max, posv, seed=31)
    assert padded.qkv.stride(0) == (H + 2 * KV) * HD + 64 and padded.qkv.stride(0) % 8 == 0 and bool(padded.qkv[:, -64:].isnan().all())
    assert torch.equal(padded.qkv[:, :-64], dense.qkv)
    if name == "decode":
        padded, dense = Case(*padded[:7], None, None), Case(*dense[:7], None, None)
    W = res = None
    if name.startswith("gemv_attn"):
        _, _, W, res = _weights(H, HD, 264, len(posv), dev)
    a, b = _run(name, padded, dev, W, res), _run(name, dense, dev, W, res)
    assert bool(torch.isfinite(a[0].float()).all())
    assert all(_same(x, y) for x, y in zip(a, b)), (name, geom)
    assert _caches_ok(a[1], a[2], _ref(dense))


# --------------------------------------------------------------------------------------------------------- g. accepted shapes
def _check_product(name, c, dev, Wc, rc, Wd, rd, worst, failures, tag):
    """A product kernel: its own attention - read out through W = identity without a residual, where y is the bf16 attention
    vector itself - within the bound of the sweep; bit-equal (output and caches) to csm_attn_decode_rope + csm_gemv_bf16, whose
    attention is within the bound too; the product within 1e-2 max|ref| of attention-rounded-to-bf16 . W + residual in float64."""
    ref = _ref(c)
    K = c.H * c.HD
    if (str(dev), K) not in _IDENTITY:
        _IDENTITY[(str(dev), K)] = torch.eye(K, dtype=BF, device=dev)
    own, ki, vi = _run(name, c, dev, _IDENTITY[(str(dev), K)], None)
    r = R.worst_ratio(own, ref)
    worst["own attention (W = I)"] = max(worst.get("own attention (W = I)", 0.0), r)
    if not r <= 1.0:
        failures.append((tag, "own attention ratio", r))
    if not _caches_ok(ki, vi, ref):
        failures.append((tag, "caches (W = I)"))
    y, kc, vc = _run(name, c, dev, Wd, rd)
    y2, k2, v2 = _run("rope+gemv", c, dev, Wd, rd)
    att, _, _ = _run("rope", c, dev)
    r = R.worst_ratio(att, ref)
    worst["csm_attn_decode_rope on the same case"] = max(worst.get("csm_attn_decode_rope on the same case", 0.0), r)
    if not r <= 1.0:
        failures.append((tag, "csm_attn_decode_rope ratio", r))
    want = R.ref_product(ref.out, Wc, rc)
    e = float((y.cpu().double() - want).abs().max() / want.abs().max())
    worst["product / (1e-2 max|ref|)"] = max(worst.get("product / (1e-2 max|ref|)", 0.0), e / 1e-2)
    if not (bool(torch.isfinite(y.float()).all()) and e <= 1e-2):
        failures.append((tag, "product", e))
    if not (_same(y, y2) and _same(kc, k2) and _same(vc, v2)):
        failures.append((tag, "not the bits of rope + gemv"))
    if not _caches_ok(kc, vc, ref):
        failures.append((tag, "caches"))


@pytest.mark.parametrize("geom,N", [("decoder", 1024), ("tiny128", 204)])
def test_gemv_attn_every_position_of_a_64_slot_cache(dev, geom, N):
    """csm_gemv_attn_bf16 keeps one key per lane of a wave: S_max 64 at every position 0 .. 63 with B = 1 .. 4 ragged rows, and
    S_max 33 at 0, 31, 32."""
    H, KV, HD = GEOMS[geom]
    worst, failures = {}, []
    for B in (1, 2, 3, 4):
        Wc, rc, Wd, rd = _weights(H, HD, N, B, dev, seed=40 + B)
        for s_max, p0s in ((64, range(64)), (33, (0, 31, 32))):
            for p0 in p0s:
                posv = [(p0 + 17 * b) % s_max for b in range(B)]
                c = R.random_case(H, KV, HD, s_max, posv, seed=41)
                _check_product("gemv_attn", c, dev, Wc, rc, Wd, rd, worst, failures, (B, s_max, posv))
    _report(f"gemv_attn {geom}", worst, failures)


def test_at_kernels_every_position_of_small_caches(dev):
    """The host-position forms accept any 1 <= S_max <= 32: S_max 1, 8, 17, 31, 32 at every position - csm_attn_decode_rope_at
    (B = 1, 4, 16) within the bound and bit-equal to csm_attn_decode_rope, csm_gemv_attn_at_bf16 as the other product kernel."""
    H, KV, HD = GEOMS["decoder"]
    worst, failures = {"rope_at": 0.0}, []
    Wc, rc, Wd, rd = _weights(H, HD, 1024, 1, dev, seed=50)
    for s_max in (1, 8, 17, 31, 32):
        for p in range(s_max):
            for B in (1, 4, 16):
                c = R.random_case(H, KV, HD, s_max, [p] * B, seed=51 + B)
                ref = _ref(c)
                out, kc, vc = _run("rope_at", c, dev)
                o2, k2, v2 = _run("rope", c, dev)
                r = R.worst_ratio(out, ref)
                worst["rope_at"] = max(worst["rope_at"], r)
                if not r <= 1.0:
                    failures.append(("rope_at", s_max, p, B, "ratio", r))
                if not (_same(out, o2) and _same(kc, k2) and _same(vc, v2)):
                    failures.append(("rope_at", s_max, p, B, "not the bits of csm_attn_decode_rope"))
                if not _caches_ok(kc, vc, ref):
                    failures.append(("rope_at", s_max, p, B, "caches"))
            c = R.random_case(H, KV, HD, s_max, [p], seed=52)
            _check_product("gemv_attn_at", c, dev, Wc, rc, Wd, rd, worst, failures, ("gemv_attn_at", s_max, p))
            y, _, _ = _run("gemv_attn_at", c, dev, Wd, rd)
            y3, _, _ = _run("gemv_attn", c, dev, Wd, rd)
            if not _same(y, y3):
                failures.append(("gemv_attn_at", s_max, p, "not the bits of csm_gemv_attn_bf16"))
    _report("host-position kernels", worst, failures)


# --------------------------------------------------------------------------------------------------------- h. refusals
def test_bad_arguments_are_refused_before_any_launch(dev):
    """Every entry point returns 1 with a message for a null pointer, head_dim 96, H % KV != 0, an S_max above its limit or 0, a row stride that is
    not a multiple of 8 and - the host-position forms - a position outside [0, S_max); output and caches keep their bits.  Positions that live in device memory
    cannot be validated by the host and are never passed out of range here."""
    from csm.hip import lib
    H, KV, HD, s_max, N = 8, 2, 128, 32, 64
    c = R.random_case(H, KV, HD, s_max, [5, 5], seed=61, fill=0.5)
    qkv, kc, vc, pos, table = c.qkv.to(dev), c.kc.to(dev), c.vc.to(dev), c.pos.to(dev), _table(c, dev)
    out = torch.full((2, H * HD), 3.0, dtype=BF, device=dev)
    y = torch.full((2, N), 3.0, dtype=BF, device=dev)
    W = torch.zeros(N, H * HD, dtype=BF, device=dev)
    st, LD = _stream(), qkv.stride(0)
    Q, K, V, O, P, T, Wp, Y = (t.data_ptr() for t in (qkv, kc, vc, out, pos, table, W, y))

    def append(q=Q, k=K, v=V, p=P, h=H, kv=KV, hd=HD, s=s_max, ld=LD):
        return lib.csm_kv_append(q, k, v, p, 2, h, kv, hd, s, ld, st)

    def decode(q=Q, k=K, v=V, o=O, p=P, h=H, kv=KV, hd=HD, s=s_max, ld=LD):
        return lib.csm_attn_decode(q, k, v, o, p, 2, h, kv, hd, s, ld, st)

    def rope(q=Q, k=K, v=V, o=O, p=P, t=T, h=H, kv=KV, hd=HD, s=s_max, ld=LD):
        return lib.csm_attn_decode_rope(q, k, v, o, p, t, 2, h, kv, hd, s, ld, st)

    def rope_at(q=Q, k=K, v=V, o=O, p=5, t=T, h=H, kv=KV, hd=HD, s=s_max, ld=LD):
        return lib.csm_attn_decode_rope_at(q, k, v, o, p, t, 2, h, kv, hd, s, ld, st)

    def gemv_attn(q=Q, k=K, v=V, p=P, t=T, w=Wp, yy=Y, h=H, kv=KV, hd=HD, s=s_max, ld=LD):
        return lib.csm_gemv_attn_bf16(q, k, v, p, t, w, yy, None, 2, N, h, kv, hd, s, ld, H * HD, N, st)

    def gemv_attn_at(q=Q, k=K, v=V, p=5, t=T, w=Wp, yy=Y, h=H, kv=KV, hd=HD, s=s_max):
        return lib.csm_gemv_attn_at_bf16(q, k, v, p, t, w, yy, None, N, h, kv, hd, s, H * HD, st)

    def refused(rc, what, text=None):
        msg = lib.csm_last_error()
        assert rc == 1 and msg, (what, rc, msg)
        assert text is None or text in msg, (what, msg)

    limits = {append: 8192, decode: 8192, rope: 8192, rope_at: 32, gemv_attn: 64, gemv_attn_at: 32}
    for fn, limit in limits.items():
        tag = fn.__name__
        for null in ("q", "k", "v"):
            refused(fn(**{null: None}), (tag, "null", null))
        refused(fn(hd=96), (tag, "head_dim 96"))
        refused(fn(h=7), (tag, "H % KV"))
        refused(fn(s=limit + 1), (tag, "S_max"))
        refused(fn(s=0), (tag, "S_max 0"))
    for fn in (append, decode, rope, rope_at, gemv_attn):                       # 16-byte loads from qkv + b * ld
        assert LD % 8 == 0
        refused(fn(ld=LD + 4), (fn.__name__, "ld % 8"))
    for fn in (decode, rope, rope_at):
        refused(fn(o=None), (fn.__name__, "null out"))
    for fn in (append, decode, rope, gemv_attn):
        refused(fn(p=None), (fn.__name__, "null pos"))
    for fn in (rope, rope_at, gemv_attn, gemv_attn_at):
        refused(fn(t=None), (fn.__name__, "null table"))
    for fn in (gemv_attn, gemv_attn_at):
        refused(fn(w=None), (fn.__name__, "null W"))
        refused(fn(yy=None), (fn.__name__, "null y"))
    for fn in (rope_at, gemv_attn_at):
        for p in (-1, s_max, s_max + 100):
            refused(fn(p=p), (fn.__name__, "position", p), b"outside the cache")
        refused(fn(p=8, s=8), (fn.__name__, "position = S_max"), b"outside the cache")
    refused(decode(hd=96), "decode hd", b"head_dim 96 unsupported")
    refused(append(hd=96), "append hd", b"head_dim 96 unsupported")
    refused(rope_at(h=4), "rope_at H = 4 KV", b"unsupported shape")
    refused(gemv_attn_at(h=4, kv=2), "gemv_attn_at H HD = 1024", b"unsupported shape")
    torch.cuda.synchronize()
    assert _same(kc, c.kc) and _same(vc, c.vc) and bool((out == 3.0).all()) and bool((y == 3.0).all())      # nothing was launched
    # and the arguments the refusals varied are fine as they stand
    for fn in limits:
        assert fn() == 0, fn.__name__
    torch.cuda.synchronize()
    assert not _same(kc, c.kc) and not bool((out == 3.0).all()) and not bool((y == 3.0).all())

