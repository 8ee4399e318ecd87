"""csm_kv_shift (csrc/generate.hip), kernel level through the C ABI, against the float64 reference of tests/kv_shift_ref.py (proved
by tests/test_kv_shift_ref_cpu.py).  No model is built.

dst lies inside a larger buffer of a bf16-exact guard pattern and EVERY element of that buffer is judged: the head, every V and
the guards bit for bit, the shifted keys within the helper's bound (half a bf16 ulp at |ref| + slack, plus slack = 3U (|x0 c| +
|x1 s|): derived in kv_shift_ref's docstring).  src is compared with what it was before the launch.

Measured on one MI355X: worst |err| / bound over all cases 0.9999 (``RATIO csm_kv_shift``: the bound is half an ulp and the
kernel rounds to nearest, so the ratio sits just below 1); three consecutive shifts leave the keys at 0.60 of the drift bound
(``DRIFT``, information); the invariance cases reach at most 0.17 of their tolerance."""
import pytest
import torch

import kv_shift_ref as R
from train_ops_ref import judge

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
_WORST = {"ratio": 0.0}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _table(hd, dev, _cache={}):
    if hd not in _cache:
        _cache[hd] = R.rope_table(R.TABLE_ROWS, hd).to(dev).contiguous()
    return _cache[hd]


def _call(src_ptr, dst_ptr, table_ptr, rows, layers, KV, HD, length, keep, drop):
    from csm.hip import lib
    rc = lib.csm_kv_shift(src_ptr, dst_ptr, table_ptr, rows, layers, KV, HD, length, keep, drop, _stream())
    torch.cuda.synchronize()
    return rc


def _shift(src_dev, keep, drop, dev):
    """Launch on a device history; -> (dst on the CPU, the whole guarded buffer on the CPU, its dst slice bounds)."""
    layers, _, KV, length, HD = src_dev.shape
    n = layers * 2 * KV * (length - drop) * HD
    buf = torch.full((R.PAD + n + R.PAD,), R.GUARD, dtype=BF, device=dev)
    rc = _call(src_dev.data_ptr(), buf.data_ptr() + 2 * R.PAD, _table(HD, dev).data_ptr(), R.TABLE_ROWS, layers, KV, HD, length, keep, drop)
    assert rc == 0, rc
    host = buf.cpu()
    return host[R.PAD:R.PAD + n].view(layers, 2, KV, length - drop, HD), host, n


def _judge_all(name, src, keep, drop, dev):
    """One launch, every element of the guarded buffer judged; -> (worst ratio, dst)."""
    src_dev = src.to(dev)
    dst, host, n = _shift(src_dev, keep, drop, dev)
    guard = torch.full((R.PAD,), R.GUARD, dtype=BF)
    judge(f"{name}.guard_before", host[:R.PAD], guard, None)
    judge(f"{name}.guard_after", host[R.PAD + n:], guard, None)
    assert host.numel() == 2 * R.PAD + dst.numel()
    assert torch.equal(src_dev.cpu().view(torch.int16), src.view(torch.int16)), "src was written"
    return R.judge_shift(name, dst, src, R.rope_table(R.TABLE_ROWS, src.shape[4]), keep, drop), dst


@pytest.mark.parametrize("case", R.CASES + [R.LATE], ids=lambda c: "x".join(map(str, c)))
def test_kv_shift_against_reference(dev, case):
    layers, KV, HD, length, keep, drop = case
    worst, _ = _judge_all("csm_kv_shift", R.random_src(layers, KV, HD, length), keep, drop, dev)
    _WORST["ratio"] = max(_WORST["ratio"], worst)
    print(f"RATIO csm_kv_shift {worst:.4f} {case}")
    assert worst <= 1.0


def test_kv_shift_ops_wrapper_and_many_planes(dev):
    """``ops.kv_shift`` (a new tensor, the parked one untouched) at the CSM-1B plane count: 16 layers x 8 kv heads."""
    from csm.hip import ops
    src = R.random_src(16, 8, 64, 21, seed=3)
    src_dev = src.to(dev)
    out = ops.kv_shift(src_dev, _table(64, dev), 2, 5)
    torch.cuda.synchronize()
    assert out.shape == (16, 2, 8, 16, 64) and out.is_contiguous() and out.data_ptr() != src_dev.data_ptr()
    assert torch.equal(src_dev.cpu().view(torch.int16), src.view(torch.int16))
    worst = R.judge_shift("ops.kv_shift", out.cpu(), src, R.rope_table(R.TABLE_ROWS, 64), 2, 5)
    _WORST["ratio"] = max(_WORST["ratio"], worst)
    assert worst <= 1.0


def test_three_consecutive_shifts(dev):
    """Each shift is judged from the device's own previous state, so the bounds do not compound.  Information: the drift of the
    final keys against rope(k_raw, final position) in float64 over its bound - (shifts + 1) half ulps (the cache's own rounding
    and one per shift, taken at the pair's magnitude) plus the table term 2^-13 |k| (``kv_shift_ref.drift_ratio``)."""
    layers, KV, HD, length = 2, 2, 64, 40
    table = R.rope_table(R.TABLE_ROWS, HD)
    g = torch.Generator().manual_seed(77)
    k_raw = torch.randn(layers, KV, length, HD, generator=g).to(BF)
    v = torch.randn(layers, KV, length, HD, generator=g).to(BF)
    state = torch.stack([R.rotated_keys(k_raw, table, 0), v], 1).contiguous()     # [layers, 2, KV, len, HD] as a cache holds it
    where = torch.arange(length)                                                 # the original position of each row
    keep, shifts = 1, (3, 5, 2)
    for i, drop in enumerate(shifts):
        worst, dst = _judge_all(f"shift{i}", state, keep, drop, dev)
        _WORST["ratio"] = max(_WORST["ratio"], worst)
        assert worst <= 1.0
        state = dst.contiguous()
        where = torch.cat([where[:keep], where[keep + drop:]])
    assert state.shape[3] == length - sum(shifts) == where.numel()
    assert torch.equal(state[:, 1].view(torch.int16), v[:, :, where].contiguous().view(torch.int16))           # values: never touched
    # final keys against the raw keys rotated, in float64, for the positions they now hold
    drift = R.drift_ratio(state[:, 0, :, keep:], k_raw[:, :, where][:, :, keep:], table[keep:], len(shifts))
    print(f"DRIFT csm_kv_shift {drift:.4f} after {len(shifts)} shifts (information)")
    print(f"RATIO csm_kv_shift {_WORST['ratio']:.4f} (all cases so far)")
    assert torch.equal(state[:, 0, :, :keep].view(torch.int16), R.rotated_keys(k_raw, table, 0)[:, :, :keep].contiguous().view(torch.int16))


def test_kv_shift_refusals(dev):
    """Every refusal returns 1 with a csm_kv_shift message and launches nothing: valid buffers stand behind each probe and dst
    keeps its guard pattern."""
    from csm.hip import lib
    layers, KV, HD, length = 2, 2, 64, 20
    src = R.random_src(layers, KV, HD, length).to(dev)
    big = torch.full((2 * src.numel() + 64,), R.GUARD, dtype=BF, device=dev)     # dst, and room to make it overlap or misalign
    tab = _table(HD, dev)
    s, d, t = src.data_ptr(), big.data_ptr(), tab.data_ptr()
    ok = dict(src=s, dst=d, table=t, rows=R.TABLE_ROWS, layers=layers, KV=KV, HD=HD, length=length, keep=3, drop=4)
    nbytes = src.numel() * 2
    inside = torch.cat([src.reshape(-1), torch.full((src.numel(),), R.GUARD, dtype=BF, device=dev)])      # src with room behind it
    probes = {
        "null src": dict(src=None), "null dst": dict(dst=None), "null table": dict(table=None),
        "HD 32": dict(HD=32), "HD 96": dict(HD=96), "layers 0": dict(layers=0), "KV 0": dict(KV=0),
        "drop 0": dict(drop=0), "drop -1": dict(drop=-1), "keep -1": dict(keep=-1),
        "keep + drop > len": dict(keep=17, drop=4), "nothing left": dict(keep=0, drop=length),
        "drop = table_rows": dict(rows=4), "drop > table_rows": dict(rows=3),
        "src misaligned": dict(src=s + 2), "dst misaligned": dict(dst=d + 2), "dst 8-byte aligned": dict(dst=d + 8),
        "dst = src": dict(src=inside.data_ptr(), dst=inside.data_ptr()),
        "dst inside src": dict(src=inside.data_ptr(), dst=inside.data_ptr() + nbytes - 16),
        "dst ends inside src": dict(src=inside.data_ptr() + 32, dst=inside.data_ptr()),
    }
    for name, change in probes.items():
        a = dict(ok, **change)
        before = inside.clone()
        rc = _call(a["src"], a["dst"], a["table"], a["rows"], a["layers"], a["KV"], a["HD"], a["length"], a["keep"], a["drop"])
        msg = lib.csm_last_error().decode()
        assert rc == 1 and msg.startswith("csm_kv_shift"), (name, rc, msg)
        assert bool((big == R.GUARD).all()) and torch.equal(inside.view(torch.int16), before.view(torch.int16)), name
    # the buffers behind the probes are valid: the same call without a change runs, and neighbours that only touch do not overlap
    assert _call(s, d, t, R.TABLE_ROWS, layers, KV, HD, length, 3, 4) == 0
    assert _call(inside.data_ptr(), inside.data_ptr() + nbytes, t, R.TABLE_ROWS, layers, KV, HD, length, 3, 4) == 0
    got = inside[src.numel():src.numel() + layers * 2 * KV * (length - 4) * HD].view(layers, 2, KV, length - 4, HD).cpu()
    assert R.judge_shift("touching", got, src.cpu(), R.rope_table(R.TABLE_ROWS, HD), 3, 4) <= 1.0


@pytest.mark.parametrize("geom,pos,d", R.INVARIANCE)
def test_attention_is_invariant_under_the_shift(dev, geom, pos, d):
    """Relative-position invariance in the sense the attention kernels use positions: after a shift with keep = 0,
    csm_attn_decode_rope on the shifted cache at position pos - d agrees with the float64 reference of tests/decode_attn_ref.py
    evaluated on the ORIGINAL cache restricted to keys d .. pos-1 at the original positions.  Tolerance: that module's
    elementwise bound plus the shift's slack carried through the scores (``kv_shift_ref.invariance_reference``: a shifted key
    element may be off by b[s, j] = hulp(|ref| + slack) + slack, a score by Delta_s = scale x sum_j |q_j| b[s, j], a softmax weight
    by a factor e^(+-2 Delta), an output element by (e^(2 Delta) - 1) sum_s p_s |v_s|).  A rotation by +d, by the neighbouring
    table row or by nothing misses it by 2x to 50x (tests/test_kv_shift_ref_cpu.py)."""
    from csm.hip import ops
    c, src = R.invariance_problem(geom, pos, d)
    ref, tol = R.invariance_reference(c, src, d)
    dst = ops.kv_shift(src.to(dev), _table(c.HD, dev), 0, d)
    assert dst.shape == (1, 2, c.KV, pos - d, c.HD)
    kc, vc = torch.zeros_like(c.kc).to(dev), torch.zeros_like(c.vc).to(dev)
    kc[0, :, :pos - d], vc[0, :, :pos - d] = dst[0, 0], dst[0, 1]
    out = torch.full((1, c.H * c.HD), 7.0, dtype=BF, device=dev)
    at = torch.tensor([pos - d], dtype=torch.int32, device=dev)
    ops.attn_decode_rope(c.qkv.to(dev), kc, vc, out, at, c.table.to(dev).contiguous(), c.H, c.KV, c.HD)
    torch.cuda.synchronize()
    ratio = R.invariance_ratio(out, ref, tol)
    print(f"RATIO kv_shift_invariance {ratio:.4f} {geom} pos {pos} d {d}")
    assert ratio <= 1.0
