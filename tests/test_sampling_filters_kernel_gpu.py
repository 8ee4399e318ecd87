"""``csm_sample_filtered_rows``: the rows sampler with a nucleus (top-p) and a min-p threshold per row, against the float64
reference of tests/sampling_filters_ref.py.  The cases' thresholds sit between two value groups, at least 4x the kernel's derived
error bound from either (tests/test_sampling_filters_ref_cpu.py proves the margins), so the kernel must keep exactly the
reference's set - probed directly: a token handed q = 1e-30 wins if and only if it is kept - and pick the reference's winner, in
the one-wave finish, in the block-wide finish and in the block-wide filter that comes down to one wave.  Rows with (1, 0) are
``csm_sample_topk_rows``, bit for bit."""
import pytest
import torch

import sampling_filters_ref as R

pytestmark = pytest.mark.gpu
ROWS, PAD = R.ROWS, 61
CASES = [(V, name, kind) for V in R.VS for name in R.SETS for kind in R.KINDS]


def _pad(x, dev):
    buf = torch.full((x.shape[0], x.shape[1] + PAD), 1e30)             # (what sits between the rows must never be read)
    buf[:, :x.shape[1]] = x
    return buf.to(dev)


def _f32(values, dev):
    return torch.tensor(values, dtype=torch.float32, device=dev)


def _i32(values, dev):
    return torch.tensor(values, dtype=torch.int32, device=dev)


def _filtered(lg, q, k, t, p, m, V):
    from csm.hip import ops
    out = torch.full((lg.shape[0],), -7, dtype=torch.int32, device=lg.device)
    ops.sample_filtered_rows(lg, q, out, k, t, p, m, V=V)
    return out.cpu()


@pytest.fixture(scope="module")
def data(dev):
    """Per V: the padded logit sets and the noise on the device (made once, never written)."""
    out = {}
    for V in R.VS:
        sets, q = R.inputs(V)
        out[V] = dict(padded={n: _pad(x, dev) for n, x in sets.items()}, q=q.to(dev), q_cpu=q)
    return out


def _case(dev, data, V, name, kind):
    c = R.cases(V)[(name, kind)]
    return c, (data[V]["padded"][name], data[V]["q"], _i32(c["topk"], dev), _f32(c["temperature"], dev), _f32(c["top_p"], dev),
               _f32(c["min_p"], dev))


@pytest.mark.parametrize("V", R.VS)
@pytest.mark.parametrize("name", R.SETS)
def test_filters_off_is_the_rows_sampler(dev, data, V, name):
    from csm.hip import ops
    lg, q = data[V]["padded"][name], data[V]["q"]
    k, t = _i32(R.TOPK, dev), _f32(R.TEMP, dev)
    want = torch.full((ROWS,), -7, dtype=torch.int32, device=dev)
    ops.sample_topk_rows(lg, q, want, k, t, V=V)
    got = _filtered(lg, q, k, t, _f32([1.0] * ROWS, dev), _f32([0.0] * ROWS, dev), V)
    assert torch.equal(got, want.cpu()), (got, want)


@pytest.mark.parametrize("V,name,kind", CASES)
def test_winner_is_the_reference_winner_twice(dev, data, V, name, kind):
    c, args = _case(dev, data, V, name, kind)
    got = _filtered(*args, V)
    want = torch.tensor([ref["winner"] for ref in c["ref"]], dtype=torch.int32)
    assert torch.equal(got, want), (got, want)
    assert torch.equal(_filtered(*args, V), got)                           # determinism: a second launch, the same indices


@pytest.mark.parametrize("V,name,kind", CASES)
def test_kept_set_boundary_probed_with_tiny_noise(dev, data, V, name, kind):
    """q = 1e-30 on one token per row: a kept token then wins, a dropped one has p = 0 and changes nothing.  Every member of the
    two tie groups at the boundary is tried (the first, the middle and the last index of large groups)."""
    c, (lg, q, k, t, p, m) = _case(dev, data, V, name, kind)
    want = torch.tensor([ref["winner"] for ref in c["ref"]], dtype=torch.int32)

    def members(group):
        return [] if not group else sorted({group[0], group[len(group) // 2], group[-1]})

    kept = [members(ref["last_kept"]) for ref in c["ref"]]
    dropped = [members(ref["first_dropped"]) for ref in c["ref"]]
    if name == "quant":                                                    # (every boundary of this set lies between tie groups)
        assert any(len(g) > 1 for g in kept) and any(len(g) > 1 for g in dropped)
    for i in range(3):
        qk, qd = q.clone(), q.clone()
        pick_k = [g[min(i, len(g) - 1)] for g in kept]
        for r in range(ROWS):
            qk[r, pick_k[r]] = 1e-30
            if dropped[r]:
                qd[r, dropped[r][min(i, len(dropped[r]) - 1)]] = 1e-30
        got = _filtered(lg, qk, k, t, p, m, V)
        assert got.tolist() == pick_k, (i, got.tolist(), pick_k)
        got = _filtered(lg, qd, k, t, p, m, V)
        assert torch.equal(got, want), (i, got, want)


@pytest.mark.parametrize("V", R.VS)
def test_any_row_count_and_rows_launched_alone(dev, data, V):
    c, (lg, q, k, t, p, m) = _case(dev, data, V, "tied", "both")
    want = torch.tensor([ref["winner"] for ref in c["ref"]], dtype=torch.int32)
    for n in (1, 5, 16):
        got = _filtered(lg[:n], q[:n], k[:n].clone(), t[:n].clone(), p[:n].clone(), m[:n].clone(), V)
        assert torch.equal(got, want[:n]), n
    for r in (4, 5, 15):                                                   # a row launched alone, from the middle of the buffers
        s = slice(r, r + 1)
        assert torch.equal(_filtered(lg[s], q[s], k[s].clone(), t[s].clone(), p[s].clone(), m[s].clone(), V), want[s]), r


@pytest.mark.parametrize("V", R.VS)
def test_wild_device_values_are_made_safe(dev, data, V):
    nan, inf = float("nan"), float("inf")
    lg, q = data[V]["padded"]["drawn"][:12], data[V]["q"][:12]
    c = R.cases(V)[("drawn", "both")]
    good_p, good_m = c["top_p"][7], c["min_p"][7]
    wild_p = [nan, 0.0, -0.5, 1.5, inf, -inf, good_p, good_p, good_p, good_p, good_p, nan]
    safe_p = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, good_p, good_p, good_p, good_p, good_p, 1.0]
    wild_m = [good_m, good_m, good_m, good_m, good_m, good_m, nan, -0.25, 1.5, inf, -inf, nan]
    safe_m = [good_m, good_m, good_m, good_m, good_m, good_m, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    wild_k = [0, -3, V + 1, 2 ** 30, 50, 50, 50, 50, V, V, V, -1]
    safe_k = [1, 1, V, V, 50, 50, 50, 50, V, V, V, 1]
    wild_t = [0.9, 0.9, 0.9, 0.9, 0.0, -1.0, nan, inf, 0.9, 0.9, 0.9, -inf]
    safe_t = [0.9, 0.9, 0.9, 0.9, 1.0, 1.0, 1.0, 1.0, 0.9, 0.9, 0.9, 1.0]
    got = _filtered(lg, q, _i32(wild_k, dev), _f32(wild_t, dev), _f32(wild_p, dev), _f32(wild_m, dev), V)
    want = _filtered(lg, q, _i32(safe_k, dev), _f32(safe_t, dev), _f32(safe_p, dev), _f32(safe_m, dev), V)
    assert torch.equal(got, want), (got, want)
    assert int(got.min()) >= 0 and int(got.max()) < V
    sets, qc = R.inputs(V)
    for r in range(12):                                                    # ... and the safe values mean what the reference says
        ref = R.reference(sets["drawn"][r], safe_k[r], safe_t[r], safe_p[r], safe_m[r], qc[r])
        if ref["topp_margin"] >= R.HEADROOM * ref["topp_bound"] and ref["minp_margin"] >= R.HEADROOM * ref["minp_bound"]:
            assert int(want[r]) == ref["winner"], r


def test_extreme_thresholds_are_greedy_top1(dev, data):
    V = 2051
    lg, q = data[V]["padded"]["tied"], data[V]["q"]
    t = _f32(R.TEMP, dev)
    ones, zeros = _f32([1.0] * ROWS, dev), _f32([0.0] * ROWS, dev)
    top1 = _filtered(lg, q, _i32([1] * ROWS, dev), t, ones, zeros, V)
    for topk in (50, V):
        k = _i32([topk] * ROWS, dev)
        assert torch.equal(_filtered(lg, q, k, t, ones, ones, V), top1)
        assert torch.equal(_filtered(lg, q, k, t, _f32([1e-6] * ROWS, dev), zeros, V), top1)


def test_entry_point_refusals_launch_nothing(dev, data):
    from csm import hip
    V = 2051
    c, (lg, q, k, t, p, m) = _case(dev, data, V, "drawn", "top_p")
    out = torch.full((ROWS,), -7, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    names = ("logits", "q", "out", "rows", "V", "ldl", "topk", "temperature", "top_p", "min_p")
    a0 = dict(logits=lg.data_ptr(), q=q.data_ptr(), out=out.data_ptr(), rows=ROWS, V=V, ldl=lg.stride(0), topk=k.data_ptr(),
              temperature=t.data_ptr(), top_p=p.data_ptr(), min_p=m.data_ptr())
    wide = 256 * 16 + 1
    bad = [dict(logits=None), dict(q=None), dict(out=None), dict(topk=None), dict(temperature=None), dict(top_p=None),
           dict(min_p=None), dict(rows=0), dict(rows=-1), dict(V=0), dict(V=-5), dict(ldl=V - 1), dict(V=wide, ldl=wide)]
    for change in bad:
        a = {**a0, **change}
        rc = hip.lib.csm_sample_filtered_rows(*[a[n] for n in names], stream)
        assert rc != 0, change
        assert b"csm_sample_filtered_rows" in hip.lib.csm_last_error(), change
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    rc = hip.lib.csm_sample_filtered_rows(*[a0[n] for n in names], stream)
    assert rc == 0 and out.cpu().tolist() == [ref["winner"] for ref in c["ref"]]
