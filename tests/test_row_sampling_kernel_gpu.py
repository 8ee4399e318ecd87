"""``csm_sample_topk_rows``: the sampler with one (topk, temperature) per row, read from device arrays.  Row r must be the bits
of ``csm_sample_topk`` with the scalars topk[r], temperature[r] and the oracle's ``sample_topk`` - for both instantiations
(V = 2051: 9 values per thread, V = 4096: 16), a padded row stride, the one-wave (<= 64 kept values) and the block-wide finish
mixed in one launch, ties at the k-th value, any row count, and whatever the device arrays hold.  For these inputs the oracle's
winner is also the float64 argmax of p / q and beats the runner-up by a factor >= 1.023 in every row of every set (worst rows:
1.117 at V = 2051, 1.023 at V = 4096), so the fp32 rounding of the kernel's exponentials cannot turn a row: torch.equal."""
import pytest
import torch

from oracle import csm_oracle as O

pytestmark = pytest.mark.gpu
ROWS, PAD = 16, 61
TOPK = [1, 2, 12, 50, 64, 65, 200, 2051, 50, 50, 64, 65, 1, 7, 300, 33]
TEMP = [0.9, 0.5, 0.8, 0.9, 1.0, 1.3, 0.7, 1.0, 0.25, 2.0, 0.9, 0.9, 1.5, 0.6, 1.1, 0.95]
VS = (2051, 4096)


@pytest.fixture(scope="module")
def data(dev):
    """Per V: the noise, the three logit sets (CPU, unpadded) and, per set, the per-row scalar-kernel and oracle results."""
    from csm.hip import ops
    out = {}
    for V in VS:
        g = torch.Generator().manual_seed(48)
        lg = torch.randn(ROWS, V, generator=g) * 2
        q = torch.empty(ROWS, V).exponential_(1, generator=g)
        tied = lg.clone()
        tied[:, 100:400] = tied[:, 100:101]
        tied[:8, 100:400] += 3.0
        sets = {"drawn": lg, "tied": tied, "quant": (lg * 4).round() / 4}
        qd = q.to(dev)
        scalar, oracle, padded = {}, {}, {}
        for name, x in sets.items():
            padded[name] = _pad(x, dev)
            one = torch.empty(1, dtype=torch.int32, device=dev)
            rows = []
            for r in range(ROWS):
                ops.sample_topk(padded[name][r:r + 1], qd[r:r + 1], one, TOPK[r], TEMP[r], V=V)
                rows.append(one.clone())
            scalar[name] = torch.cat(rows).cpu()
            oracle[name] = torch.cat([O.sample_topk(x[r], TOPK[r], TEMP[r], q[r]) for r in range(ROWS)])
        out[V] = dict(q=qd, sets=sets, padded=padded, scalar=scalar, oracle=oracle)
    return out


def _pad(x, dev):
    buf = torch.full((x.shape[0], x.shape[1] + PAD), 1e30)             # (what sits between the rows must never be read)
    buf[:, :x.shape[1]] = x
    return buf.to(dev)


def _params(dev, topk=TOPK, temp=TEMP):
    return torch.tensor(topk, dtype=torch.int32, device=dev), torch.tensor(temp, dtype=torch.float32, device=dev)


def _rows(lg, q, k, t, V):
    from csm.hip import ops
    out = torch.full((lg.shape[0],), -7, dtype=torch.int32, device=lg.device)
    ops.sample_topk_rows(lg, q, out, k, t, V=V)
    return out.cpu()


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("name", ["drawn", "tied", "quant"])
def test_rows_equal_scalar_kernel_and_oracle(dev, data, V, name):
    d = data[V]
    k, t = _params(dev)
    got = _rows(d["padded"][name], d["q"], k, t, V)
    assert torch.equal(got, d["scalar"][name]), (got, d["scalar"][name])
    assert torch.equal(got, d["oracle"][name]), (got, d["oracle"][name])
    assert int(got.min()) >= 0 and int(got.max()) < V
    if name == "drawn":
        # the mixed launch ran both finishes: topk <= 64 without ties keeps <= 64 values, topk >= 65 keeps more; and the
        # parameters matter - with one pair for every row other codes come out
        assert sum(kk <= 64 for kk in TOPK) and sum(kk > 64 for kk in TOPK)
        same = _rows(d["padded"][name], d["q"], *_params(dev, [50] * ROWS, [0.9] * ROWS), V)
        assert not torch.equal(same, got)


@pytest.mark.parametrize("V", VS)
def test_any_row_count_and_rows_launched_alone(dev, data, V):
    d = data[V]
    lg, q, want = d["padded"]["tied"], d["q"], d["scalar"]["tied"]
    k, t = _params(dev)
    for n in (1, 5, 16):
        assert torch.equal(_rows(lg[:n], q[:n], k[:n].clone(), t[:n].clone(), V), want[:n]), n
    for r in (4, 5, 15):                                                   # a row launched alone, from the middle of the buffers
        assert torch.equal(_rows(lg[r:r + 1], q[r:r + 1], k[r:r + 1].clone(), t[r:r + 1].clone(), V), want[r:r + 1]), r


@pytest.mark.parametrize("V", VS)
def test_wild_device_values_are_made_safe(dev, data, V):
    d = data[V]
    lg, q = d["padded"]["drawn"][:8], d["q"][:8]
    wild_k = [0, -3, V + 1, 2 ** 30, 50, 50, 50, 50]
    safe_k = [1, 1, V, V, 50, 50, 50, 50]
    wild_t = [0.9, 0.9, 0.9, 0.9, 0.0, -1.0, float("nan"), float("inf")]
    safe_t = [0.9, 0.9, 0.9, 0.9, 1.0, 1.0, 1.0, 1.0]
    got = _rows(lg, q, *_params(dev, wild_k, wild_t), V)
    want = _rows(lg, q, *_params(dev, safe_k, safe_t), V)
    assert torch.equal(got, want), (got, want)
    assert int(got.min()) >= 0 and int(got.max()) < V
    # ... and the safe rows are the scalar kernel's with those values
    from csm.hip import ops
    one = torch.empty(1, dtype=torch.int32, device=dev)
    for r in range(8):
        ops.sample_topk(lg[r:r + 1], q[r:r + 1], one, safe_k[r], safe_t[r], V=V)
        assert int(one) == int(want[r]), r
    # every row wild at once, both ways
    got = _rows(lg, q, *_params(dev, [-1] * 8, [float("-inf")] * 8), V)
    assert torch.equal(got, _rows(lg, q, *_params(dev, [1] * 8, [1.0] * 8), V))


def test_entry_point_refusals_launch_nothing(dev, data):
    from csm import hip
    V = 2051
    d = data[V]
    lg, q = d["padded"]["drawn"], d["q"]
    k, t = _params(dev)
    out = torch.full((ROWS,), -7, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    p = dict(logits=lg.data_ptr(), q=q.data_ptr(), out=out.data_ptr(), rows=ROWS, V=V, ldl=lg.stride(0), topk=k.data_ptr(),
             temperature=t.data_ptr())
    wide = 256 * 16 + 1
    bad = [dict(logits=None), dict(q=None), dict(out=None), dict(topk=None), dict(temperature=None), dict(rows=0), dict(rows=-1),
           dict(V=0), dict(V=-5), dict(ldl=V - 1), dict(V=wide, ldl=wide)]
    for change in bad:
        a = {**p, **change}
        rc = hip.lib.csm_sample_topk_rows(a["logits"], a["q"], a["out"], a["rows"], a["V"], a["ldl"], a["topk"], a["temperature"],
                                          stream)
        assert rc != 0, change
        assert b"csm_sample_topk_rows" in hip.lib.csm_last_error(), change
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    rc = hip.lib.csm_sample_topk_rows(*[p[n] for n in ("logits", "q", "out", "rows", "V", "ldl", "topk", "temperature")], stream)
    assert rc == 0 and torch.equal(out.cpu(), d["scalar"]["drawn"])
