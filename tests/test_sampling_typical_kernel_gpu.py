"""``csm_sample_typical_rows``: the processed rows sampler with locally typical sampling as its last filter, against the float64
reference of tests/sampling_typical_ref.py.  The cases' ``typical_p`` clear the kernel's derived error bounds 4x
(tests/test_sampling_typical_ref_cpu.py), so the kernel must pick the reference's winner and keep exactly its set T - probed with
tiny noise on both sides of the cut, and on the argmax where T lacks it.  Then: ``typical_p = 1`` is ``csm_sample_processed_rows``
bit for bit, ring and counter included; wild device values count as 1; what the kernel writes to ring and counter; any row count and
the decode state's strided rings; refusals launch nothing."""
import pytest
import torch

import sampling_filters_ref as R
import sampling_processors_ref as P
import sampling_typical_ref as T

pytestmark = pytest.mark.gpu
ROWS, PAD, HIST = R.ROWS, 61, P.HIST
CASES = [(V, name, kind) for V in R.VS for name in R.SETS for kind in T.KINDS]


def _pad(x, dev):
    buf = torch.full((x.shape[0], x.shape[1] + PAD), 1e30)             # (what sits between the rows must never be read)
    buf[:, :x.shape[1]] = x
    return buf.to(dev)


def _f32(values, dev):
    return torch.tensor(values, dtype=torch.float32, device=dev)


def _i32(values, dev):
    return torch.tensor(values, dtype=torch.int32, device=dev)


def _typical(lg, q, k, t, p, m, pen, win, hist, frame, y, live, V, advance=False):
    """One launch on copies of ``hist`` / ``frame``: (out, hist after, frame after), on the host."""
    from csm.hip import ops
    out = torch.full((lg.shape[0],), -7, dtype=torch.int32, device=lg.device)
    hist, frame = hist.clone(), frame.clone()
    ops.sample_typical_rows(lg, q, out, k, t, p, m, pen, win, hist, frame, live, y, advance=advance, V=V)
    return out.cpu(), hist.cpu(), frame.cpu()


def _processed(lg, q, k, t, p, m, pen, win, hist, frame, live, V, advance=False):
    from csm.hip import ops
    out = torch.full((lg.shape[0],), -7, dtype=torch.int32, device=lg.device)
    hist, frame = hist.clone(), frame.clone()
    ops.sample_processed_rows(lg, q, out, k, t, p, m, pen, win, hist, frame, live, advance=advance, V=V)
    return out.cpu(), hist.cpu(), frame.cpu()


@pytest.fixture(scope="module")
def data(dev):
    """Per V: the padded RAW logit sets (the kernel applies the penalty), the noise, the rings - on the device, made once, never
    written (the launches run on copies)."""
    out = {}
    for V in R.VS:
        sets, q = R.inputs(V)
        c = T.cases(V)
        out[V] = dict(padded={n: _pad(x, dev) for n, x in sets.items()}, q=q.to(dev),
                      hist={n: c[(n, "chain")]["hist"].to(dev) for n in R.SETS},
                      pen=_f32(P.PEN, dev), win=_i32(P.WINDOW, dev), frame=_i32(P.FRAME, dev),
                      live=_i32([1] * ROWS, dev), idle=_i32([0] * ROWS, dev))
    return out


def _case(dev, data, V, name, kind):
    c, d = T.cases(V)[(name, kind)], data[V]
    return c, (d["padded"][name], d["q"], _i32(c["topk"], dev), _f32(c["temperature"], dev), _f32(c["top_p"], dev),
               _f32(c["min_p"], dev), d["pen"], d["win"], d["hist"][name], d["frame"], _f32(c["typical_p"], dev))


def _winners(c):
    return torch.tensor([ref["winner"] for ref in c["ref"]], dtype=torch.int32)


@pytest.mark.parametrize("V,name,kind", CASES)
def test_winner_is_the_reference_winner_twice(dev, data, V, name, kind):
    c, args = _case(dev, data, V, name, kind)
    got, _, _ = _typical(*args, data[V]["live"], V)
    want = _winners(c)
    assert torch.equal(got, want), (got, want)
    assert torch.equal(_typical(*args, data[V]["live"], V)[0], got)        # determinism: a second launch, the same indices


@pytest.mark.parametrize("V,name,kind", CASES)
def test_kept_set_boundary_probed_with_tiny_noise(dev, data, V, name, kind):
    """q = 1e-30 on one token per row: a kept token then wins, a dropped one has p = 0 and changes nothing.  Every member of the two
    delta groups at the cut is tried (first, middle, last of large groups)."""
    c, (lg, q, k, t, p, m, pen, win, hist, frame, y) = _case(dev, data, V, name, kind)
    live = data[V]["idle"]
    want = _winners(c)

    def members(group):
        return [] if not group else sorted({group[0], group[len(group) // 2], group[-1]})

    kept = [members(ref["last_kept"]) for ref in c["ref"]]
    dropped = [members(ref["first_dropped"]) for ref in c["ref"]]
    for i in range(3):
        qk, qd = q.clone(), q.clone()
        pick_k = [g[min(i, len(g) - 1)] for g in kept]
        for r in range(ROWS):
            qk[r, pick_k[r]] = 1e-30
            if dropped[r]:
                qd[r, dropped[r][min(i, len(dropped[r]) - 1)]] = 1e-30
        got = _typical(lg, qk, k, t, p, m, pen, win, hist, frame, y, live, V)[0]
        assert got.tolist() == pick_k, (i, got.tolist(), pick_k)
        got = _typical(lg, qd, k, t, p, m, pen, win, hist, frame, y, live, V)[0]
        assert torch.equal(got, want), (i, got, want)


@pytest.mark.parametrize("V,name,kind", CASES)
def test_a_dropped_argmax_cannot_win(dev, data, V, name, kind):
    c, (lg, q, k, t, p, m, pen, win, hist, frame, y) = _case(dev, data, V, name, kind)
    rows = [r for r, ref in enumerate(c["ref"]) if ref["drops_argmax"]]
    assert rows, "no row of this case drops the argmax"
    qa = q.clone()
    for r in rows:                                                         # (the penalised, scaled row's largest value: in N, not in T)
        top = int(torch.from_numpy(R.scaled(c["xp"][r], c["temperature"][r])).argmax())
        assert c["ref"][r]["N"][top] and not c["ref"][r]["T"][top]
        qa[r, top] = 1e-30
    got = _typical(lg, qa, k, t, p, m, pen, win, hist, frame, y, data[V]["idle"], V)[0]
    assert torch.equal(got, _winners(c)), (got, _winners(c))
    # ... and at typical_p = 1 it does win: the probe is decisive
    ones = _f32([1.0] * ROWS, dev)
    got = _typical(lg, qa, k, t, p, m, pen, win, hist, frame, ones, data[V]["idle"], V)[0]
    for r in rows:
        assert int(got[r]) == int(torch.from_numpy(R.scaled(c["xp"][r], c["temperature"][r])).argmax()), r


@pytest.mark.parametrize("V", R.VS)
@pytest.mark.parametrize("name", R.SETS)
def test_typical_p_one_is_the_processed_sampler_bit_for_bit(dev, data, V, name):
    for kind in T.KINDS:
        c, (lg, q, k, t, p, m, pen, win, hist, frame, y) = _case(dev, data, V, name, kind)
        ones = _f32([1.0] * ROWS, dev)
        for live, advance in ((data[V]["live"], False), (data[V]["live"], True), (data[V]["idle"], True)):
            want = _processed(lg, q, k, t, p, m, pen, win, hist, frame, live, V, advance=advance)
            got = _typical(lg, q, k, t, p, m, pen, win, hist, frame, ones, live, V, advance=advance)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (kind, advance)
        assert _typical(lg, q, k, t, p, m, pen, win, hist, frame, ones, data[V]["live"], V)[0].tolist() == [
            ref["winner"] for ref in c["proc"]]


@pytest.mark.parametrize("V", R.VS)
def test_wild_typical_p_counts_as_one(dev, data, V):
    nan, inf = float("nan"), float("inf")
    c, (lg, q, k, t, p, m, pen, win, hist, frame, y) = _case(dev, data, V, "drawn", "chain")
    live = data[V]["live"]
    want = _processed(lg, q, k, t, p, m, pen, win, hist, frame, live, V, advance=True)
    wild = [nan, 0.0, -0.5, 1.5, inf, -inf, -0.0, 1.0000001, nan, 0.0, -1.0, 2.0, inf, -inf, 1e30, -1e-30]
    got = _typical(lg, q, k, t, p, m, pen, win, hist, frame, _f32(wild, dev), live, V, advance=True)
    assert all(torch.equal(a, b) for a, b in zip(got, want)), (got[0], want[0])
    # a tiny but valid typical_p keeps the most typical delta group alone and still draws inside the vocabulary
    got = _typical(lg, q, k, t, p, m, pen, win, hist, frame, _f32([1e-30] * ROWS, dev), live, V)[0]
    assert int(got.min()) >= 0 and int(got.max()) < V


@pytest.mark.parametrize("V", R.VS)
def test_ring_and_frame_writes(dev, data, V):
    c, args = _case(dev, data, V, "drawn", "chain")
    d = data[V]
    want = _winners(c)
    before, frame0 = c["hist"], torch.tensor(P.FRAME, dtype=torch.int32)
    slot = [f % HIST for f in P.FRAME]
    expect = before.clone()
    expect[torch.arange(ROWS), torch.tensor(slot)] = want
    # live, no advance: the winner in slot frame % 64, every other slot and the counter unchanged
    out, hist, frame = _typical(*args, d["live"], V)
    assert torch.equal(out, want) and torch.equal(hist, expect) and torch.equal(frame, frame0)
    # live, advance: the same ring, the counter one further
    out, hist, frame = _typical(*args, d["live"], V, advance=True)
    assert torch.equal(out, want) and torch.equal(hist, expect) and torch.equal(frame, frame0 + 1)
    # not live: the ring and the counter untouched, with and without advance; out is still the winner
    for advance in (False, True):
        out, hist, frame = _typical(*args, d["idle"], V, advance=advance)
        assert torch.equal(out, want) and torch.equal(hist, before) and torch.equal(frame, frame0), advance
    # a mix: live rows only
    mix = [1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 0, 0, 1, 0, 1, 1]
    out, hist, frame = _typical(*args, _i32(mix, dev), V, advance=True)
    on = torch.tensor(mix, dtype=torch.bool)
    assert torch.equal(out, want)
    assert torch.equal(hist, torch.where(on[:, None], expect, before)) and torch.equal(frame, frame0 + on.int())


@pytest.mark.parametrize("V", R.VS)
def test_any_row_count_and_a_row_alone_from_strided_buffers(dev, data, V):
    c, (lg, q, k, t, p, m, pen, win, hist, frame, y) = _case(dev, data, V, "tied", "chain")
    want = _winners(c)
    live = data[V]["live"]
    for n in (1, 5, 16):
        got, hist_after, frame_after = _typical(lg[:n], q[:n], k[:n].clone(), t[:n].clone(), p[:n].clone(), m[:n].clone(),
                                                pen[:n].clone(), win[:n].clone(), hist[:n], frame[:n], y[:n].clone(),
                                                live[:n].clone(), V, advance=True)
        assert torch.equal(got, want[:n]), n
        assert frame_after.tolist() == [f + 1 for f in P.FRAME[:n]]
    # the decode state's layout: rings [B, K, 64], codebook i's view has row stride K * 64; the neighbours must stay as they are
    from csm.hip import ops
    Kc, i = 3, 1
    big = torch.full((ROWS, Kc, HIST), -9, dtype=torch.int32, device=dev)
    big[:, i] = hist
    view = big[:, i]
    assert view.stride(0) == Kc * HIST
    fr = frame.clone()
    out = torch.full((ROWS,), -7, dtype=torch.int32, device=dev)
    ops.sample_typical_rows(lg, q, out, k, t, p, m, pen, win, view, fr, live, y, advance=True, V=V)
    assert torch.equal(out.cpu(), want)
    assert bool((big[:, 0] == -9).all()) and bool((big[:, 2] == -9).all())
    assert torch.equal(big[torch.arange(ROWS), i, (frame.long() % HIST)].cpu(), want)
    for r in (4, 5, 15):                                                   # a row launched alone, from the middle of the buffers
        s = slice(r, r + 1)
        big[:, i] = hist
        fr = frame[s].clone()
        out = torch.full((1,), -7, dtype=torch.int32, device=dev)
        ops.sample_typical_rows(lg[s], q[s], out, k[s].clone(), t[s].clone(), p[s].clone(), m[s].clone(), pen[s].clone(),
                                win[s].clone(), big[s, i], fr, live[s].clone(), y[s].clone(), advance=True, V=V)
        assert int(out) == int(want[r]) and int(fr) == P.FRAME[r] + 1, r
        after = big[:, i].cpu()
        expect = hist.cpu().clone()
        expect[r, P.FRAME[r] % HIST] = want[r]
        assert torch.equal(after, expect), r


def test_entry_point_refusals_launch_nothing(dev, data):
    from csm import hip
    V = 2051
    c, (lg, q, k, t, p, m, pen, win, hist, frame, y) = _case(dev, data, V, "drawn", "typical")
    hist, frame, live = hist.clone(), frame.clone(), data[V]["live"]
    hist0, frame0 = hist.clone(), frame.clone()
    out = torch.full((ROWS,), -7, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    names = ("logits", "q", "out", "rows", "V", "ldl", "topk", "temperature", "top_p", "min_p", "penalty", "window", "hist", "ldh",
             "frame", "live", "advance", "typical_p")
    a0 = dict(logits=lg.data_ptr(), q=q.data_ptr(), out=out.data_ptr(), rows=ROWS, V=V, ldl=lg.stride(0), topk=k.data_ptr(),
              temperature=t.data_ptr(), top_p=p.data_ptr(), min_p=m.data_ptr(), penalty=pen.data_ptr(), window=win.data_ptr(),
              hist=hist.data_ptr(), ldh=HIST, frame=frame.data_ptr(), live=live.data_ptr(), advance=1, typical_p=y.data_ptr())
    wide = 256 * 16 + 1
    bad = [dict(logits=None), dict(q=None), dict(out=None), dict(topk=None), dict(temperature=None), dict(top_p=None),
           dict(min_p=None), dict(penalty=None), dict(window=None), dict(hist=None), dict(frame=None), dict(live=None),
           dict(typical_p=None), dict(rows=0), dict(rows=-1), dict(V=0), dict(V=-5), dict(ldl=V - 1), dict(V=wide, ldl=wide),
           dict(ldh=HIST - 1), dict(ldh=0), dict(ldh=-HIST)]
    for change in bad:
        a = {**a0, **change}
        rc = hip.lib.csm_sample_typical_rows(*[a[n] for n in names], stream)
        assert rc != 0, change
        assert b"csm_sample_typical_rows" in hip.lib.csm_last_error(), change
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and torch.equal(hist, hist0) and torch.equal(frame, frame0)
    rc = hip.lib.csm_sample_typical_rows(*[a0[n] for n in names], stream)
    winners = [ref["winner"] for ref in c["ref"]]
    assert rc == 0 and out.cpu().tolist() == winners
    assert frame.cpu().tolist() == [f + 1 for f in P.FRAME]
    assert hist.cpu()[torch.arange(ROWS), torch.tensor(P.FRAME) % HIST].tolist() == winners
