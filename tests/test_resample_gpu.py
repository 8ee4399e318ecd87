"""The device resampler (csrc/resample.hip, csm/codec/resample.py) on the GPU.

1. One-shot against ``csm.data.resample`` in float64, under a derived bound: an fp32 dot of T terms over fp32-rounded taps errs
   by at most (T + 3) * 2^-24 * sum_t |taps64[p][t]| * |xbar_t| (gamma_T for the accumulation, one ulp for the table rounding, one
   spare); the test computes that bound per output in float64 and asserts worst |err| / bound < 1.
2. The stream equals the one-shot form bit for bit for any cutting of the input.
3. The rows form equals single streams bit for bit, whatever the batch-mates do; the ABI's refusals launch nothing.
4. ``hear(speaker, sample_rate=)`` enters the history ``add`` of the resampled whole signal enters.
5. ``output_sample_rate=`` on the server, ``generate_stream``, ``generate_batch``: same codes, audio = the resampled audio.
Everything but 1 is ``torch.equal``: every form runs one fmaf chain in ascending tap order per output."""
import math

import pytest
import torch

from test_stream_gpu import Tok, _hf_model, _tiny

pytestmark = pytest.mark.gpu

PAIRS = [(48000, 24000), (16000, 24000), (44100, 24000), (24000, 48000), (24000, 8000), (24000, 44100)]
IDS = [f"{a}to{b}" for a, b in PAIRS]
FRAME = 1920
PERM = [5, 0, 11, 7, 14, 1, 9, 3, 2, 15, 4, 12, 6, 8, 13, 10]
NAN = float("nan")


def _sig(n, seed, rows=None):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * 0.2 if rows is None else torch.randn(rows, n, generator=g) * 0.2


def _bound64(x64, pair):
    """(T + 3) * 2^-24 * sum_t |taps64[j mod n][t]| * |xbar[(j div n) * o - width + t]| for every output j of x64 [R, N]."""
    from csm.codec.resample import design
    o, n, width, taps = design(*pair)
    T = taps.shape[1]
    k = torch.from_numpy(taps).abs()
    xp = torch.nn.functional.pad(x64.abs()[:, None, :], (width, width + o))
    s = torch.nn.functional.conv1d(xp, k[:, None, :], stride=o).transpose(1, 2).reshape(x64.shape[0], -1)
    return (T + 3) * 2.0 ** -24 * s[:, :math.ceil(n * x64.shape[1] / o)]


# ------------------------------------------------------------------------------------------------------------- 1. one-shot
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_one_shot_against_float64(dev, pair):
    from csm.codec.resample import Resampler, geometry
    from csm.data.training_data import resample as host_resample
    from csm.hip import ops
    o, n, width, T = geometry(*pair)
    rs = Resampler(*pair, device="cuda")
    worst = 0.0
    for N in (1, width, width + o - 1, width + o, 2 * T + 3, 1920, 5003):
        for R in (1, 3):
            x = _sig(N, N * 7 + R + pair[0], rows=R)
            y = rs(x.cuda())
            ref = host_resample(x.double(), *pair)
            assert y.shape == ref.shape == (R, math.ceil(n * N / o)) and y.dtype == torch.float32
            bound = _bound64(x.double(), pair)
            err = (y.cpu().double() - ref).abs()
            assert bool((err[bound == 0] == 0).all())                # (no input under any tap: the output is exactly zero)
            ratio = float((err / bound)[bound > 0].max())
            worst = max(worst, ratio)
            assert ratio < 1.0, (pair, N, R, ratio)
    print(f"resample {pair[0]} -> {pair[1]}: worst |err| / bound = {worst:.3f}")
    x = _sig(700, 3)
    assert torch.equal(ops.resample(x.cuda(), *pair), rs(x.cuda()))                        # the thin wrapper
    assert rs(x.cuda().reshape(2, 5, 70)).shape == (2, 5, math.ceil(n * 70 / o))          # leading dimensions are rows


# ------------------------------------------------------------------------------------------------------------- 2. stream
def _cuts(kind, N, o, seed):
    g = torch.Generator().manual_seed(seed)
    out, left = [], N
    while left:
        k = {"random": int(torch.randint(1, 401, (1,), generator=g)), "ones": 1, "below_o": max(1, o - 1), "whole": left}[kind]
        out.append(min(k, left))
        left -= out[-1]
    return out


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_stream_equals_one_shot_bitwise(dev, pair):
    from csm.codec.resample import Resampler
    rs = Resampler(*pair, device="cuda")
    N = 5003
    x = _sig(N, pair[1] + 1).cuda()
    ref = rs(x)
    st = rs.stream(max_in=400)
    assert st.flush().numel() == 0                                       # a flush on an empty stream
    for kind in ("random", "below_o", "whole", "random"):
        st.reset()
        at, got = 0, []
        for k in _cuts(kind, N, rs.o, N + len(kind)):
            got.append(st.feed(x[at:at + k]))
            at += k
            assert st.pos == at
        got.append(st.flush())
        y = torch.cat(got)
        assert y.shape == ref.shape and torch.equal(y, ref), (pair, kind)
        with pytest.raises(RuntimeError, match="flushed"):
            st.feed(x[:1])
    short = x[:2 * rs.T + 3 + rs.o]                                      # sample by sample, on one short input
    st.reset()
    got = [st.feed(short[i:i + 1]) for i in range(short.numel())] + [st.flush()]
    assert torch.equal(torch.cat(got), rs(short)), pair
    assert rs.stream().max_in == pair[0]                                 # the default: one second a launch


# ------------------------------------------------------------------------------------------------------------- 3. rows
def _run_rows(rows, utts, slot_order, max_in, alone=None):
    """Feed the utterances through ``rows``: utterance u joins at step u % 4 (or when a slot is free again), every step gives each
    active row its own piece - sizes cycle through 1, max_in and odd ones at a per-row phase - and a row's last piece ends its
    stream (``final``).  ``alone``: only that utterance is run (same pieces, no batch-mates).  Returns the outputs per utterance
    and the widest step."""
    sizes = [1, max_in, 37, 2, max_in - 1, 150, 3]
    free, waiting, active = list(slot_order), list(range(len(utts))), {}
    got = [[] for _ in utts]
    widest, t = 0, 0
    while waiting or active:
        while waiting and free and waiting[0] % 4 <= t:
            s, u = free.pop(0), waiting.pop(0)
            if alone is None or u == alone:
                rows.open(s)
            active[s] = [u, 0, 0]
        part = list(active)
        xs, fin = [], []
        for s in part:
            u, at, i = active[s]
            k = min(sizes[(u + i) % len(sizes)], utts[u].numel() - at)
            xs.append(utts[u][at:at + k])
            active[s] = [u, at + k, i + 1]
            if at + k == utts[u].numel():
                fin.append(s)
        keep = [j for j, s in enumerate(part) if alone is None or active[s][0] == alone]
        if keep:
            ys = rows.step([part[j] for j in keep], [xs[j] for j in keep], final=[s for s in fin if part.index(s) in keep])
            widest = max(widest, len(keep))
            for j, y in zip(keep, ys):
                got[active[part[j]][0]].append(y.clone())
        for s in fin:
            del active[s]
            free.append(s)
        t += 1
    return [torch.cat(g) if g else None for g in got], widest


@pytest.mark.parametrize("pair", [(16000, 24000), (44100, 24000), (24000, 48000)], ids=["16000to24000", "44100to24000", "24000to48000"])
def test_rows_equal_single_streams_bitwise(dev, pair):
    from csm.codec.resample import Resampler
    rs = Resampler(*pair, device="cuda")
    max_in = 211
    # 20 utterances on 16 slots (the first slots that end are taken again), then 3 on a 4-slot stream
    for n_utts, order, slots in ((20, PERM, 16), (3, [2, 0, 3], 4)):
        utts = [_sig(300 + 97 * u, 100 + u).cuda() for u in range(n_utts)]
        rows = rs.stream_rows(slots, max_in)
        got, widest = _run_rows(rows, utts, order, max_in)
        assert widest == min(n_utts, slots)
        for u, x in enumerate(utts):
            assert torch.equal(got[u], rs(x)), (pair, u)                 # = the one-shot form, hence = a single stream
        single = rs.stream(max_in)
        pieces = [single.feed(utts[1][i:i + 50]) for i in range(0, utts[1].numel(), 50)] + [single.flush()]
        assert torch.equal(torch.cat(pieces), got[1])
        for u in (0, n_utts - 1):                                        # the same row alone, in the same slot, the same pieces
            alone, w1 = _run_rows(rs.stream_rows(slots, max_in), utts, order, max_in, alone=u)
            assert w1 == 1 and torch.equal(alone[u], got[u]), (pair, u)
    with pytest.raises(ValueError, match="distinct slots"):
        rows.step([1, 1], [utts[0][:4], utts[0][:4]])
    with pytest.raises(ValueError, match="not open"):
        rows.step([1], [utts[0][:4]])
    rows.open(1)
    with pytest.raises(ValueError, match="max_in"):
        rows.step([1], [utts[0][:max_in + 1]])
    with pytest.raises(ValueError, match="none only when it ends"):
        rows.step([1], [None])


def test_rows_refusals_launch_nothing(dev):
    from csm.codec.resample import Resampler
    from csm.hip import CsmHipError, lib, ops
    import ctypes
    rs = Resampler(16000, 24000, device="cuda")
    H = rs.T - 1
    arena = torch.full((8, 2, H), 7.0, device="cuda")
    y = torch.full((2, 64), 3.0, device="cuda")
    x = [_sig(8, 1).cuda(), _sig(8, 2).cuda()]
    stream = torch.cuda.current_stream().cuda_stream

    def raw(R=2, slots=(3, 1), parity=(0, 1), n_in=(8, 5), pos=(0, 40), mask=0, n_slots=8, max_in=8, o=rs.o, n=rs.n, ldy=64):
        ptrs = (ctypes.c_void_p * len(slots))(*[x[r % 2].data_ptr() for r in range(len(slots))])
        return lib.csm_resample_stream_rows_f32(arena.data_ptr(), ptrs, rs.taps.data_ptr(), y.data_ptr(), ldy, R, ops._ints(slots),
                                                ops._ints(parity), ops._ints(n_in), (ctypes.c_longlong * len(pos))(*pos), mask, n_slots,
                                                max_in, o, n, rs.width, stream)

    many = dict(R=17, slots=tuple(range(17)), parity=(0,) * 17, n_in=(8,) * 17, pos=(0,) * 17, n_slots=32)
    for kw, text in ((dict(R=0), b"1..16"), (many, b"1..16"), (dict(slots=(3, 8)), b"outside [0, 8)"), (dict(slots=(-1, 2)), b"outside"),
                     (dict(slots=(3, 3)), b"named twice"), (dict(parity=(0, 2)), b"parity"), (dict(mask=4), b"names a row >= R = 2"),
                     (dict(n_in=(8, 9)), b"max_in"), (dict(n_in=(0, 5)), b"final bit"), (dict(pos=(0, -1)), b"position"),
                     (dict(ldy=3), b"ldy"), (dict(o=3, n=3), b"equal rates"), (dict(o=4, n=6), b"lowest terms")):
        assert raw(**kw) == 1 and text in lib.csm_last_error(), (kw, lib.csm_last_error())
    with pytest.raises(CsmHipError, match="named twice"):
        ops.resample_stream_rows_f32(arena, x, rs.taps, y, [2, 2], [0, 0], [0, 0], [], 8, rs.o, rs.n, rs.width)
    torch.cuda.synchronize()
    assert bool((y == 3.0).all()) and bool((arena == 7.0).all())         # nothing was launched
    arena[3, 0], arena[1, 1] = 0.0, 0.0
    assert raw(pos=(0, 0)) == 0                                          # the legal call goes through
    torch.cuda.synchronize()
    assert torch.equal(arena[3, 1, -8:], x[0]) and torch.equal(arena[1, 0, -5:], x[1][:5])
    arena[3], arena[1] = 7.0, 7.0
    assert bool((arena == 7.0).all())                                    # ... and touched its own slots only


# ------------------------------------------------------------------------------------------------------------- 4. / 5. model
MS = 6 * 80
TEMP, TOPK = 0.9, 50


@pytest.fixture(scope="module")
def gen(dev):
    from csm.codec import MimiCodec
    from csm.generator import Generator
    return Generator(_tiny(), text_tokenizer=Tok(), audio_tokenizer=MimiCodec(_hf_model().state_dict(), device="cuda"))


def _pieces(total, sizes):
    at, i = 0, 0
    while at < total:
        yield at, min(at + sizes[i % len(sizes)], total)
        at, i = min(at + sizes[i % len(sizes)], total), i + 1


def test_hear_at_other_rates_equals_add_of_the_resampled_turn(dev, gen):
    from csm.generator import Segment
    from csm.hip import ops
    k = 5
    sig16 = [_sig(1280 * k, 200 + i) for i in range(3)]                  # k frames each at 16 kHz
    sig48 = _sig(3840 * k, 210)
    sizes = [700, 1, 3000, 77, 1279]

    def added(make, whole, rate):
        conv = make()
        conv.add(Segment(1, "and then?", ops.resample(whole.cuda(), rate, 24000)))
        return conv.tokens.clone(), conv.mask.clone()

    def same(conv, ref):
        assert torch.equal(conv.tokens, ref[0]) and torch.equal(conv.mask, ref[1])
        assert int((ref[0][:, :32] != 0).any(1).sum()) >= k

    # Generator.conversation() and a server without hear_slots: the turn owns its ResampleStream
    ref = added(gen.conversation, sig16[0], 16000)
    conv = gen.conversation()
    turn = conv.hear(1, sample_rate=16000)
    for a, b in _pieces(sig16[0].numel(), sizes):
        turn.feed(sig16[0][a:b])
    assert turn.frames == k - 1 and turn.pending == 0                   # the last frame waits for the resampler's lag
    turn.end("and then?")
    same(conv, ref)
    turn = conv.hear(1, sample_rate=16000)                               # a second turn at the same rate: the stream starts anew
    turn.feed(sig16[0].cuda())
    turn.end("and then?")
    assert torch.equal(conv.tokens[ref[0].shape[0]:], ref[0])

    srv = gen.serve(slots=4, chunk_frames=2, temperature=TEMP, topk=TOPK)
    ref = added(srv.conversation, sig16[1], 16000)
    conv = srv.conversation()
    turn = conv.hear(1, sample_rate=16000)
    for a, b in _pieces(sig16[1].numel(), sizes[::-1]):
        turn.feed(sig16[1][a:b])
    turn.end("and then?")
    same(conv, ref)

    # hear_slots = 4: three conversations at 16 kHz and one at 48 kHz in the same hear_step, ended together
    srv = gen.serve(slots=4, chunk_frames=2, temperature=TEMP, topk=TOPK, hear_slots=4)
    wholes = [(s, 16000) for s in sig16] + [(sig48, 48000)]
    refs = [added(srv.conversation, w, r) for w, r in wholes]
    convs = [srv.conversation() for _ in wholes]
    turns = [c.hear(1, sample_rate=r) for c, (_, r) in zip(convs, wholes)]
    assert [t.slot for t in turns] == [0, 1, 2, 3] and set(srv._hear_rs) == {16000, 48000}
    cuts = [list(_pieces(w.numel(), sizes[i:] + sizes[:i])) for i, (w, _) in enumerate(wholes)]
    for step in range(max(len(c) for c in cuts)):
        for t, (w, _), c in zip(turns, wholes, cuts):
            if step < len(c):
                before = t.frames
                t.feed(w[c[step][0]:c[step][1]])
                assert t.frames == before                                # feed only buffers
        want = [t.frames + t.pending for t in turns]
        srv.hear_step()
        assert [t.frames for t in turns] == want and all(t.pending == 0 for t in turns)
    assert [t.frames for t in turns] == [k - 1] * 4
    srv.end_heard([(t, "and then?") for t in turns[::-1]])
    assert srv._hearing == [None] * 4
    for conv, ref in zip(convs, refs):
        same(conv, ref)

    # without a rate (and with the codec's own): the path it always took
    sig24 = _sig(FRAME * 3 + 500, 220)
    outs = []
    for rate in ("absent", None, 24000):
        conv = gen.conversation()
        turn = conv.hear(1) if rate == "absent" else conv.hear(1, sample_rate=rate)
        assert turn._rs is None
        for a, b in _pieces(sig24.numel(), sizes):
            turn.feed(sig24[a:b])
        turn.end("and then?")
        outs.append((conv.tokens.clone(), conv.mask.clone()))
    enc = gen._audio_tokenizer.encode_stream()                           # ... which is feed + flush of the encode stream
    codes = torch.cat([enc.feed(sig24.cuda().reshape(1, 1, -1)), enc.flush()], 2)[0]
    assert all(torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) for o in outs)
    assert torch.equal(outs[0][0][-5:-1, :32], codes.t())


def test_speaking_at_other_rates(dev, gen):
    from csm.hip import ops
    texts = [("the one we look at", 7 * 80), ("short", 3 * 80), ("a third one that is longer", 9 * 80)]

    def served(**kw):
        srv = gen.serve(slots=4, chunk_frames=2, temperature=TEMP, topk=TOPK, **kw)
        reqs = [srv.submit(t, i, [], seed=30 + i, max_audio_length_ms=ms) for i, (t, ms) in enumerate(texts)]
        parts = {r.id: [] for r in reqs}
        for r, part, _ in srv.run():
            parts[r.id].append(part)
        assert all(r.done for r in reqs)
        return srv, reqs, parts

    _, base, _ = served()
    srv, reqs, parts = served(output_sample_rate=48000)
    assert srv.sample_rate == 48000
    for a, b in zip(base, reqs):
        assert a.sample_rate == 24000 and b.sample_rate == 48000
        assert torch.equal(a.codes(), b.codes()) and a.codes().shape[1] > 0
        want = ops.resample(a.audio(), 24000, 48000)
        assert want.numel() == 2 * a.audio().numel()
        assert torch.equal(b.audio(), want)
        assert sum(p.numel() for p in parts[b.id]) == want.numel()
    for rate in (None, 24000):                                           # today's tensors
        _, same, _ = served(output_sample_rate=rate)
        assert all(torch.equal(a.audio(), b.audio()) and torch.equal(a.codes(), b.codes()) for a, b in zip(base, same))

    torch.manual_seed(5)
    ref = gen.generate("ok there", 1, [], max_audio_length_ms=80 * 7)
    assert ref.numel() == 7 * FRAME
    for rate in (None, 24000):
        torch.manual_seed(5)
        assert torch.equal(gen.generate("ok there", 1, [], max_audio_length_ms=80 * 7, output_sample_rate=rate), ref)
    torch.manual_seed(5)
    assert torch.equal(gen.generate("ok there", 1, [], max_audio_length_ms=80 * 7, output_sample_rate=16000),
                       ops.resample(ref, 24000, 16000))
    torch.manual_seed(5)
    chunks = list(gen.generate_stream("ok there", 1, [], max_audio_length_ms=80 * 7, chunk_frames=3, output_sample_rate=16000))
    assert len(chunks) == 4 and torch.equal(torch.cat(chunks), ops.resample(ref, 24000, 16000))
    torch.manual_seed(5)
    plain = list(gen.generate_stream("ok there", 1, [], max_audio_length_ms=80 * 7, chunk_frames=3))
    assert torch.equal(torch.cat(plain), ref) and len(plain) == 3

    conv = gen.conversation()
    torch.manual_seed(5)
    assert torch.equal(conv.generate("ok there", 1, max_audio_length_ms=80 * 7, output_sample_rate=16000), ops.resample(ref, 24000, 16000))
    conv = gen.conversation()
    torch.manual_seed(5)
    got = list(conv.generate_stream("ok there", 1, max_audio_length_ms=80 * 7, chunk_frames=3, output_sample_rate=48000))
    assert torch.equal(torch.cat(got), ops.resample(ref, 24000, 48000))

    args = (["one", "and two", "three"], [0, 1, 2], [[], [], []])
    torch.manual_seed(9)
    batch = gen.generate_batch(*args, max_audio_length_ms=80 * 5)
    torch.manual_seed(9)
    low = gen.generate_batch(*args, max_audio_length_ms=80 * 5, output_sample_rate=8000)
    for a, b in zip(batch, low):
        assert a.numel() == 5 * FRAME and torch.equal(b, ops.resample(a, 24000, 8000))
    torch.manual_seed(9)
    assert all(torch.equal(a, b) for a, b in zip(batch, gen.generate_batch(*args, max_audio_length_ms=80 * 5, output_sample_rate=24000)))
