"""The rows form of the Mimi encode stream on the GPU: csm_conv1d_stream_strided_rows_f32 row by row against
csm_conv1d_stream_strided_f32, MimiCodec.encode_stream_rows against MimiCodec.encode / MimiEncodeStream, and a server with
hear_slots against the same dialogue built with conv.add.

Every row of a rows launch goes through conv1d_accum / attn_window_row / linear_epilogue with the operands of the one-row
kernels, so every comparison here is torch.equal: no tolerance."""
import pytest
import torch

from test_mimi_encode_stream_gpu import CASES
from test_stream_gpu import Tok, _hf_model, _rand, _tiny

pytestmark = pytest.mark.gpu

FRAME = 1920
NAN = float("nan")
PERM = [5, 0, 11, 7, 14, 1, 9, 3, 2, 15, 4, 12, 6, 8, 13, 10]        # slot of row r: no row sits in its own slot


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("R", [1, 3, 16])
@pytest.mark.parametrize("case", CASES)
def test_strided_rows_kernel_bitwise(dev, case, R):
    """Three chunks per row (1, 3, 2 outputs: the first has H > n_in in the dilated case), permuted slots, mixed parities, the
    edge-first flag mixed per row, input ELU / bias / residual on and off: every row's outputs and next history equal the
    one-row kernel's on that row alone, and no arena element outside the rows' slots is written."""
    from csm.hip import ops
    C_in, C_out, k, stride, dil, groups = case
    H = (k - 1) * dil + 1 - stride
    assert H > 0
    g = torch.Generator().manual_seed(sum(case) + R)
    w = _rand(C_out, C_in // groups, k, g=g)
    bias = _rand(C_out, g=g)
    slots = PERM[:R]
    assert all(s != r for r, s in enumerate(slots))
    edges = [[r % 3 == 1 for r in range(R)]] if R > 1 else [[False], [True]]
    for edge in edges:
        for elu in (False, True):
            for b in (None, bias):
                par = [(r * 5 + 1) % 3 % 2 for r in range(R)]              # 1, 0, 0, 1, ... : mixed
                arena = torch.full((16, 2, C_in, H), NAN, device="cuda")
                ref_hist = []
                for r in range(R):
                    bufs = [torch.full((C_in, H), NAN, device="cuda") for _ in range(2)]
                    if not edge[r]:                                        # (edge-first: the first chunk must not read its history)
                        arena[slots[r], par[r]].zero_()
                        bufs[par[r]].zero_()
                    ref_hist.append(bufs)
                for i, n_out in enumerate((1, 3, 2)):
                    x = _rand(R, C_in, n_out * stride, g=g)
                    res = _rand(R, C_out, n_out, g=g) if elu else None
                    y = torch.full((R, C_out, n_out), NAN, device="cuda")
                    ops.conv1d_stream_strided_rows_f32(arena, x, w, b, y, slots, par, stride, dil, elu, res,
                                                       [e and i == 0 for e in edge])
                    for r in range(R):
                        yr = torch.empty(C_out, n_out, device="cuda")
                        ops.conv1d_stream_strided_f32(ref_hist[r][par[r]], x[r].contiguous(), w, b, yr, ref_hist[r][par[r] ^ 1], stride,
                                                      dil, elu, None if res is None else res[r].contiguous(), edge[r] and i == 0)
                        where = (case, R, edge[r], elu, b is not None, i, r)
                        assert torch.equal(y[r], yr), where
                        assert torch.equal(arena[slots[r], par[r] ^ 1], ref_hist[r][par[r] ^ 1]), where
                        assert not bool(torch.isnan(yr).any()), where
                    par = [p ^ 1 for p in par]
                others = [s for s in range(16) if s not in slots]
                assert bool(torch.isnan(arena[others]).all()), (case, R)


def test_strided_rows_kernel_refusals(dev):
    from csm.hip import CsmHipError, lib, ops
    C_in, C_out, k, stride = 4, 8, 8, 4
    g = torch.Generator().manual_seed(3)
    x, w = _rand(2, C_in, 8, g=g), _rand(C_out, C_in, k, g=g)
    arena = torch.full((16, 2, C_in, 4), 7.0, device="cuda")
    y = torch.full((2, C_out, 2), 3.0, device="cuda")

    def raw(R=2, slots=(3, 1), parity=(0, 1), mask=0, n_slots=16, n_in=8, st=stride, kk=k, arena_ptr=arena.data_ptr()):
        return lib.csm_conv1d_stream_strided_rows_f32(arena_ptr, x.data_ptr(), w.data_ptr(), None, None, y.data_ptr(), R,
                                                      ops._ints(slots), ops._ints(parity), mask, n_slots, C_in, C_out, n_in, kk, st, 1, 1,
                                                      0, _stream())

    rows_text = b"1..16 rows with distinct slots in [0, 16) and parities 0 / 1"
    for kw in (dict(R=0), dict(R=17, slots=tuple(range(17)), parity=(0,) * 17), dict(slots=(3, 3)), dict(slots=(3, 16)),
               dict(slots=(-1, 2)), dict(parity=(0, 2)), dict(parity=(-1, 0))):
        assert raw(**kw) == 1 and rows_text in lib.csm_last_error(), kw
    assert raw(slots=(3, 4), n_slots=4) == 1 and b"slots in [0, 4)" in lib.csm_last_error()
    assert raw(n_in=7) == 1 and b"n_in 7 is not a multiple of stride 4" in lib.csm_last_error()
    assert raw(n_in=6) == 1 and lib.csm_last_error().startswith(b"csm_conv1d_stream_strided_rows_f32")
    assert raw(st=8, kk=4) == 1 and b"exceeds the kernel's extent" in lib.csm_last_error()          # H < 0
    assert raw(arena_ptr=None) == 1 and b"needs the history arena" in lib.csm_last_error()           # H > 0, no arena
    assert raw(mask=4) == 1 and b"names a row >= R = 2" in lib.csm_last_error()
    assert raw(n_in=0) == 1 and raw(st=0) == 1
    with pytest.raises(CsmHipError, match="distinct slots"):
        ops.conv1d_stream_strided_rows_f32(arena, x, w, None, y, [2, 2], [0, 0], stride)
    with pytest.raises(CsmHipError, match="not a multiple of stride"):
        ops.conv1d_stream_strided_rows_f32(arena, x[:, :, :7].contiguous(), w, None, torch.empty(2, C_out, 1, device="cuda"), [0, 1],
                                           [0, 0], stride)
    torch.cuda.synchronize()
    assert bool((y == 3.0).all()) and bool((arena == 7.0).all())                                      # nothing was launched
    assert raw() == 0                                                                                 # the legal call goes through
    torch.cuda.synchronize()
    assert not bool((y == 3.0).any())
    assert torch.equal(arena[3, 1], x[0, :, 4:]) and torch.equal(arena[1, 0], x[1, :, 4:])
    arena[3, 1], arena[1, 0] = 7.0, 7.0
    assert bool((arena == 7.0).all())


# ------------------------------------------------------------------------------------------------------------- codec
@pytest.fixture(scope="module")
def hf_sd():
    return _hf_model().state_dict()


@pytest.fixture(scope="module")
def codec(dev, hf_sd):
    from csm.codec import MimiCodec
    return MimiCodec(hf_sd, device="cuda")


def _wav(n, seed):
    return (torch.randn(1, 1, n, generator=torch.Generator().manual_seed(seed)) * 0.2).cuda()


def _run_rows(stream, wavs, slot_order, cycle, opens_per_step):
    """Encode the utterances ``wavs`` ([1, 1, frames * FRAME] each) through ``stream``: ``opens_per_step`` of them join at every
    step while a slot of ``slot_order`` is free (a slot whose utterance ended is taken again), every step takes its chunk size
    from ``cycle`` - the rows that have fewer frames left sit it out; when all do, the step shrinks to the least of them.
    Returns (codes per utterance [K, frames], slots that were taken a second time, rows per step)."""
    free, waiting, active = list(slot_order), list(range(len(wavs))), {}
    got = [[] for _ in wavs]
    used, reused, widths, t = set(), [], [], 0
    while waiting or active:
        for _ in range(opens_per_step):
            if waiting and free:
                s = free.pop(0)
                stream.open(s)
                if s in used:
                    reused.append(s)
                used.add(s)
                active[s] = [waiting.pop(0), 0]
        left = {s: wavs[u].shape[2] // FRAME - at for s, (u, at) in active.items()}
        n = cycle[t % len(cycle)]
        if all(v < n for v in left.values()):
            n = min(left.values())
        part = [s for s in active if left[s] >= n]
        codes = stream.step(part, torch.stack([wavs[active[s][0]][0, 0, active[s][1] * FRAME:(active[s][1] + n) * FRAME] for s in part]))
        assert codes.shape == (len(part), 32, n) and codes.dtype == torch.int64
        widths.append(len(part))
        for r, s in enumerate(part):
            got[active[s][0]].append(codes[r])
            active[s][1] += n
            assert stream.pos[s] == active[s][1]
            if left[s] == n:
                del active[s]
                free.append(s)
        t += 1
    return [torch.cat(c, 1) for c in got], reused, widths


def test_encode_rows_16_rows_bitwise_equals_encode(dev, codec):
    """17 utterances of 10..14 frames on 16 slots: six join per step (all 16 slots run from the third step on, at three
    different phases), chunk sizes 1, 2, 4, 5, the first slot that ends is taken again by the 17th."""
    wavs = [_wav((10 + u % 5) * FRAME, 20 + u) for u in range(17)]
    refs = [codec.encode(w)[0] for w in wavs]
    stream = codec.encode_stream_rows(slots=16, max_chunk_frames=8)
    got, reused, widths = _run_rows(stream, wavs, PERM, [1, 2, 4, 5], 6)
    assert len(reused) == 1 and max(widths) == 16
    for u, (a, b) in enumerate(zip(got, refs)):
        assert a.shape == b.shape == (32, 10 + u % 5) and torch.equal(a, b), u
    with pytest.raises(ValueError, match="max_chunk_frames"):
        stream.step([0], wavs[0][0, :, :9 * FRAME])
    with pytest.raises(ValueError, match="distinct slots"):
        stream.step([1, 1], torch.zeros(2, FRAME, device="cuda"))
    with pytest.raises(ValueError, match="wav must be"):
        stream.step([1], torch.zeros(1, FRAME + 1, device="cuda"))


def test_encode_rows_small_window_ring_wraps(dev, hf_sd):
    """window 37, ring 37 + 2 * 4 - 1 = 44 rows, 80 positions per row: every row's ring wraps about twice, at its own phase."""
    from csm.codec import MimiCodec
    small = MimiCodec(hf_sd, device="cuda", window=37)
    wavs = [_wav(40 * FRAME, 40 + u) for u in range(3)]
    refs = [small.encode(w)[0] for w in wavs]
    stream = small.encode_stream_rows(slots=4, max_chunk_frames=4)
    assert stream.ring == 44
    got, _, widths = _run_rows(stream, wavs, [2, 0, 3], [1, 2, 4, 3], 1)
    assert max(widths) == 3
    for u, (a, b) in enumerate(zip(got, refs)):
        assert a.shape == (32, 40) and torch.equal(a, b), u


def test_encode_rows_feed_drain_flush(dev, codec):
    """Ragged pieces per slot, cut in the middle of frames, drained at different backlogs (1 / 3 / 4 and 5 / 3 / 0 frames, with
    max_chunk_frames = 2: the drains peel and split): the drained codes are encode's whole frames, a flushed slot's equal
    encode(zero-padded wav)."""
    stream = codec.encode_stream_rows(slots=4, max_chunk_frames=2)
    sizes = {3: 6 * FRAME + 700, 0: 9 * FRAME + 13, 2: 4 * FRAME}
    pieces = {3: [1000, 1, 5000, 0, 1919, 1920, 2380], 0: [FRAME // 2] * 18 + [13], 2: [3 * FRAME + 1, FRAME - 1]}
    wavs = {s: _wav(n, 50 + s) for s, n in sizes.items()}
    got, at = {s: [] for s in sizes}, dict.fromkeys(sizes, 0)
    for s in sizes:
        assert sum(pieces[s]) == sizes[s]
        stream.open(s)
    i = 0
    while any(at[s] < sizes[s] for s in sizes):
        for s in sizes:
            if i < len(pieces[s]):
                p = pieces[s][i]
                fed = stream.feed(s, wavs[s][0, 0, at[s]:at[s] + p] if i % 2 else wavs[s][0, 0, at[s]:at[s] + p].cpu())
                at[s] += p
                assert fed == stream.pending(s) == at[s] // FRAME - sum(c.shape[1] for c in got[s])
        if i in (2, 12) or i > 12:
            want = {s: stream.pending(s) for s in sizes}
            out = stream.drain() if i % 2 else stream.drain([0, 2, 3])
            assert sorted(out) == [0, 2, 3]
            for s, c in out.items():
                assert c.shape == (32, want[s]) and c.dtype == torch.int64 and stream.pending(s) == 0
                got[s].append(c)
        i += 1
    out = stream.drain()
    for s in sizes:
        got[s].append(out[s])
        whole = sizes[s] // FRAME
        codes = torch.cat(got[s], 1)
        assert codes.shape == (32, whole) and stream.pos[s] == whole
        assert torch.equal(codes, codec.encode(wavs[s][:, :, :whole * FRAME])[0]), s
    last = stream.drain([0, 3, 2], flush=[3, 2])                            # slot 2 holds nothing: flushing it gives nothing
    assert last[2].shape == (32, 0) and last[0].shape == (32, 0) and last[3].shape == (32, 1)
    padded = torch.cat([wavs[3], torch.zeros(1, 1, FRAME - 700, device="cuda")], 2)
    assert torch.equal(torch.cat(got[3] + [last[3]], 1), codec.encode(padded)[0])
    assert stream.drain(flush=[3])[3].shape == (32, 0) and stream.pos[3] == 7
    with pytest.raises(ValueError, match="flushes only slots it drains"):
        stream.drain([0], flush=[3])
    stream.close(0)
    assert stream.open_slots == [2, 3]
    with pytest.raises(ValueError, match="not open"):
        stream.feed(0, wavs[0][0, 0, :10])
    # a second utterance in a slot that still held a remainder when it was opened again
    stream.feed(3, wavs[3][0, 0, :100])
    stream.open(3)
    stream.feed(3, wavs[2][0, 0])
    assert torch.equal(stream.drain([3])[3], codec.encode(wavs[2])[0])


def test_encode_rows_one_row_equals_encode_stream(dev, codec):
    wav = _wav(12 * FRAME, 60)
    one, rows = codec.encode_stream(max_chunk_frames=8), codec.encode_stream_rows(slots=2, max_chunk_frames=8)
    rows.open(1)
    t0 = 0
    for n in (1, 2, 4, 5):
        piece = wav[:, :, t0 * FRAME:(t0 + n) * FRAME]
        assert torch.equal(rows.step([1], piece[0])[0], one.step(piece)[0]), n
        t0 += n
    assert rows.pos == [0, 12] and one.pos == 12


# ------------------------------------------------------------------------------------------------------------- serving
MS = 6 * 80                 # six frames per spoken turn: the tiny backbone holds 128 positions
TEMP, TOPK = 0.9, 50


@pytest.fixture(scope="module")
def gen(codec):
    from csm.generator import Generator
    return Generator(_tiny(), text_tokenizer=Tok(), audio_tokenizer=codec)


def _audio(frames, seed):
    return torch.randn(frames * FRAME, generator=torch.Generator().manual_seed(seed)) * 0.2


def test_hear_slots_equals_add_on_served_conversations(dev, gen):
    from csm.generator import Segment
    heard = [_audio(9 + i, 80 + i) for i in range(3)]
    piece = [2 * FRAME + 300, 3 * FRAME - 100, FRAME + 77]                  # per conversation: all cut in the middle of frames
    outs = []
    for form in ("add", "hear"):
        srv = gen.serve(slots=16, chunk_frames=4, temperature=TEMP, topk=TOPK, hear_slots=4)
        convs = [srv.conversation(seed=70 + i) for i in range(3)]
        r1 = [c.say("one", 0, max_audio_length_ms=MS) for c in convs]
        for _ in srv.run():
            pass
        if form == "add":
            for c, a in zip(convs, heard):
                c.add(Segment(1, "and then?", a))
        else:
            other = srv.conversation(seed=5)
            o = other.say("someone else speaks meanwhile", 2, max_audio_length_ms=12 * 80)
            turns = [c.hear(1) for c in convs]
            assert [t.slot for t in turns] == [0, 1, 2]
            extra = srv.conversation().hear(1)
            with pytest.raises(RuntimeError, match="hear_slots"):           # a fifth
                srv.conversation().hear(1)
            extra.cancel()
            again = srv.conversation()
            assert again.hear(1).slot == 3                                  # after a cancel there is room again
            again.close()
            L = [c.tokens.shape[0] for c in convs]
            at = [0, 0, 0]
            while any(at[i] < heard[i].numel() for i in range(3)):
                for i, t in enumerate(turns):
                    before = t.frames
                    t.feed(heard[i][at[i]:at[i] + piece[i]])
                    at[i] = min(at[i] + piece[i], heard[i].numel())
                    assert t.frames == before and t.frames + t.pending == at[i] // FRAME       # feed only buffers
                srv.step()
                assert all(t.pending == 0 for t in turns)
            assert [t.frames for t in turns] == [9, 10, 11] and o.done
            assert [c.tokens.shape[0] for c in convs] == L
            srv.end_heard([(turns[2], "and then?"), (turns[0], "and then?")])
            turns[1].end("and then?")
            assert srv._hearing == [None] * 4
        r2 = [c.say("two", 0, max_audio_length_ms=MS) for c in convs]
        for _ in srv.run():
            pass
        assert all(r.done for r in r1 + r2)
        outs.append([(c.tokens.clone(), c.mask.clone(), c.cached, a.codes(), b.codes(), b.audio()) for c, a, b in zip(convs, r1, r2)])
    for i, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2], i
        assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]) and torch.equal(a[5], b[5]) and a[5].numel() == 6 * FRAME, i
        assert int((a[0][:, :32] != 0).any(1).sum()) >= 9 + i               # the heard frames are in the history
