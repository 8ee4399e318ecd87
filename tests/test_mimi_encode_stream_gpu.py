"""The streaming Mimi encoder on the GPU: csm_conv1d_stream_strided_f32 chunk by chunk against csm_conv1d_f32 on the whole
input, MimiCodec.encode_stream against MimiCodec.encode, and conv.hear / feed / end against conv.add on Conversation and
ServedConversation.

Every encoder op is causal and every kernel computes an output through helpers whose reduction order does not depend on the
sequence length (conv1d_accum, attn_window_row, linear_epilogue), so every comparison here is torch.equal: no tolerance."""
import pytest
import torch

from test_stream_gpu import Tok, _chunks, _hf_model, _rand, _tiny

pytestmark = pytest.mark.gpu

FRAME = 1920


# ------------------------------------------------------------------------------------------------------------- kernel
CASES = [   # C_in, C_out, k, stride, dil, groups
    (4, 8, 8, 4, 1, 1),                                  # a SEANet downsampling shape (k = 2r, stride r)
    (8, 8, 4, 2, 1, 1),                                  # downsample: with edge_first against pad_mode 1
    (6, 4, 3, 2, 2, 1),                                  # H = 3 > n_in = 2: the next history mixes old and new columns
    (8, 8, 16, 8, 1, 8),                                 # grouped (depthwise)
    (1, 4, 7, 1, 1, 1),                                  # stride 1 through the new entry
]
T_OUT = 53                                               # outputs per run (more than one schedule cycle, odd)


def _out_schedule(kind):
    """Chunk sizes in OUTPUT columns summing to T_OUT."""
    if kind == "ones":
        return [1] * T_OUT
    if kind == "whole":
        return [T_OUT]
    out, cyc, i = [], [1, 3, 2, 5], 0
    while sum(out) < T_OUT:
        out.append(min(cyc[i % 4], T_OUT - sum(out)))
        i += 1
    return out


def _full_conv(x, w, b, res, k, stride, dil, groups, elu, pad_mode):
    from csm.hip import check, lib
    C_in, T_in = x.shape
    C_out = w.shape[0]
    H = (k - 1) * dil + 1 - stride
    y = torch.empty(C_out, T_in // stride, device="cuda")
    check(lib.csm_conv1d_f32(x.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(), None if res is None else res.data_ptr(),
                             y.data_ptr(), C_in, C_out, T_in, T_in // stride, k, stride, dil, H, pad_mode, groups, int(elu),
                             torch.cuda.current_stream().cuda_stream), "csm_conv1d_f32")
    return y


@pytest.mark.parametrize("replicate", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_strided_stream_kernel_bitwise(dev, case, replicate):
    """Outputs and the final history, input ELU on / off, with / without bias (and a residual with the ELU), three schedules;
    ``replicate``: edge_first on the first chunk against csm_conv1d_f32's pad_mode 1."""
    from csm.hip import ops
    C_in, C_out, k, stride, dil, groups = case
    H = (k - 1) * dil + 1 - stride
    g = torch.Generator().manual_seed(sum(case) + 100 * replicate)
    x = _rand(C_in, T_OUT * stride, g=g)
    w = _rand(C_out, C_in // groups, k, g=g)
    bias = _rand(C_out, g=g)
    resid = _rand(C_out, T_OUT, g=g)
    left = x[:, :1].expand(C_in, H) if replicate else torch.zeros(C_in, H, device="cuda")
    want_hist = torch.cat([left, x], 1)[:, T_OUT * stride:]
    for elu in (False, True):
        for b in (None, bias):
            res = resid if elu else None
            full = _full_conv(x, w, b, res, k, stride, dil, groups, elu, int(replicate))
            for kind in ("ones", "ragged", "whole"):
                hist = [torch.full((C_in, H), float("nan"), device="cuda") for _ in range(2)] if H else [None, None]
                if H and not replicate:
                    hist[0].zero_()                      # (replicate: the first chunk must not read its history - it stays NaN)
                ys = []
                for i, (t0, t1) in enumerate(_chunks(T_OUT, _out_schedule(kind))):
                    y = torch.empty(C_out, t1 - t0, device="cuda")
                    ops.conv1d_stream_strided_f32(hist[i % 2], x[:, t0 * stride:t1 * stride].contiguous(), w, b, y, hist[(i + 1) % 2],
                                                  stride, dil, elu, None if res is None else res[:, t0:t1].contiguous(),
                                                  edge_first=replicate and i == 0)
                    ys.append(y)
                assert torch.equal(torch.cat(ys, 1), full), (case, replicate, elu, b is not None, kind)
                if H:
                    assert torch.equal(hist[(i + 1) % 2], want_hist), (case, replicate, kind)


def test_strided_stream_kernel_refusals(dev):
    from csm.hip import CsmHipError, lib, ops
    C_in, C_out, k, stride = 4, 8, 8, 4
    g = torch.Generator().manual_seed(3)
    x, w = _rand(C_in, 8, g=g), _rand(C_out, C_in, k, g=g)
    h0, h1 = torch.zeros(C_in, 4, device="cuda"), torch.full((C_in, 4), 7.0, device="cuda")
    y = torch.full((C_out, 2), 3.0, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def raw(hist=h0, hist_out=h1, n_in=8, st=stride, kk=k):
        return lib.csm_conv1d_stream_strided_f32(hist.data_ptr(), x.data_ptr(), w.data_ptr(), None, None, y.data_ptr(), hist_out.data_ptr(),
                                                 C_in, C_out, n_in, kk, st, 1, 1, 0, 0, s)

    assert raw(n_in=7) == 1 and b"n_in 7 is not a multiple of stride 4" in lib.csm_last_error()
    assert raw(n_in=6) == 1 and lib.csm_last_error().startswith(b"csm_conv1d_stream_strided_f32")
    assert raw(hist_out=h0) == 1 and b"two distinct history buffers" in lib.csm_last_error()
    assert raw(n_in=0) == 1 and raw(st=0) == 1
    assert raw(st=8, kk=4) == 1 and b"exceeds the kernel's extent" in lib.csm_last_error()
    with pytest.raises(CsmHipError, match="not a multiple of stride"):
        ops.conv1d_stream_strided_f32(h0, x[:, :7].contiguous(), w, None, torch.empty(C_out, 1, device="cuda"), h1, stride)
    with pytest.raises(CsmHipError, match="two distinct history buffers"):
        ops.conv1d_stream_strided_f32(h0, x, w, None, y, h0, stride)
    torch.cuda.synchronize()
    assert bool((y == 3.0).all()) and bool((h1 == 7.0).all()) and bool((h0 == 0.0).all())      # nothing was launched
    ops.conv1d_stream_strided_f32(h0, x, w, None, y, h1, stride)                               # the legal call goes through
    torch.cuda.synchronize()
    assert not bool((y == 3.0).any()) and torch.equal(h1, x[:, 4:])


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


def _frame_schedule(kind, total):
    if kind == "mixed":
        out, cyc, i = [], [1, 2, 4, 5], 0
        while sum(out) < total:
            out.append(min(cyc[i % 4], total - sum(out)))
            i += 1
        return out
    return [min(kind, total - t) for t in range(0, total, kind)]


def _run_steps(stream, wav, sched):
    return torch.cat([stream.step(wav[:, :, t0 * FRAME:t1 * FRAME]) for t0, t1 in _chunks(wav.shape[2] // FRAME, sched)], dim=2)


@pytest.fixture(scope="module")
def long_ref(codec):
    """150 frames = 300 encoder-transformer positions, past the 250-position window: (wav, encode(wav))."""
    wav = _wav(150 * FRAME, 0)
    ref = codec.encode(wav)
    assert ref.shape == (1, 32, 150) and ref.dtype == torch.int64
    return wav, ref


@pytest.mark.parametrize("kind", [1, "mixed", 32])
def test_encode_stream_bitwise_equals_encode(dev, codec, long_ref, kind):
    wav, ref = long_ref
    stream = codec.encode_stream()
    out = _run_steps(stream, wav, _frame_schedule(kind, 150))
    assert out.dtype == torch.int64 and out.shape == ref.shape
    assert torch.equal(out[0], ref[0]), kind
    assert stream.pos == 150
    for bad in (0, 1, FRAME - 1, FRAME + 1):
        with pytest.raises(ValueError, match="whole number"):
            stream.step(wav[:, :, :bad])


def test_encode_stream_small_window_ring_wraps(dev, hf_sd):
    """window 37, ring 37 + 2 * 4 - 1 = 44 rows, 80 positions: the ring wraps about twice and the window slides over it."""
    from csm.codec import MimiCodec
    small = MimiCodec(hf_sd, device="cuda", window=37)
    wav = _wav(40 * FRAME, 1)
    ref = small.encode(wav)
    for kind, mcf in ((1, 4), ("mixed", 4), (32, 32)):
        stream = small.encode_stream(max_chunk_frames=mcf)          # "mixed" has chunks of 5 > 4: several attention launches
        assert torch.equal(_run_steps(stream, wav, _frame_schedule(kind, 40))[0], ref[0]), kind


def test_encode_stream_feed_flush_reset(dev, codec):
    n = 20 * FRAME + 700
    wav = _wav(n, 2)
    ref = codec.encode(wav)                                                                   # 21 frames: every layer padded on the right
    padded = torch.cat([wav, torch.zeros(1, 1, FRAME - 700, device="cuda")], 2)
    ref_pad = codec.encode(padded)
    assert ref.shape[2] == ref_pad.shape[2] == 21
    stream = codec.encode_stream()
    pieces, at, got = [1000, 1, 5000, 0, 1919, 1920, 1, 3839, 0, 7], 0, []
    i = 0
    while at < n:
        p = min(pieces[i % len(pieces)] if i < len(pieces) else 6001, n - at)
        c = stream.feed(wav[:, :, at:at + p])
        assert c.shape[:2] == (1, 32) and c.dtype == torch.int64 and c.shape[2] == (at + p) // FRAME - at // FRAME
        got.append(c)
        at += p
        i += 1
    assert stream.feed(wav[:, :, :0]).shape == (1, 32, 0)
    whole = torch.cat(got, 2)
    assert whole.shape[2] == 20 and torch.equal(whole[0], ref[0, :, :20]) and torch.equal(whole[0], ref_pad[0, :, :20])
    last = stream.flush()
    assert last.shape == (1, 32, 1) and torch.equal(torch.cat([whole, last], 2)[0], ref_pad[0])
    assert stream.flush().shape == (1, 32, 0) and stream.pos == 21
    # a second utterance after reset(), with a remainder dropped by it
    stream.feed(wav[:, :, :100])
    stream.reset()
    wav2 = _wav(9 * FRAME, 3)
    assert torch.equal(torch.cat([stream.feed(wav2[:, :, :5000]), stream.feed(wav2[:, :, 5000:])], 2)[0], codec.encode(wav2)[0])
    assert stream.flush().shape == (1, 32, 0)


# ------------------------------------------------------------------------------------------------------------- conversations
MS = 6 * 80                 # six frames per turn: the tiny backbone holds 128 positions
TEMP, TOPK = 0.9, 50


@pytest.fixture(scope="module")
def gen(codec):
    from csm.generator import Generator
    return Generator(_tiny(), text_tokenizer=Tok(), audio_tokenizer=codec)


def _audio(frames, seed):
    return torch.randn(frames * FRAME, generator=torch.Generator().manual_seed(seed)) * 0.2


def _feed_in_pieces(turn, audio):
    """1-, 2-, 3-, 4-frame pieces, one of them cut in the middle of a frame."""
    at, sizes, i = 0, [FRAME, 2 * FRAME, 3 * FRAME - 500, 500 + 4 * FRAME], 0
    while at < audio.numel():
        p = min(sizes[i % 4], audio.numel() - at)
        turn.feed(audio[at:at + p])
        at += p
        i += 1
    assert turn.frames == audio.numel() // FRAME


def test_hear_equals_add_on_conversation(dev, gen):
    from csm.generator import Segment
    heard = _audio(11, 5)
    outs = []
    for form in ("add", "hear"):
        conv = gen.conversation()
        torch.manual_seed(41)
        first = conv.generate("one", 0, max_audio_length_ms=MS)
        if form == "add":
            conv.add(Segment(1, "and then?", heard))
        else:
            turn = conv.hear(1)
            L, cached = conv.tokens.shape[0], conv.cached
            _feed_in_pieces(turn, heard)
            assert conv.tokens.shape[0] == L and conv.cached == cached          # feed touches neither history nor cache
            turn.end("and then?")
        torch.manual_seed(42)
        outs.append((conv.tokens.clone(), conv.mask.clone(), first, conv.generate("two", 0, max_audio_length_ms=MS), conv.cached))
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and a[3].numel() == 6 * FRAME and a[4] == b[4]
    assert int((a[0][:, :32] != 0).any(1).sum()) >= 11                          # the heard frames are in the history


def test_hear_equals_add_on_served_conversation(dev, gen):
    from csm.generator import Segment
    heard = _audio(9, 6)
    outs = []
    for form in ("add", "hear"):
        srv = gen.serve(slots=16, chunk_frames=4, temperature=TEMP, topk=TOPK)
        conv = srv.conversation(seed=77)
        r1 = conv.say("one", 0, max_audio_length_ms=MS)
        for _ in srv.run():
            pass
        if form == "add":
            conv.add(Segment(1, "and then?", heard))
        else:
            other = srv.conversation(seed=5)
            o = other.say("someone else speaks meanwhile", 2, max_audio_length_ms=12 * 80)
            turn = conv.hear(1)
            L = conv.tokens.shape[0]
            for lo in range(0, heard.numel(), 3 * FRAME):                       # a 3-frame piece between the server's steps
                turn.feed(heard[lo:lo + 3 * FRAME])
                srv.step()
            assert turn.frames == 9 and conv.tokens.shape[0] == L and o.done
            turn.end("and then?")
        r2 = conv.say("two", 0, max_audio_length_ms=MS)
        for _ in srv.run():
            pass
        assert r1.done and r2.done
        outs.append((conv.tokens.clone(), conv.mask.clone(), r1.codes(), r2.codes(), r2.audio(), conv.cached))
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[5] == b[5]
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]) and a[4].numel() == 6 * FRAME
