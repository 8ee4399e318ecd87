"""Streaming generation: the csm_*_stream_f32 kernels, MimiCodec.decode_stream and Generator.generate_stream.

Every decoder op of the codec is causal and computes each output with a reduction order that does not depend on the
sequence length, so a streaming decoder that carries the right state is BIT-identical to a whole-sequence decode: every
comparison below against our own full-sequence path is torch.equal.  Against the Hugging Face port (CPU, fp32, different
summation orders) the tolerance is that of tests/test_mimi_gpu.py: 2e-4 of the max magnitude."""
import wave

import pytest
import torch

pytestmark = pytest.mark.gpu

SCHEDULES = ("ones", "ragged", "whole")


def _hf_model(seed=0):
    from transformers import MimiConfig, MimiModel
    torch.manual_seed(seed)
    m = MimiModel(MimiConfig()).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, buf in m.named_buffers():
            if name.endswith("embed_sum"):
                buf.copy_(torch.randn(buf.shape, generator=g))
        for mod in m.modules():
            if hasattr(mod, "_embed"):
                mod._embed = None
        for name, p in m.named_parameters():        # layer scales start at 0.01: make the transformers matter
            if name.endswith("layer_scale.scale"):
                p.copy_(0.5 + 0.1 * torch.randn(p.shape, generator=g))
    return m


class Tok:
    def encode(self, text):
        return [1] + [3 + (b % 200) for b in text.encode()] + [2]


def _schedule(kind, total):
    """Chunk sizes summing to ``total``: all 1s, a ragged cycle, or one chunk."""
    if kind == "ones":
        return [1] * total
    if kind == "whole":
        return [total]
    out, cyc, i = [], [3, 1, 7, 2, 5, 11, 1, 4], 0
    while sum(out) < total:
        out.append(min(cyc[i % len(cyc)], total - sum(out)))
        i += 1
    return out


def _chunks(total, sched):
    t0 = 0
    for n in sched:
        yield t0, t0 + n
        t0 += n


def _rand(*shape, g):
    return torch.randn(*shape, generator=g).cuda()


# ------------------------------------------------------------------------------------------------------------- kernels
CONV_CASES = [   # C_in, C_out, k, dil, groups, elu, residual, bias
    (5, 7, 3, 1, 1, True, False, True),
    (8, 8, 7, 1, 1, False, False, True),
    (6, 9, 3, 2, 3, True, True, False),
    (4, 4, 5, 3, 4, False, True, True),
    (16, 6, 1, 1, 1, True, True, True),                 # k = 1: no history
    (12, 12, 2, 1, 2, True, False, False),
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv1d_stream_kernel_bitwise(dev, case):
    from csm.hip import check, lib, ops
    C_in, C_out, k, dil, groups, elu, use_res, use_bias = case
    T = 41
    g = torch.Generator().manual_seed(hash(case) % 1000)
    x = _rand(C_in, T, g=g)
    w = _rand(C_out, C_in // groups, k, g=g)
    b = _rand(C_out, g=g) if use_bias else None
    res = _rand(C_out, T, g=g) if use_res else None
    H = (k - 1) * dil
    full = torch.empty(C_out, T, device="cuda")
    check(lib.csm_conv1d_f32(x.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(), None if res is None else res.data_ptr(),
                             full.data_ptr(), C_in, C_out, T, T, k, 1, dil, H, 0, groups, int(elu), torch.cuda.current_stream().cuda_stream))
    for kind in SCHEDULES:
        hist = [torch.zeros(C_in, H, device="cuda"), torch.full((C_in, H), float("nan"), device="cuda")] if H else [None, None]
        ys = []
        for i, (t0, t1) in enumerate(_chunks(T, _schedule(kind, T))):
            y = torch.empty(C_out, t1 - t0, device="cuda")
            ops.conv1d_stream_f32(hist[i % 2], x[:, t0:t1].contiguous(), w, b, y, hist[(i + 1) % 2], dil, elu,
                                  None if res is None else res[:, t0:t1].contiguous())
            ys.append(y)
        assert torch.equal(torch.cat(ys, 1), full), (case, kind)


CONVT_CASES = [  # C_in, C_out, k, stride, groups, elu, bias
    (8, 8, 4, 2, 8, False, True),                       # the depthwise 2x upsample
    (6, 3, 16, 8, 1, True, True),                       # k = 2r, s = r decoder layer
    (5, 4, 10, 5, 1, True, False),
    (4, 6, 7, 2, 2, True, True),                        # 3 history columns
    (3, 5, 2, 2, 1, False, True),                       # k <= stride: no history
]


@pytest.mark.parametrize("case", CONVT_CASES)
def test_conv_transpose1d_stream_kernel_bitwise(dev, case):
    from csm.hip import check, lib, ops
    C_in, C_out, k, s, groups, elu, use_bias = case
    T = 29
    g = torch.Generator().manual_seed(hash(case) % 1000)
    x = _rand(C_in, T, g=g)
    w = _rand(C_in, C_out // groups, k, g=g)
    b = _rand(C_out, g=g) if use_bias else None
    H = (k - 1) // s
    full = torch.empty(C_out, T * s, device="cuda")
    check(lib.csm_conv_transpose1d_f32(x.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(), full.data_ptr(), C_in, C_out,
                                       T, T * s, k, s, 0, groups, int(elu), torch.cuda.current_stream().cuda_stream))
    for kind in SCHEDULES:
        hist = [torch.zeros(C_in, H, device="cuda"), torch.full((C_in, H), float("nan"), device="cuda")] if H else [None, None]
        ys = []
        for i, (t0, t1) in enumerate(_chunks(T, _schedule(kind, T))):
            y = torch.empty(C_out, (t1 - t0) * s, device="cuda")
            ops.conv_transpose1d_stream_f32(hist[i % 2], x[:, t0:t1].contiguous(), w, b, y, hist[(i + 1) % 2], t0, s, groups, elu)
            ys.append(y)
        assert torch.equal(torch.cat(ys, 1), full), (case, kind)


@pytest.mark.parametrize("window", [250, 37])
def test_attn_window_stream_kernel_bitwise(dev, window):
    """430 positions: the window slides and the ring wraps several times."""
    from csm.hip import CsmHipError, check, lib, ops
    T, H, hd = 430, 8, 64
    D = H * hd
    g = torch.Generator().manual_seed(window)
    qkv = _rand(T, 3 * D, g=g)
    full = torch.empty(T, D, device="cuda")
    check(lib.csm_attn_window_f32(qkv.data_ptr(), full.data_ptr(), T, H, hd, window, torch.cuda.current_stream().cuda_stream))
    for kind in SCHEDULES:
        sched = _schedule(kind, T)
        ring = window + max(sched) - 1
        kc = torch.full((ring, D), float("nan"), device="cuda")
        vc = torch.full((ring, D), float("nan"), device="cuda")
        outs = []
        for t0, t1 in _chunks(T, sched):
            o = torch.empty(t1 - t0, D, device="cuda")
            ops.attn_window_stream_f32(qkv[t0:t1], kc, vc, o, t0, H, window)
            outs.append(o)
        assert torch.equal(torch.cat(outs, 0), full), kind
    with pytest.raises(CsmHipError):          # one slot short: the chunk would overwrite keys its own queries read
        ops.attn_window_stream_f32(qkv[:8], kc[:window + 6], vc[:window + 6], torch.empty(8, D, device="cuda"), 0, H, window)


@pytest.mark.parametrize("epi", ["plain", "gelu", "res", "scale"])
def test_linear_few_rows_bitwise(dev, epi):
    """csm_linear_f32 on a few rows (the streaming decoder's 2n positions: one thread per output) gives the bits of the tiled
    path that a whole-sequence decode takes for the same rows."""
    from csm.hip import check, lib
    g = torch.Generator().manual_seed(len(epi))
    s = torch.cuda.current_stream().cuda_stream
    for N, K in ((512, 2048), (1536, 512), (300, 256)):
        T = 80
        x, W = _rand(T, K, g=g), _rand(N, K, g=g) * 0.05
        res = _rand(T, N, g=g) if epi in ("res", "scale") else None
        scale = _rand(N, g=g) if epi == "scale" else None
        act = int(epi == "gelu")

        def lin(rows):
            y = torch.empty(rows, N, device="cuda")
            check(lib.csm_linear_f32(x.data_ptr(), W.data_ptr(), None if scale is None else scale.data_ptr(),
                                     None if res is None else res.data_ptr(), y.data_ptr(), rows, N, K, K, act, s))
            return y

        full = lin(T)
        for rows in (1, 2, 5, 16):
            assert torch.equal(lin(rows), full[:rows]), (N, K, rows)


# ------------------------------------------------------------------------------------------------------------- codec
@pytest.fixture(scope="module")
def hf_codec():
    from csm.codec import MimiCodec
    hf = _hf_model()
    return hf, MimiCodec(hf.state_dict(), device="cuda")


def _codes(T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 2048, (1, 32, T), generator=g)


def _run_stream(stream, codes, sched):
    return torch.cat([stream.step(codes[:, :, t0:t1]) for t0, t1 in _chunks(codes.shape[2], sched)], dim=2)


def test_decode_stream_bitwise_equals_decode(dev, hf_codec):
    """150 frames = 300 decoder-transformer positions, past the 250-position window."""
    _, codec = hf_codec
    codes = _codes(150, 0).cuda()
    full = codec.decode(codes)
    assert full.shape == (1, 1, 150 * 1920)
    stream = codec.decode_stream(max_chunk_frames=8)            # the ragged schedule's 11s and the 40 need several launches
    for sched in ([1] * 150, [4] * 150, [3, 1, 7, 2, 40, 11, 1, 5] + [4] * 20):
        sched = sched[:next(i for i in range(len(sched) + 1) if sum(sched[:i]) >= 150)]
        sched[-1] -= sum(sched) - 150
        stream.reset()
        out = _run_stream(stream, codes, sched)
        assert torch.equal(out, full), sched[:8]
        assert stream.pos == 150
    stream.reset()                                              # a second, shorter utterance after reset()
    codes2 = _codes(37, 1).cuda()
    assert torch.equal(_run_stream(stream, codes2, [2] * 18 + [1]), codec.decode(codes2))


def test_decode_stream_vs_hf(dev, hf_codec):
    """The streamed audio of 150 frames against the Hugging Face decode of the same codes (this crosses the 250-position
    window, which tests/test_mimi_gpu.py's 25 frames never reach)."""
    hf, codec = hf_codec
    codes = _codes(150, 2)
    with torch.no_grad():
        ref = hf.decode(codes).audio_values
    stream = codec.decode_stream()
    out = _run_stream(stream, codes.cuda(), [5] * 30).cpu()
    assert out.shape == ref.shape
    err = (out - ref).abs().max().item() / ref.abs().max().item()
    assert err < 2e-4, f"streamed waveform rel err {err:.2e} vs HF"


# ------------------------------------------------------------------------------------------------------------- generator
def _tiny(seed=1):
    from csm.models.model import Model, ModelArgs
    return Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", 300, 2051, 32), device="cuda", seed=seed)


@pytest.fixture(scope="module")
def gen(hf_codec):
    from csm.generator import Generator
    return Generator(_tiny(), text_tokenizer=Tok(), audio_tokenizer=hf_codec[1])


def _seg():
    from csm.generator import Segment
    return Segment(0, "hi", torch.randn(24000, generator=torch.Generator().manual_seed(1)) * 0.2)


def _check_stream_equals_generate(gen, seed, frames=20, chunks=(1, 3, 8), ctx=None):
    ctx = [_seg()] if ctx is None else ctx
    torch.manual_seed(seed)
    ref = gen.generate("ok there", 1, ctx, max_audio_length_ms=80 * frames)
    assert ref.numel() == frames * 1920
    for c in chunks:
        torch.manual_seed(seed)
        parts = list(gen.generate_stream("ok there", 1, ctx, max_audio_length_ms=80 * frames, chunk_frames=c))
        assert all(p.dim() == 1 for p in parts)
        assert [p.numel() for p in parts[:-1]] == [c * 1920] * (len(parts) - 1) and 0 < parts[-1].numel() <= c * 1920
        assert torch.equal(torch.cat(parts), ref), c


def test_generate_stream_equals_generate(dev, gen):
    _check_stream_equals_generate(gen, 11)


def test_generate_stream_live_lora(dev, hf_codec):
    from csm.generator import Generator
    from csm.training.lora import apply_lora_to_model
    m = _tiny(2)
    apply_lora_to_model(m, r=8, alpha=16.0, target_modules=["q_proj", "v_proj"], seed=3)
    g = torch.Generator(device="cuda").manual_seed(99)
    with torch.no_grad():
        for ad in m.lora.adapters.values():
            ad.B[:, :8].copy_((torch.randn(ad.B.shape[0], 8, generator=g, device="cuda") * 0.05).to(torch.bfloat16))
    gl = Generator(m, text_tokenizer=Tok(), audio_tokenizer=hf_codec[1])
    _check_stream_equals_generate(gl, 5, frames=12, chunks=(1, 3, 8))


def test_generate_stream_scripted_eos(dev, gen, hf_codec):
    codec = hf_codec[1]
    m = gen._model
    script = [torch.randint(1, 2048, (1, 32), device="cuda", generator=torch.Generator("cuda").manual_seed(i)) for i in range(16)]
    script[5] = torch.zeros(1, 32, dtype=torch.long, device="cuda")
    ref = codec.decode(torch.stack(script[:5]).permute(1, 2, 0)).reshape(-1)
    try:
        for c in (1, 2, 4, 5, 8):
            calls = []
            m.generate_frame = lambda *a, _c=calls, **k: (_c.append(1), script[len(_c) - 1])[1]
            parts = list(gen.generate_stream("ok", 1, [], max_audio_length_ms=16 * 80, chunk_frames=c))
            assert sum(p.numel() for p in parts) == 5 * 1920, c
            assert torch.equal(torch.cat(parts), ref), c
            assert len(calls) == -(-6 // c) * c, c              # sampling stops with the chunk that holds the EOS frame
        script[0] = torch.zeros(1, 32, dtype=torch.long, device="cuda")
        calls = []
        m.generate_frame = lambda *a, _c=calls, **k: (_c.append(1), script[len(_c) - 1])[1]
        assert list(gen.generate_stream("ok", 1, [], max_audio_length_ms=16 * 80, chunk_frames=3)) == []
    finally:
        del m.generate_frame


def test_generate_stream_lifecycle(dev, gen, hf_codec):
    from csm.generator import Generator
    codec = hf_codec[1]

    class NoStream:                                      # Mimi's protocol without the stateful decoder
        sample_rate = codec.sample_rate
        encode, decode = codec.encode, codec.decode

    m = _tiny(4)
    calls = []
    orig = m.generate_frame
    m.generate_frame = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    with pytest.raises(TypeError):
        Generator(m, text_tokenizer=Tok(), audio_tokenizer=NoStream()).generate_stream("ok", 1, [], max_audio_length_ms=400)
    assert calls == []
    with pytest.raises(ValueError):
        gen.generate_stream("ok", 1, [], chunk_frames=0)
    with pytest.raises(ValueError):                      # the prompt-length rule of generate()
        next(gen.generate_stream("ok " * 200, 1, [], max_audio_length_ms=400))

    torch.manual_seed(21)
    fresh = gen.generate("ok", 1, [_seg()], max_audio_length_ms=10 * 80)
    # a new generate() invalidates an open stream
    s = gen.generate_stream("ok", 1, [], max_audio_length_ms=10 * 80, chunk_frames=2)
    assert next(s).numel() == 2 * 1920
    gen.generate("ok", 1, [], max_audio_length_ms=2 * 80)
    with pytest.raises(RuntimeError):
        next(s)
    # so does a new stream, and a stream that was never started
    s1 = gen.generate_stream("ok", 1, [], max_audio_length_ms=10 * 80, chunk_frames=2)
    s2 = gen.generate_stream("ok", 1, [], max_audio_length_ms=10 * 80, chunk_frames=2)
    with pytest.raises(RuntimeError):
        next(s1)
    assert next(s2).numel() == 2 * 1920
    # abandoning a stream leaves the Generator usable
    for _ in gen.generate_stream("ok", 1, [], max_audio_length_ms=10 * 80, chunk_frames=3):
        break
    torch.manual_seed(21)
    assert torch.equal(gen.generate("ok", 1, [_seg()], max_audio_length_ms=10 * 80), fresh)


# ------------------------------------------------------------------------------------------------------------- CLI
def test_cli_generate_stream_same_bytes(dev, tmp_path, monkeypatch, capsys):
    from csm.cli import generate as cli_gen
    from csm.codec import MimiCodec
    from csm.generator import Generator

    def tiny_loader(ckpt, device, mimi_weights=None, tokenizer_path=None):
        assert ckpt == "ckpt.pt" and mimi_weights == "m.safetensors" and tokenizer_path == "tokdir"
        return Generator(_tiny(2), text_tokenizer=Tok(), audio_tokenizer=MimiCodec(_hf_model(5).state_dict(), device="cuda"))

    monkeypatch.setattr(cli_gen, "load_csm_1b", tiny_loader)
    args = ["--model-path", "ckpt.pt", "--text", "hello", "--voice", "warm", "--max-audio-length-ms", "640",
            "--mimi-weights", "m.safetensors", "--text-tokenizer", "tokdir"]
    out = {}
    for mode, extra in (("plain", []), ("stream", ["--stream", "--chunk-frames", "2"])):
        torch.manual_seed(123)
        path = tmp_path / mode / "out.wav"
        assert cli_gen.main(args + ["--output", str(path)] + extra) == 0
        out[mode] = path.read_bytes()
    assert "first chunk after" in capsys.readouterr().out
    with wave.open(str(tmp_path / "stream" / "out.wav"), "rb") as w:
        assert w.getframerate() == 24000 and w.getnframes() == 8 * 1920
    assert out["stream"] == out["plain"]
