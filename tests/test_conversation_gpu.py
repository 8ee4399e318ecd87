"""Conversations: csm_attn_append (a chunk of new positions against the KV cache), DecodeState.append / truncate and
Generator.conversation.

Accuracy bounds are relative to the path that exists today on the same problem: csm_attn_append may err at most 2x what
csm_attn_fwd errs against fp32 attention over the same cases, and prefill + append at most 2x what one prefill errs against the
fp32 oracle - both kernels round at the same points and differ only in summation order, so their errors are draws from the
same distribution and 2x covers the spread.  Everything that compares our own paths with each other is torch.equal."""
import wave

import pytest
import torch

pytestmark = pytest.mark.gpu

HD = 64
SHAPES = [(4, 2), (32, 8)]                       # (H, KV): the tiny and the CSM-1B backbone
S_MAX = 2048


# ------------------------------------------------------------------------------------------------------------- kernel
def _bits(t):
    return t.view(torch.int16)


def _rand_qkv(S, H, KV, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(S, (H + 2 * KV) * HD, generator=g).to(torch.bfloat16).cuda()


def _split(qkv, H, KV):
    S = qkv.shape[0]
    q = qkv[:, :H * HD].reshape(S, H, HD)
    k = qkv[:, H * HD:(H + KV) * HD].reshape(S, KV, HD)
    v = qkv[:, (H + KV) * HD:].reshape(S, KV, HD)
    return q, k, v


def _caches(qkv, H, KV, pos0, s_max=S_MAX, B=1, row=0, fill=0.0):
    """Caches [B, KV, s_max, HD] whose row ``row`` holds the first ``pos0`` positions of ``qkv``; ``fill`` everywhere else."""
    _, k, v = _split(qkv, H, KV)
    kc = torch.full((B, KV, s_max, HD), fill, dtype=torch.bfloat16, device="cuda")
    vc = torch.full((B, KV, s_max, HD), fill, dtype=torch.bfloat16, device="cuda")
    kc[row, :, :pos0] = k[:pos0].permute(1, 0, 2)
    vc[row, :, :pos0] = v[:pos0].permute(1, 0, 2)
    return kc, vc


def _ref_rows(qkv, H, KV, pos0):
    """fp32 attention of rows pos0.. of the full causal problem: [S - pos0, H * HD] fp32."""
    q, k, v = _split(qkv.float(), H, KV)
    S, rep = qkv.shape[0], H // KV
    k, v = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)
    s = torch.einsum("qhd,khd->hqk", q[pos0:], k) / HD ** 0.5
    qpos = torch.arange(pos0, S, device="cuda")[:, None]
    s = s.masked_fill(torch.arange(S, device="cuda")[None, :] > qpos, float("-inf"))
    return torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), v).reshape(S - pos0, H * HD)


def _append(qkv_new, kc, vc, pos0, H, KV, row=0):
    from csm.hip import ops
    out = torch.empty(qkv_new.shape[0], H * HD, dtype=torch.bfloat16, device="cuda")
    ops.attn_append(qkv_new.contiguous(), kc, vc, out, row, pos0, H, KV, HD)
    return out


def test_attn_append_accuracy_vs_fp32(dev):
    """Measured on one MI355X, max abs error over the 42 cases of each shape: H/KV = 4/2 append 7.9e-3, csm_attn_fwd 8.4e-3;
    32/8 append 9.0e-3, csm_attn_fwd 9.2e-3 (bound 1.85e-2)."""
    from csm.hip import ops
    worst_app, worst_fwd = 0.0, 0.0
    for H, KV in SHAPES:
        w_app, w_fwd = 0.0, 0.0
        for n in (1, 5, 16, 17, 64, 200):
            for pos0 in (0, 1, 63, 64, 65, 1000, S_MAX - n):
                S = pos0 + n
                qkv = _rand_qkv(S, H, KV, seed=1000 * n + pos0 + H)
                ref = _ref_rows(qkv, H, KV, pos0)
                kc, vc = _caches(qkv, H, KV, pos0)
                got = _append(qkv[pos0:], kc, vc, pos0, H, KV)
                full = torch.empty(S, H * HD, dtype=torch.bfloat16, device="cuda")
                lse = torch.empty(1, H, S, dtype=torch.float32, device="cuda")
                ops.attn_fwd(qkv, full, lse, 1, S, H, KV, HD)
                e_app = float((got.float() - ref).abs().max())
                e_fwd = float((full[pos0:].float() - ref).abs().max())
                assert e_app == e_app, (H, KV, n, pos0)                  # NaN
                w_app, w_fwd = max(w_app, e_app), max(w_fwd, e_fwd)
        print(f"attn_append H={H} KV={KV}: max |err| vs fp32 append {w_app:.3e}, attn_fwd {w_fwd:.3e}")
        worst_app, worst_fwd = max(worst_app, w_app), max(worst_fwd, w_fwd)
    print(f"attn_append all cases: append {worst_app:.3e}, attn_fwd {worst_fwd:.3e}, bound {2 * worst_fwd:.3e}")
    assert worst_app <= 2 * worst_fwd, (worst_app, worst_fwd)


@pytest.mark.parametrize("H,KV", SHAPES)
@pytest.mark.parametrize("pos0", [0, 333])
def test_attn_append_bit_invariance(dev, H, KV, pos0):
    n = 200
    qkv = _rand_qkv(pos0 + n, H, KV, seed=7 + pos0)
    kc1, vc1 = _caches(qkv, H, KV, pos0)
    one = _append(qkv[pos0:], kc1, vc1, pos0, H, KV)
    for sched in ([1, 15, 16, 17, 151], [1] * n):
        kc, vc = _caches(qkv, H, KV, pos0)
        outs, p = [], pos0
        for c in sched:
            outs.append(_append(qkv[p:p + c], kc, vc, p, H, KV))
            p += c
        assert torch.equal(_bits(torch.cat(outs)), _bits(one)), (H, KV, sched[:5])
        assert torch.equal(_bits(kc), _bits(kc1)) and torch.equal(_bits(vc), _bits(vc1))


@pytest.mark.parametrize("H,KV", SHAPES)
def test_attn_append_cache_writes(dev, H, KV):
    B, row, s_max, pos0, n = 3, 1, 96, 40, 37
    qkv = _rand_qkv(pos0 + n, H, KV, seed=3)
    kc, vc = _caches(qkv, H, KV, pos0, s_max=s_max, B=B, row=row, fill=0.1005859375)      # guard pattern: every other element
    want_k, want_v = kc.clone(), vc.clone()
    _, k, v = _split(qkv, H, KV)
    want_k[row, :, pos0:pos0 + n] = k[pos0:].permute(1, 0, 2)
    want_v[row, :, pos0:pos0 + n] = v[pos0:].permute(1, 0, 2)
    _append(qkv[pos0:], kc, vc, pos0, H, KV, row=row)
    assert torch.equal(_bits(kc), _bits(want_k)) and torch.equal(_bits(vc), _bits(want_v))
    # up to the last row of the cache: the heads that follow in memory keep their guard
    kc2, vc2 = _caches(qkv, H, KV, s_max - n, s_max=s_max, B=B, row=row, fill=0.1005859375)
    g_k, g_v = kc2.clone(), vc2.clone()
    q2 = _rand_qkv(n, H, KV, seed=4)
    _, k2, v2 = _split(q2, H, KV)
    g_k[row, :, s_max - n:] = k2.permute(1, 0, 2)
    g_v[row, :, s_max - n:] = v2.permute(1, 0, 2)
    _append(q2, kc2, vc2, s_max - n, H, KV, row=row)
    assert torch.equal(_bits(kc2), _bits(g_k)) and torch.equal(_bits(vc2), _bits(g_v))


def test_attn_append_bad_arguments(dev):
    from csm.hip import CsmHipError, check, lib, ops
    H, KV, s_max = 4, 2, 64
    qkv = _rand_qkv(8, H, KV, seed=5)
    kc, vc = _caches(qkv, H, KV, 0, s_max=s_max, B=2, fill=0.5)
    k0, v0 = kc.clone(), vc.clone()
    out = torch.full((8, H * HD), 3.0, dtype=torch.bfloat16, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def raw(row=0, pos0=0, n=8, hd=HD, h=H, kv=KV):
        return lib.csm_attn_append(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), row, pos0, n, h, kv, hd, s_max, 0.125, stream)

    assert raw(pos0=s_max - 7) == 1 and b"outside the cache" in lib.csm_last_error()
    assert raw(n=0) == 1 and raw(n=-3) == 1
    assert raw(pos0=-1) == 1
    assert raw(row=-1) == 1
    assert raw(hd=128) == 1 and b"head_dim 128 unsupported" in lib.csm_last_error()
    assert raw(h=5) == 1
    assert lib.csm_attn_append(None, kc.data_ptr(), vc.data_ptr(), out.data_ptr(), 0, 0, 8, H, KV, HD, s_max, 0.125, stream) == 1
    for row in (-1, 2):
        with pytest.raises(CsmHipError):
            ops.attn_append(qkv, kc, vc, out, row, 0, H, KV, HD)
    with pytest.raises(CsmHipError):
        ops.attn_append(qkv, kc, vc, out, 0, s_max - 7, H, KV, HD)
    torch.cuda.synchronize()
    assert torch.equal(kc, k0) and torch.equal(vc, v0) and bool((out == 3.0).all())          # nothing was launched
    check(raw(pos0=s_max - 8), "csm_attn_append")                                            # the last legal position is fine
    torch.cuda.synchronize()
    assert not torch.equal(kc, k0)


# ------------------------------------------------------------------------------------------------------------- engine
def _oracle():
    from oracle import csm_oracle as O
    return O, O.tiny_cfg()


def _tiny_oracle_model(seed=11):
    from csm.models.model import Model, ModelArgs
    O, T = _oracle()
    m = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", T.text_vocab, T.audio_vocab, T.n_codebooks), device="cuda")
    p32 = O.init_params(T, seed=seed)
    m.load_state_dict(p32)
    m.setup_caches(1)
    return m, p32


def _noise(step):
    _, T = _oracle()
    g = torch.Generator().manual_seed(700 + step)
    return [torch.empty(1, T.audio_vocab).exponential_(1, generator=g) for _ in range(T.n_codebooks)]


def _audio_frame(sample):
    K = sample.shape[1]
    tok = torch.cat([sample.long().cpu(), torch.zeros(1, 1, dtype=torch.long)], 1).unsqueeze(1)
    msk = torch.cat([torch.ones(1, K, dtype=torch.bool), torch.zeros(1, 1, dtype=torch.bool)], 1).unsqueeze(1)
    return tok, msk


def _c0_logits(m, last_h):
    from csm.hip import ops
    lg = torch.empty(1, m.vocab_pad, dtype=torch.float32, device="cuda")
    ops.gemv(last_h.contiguous(), m.block("codebook0_head.padded"), lg)
    return lg[0, :m.args.audio_vocab_size].clone()


def _decode(m, st, sample, step):
    """Feed ``sample`` on state ``st`` through Model.generate_frame (the GEMV decode path), return the next sample."""
    tok, msk = _audio_frame(sample)
    m._decode_state = st
    return m.generate_frame(tok, msk, torch.ones(1, 1, dtype=torch.long), 0.8, 12, noise=_noise(step))


def _append_vs_prefill(m, p32, lora=None, adapters=None, between=0, S1=17, n=13, seed=21):
    """(error of prefill(S1) [+ ``between`` decode frames] + append(n), error of ONE prefill of the same sequence), both as
    max |codebook-0 logits - fp32 oracle| of the next frame."""
    from csm.engine import DecodeState
    O, T = _oracle()
    e = m.engine
    e._need()
    tokens, mask, _ = O.synthetic_batch(T, 1, S1 + n, seed=seed)
    st = DecodeState(e, 1, adapters)
    last_h = st.prefill(tokens[:, :S1].cuda(), mask[:, :S1].cuda())
    seq_t, seq_m = [tokens[0, :S1]], [mask[0, :S1]]
    if between:
        sample = e._frame_tail(st, last_h, 0.8, 12, _noise(0))
        for step in range(between):
            tok, msk = _audio_frame(sample)
            seq_t.append(tok[0])
            seq_m.append(msk[0])
            sample = _decode(m, st, sample, 1 + step)
        assert st.cur == S1 + between - 1
    seq_t.append(tokens[0, S1:])
    seq_m.append(mask[0, S1:])
    got = _c0_logits(m, st.append(tokens[0, S1:].cuda(), mask[0, S1:].cuda()))
    assert st.cur == S1 + between + n - 1 and int(st.bb.pos[0]) == st.cur
    full_t, full_m = torch.cat(seq_t, 0).unsqueeze(0), torch.cat(seq_m, 0).unsqueeze(0)
    st2 = DecodeState(e, 1, adapters)
    one = _c0_logits(m, st2.prefill(full_t.cuda(), full_m.cuda()))
    with torch.no_grad():
        hid = O.backbone_hidden(p32, T, full_t, full_m, lora=lora, lora_scaling=2.0)
        ref = hid[0, -1].float() @ p32["codebook0_head.weight"].t().float()
    m._decode_state = None
    return float((got.cpu() - ref).abs().max()), float((one.cpu() - ref).abs().max()), float(ref.abs().max())


@pytest.mark.parametrize("between", [0, 6])
def test_append_vs_one_prefill_against_oracle(dev, between):
    """Measured on one MI355X (max |logit| 0.65): append 4.2e-3 against one prefill 5.2e-3; with 6 decode frames between
    5.0e-3 against 4.6e-3.  With a q_proj / v_proj adapter (live and bank alike): 5.2e-3 against 5.0e-3, and 5.5e-3 against
    5.1e-3 with the decode frames."""
    m, p32 = _tiny_oracle_model()
    e_app, e_one, scale = _append_vs_prefill(m, p32, between=between)
    print(f"append vs oracle (decode frames between: {between}): append {e_app:.3e}, one prefill {e_one:.3e}, max |logit| {scale:.3e}")
    assert e_app <= 2 * e_one, (e_app, e_one)


@pytest.mark.parametrize("kind", ["live", "bank"])
@pytest.mark.parametrize("between", [0, 6])
def test_append_with_adapters_against_oracle(dev, kind, between):
    from csm.training.lora import LoRAState, apply_lora_to_model
    m, p32 = _tiny_oracle_model()
    if kind == "live":
        apply_lora_to_model(m, r=8, alpha=16.0, target_modules=["q_proj", "v_proj"], seed=3)
        state, adapters = m.lora, None
    else:
        state = LoRAState(m, 8, 16.0, 0.0, ["q_proj", "v_proj"], None, False, seed=3, grad=False)
        adapters = [state]
    g = torch.Generator(device="cuda").manual_seed(99)
    with torch.no_grad():
        for ad in state.adapters.values():
            ad.B[:, :8].copy_((torch.randn(ad.B.shape[0], 8, generator=g, device="cuda") * 0.05).to(torch.bfloat16))
    lora = {k: v.detach().float().cpu() for k, v in state.named_tensors()}
    e_app, e_one, scale = _append_vs_prefill(m, p32, lora=lora, adapters=adapters, between=between)
    e_none, _, _ = _append_vs_prefill(m, p32, lora=None, adapters=adapters, between=between)
    print(f"append vs oracle, {kind} adapter (decode frames between: {between}): append {e_app:.3e}, one prefill {e_one:.3e}, "
          f"max |logit| {scale:.3e}; against the oracle WITHOUT the adapter {e_none:.3e}")
    assert e_app <= 2 * e_one, (e_app, e_one)
    assert e_none > e_app, "the adapter must matter for this to test anything"


@pytest.mark.parametrize("graph", [True, False])
def test_append_truncate_bits_and_graph_survives(dev, graph):
    from csm.engine import DecodeState
    O, T = _oracle()
    m, _ = _tiny_oracle_model()
    tokens, mask, _ = O.synthetic_batch(T, 1, 40, seed=5)
    tokens, mask = tokens.cuda(), mask.cuda()
    S1, n = 11, 9

    def run(use_graph):
        m.use_hip_graph = use_graph
        try:
            st = DecodeState(m.engine, 1)
            last_h = st.prefill(tokens[:, :S1], mask[:, :S1])
            out = [m.engine._frame_tail(st, last_h, 0.8, 12, _noise(0))]
            for step in range(1, 4):
                out.append(_decode(m, st, out[-1], step))
            g0, cur0 = st.graph, st.cur
            if use_graph:
                assert g0 is not None
            h1 = st.append(tokens[0, S1:S1 + n], mask[0, S1:S1 + n]).clone()
            k1 = [k.clone() for k in st.bb.k]
            assert st.cur == cur0 + n and int(st.bb.pos[0]) == st.cur
            st.truncate(cur0 + 1)
            assert st.cur == cur0 and int(st.bb.pos[0]) == cur0
            h2 = st.append(tokens[0, S1:S1 + n], mask[0, S1:S1 + n]).clone()
            assert torch.equal(h1, h2) and all(torch.equal(a, b) for a, b in zip(k1, st.bb.k))
            assert st.graph is g0                                      # no re-capture between turns
            out.append(m.engine._frame_tail(st, h2, 0.8, 12, _noise(10)))
            for step in range(11, 14):
                out.append(_decode(m, st, out[-1], step))
            assert st.graph is g0 and st.cur == cur0 + n + 3
            with pytest.raises(ValueError):
                st.truncate(st.cur + 2)
            with pytest.raises(ValueError):
                st.truncate(0)
            return torch.cat(out).cpu()
        finally:
            m.use_hip_graph = True
            m._decode_state = None

    a = run(graph)
    if graph:
        assert torch.equal(a, run(False))                             # replayed frames after an append equal eager ones


# ------------------------------------------------------------------------------------------------------------- generator
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
        for name, p in m.named_parameters():
            if name.endswith("layer_scale.scale"):
                p.copy_(0.5 + 0.1 * torch.randn(p.shape, generator=g))
    return m


class Tok:
    def encode(self, text):
        return [1] + [3 + (b % 200) for b in text.encode()] + [2]


class CountingCodec:
    """The codec with its ``encode`` calls counted (lengths in samples)."""

    def __init__(self, codec):
        self._c, self.encoded = codec, []
        self.sample_rate = codec.sample_rate
        self.decode, self.decode_stream = codec.decode, codec.decode_stream

    def encode(self, audio):
        self.encoded.append(audio.shape[-1])
        return self._c.encode(audio)


@pytest.fixture(scope="module")
def codec():
    from csm.codec import MimiCodec
    return MimiCodec(_hf_model().state_dict(), device="cuda")


def _tiny(seed=1):
    from csm.models.model import Model, ModelArgs
    return Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", 300, 2051, 32), device="cuda", seed=seed)


@pytest.fixture(scope="module")
def gen(codec):
    from csm.generator import Generator
    return Generator(_tiny(), text_tokenizer=Tok(), audio_tokenizer=CountingCodec(codec))


def _seg(seed=1, frames=5, speaker=0, text="hi"):
    from csm.generator import Segment
    return Segment(speaker, text, torch.randn(frames * 1920, generator=torch.Generator().manual_seed(seed)) * 0.2)


MS = 6 * 80                 # six frames per turn: the tiny backbone holds 128 positions


def _pos(conv):
    return int(conv._state.bb.pos[0]) + 1


@pytest.mark.parametrize("ctx", [0, 2])
def test_first_turn_equals_generate(dev, gen, ctx):
    context = [_seg(i + 1, speaker=i % 2) for i in range(ctx)]
    torch.manual_seed(31)
    ref = gen.generate("ok there", 1, context, max_audio_length_ms=MS)
    torch.manual_seed(31)
    conv = gen.conversation(context=context)
    got = conv.generate("ok there", 1, max_audio_length_ms=MS)
    assert ref.numel() == 6 * 1920 and torch.equal(got, ref)
    torch.manual_seed(31)
    parts = list(gen.conversation(context=context).generate_stream("ok there", 1, max_audio_length_ms=MS, chunk_frames=4))
    assert torch.equal(torch.cat(parts), ref)


def test_three_turns_with_add(dev, gen, monkeypatch):
    import csm.conversation as C
    made = []

    class Counting(C.DecodeState):
        def __init__(self, *a, **k):
            made.append(1)
            super().__init__(*a, **k)

    monkeypatch.setattr(C, "DecodeState", Counting)
    cc = gen._audio_tokenizer
    cc.encoded.clear()
    conv = gen.conversation(context=[_seg(1)])
    assert cc.encoded == [5 * 1920] and conv.cached == 0
    torch.manual_seed(3)
    a1 = conv.generate("one", 0, max_audio_length_ms=MS)
    L1 = conv.tokens.shape[0]
    # the frame limit was hit: 6 frames kept + the EOS frame in the history, the last frame and the EOS frame not cached yet
    assert a1.numel() == 6 * 1920 and conv.cached == L1 - 2 == _pos(conv) and not conv.tokens[-1].any()
    conv.add(_seg(2, frames=4, speaker=1, text="and?"))
    assert cc.encoded == [5 * 1920, 4 * 1920] and conv.cached == L1 - 2
    a2 = conv.generate("two", 0, max_audio_length_ms=MS)
    L2 = conv.tokens.shape[0]
    assert conv.cached == L2 - 2 == _pos(conv)
    g = conv._state.graph
    a3 = conv.generate("three", 0, max_audio_length_ms=MS, eos_check_every=1)
    assert conv.cached == conv.tokens.shape[0] - 2 == _pos(conv)
    assert cc.encoded == [5 * 1920, 4 * 1920] and made == [1]
    assert g is not None and conv._state.graph is g
    assert a2.numel() == a3.numel() == 6 * 1920
    assert bool(conv.mask[:, :-1].any(1).logical_xor(conv.mask[:, -1]).all())     # every frame is text or audio


def _three(gen, disturb):
    """Turn 3 of a seeded conversation; ``disturb`` runs other work on the same Generator between the turns."""
    conv = gen.conversation(context=[_seg(1)])
    torch.manual_seed(4)
    conv.generate("one", 0, max_audio_length_ms=MS)
    conv.add(_seg(2, frames=4, speaker=1, text="and?"))
    conv.generate("two", 0, max_audio_length_ms=MS)
    if disturb:
        gen.generate("elsewhere", 1, [_seg(3)], max_audio_length_ms=MS)
        other = gen.conversation()
        other.generate("someone else", 1, max_audio_length_ms=MS)
        other.generate("again", 1, max_audio_length_ms=MS)
    torch.manual_seed(5)
    return conv, conv.generate("three", 0, max_audio_length_ms=MS)


def test_isolation_and_stream_equals_plain(dev, gen):
    c1, ref = _three(gen, False)
    c2, got = _three(gen, True)
    assert torch.equal(got, ref) and torch.equal(c1.tokens, c2.tokens) and c1.cached == c2.cached
    # the same fourth turn through generate and through generate_stream
    torch.manual_seed(6)
    plain = c1.generate("four", 1, max_audio_length_ms=MS, eos_check_every=4)
    torch.manual_seed(6)
    s = c2.generate_stream("four", 1, max_audio_length_ms=MS, chunk_frames=4)
    parts = list(s)
    assert [p.numel() for p in parts] == [4 * 1920, 2 * 1920] and torch.equal(torch.cat(parts), plain)
    assert torch.equal(c1.tokens, c2.tokens) and c1.cached == c2.cached == _pos(c2)
    # its own next call invalidates a conversation's open stream; what was handed out stays in the history
    s = c2.generate_stream("five", 1, max_audio_length_ms=MS, chunk_frames=2)
    next(s)
    L = c2.tokens.shape[0]
    gen.generate("elsewhere", 1, [], max_audio_length_ms=MS)          # not this conversation's call: the stream lives on
    next(s)
    c2.add(_seg(4, frames=3))
    with pytest.raises(RuntimeError):
        next(s)
    assert c2.cached == _pos(c2) == L + 3 and not c2.tokens[L + 4].any() and bool(c2.tokens[L + 3].any())


def _capture_tail(m, into):
    orig = m.engine._frame_tail

    def tail(st, last_h, *a, **k):
        into.append(_c0_logits(m, last_h))
        return orig(st, last_h, *a, **k)
    m.engine._frame_tail = tail


def test_scripted_eos_truncates_cache(dev, gen):
    m = gen._model
    orig = m.generate_frame
    logits = []
    try:
        _capture_tail(m, logits)
        convs = []
        for every in (8, 1):
            calls = []

            def scripted(*a, _c=calls, **k):                          # the real frame (the cache is fed), a scripted result
                out = orig(*a, **k)
                _c.append(1)
                return torch.zeros_like(out) if len(_c) == 3 else out
            m.generate_frame = scripted
            torch.manual_seed(8)
            conv = gen.conversation(context=[_seg(1)])
            audio = conv.generate("one", 0, max_audio_length_ms=12 * 80, eos_check_every=every)
            m.generate_frame = orig
            T = len(Tok().encode("[0]one"))
            base = conv.tokens.shape[0] - 4
            assert audio.numel() == 3 * 1920 and len(calls) == (7 if every == 8 else 3)
            assert not conv.tokens[-1].any() and bool(conv.tokens[-2].any()) and conv.mask[base - 1, -1]      # exactly one zero frame
            # the cache is cut back to the EOS frame's position: the frame itself re-enters with the next turn, whenever it was seen
            assert conv.cached == _pos(conv) == conv.tokens.shape[0] - 1
            assert T > 0
            torch.manual_seed(9)
            conv.generate("two", 1, max_audio_length_ms=MS)
            convs.append(conv)
        assert torch.equal(convs[0].tokens, convs[1].tokens)
        assert len(logits) == 4 and torch.equal(logits[1], logits[3])          # the next turn's first-frame logits
    finally:
        m.generate_frame = orig
        del m.engine._frame_tail
        if "generate_frame" in m.__dict__:
            del m.generate_frame


def test_drop_oldest_equals_fresh_prefill(dev, gen):
    from csm.engine import DecodeState
    m = gen._model
    conv = gen.conversation(context=[_seg(1, frames=20), _seg(2, frames=20, speaker=1)], on_overflow="drop_oldest")
    strict = gen.conversation(context=[_seg(1, frames=20), _seg(2, frames=20, speaker=1)])
    torch.manual_seed(10)
    conv.generate("one", 0, max_audio_length_ms=MS)
    first = len(Tok().encode("[0]hi")) + 21
    before = conv.tokens.clone()
    big = (128 - before.shape[0]) * 80                               # history + text + frames >= max_seq_len
    strict.generate("one", 0, max_audio_length_ms=MS)
    with pytest.raises(ValueError, match="Inputs too long, must be below max_seq_len - max_audio_frames"):
        strict.generate("two", 0, max_audio_length_ms=big)
    logits = []
    try:
        _capture_tail(m, logits)
        conv.generate("two", 0, max_audio_length_ms=big, eos_check_every=1)
    finally:
        del m.engine._frame_tail
    T = len(Tok().encode("[0]two"))
    kept = before[first:]
    assert torch.equal(conv.tokens[:kept.shape[0] + T], torch.cat([kept, gen._tokenize_text_segment("two", 0)[0]], 0))
    n = kept.shape[0] + T
    fresh = DecodeState(m.engine, 1)
    ref = _c0_logits(m, fresh.prefill(conv.tokens[:n].unsqueeze(0), conv.mask[:n].unsqueeze(0)))
    assert torch.equal(logits[0], ref)


def test_cli_next_text_same_bytes(dev, tmp_path, monkeypatch, capsys):
    from csm.cli import generate as cli_gen
    from csm.codec import MimiCodec
    from csm.generator import Generator

    def make():
        return Generator(_tiny(2), text_tokenizer=Tok(), audio_tokenizer=MimiCodec(_hf_model(5).state_dict(), device="cuda"))

    monkeypatch.setattr(cli_gen, "load_csm_1b", lambda ckpt, device, mimi_weights=None, tokenizer_path=None: make())
    base = ["--model-path", "ckpt.pt", "--text", "hello", "--speaker", "1", "--max-audio-length-ms", "480",
            "--mimi-weights", "m.safetensors", "--text-tokenizer", "tokdir"]
    nxt = ["--next-text", "and then", "--next-speaker", "0", "--next-text", "bye", "--next-speaker", "1"]
    torch.manual_seed(77)                                            # (the codec's construction reseeds: same order as the CLI's)
    g = make()
    conv = g.conversation()
    turns = [conv.generate(t, s, max_audio_length_ms=480, temperature=0.9, topk=50) for t, s in (("hello", 1), ("and then", 0), ("bye", 1))]
    want = tmp_path / "want.wav"
    g.save_wav(str(want), torch.cat(turns))
    for mode, extra in (("plain", []), ("stream", ["--stream", "--chunk-frames", "2"])):
        torch.manual_seed(77)
        path = tmp_path / mode / "out.wav"
        assert cli_gen.main(base + nxt + ["--output", str(path)] + extra) == 0
        assert path.read_bytes() == want.read_bytes(), mode
    with wave.open(str(want), "rb") as w:
        assert w.getnframes() == 3 * 6 * 1920
    # without the new flags: today's one-shot path
    torch.manual_seed(77)
    assert cli_gen.main(base + ["--output", str(tmp_path / "one.wav")]) == 0
    torch.manual_seed(77)
    g = make()
    g.save_wav(str(tmp_path / "one_ref.wav"), g.generate("hello", 1, [], max_audio_length_ms=480))
    assert (tmp_path / "one.wav").read_bytes() == (tmp_path / "one_ref.wav").read_bytes()
    assert "turn 3" in capsys.readouterr().out
