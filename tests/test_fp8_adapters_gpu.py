"""Per-utterance LoRA adapters on the FP8 base (Model.fp8_adapters with decode_weights = "fp8": csm_gemv_fp8w_kext_rows under
``_DecodeStack._product``) at the engine and the public surface: the opt-in and what stays refused, graph replay against eager,
rows without adapter against the adapter-free FP8 batch, rows with adapters against their batch-mates, FP8 + adapters against
bf16 + adapters on grid-snapped weights (the criteria of test_fp8_decode_gpu.py, unchanged), and a served request against its
slot and neighbours.  Quantisation loss is not asserted anywhere: see test_fp8_decode_gpu.py."""
import pytest
import torch

from oracle import csm_oracle as O
from test_fp8_decode_gpu import TINY, _noise, _prompts, _snap_model, _tiny, gclose
from test_lora_bank_gpu import adapter

pytestmark = pytest.mark.gpu


def _decode(m, toks, msks, frames, use_graph, adapters=None, rows=None):
    """``frames`` frames of a ragged batch with the shared noise rows ``rows`` (test_fp8_decode_gpu._decode + adapters)."""
    dev = m.device
    K, V = m.args.audio_num_codebooks, m.args.audio_vocab_size
    B = len(toks)
    m.setup_caches(B)
    m.reset_caches()
    m.use_hip_graph = use_graph
    try:
        f = m.engine.generate_first_frames(toks, msks, 0.8, 12, noise=_noise(B, K, V, 0, rows), adapters=adapters)
        out = [f.cpu()]
        mask = torch.cat([torch.ones(B, K, dtype=torch.bool), torch.zeros(B, 1, dtype=torch.bool)], 1).unsqueeze(1).to(dev)
        pad = torch.zeros(B, 1, dtype=torch.long, device=dev)
        pos = torch.ones(B, 1, dtype=torch.long, device=dev)
        for step in range(1, frames):
            f = m.generate_frame(torch.cat([f.long(), pad], 1).unsqueeze(1), mask, pos, 0.8, 12, noise=_noise(B, K, V, step, rows))
            out.append(f.cpu())
    finally:
        m.use_hip_graph = True
    return torch.stack(out)


def test_flag_state_and_what_stays_refused(dev):
    from csm.hip import lib
    from csm.training.lora import apply_lora_to_model
    m = _tiny(dev)
    assert m.fp8_adapters is False
    toks, msks = _prompts(TINY, 2, seed=2)
    st = adapter(m, 4, modules=["q_proj", "v_proj", "w2"])
    m.decode_weights = "fp8"
    with pytest.raises(ValueError, match="merge the adapters first") as e:
        m.engine.generate_first_frames(toks, msks, 0.8, 12, adapters=[st, None])
    assert 'decode_weights = "bf16"' in str(e.value) and "fp8_adapters" in str(e.value)
    m.engine.generate_first_frames(toks, msks, 0.8, 12)
    assert m._decode_state is not None
    m.fp8_adapters = True
    assert m.fp8_adapters is True and m._decode_state is None, "changing the flag drops the decode state"
    m.use_hip_graph = False
    try:
        f = m.engine.generate_first_frames(toks, msks, 0.8, 12, adapters=[st, None])
    finally:
        m.use_hip_graph = True
    assert f.shape == (2, TINY.n_codebooks)
    assert lib.csm_gemv_last_kernel().decode() != ""
    for stack in (m._decode_state.bb, m._decode_state.dc):
        assert stack.w8 is not None and stack.lora_rows is not None
    assert m._decode_state.decode_weights == "fp8"
    m.fp8_adapters = True                                      # the same value: nothing is dropped
    assert m._decode_state is not None
    # live model.lora stays refused with the flag on, and the message points to the bank
    apply_lora_to_model(m, r=8, alpha=16.0, target_modules=["q_proj", "v_proj", "w2"], seed=3)
    with pytest.raises(ValueError, match="bank") as e:
        m.engine.generate_first_frames(toks, msks, 0.8, 12)
    assert "merge the adapters first" in str(e.value) and 'decode_weights = "bf16"' in str(e.value)
    m.fp8_adapters = False
    with pytest.raises(ValueError, match="merge the adapters first"):
        m.engine.generate_first_frames(toks, msks, 0.8, 12)


def test_extended_fp8_products_run_under_the_engine(dev):
    """The adapted products of a mixed batch really go through ops.gemv_fp8w_kext_rows: every product of every layer of both
    stacks at least once in a frame (the adapter below extends all seven projections)."""
    from csm import engine as E
    m = _tiny(dev)
    m.decode_weights, m.fp8_adapters = "fp8", True
    st = adapter(m, 1)
    seen = []
    orig = E.ops.gemv_fp8w_kext_rows
    E.ops.gemv_fp8w_kext_rows = lambda *a, **k: (seen.append(a[1].shape), orig(*a, **k))[1]
    try:
        toks, msks = _prompts(TINY, 2, seed=2)
        m.use_hip_graph = False
        m.engine.generate_first_frames(toks, msks, 0.8, 12, adapters=[st, None])
    finally:
        E.ops.gemv_fp8w_kext_rows = orig
        m.use_hip_graph = True
    assert len(seen) >= 4 * (m.bb.num_layers + m.dc.num_layers), len(seen)      # every product of a layer, both stacks


@pytest.mark.parametrize("B", [4, 16])
def test_graph_rows_without_adapter_and_batch_mates(dev, B):
    m = _tiny(dev)
    a, b = adapter(m, 1), adapter(m, 2, use_bias=True)
    m.decode_weights, m.fp8_adapters = "fp8", True
    toks, msks = _prompts(TINY, B, seed=21)
    rows = list(range(B))
    ads = [[a, None, b, a][r % 4] for r in rows]
    eager = _decode(m, toks, msks, 5, False, ads, rows)
    graph = _decode(m, toks, msks, 5, True, ads, rows)
    assert m._decode_state.bb.w8 is not None and m._decode_state.bb.lora_rows is not None
    assert torch.equal(eager, graph), "captured-graph replay must reproduce the eager frames bit for bit"
    plain = _decode(m, toks, msks, 5, True, None, rows)
    assert m._decode_state.bb.lora_rows is None and m._decode_state.bb.w8 is not None
    for r in rows:
        if ads[r] is None:
            assert torch.equal(graph[:, r], plain[:, r]), f"row {r} has no adapter: the adapter-free FP8 batch's frames"
        else:
            assert not torch.equal(graph[:, r], plain[:, r]), f"row {r}: its adapter changes nothing"
    # other adapters on the batch-mates: rows 0 (adapter a) and 1 (none) keep their frames
    other = [ads[r] if r < 2 else [b, a, None, b][r % 4] for r in rows]
    got = _decode(m, toks, msks, 5, True, other, rows)
    assert torch.equal(got[:, :2], graph[:, :2]), "a row's frames depend on its batch-mates' adapters"
    assert not torch.equal(got[:, 2:], graph[:, 2:])
    if B == 16:                                                # five of the rows alone, in another order: the same frames
        sub = [11, 3, 7, 0, 14]
        alone = _decode(m, [toks[r] for r in sub], [msks[r] for r in sub], 5, True, [ads[r] for r in sub], sub)
        assert torch.equal(alone, graph[:, sub])
    else:                                                      # two of the four rows decoded on their own
        # (not one: at one utterance the depth decoder's output projection keeps its bf16 weight, other numbers)
        alone = _decode(m, toks[2:4], msks[2:4], 5, True, ads[2:4], [2, 3])
        assert torch.equal(alone, graph[:, 2:4])


def _teacher_forced(m, cfg, B, mode, ads, history, capture):
    """test_fp8_decode_gpu._teacher_forced with per-row adapters."""
    K = cfg.n_codebooks
    tokens, mask, _ = O.synthetic_batch(cfg, B, 20, seed=12)

    def noise(step):
        g = torch.Generator().manual_seed(500 + step)
        return [torch.empty(16, cfg.audio_vocab).exponential_(1, generator=g)[:B] for _ in range(K)]

    m.decode_weights = mode
    m.setup_caches(B)
    m.reset_caches()
    eng = m.engine
    orig = eng._frame_tail_body
    eng._frame_tail_body = lambda st, last_h, t, k: (capture.append(last_h.clone()), orig(st, last_h, t, k))[1]
    m.use_hip_graph = False
    try:
        cur_t, cur_m, cur_p = tokens[:, :11], mask[:, :11], torch.arange(11).unsqueeze(0).repeat(B, 1)
        frames = []
        for step in range(8):
            f = m.generate_frame(cur_t, cur_m, cur_p, 0.8, 12, noise=noise(step), adapters=ads).cpu()
            frames.append(f)
            nxt = history[step] if history is not None else f
            cur_t = torch.cat([nxt.long(), torch.zeros(B, 1, dtype=torch.long)], dim=1).unsqueeze(1)
            cur_m = torch.cat([torch.ones(B, K, dtype=torch.bool), torch.zeros(B, 1, dtype=torch.bool)], dim=1).unsqueeze(1)
            cur_p = cur_p[:, -1:] + 1
    finally:
        m.use_hip_graph = True
        del eng._frame_tail_body
    return torch.stack(frames)


def _check_snapped(m, cfg, B, dev):
    """FP8 + adapters vs bf16 + adapters on weights both modes hold exactly, teacher-forced on the bf16 history: the criteria of
    test_fp8_decode_gpu._check_fp8_vs_bf16_on_snapped (>= 0.9 of the codes, codebook-0 logits within 1.5e-2)."""
    from csm.hip import ops
    _snap_model(m)
    a, b = adapter(m, 1), adapter(m, 2)
    ads = [[a, b, None][r % 3] for r in range(B)]
    m.fp8_adapters = True
    try:
        h_bf, h_f8 = [], []
        bf = _teacher_forced(m, cfg, B, "bf16", ads, None, h_bf)
        assert m._decode_state.bb.w8 is None and m._decode_state.bb.lora_rows is not None
        f8 = _teacher_forced(m, cfg, B, "fp8", ads, bf, h_f8)
        assert m._decode_state.bb.w8 is not None and m._decode_state.bb.lora_rows is not None
    finally:
        m.decode_weights = "bf16"
    agree = (bf == f8).float().mean().item()
    agree1 = (bf[1] == f8[1]).float().mean().item()
    print(f"B={B}: FP8 + adapters vs bf16 + adapters: codes agree {agree:.1%} over 8 frames, {agree1:.1%} on the first decode frame")
    assert agree >= 0.9, f"FP8 + adapters and bf16 + adapters on identical numbers agree on only {agree:.1%} of the sampled codes"
    lg = [torch.empty(B, m.vocab_pad, dtype=torch.float32, device=dev) for _ in range(2)]
    ops.gemv(h_bf[1], m.block("codebook0_head.padded"), lg[0])
    ops.gemv(h_f8[1], m.block("codebook0_head.padded"), lg[1])
    V = cfg.audio_vocab
    gclose(f"B={B} first decode frame codebook-0 logits, FP8 + adapters vs bf16 + adapters", lg[1][:, :V], lg[0][:, :V], 1.5e-2)


@pytest.mark.parametrize("B", [1, 4, 16])
def test_fp8_adapters_vs_bf16_adapters_on_grid_snapped_weights_tiny(dev, B):
    _check_snapped(_tiny(dev), TINY, B, dev)


def test_fp8_adapters_vs_bf16_adapters_on_grid_snapped_weights_csm1b_width(dev):
    from csm.models.model import Model, ModelArgs
    m = Model(ModelArgs("llama-1B-L1", "llama-100M-L1", 300, 2051, 32), device=dev, seed=0)
    cfg = O.CsmCfg(backbone=TINY.backbone, decoder=TINY.decoder, text_vocab=300, audio_vocab=2051, n_codebooks=32)
    _check_snapped(m, cfg, 16, dev)


def test_served_request_does_not_depend_on_slot_or_neighbours(dev):
    """A 4-slot serve() in FP8 mode with a two-adapter bank: a seeded request with an adapter, alone in slot 0 and later among
    three others with other adapters in another slot."""
    from csm.codec import MimiCodec
    from csm.generator import Generator, Segment
    from csm.models.model import Model, ModelArgs
    from test_serving_gpu import TEMP, TOPK, Tok, _adapter, _hf_mimi
    codec = MimiCodec(_hf_mimi().state_dict(), device="cuda")
    m = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", 300, 2051, 32), device="cuda", seed=2)
    gen = Generator(m, text_tokenizer=Tok(), audio_tokenizer=codec)
    for name, seed in (("a1", 1), ("a2", 2)):
        gen.add_adapter(name, _adapter(m, seed))
    ctx = [Segment(0, "hi", torch.randn(24000, generator=torch.Generator().manual_seed(1)) * 0.2)]
    m.decode_weights = "fp8"
    with pytest.raises(ValueError, match="merge the adapters first"):
        gen.serve(slots=4)
    m.fp8_adapters = True

    def probe(srv, ad):
        return srv.submit("the line we follow", 1, ctx, adapter=ad, seed=1234, max_audio_length_ms=10 * 80)

    codes = {}
    for ad in ("a1", None):
        srv = gen.serve(slots=4, chunk_frames=4, temperature=TEMP, topk=TOPK)
        r = probe(srv, ad)
        for _ in srv.run():
            pass
        assert r.done and r.codes().shape[1] == 10
        codes[ad] = r.codes()
    assert not torch.equal(codes["a1"], codes[None]), "the adapter changes what is said"
    srv = gen.serve(slots=4, chunk_frames=4, temperature=TEMP, topk=TOPK)
    others = [srv.submit("n" * (3 + 2 * i), i % 3, ctx if i == 1 else [], adapter=["a2", None, "a1"][i], seed=i + 1,
                         max_audio_length_ms=(12 + 3 * i) * 80) for i in range(3)]
    srv.step()
    rs = {ad: probe(srv, ad) for ad in ("a1",)}
    more = [srv.submit("later", 2, [], adapter="a2", seed=77, max_audio_length_ms=5 * 80)]
    srv.step()
    assert rs["a1"].slot not in (None, 0) and len(srv.active) == 4
    for _ in srv.run():
        pass
    assert all(o.done for o in others + more) and rs["a1"].done
    assert torch.equal(rs["a1"].codes(), codes["a1"]), "codes differ between slot 0 alone and another slot among neighbours with other adapters"
    m.reset_caches()
