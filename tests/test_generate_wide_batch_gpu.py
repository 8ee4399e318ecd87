"""Decoding 5 to 16 utterances at once: the MFMA decode products (gemv_mfma_kernel, csm_gemv_bf16 / _ex at B = 5..16) and
everything above them (DecodeState, the captured frame graph, Generator.generate_batch).

Numerics contract pinned here:
  * each product against the fp32 product of the same bf16 operands (x^ rounded to bf16 as the RMSNorm prologue rounds it);
  * batch invariance, bit for bit: a row's output depends on that row's inputs only - any B in 5..16, any position of the row,
    any contents of the other rows - for every fusion, split-K shapes included;
  * at frame level: eager == graph replay, a subset of the rows decoded on its own reproduces their frames, and the KV-cache
    path agrees with the cache-free recompute path as closely as it does at B <= 4.
"""
import gc
import math

import pytest
import torch

from oracle import csm_oracle as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TINY = O.tiny_cfg()


def gclose(name, got, ref, tol):
    got, ref = got.float().cpu(), ref.float().cpu()
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-12
    assert math.isfinite(err) and err <= tol * scale, f"{name}: max abs err {err:.4g} vs scale {scale:.4g} (tol {tol})"


def xhat(x, w, eps=1e-5):
    """x RMS-normalised and scaled as the decode prologues compute it, rounded to bf16 (fp32 rstd of the bf16 row)."""
    xf = x.float()
    rs = torch.rsqrt((xf * xf).mean(-1, keepdim=True) + eps)
    return (xf * rs * w.float()).to(BF).float()


def forms(ops, dev, W, w, table, N):
    """The six forms of the decode products, each as f(x, R, idx, B) -> output."""
    def plain(x, R, idx, B):
        y = torch.empty(B, N, dtype=BF, device=dev); ops.gemv(x, W, y); return y

    def resid(x, R, idx, B):
        y = torch.empty(B, N, dtype=BF, device=dev); ops.gemv(x, W, y, residual=R); return y

    def norm(x, R, idx, B):
        y = torch.empty(B, N, dtype=BF, device=dev); ops.gemv_ex(x, W, y, residual=R, norm_scale=w, eps=1e-5); return y

    def swiglu(x, R, idx, B):
        y = torch.empty(B, N // 2, dtype=BF, device=dev); ops.gemv_ex(x, W, y, norm_scale=w, eps=1e-5, swiglu=True); return y

    def f32(x, R, idx, B):
        y = torch.empty(B, N, dtype=torch.float32, device=dev); ops.gemv_ex(x, W, y, norm_scale=w, eps=1e-5); return y

    def gather(x, R, idx, B):
        y = torch.empty(B, N, dtype=BF, device=dev); ops.gemv_ex(table, W, y, row_index=idx, row_offset=7); return y

    return {"plain": plain, "residual": resid, "norm": norm, "norm+swiglu": swiglu, "f32": f32, "gather": gather}


def references(W, w, table, x, R, idx):
    Wf = W.float()
    xn = xhat(x, w)
    gu = (xn @ Wf.t()).to(BF).float()
    return {"plain": x.float() @ Wf.t(), "residual": x.float() @ Wf.t() + R.float(), "norm": xn @ Wf.t() + R.float(),
            "norm+swiglu": torch.nn.functional.silu(gu[:, 0::2]) * gu[:, 1::2], "f32": xn @ Wf.t(),
            "gather": table[idx.long() + 7].float() @ Wf.t()}


# CSM-1B's decode products (N, K, forms the model uses) and tiny shapes: K = 256 / 512, K % 64 == 32, N not a multiple of 16
SHAPES = [
    (3072, 2048, ["norm"]), (2048, 2048, ["residual"]), (16384, 2048, ["norm+swiglu"]), (2048, 8192, ["residual"]),
    (2112, 2048, ["f32", "plain"]), (1024, 2048, ["plain", "gather"]),
    (1536, 1024, ["norm"]), (1024, 1024, ["residual"]), (16384, 1024, ["norm+swiglu"]), (1024, 8192, ["residual"]),
    (2112, 1024, ["f32"]),
    (1024, 256, "all"), (300, 512, "all"), (66, 96, "all"),
]


@pytest.mark.parametrize("N,K,which", SHAPES, ids=[f"{n}x{k}" for n, k, _ in SHAPES])
def test_wide_batch_products_vs_fp32(dev, N, K, which):
    from csm.hip import ops
    g = torch.Generator().manual_seed(N * 7 + K)
    W = (torch.randn(N, K, generator=g) * 0.02).to(BF).to(dev)
    w = (1 + 0.1 * torch.randn(K, generator=g)).to(BF).to(dev)
    table = torch.randn(64, K, generator=g).to(BF).to(dev)
    fs = forms(ops, dev, W, w, table, N)
    names = list(fs) if which == "all" else which
    for B in (5, 8, 13, 16):
        x = torch.randn(B, K, generator=g).to(BF).to(dev)
        R = torch.randn(B, N, generator=g).to(BF).to(dev)
        idx = torch.randint(0, 50, (B,), generator=g).to(torch.int32).to(dev)
        refs = references(W, w, table, x, R, idx)
        for name in names:
            gclose(f"{N}x{K} B={B} {name}", fs[name](x, R, idx, B), refs[name], 1.5e-2)


@pytest.mark.parametrize("N,K", [(1536, 1024), (2048, 8192), (1024, 256), (300, 96)])
def test_wide_batch_products_are_batch_invariant(dev, N, K):
    """Rows of a B = 16 launch, the same rows in another order in a B = 5 launch, and the same rows at other positions of a
    B = 16 launch whose other rows hold different data: the same bits, every form."""
    from csm.hip import ops
    g = torch.Generator().manual_seed(N + K)
    W = (torch.randn(N, K, generator=g) * 0.02).to(BF).to(dev)
    w = (1 + 0.1 * torch.randn(K, generator=g)).to(BF).to(dev)
    table = torch.randn(64, K, generator=g).to(BF).to(dev)
    fs = forms(ops, dev, W, w, table, N)
    x = torch.randn(16, K, generator=g).to(BF).to(dev)
    R = torch.randn(16, N, generator=g).to(BF).to(dev)
    idx = torch.randint(0, 50, (16,), generator=g).to(torch.int32).to(dev)
    perm = torch.tensor([9, 2, 15, 0, 7])
    at = torch.tensor([4, 13, 1, 8, 11])                       # where the five rows sit in the third launch
    x3 = torch.randn(16, K, generator=g).to(BF).to(dev)
    R3 = torch.randn(16, N, generator=g).to(BF).to(dev)
    idx3 = torch.randint(0, 50, (16,), generator=g).to(torch.int32).to(dev)
    x3[at], R3[at], idx3[at] = x[perm], R[perm], idx[perm]
    for name, f in fs.items():
        y16 = f(x, R, idx, 16)
        y5 = f(x[perm].contiguous(), R[perm].contiguous(), idx[perm].contiguous(), 5)
        y3 = f(x3, R3, idx3, 16)
        assert torch.equal(y5, y16[perm]), f"{N}x{K} {name}: B = 5 subset vs B = 16"
        assert torch.equal(y3[at], y16[perm]), f"{N}x{K} {name}: other positions, other batch-mates"
        for B in (6, 12):                                      # every width of the range: the first B rows
            assert torch.equal(f(x[:B].contiguous(), R[:B].contiguous(), idx[:B].contiguous(), B), y16[:B]), f"{N}x{K} {name} B={B}"


def test_wide_batch_abi_limits(dev):
    """B = 17 is refused; the K-extension (live LoRA) kernels stay at B <= 4; B <= 4 keeps its kernels."""
    from csm.hip import ops
    g = torch.Generator().manual_seed(3)
    W = (torch.randn(64, 256, generator=g) * 0.02).to(BF).to(dev)
    with pytest.raises(Exception, match="B=17"):
        ops.gemv(torch.randn(17, 256, generator=g).to(BF).to(dev), W, torch.empty(17, 64, dtype=BF, device=dev))
    with pytest.raises(Exception, match="K % 32"):
        ops.gemv(torch.randn(5, 264, generator=g).to(BF).to(dev), (torch.randn(64, 264, generator=g)).to(BF).to(dev),
                 torch.empty(5, 64, dtype=BF, device=dev))
    t = torch.zeros(5, 16, dtype=BF, device=dev)
    Bx = torch.zeros(64, 16, dtype=BF, device=dev)
    with pytest.raises(Exception, match="at most 4"):
        ops.gemv_kext(torch.randn(5, 256, generator=g).to(BF).to(dev), W, torch.empty(5, 64, dtype=BF, device=dev), t, Bx)


# ------------------------------------------------------------------------------------------------------------ engine level
def _prompts(cfg, B, seed, lo=8, hi=20):
    tokens, mask, _ = O.synthetic_batch(cfg, B, hi, seed=seed)
    lens = [lo + (b * 5) % (hi - lo + 1) for b in range(B)]
    return [tokens[b, :lens[b]] for b in range(B)], [mask[b, :lens[b]] for b in range(B)]


def _noise(B, K, V, step, rows=None):
    g = torch.Generator().manual_seed(900 + step)
    q = [torch.empty(16, V).exponential_(1, generator=g) for _ in range(K)]
    return [qi[:B] if rows is None else qi[rows] for qi in q]


def _decode(m, toks, msks, frames, use_graph, rows=None):
    """generate_first_frames + (frames - 1) decode frames; the noise of row b is that of row rows[b] of a 16-row draw."""
    dev = m.device
    K, V = m.args.audio_num_codebooks, m.args.audio_vocab_size
    B = len(toks)
    if not m.caches_are_enabled():
        m.setup_caches(16)
    m.use_hip_graph = use_graph
    try:
        f = m.engine.generate_first_frames(toks, msks, 0.8, 12, noise=_noise(B, K, V, 0, rows))
        out = [f.cpu()]
        mask = torch.cat([torch.ones(B, K, dtype=torch.bool), torch.zeros(B, 1, dtype=torch.bool)], 1).unsqueeze(1).to(dev)
        pad = torch.zeros(B, 1, dtype=torch.long, device=dev)
        pos = torch.ones(B, 1, dtype=torch.long, device=dev)
        for step in range(1, frames):
            f = m.generate_frame(torch.cat([f.long(), pad], 1).unsqueeze(1), mask, pos, 0.8, 12, noise=_noise(B, K, V, step, rows))
            out.append(f.cpu())
    finally:
        m.use_hip_graph = True
    return torch.stack(out)                                                          # [frames, B, K]


def _tiny(dev, seed=11):
    from csm.models.model import Model, ModelArgs
    m = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", TINY.text_vocab, TINY.audio_vocab, TINY.n_codebooks), device="cuda")
    m.load_state_dict(O.init_params(TINY, seed=seed))
    return m


def test_engine_sixteen_ragged_rows_tiny(dev):
    m = _tiny(dev)
    toks, msks = _prompts(TINY, 16, seed=21)
    eager = _decode(m, toks, msks, 6, False)
    graph = _decode(m, toks, msks, 6, True)
    assert eager.shape == (6, 16, TINY.n_codebooks)
    assert torch.equal(eager, graph), "captured-graph replay at B = 16 must reproduce the eager frames bit for bit"
    assert m._decode_state.B == 16 and m._decode_state.noise_buf.shape[1] == 16 and m._decode_state.bb.pos.numel() == 16
    assert all(p.numel() == 16 for p in m._decode_state.dpos)
    rows = [11, 3, 7, 0, 14]
    sub = _decode(m, [toks[r] for r in rows], [msks[r] for r in rows], 6, True, rows=rows)
    assert torch.equal(sub, graph[:, rows]), "five of the rows, decoded on their own in another order: the same frames"
    assert len({tuple(graph[:, b].reshape(-1).tolist()) for b in range(16)}) > 8, "the rows really differ"


def test_engine_sixteen_rows_kv_cache_vs_recompute(dev):
    """The pattern of test_generate_kv_cache_vs_recompute_and_graph at B = 16: same history (teacher-forced) and noise."""
    m = _tiny(dev)
    K, B = TINY.n_codebooks, 16
    tokens, mask, _ = O.synthetic_batch(TINY, B, 20, seed=12)

    def noise(step):
        g = torch.Generator().manual_seed(500 + step)
        return [torch.empty(B, TINY.audio_vocab).exponential_(1, generator=g) for _ in range(K)]

    def run(use_cache, history):
        m.use_kv_cache = use_cache
        m.setup_caches(B)
        m.reset_caches()
        cur_t, cur_m, cur_p = tokens[:, :11], mask[:, :11], torch.arange(11).unsqueeze(0).repeat(B, 1)
        frames = []
        for step in range(8):
            f = m.generate_frame(cur_t, cur_m, cur_p, 0.8, 12, noise=noise(step)).cpu()
            frames.append(f)
            nxt = history[step] if history is not None else f
            cur_t = torch.cat([nxt.long(), torch.zeros(B, 1, dtype=torch.long)], dim=1).unsqueeze(1)
            cur_m = torch.cat([torch.ones(B, K, dtype=torch.bool), torch.zeros(B, 1, dtype=torch.bool)], dim=1).unsqueeze(1)
            cur_p = cur_p[:, -1:] + 1
        return torch.stack(frames)

    try:
        kv = run(True, None)
        m.engine.capture_logits = []
        rc = run(False, kv)
        lg_rc = m.engine.capture_logits[0]                      # codebook 0 of the prefill frame, recompute path (GEMM)
    finally:
        m.use_kv_cache = True
        m.engine.capture_logits = None
    agree = (kv == rc).float().mean().item()
    assert agree >= 0.9, f"KV-cache and recompute paths agree on only {agree:.1%} of the sampled codes"
    agree0 = (kv[0] == rc[0]).float().mean().item()
    assert agree0 >= 0.9, f"the prefill frame: {agree0:.1%} of its codes agree"
    # the prefill frame's codebook-0 logits: the B = 16 decode product (MFMA kernel) vs the recompute path's GEMM
    from csm.hip import ops
    h = m.engine.hidden_states(tokens[:, :11], mask[:, :11])[:, -1].contiguous()
    lg = torch.empty(B, m.vocab_pad, dtype=torch.float32, device=dev)
    ops.gemv(h, m.block("codebook0_head.padded"), lg)
    gclose("prefill codebook-0 logits, decode product vs GEMM", lg[:, :TINY.audio_vocab], lg_rc, 1.5e-2)


def test_engine_sixteen_rows_at_csm1b_width(dev):
    """One-layer stacks of CSM-1B's width (every decode product's real N x K): 16 ragged prompts, 4 frames."""
    from csm.models.model import Model, ModelArgs
    m = Model(ModelArgs("llama-1B-L1", "llama-100M-L1", 300, 2051, 32), device=dev, seed=0)
    cfg = O.CsmCfg(backbone=TINY.backbone, decoder=TINY.decoder, text_vocab=300, audio_vocab=2051, n_codebooks=32)
    toks, msks = _prompts(cfg, 16, seed=5, lo=6, hi=30)
    eager = _decode(m, toks, msks, 4, False)
    graph = _decode(m, toks, msks, 4, True)
    assert torch.equal(eager, graph), "eager vs graph replay at CSM-1B width"
    rows = [15, 6, 1, 9, 4]
    sub = _decode(m, [toks[r] for r in rows], [msks[r] for r in rows], 4, True, rows=rows)
    assert torch.equal(sub, graph[:, rows]), "subset invariance at CSM-1B width"


def _hf_mimi(seed=0):
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


class _Tok:
    def encode(self, text):
        return [1] + [3 + (b % 200) for b in text.encode()] + [2]


def test_generate_batch_sixteen_utterances(dev):
    from csm.codec import MimiCodec
    from csm.generator import Generator, Segment
    from csm.models.model import Model, ModelArgs
    codec = MimiCodec(_hf_mimi(3).state_dict(), device="cuda", num_codebooks=32)
    m = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", 300, 2051, 32), device="cuda", seed=1)
    gen = Generator(m, text_tokenizer=_Tok(), audio_tokenizer=codec)
    seg = Segment(0, "hi", torch.randn(24000, generator=torch.Generator().manual_seed(1)) * 0.2)
    texts = [f"utterance {i}" + " la" * (i % 5) for i in range(16)]
    ctxs = [[seg] if i % 3 == 0 else [] for i in range(16)]
    frames = []
    first, frame = m.engine.generate_first_frames, m.generate_frame
    m.engine.generate_first_frames = lambda *a, **k: (lambda f: (frames.append(f.clone()), f)[1])(first(*a, **k))
    m.generate_frame = lambda *a, **k: (lambda f: (frames.append(f.clone()), f)[1])(frame(*a, **k))
    decoded = []
    codec_decode = codec.decode
    codec.decode = lambda c: (decoded.append(c.clone()), codec_decode(c))[1]
    try:
        outs = gen.generate_batch(texts, list(range(16)), ctxs, max_audio_length_ms=6 * 80, eos_check_every=4)
    finally:
        del m.engine.generate_first_frames, m.generate_frame
        codec.decode = codec_decode
    assert len(outs) == 16
    codes = torch.stack(frames, 2)                                                     # [16, K, T]
    assert codes.shape[0] == 16 and codes.shape[2] >= 6
    k = 0
    for b in range(16):
        hit = (codes[b] == 0).all(dim=0).nonzero()
        n = int(hit[0]) if hit.numel() else 6
        assert outs[b].dim() == 1 and outs[b].numel() == n * 1920 and bool(torch.isfinite(outs[b]).all()), b
        if n:
            assert torch.equal(decoded[k][0], codes[b, :, :n]), f"row {b}: decoded codes"
            k += 1
    with pytest.raises(ValueError, match="1..16"):
        gen.generate_batch(["x"] * 17, list(range(17)), [[] for _ in range(17)], max_audio_length_ms=160)
    # free the frame graph captured under generate_batch's inference mode now: while it lives, the CUDA generator's graph
    # state holds inference tensors that a later capture outside inference mode may not update
    m.reset_caches()
    del gen, m
    gc.collect()


def test_live_lora_refuses_more_than_four_rows(dev):
    from csm.training.lora import apply_lora_to_model
    m = _tiny(dev)
    apply_lora_to_model(m, r=8, alpha=16.0, target_modules=["q_proj", "v_proj", "w2"], seed=3)
    g = torch.Generator(device="cuda").manual_seed(99)
    with torch.no_grad():
        for ad in m.lora.adapters.values():
            ad.B[:, :8].copy_((torch.randn(ad.B.shape[0], 8, generator=g, device="cuda") * 0.05).to(BF))
    toks, msks = _prompts(TINY, 5, seed=2)
    with pytest.raises(ValueError, match="merge_lora_weights"):
        m.engine.generate_first_frames(toks, msks, 0.8, 12)
    f = m.engine.generate_first_frames(toks[:4], msks[:4], 0.8, 12)
    assert f.shape == (4, TINY.n_codebooks)
    # merged adapters take any batch size
    m.merge_lora_weights()
    f = m.engine.generate_first_frames(toks, msks, 0.8, 12)
    assert f.shape == (5, TINY.n_codebooks)
