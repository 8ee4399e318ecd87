"""Generation with live (un-merged) LoRA adapters: the K-extension decode kernels (csm_lora_project_bf16, csm_gemv_bf16_kext)
against fp32, the engine's decode path against its own recompute path and against merged weights, and the public API
(Generator, CSMLoRATrainer.generate_sample, csm-finetune-lora --generate-samples)."""
import wave

import pytest
import torch

from oracle import csm_oracle as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TINY = O.tiny_cfg()
ALL7 = ["q_proj", "k_proj", "v_proj", "output_proj", "w1", "w2", "w3"]


def tiny_model(dev, seed=11):
    from csm.models.model import Model, ModelArgs
    m = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", TINY.text_vocab, TINY.audio_vocab, TINY.n_codebooks), device="cuda")
    m.load_state_dict(O.init_params(TINY, seed=seed))
    return m


def lora_model(dev, modules=ALL7, seed=11, b_scale=0.05, **kw):
    """The tiny model with adapters whose B is non-zero (a fresh adapter has B = 0 and changes nothing)."""
    from csm.training.lora import apply_lora_to_model
    m = tiny_model(dev, seed)
    apply_lora_to_model(m, r=8, alpha=16.0, target_modules=list(modules), seed=3, **kw)
    g = torch.Generator(device="cuda").manual_seed(99)
    with torch.no_grad():
        for ad in m.lora.adapters.values():
            ad.B[:, :8].copy_((torch.randn(ad.B.shape[0], 8, generator=g, device="cuda") * b_scale).to(BF))
            if ad.bias is not None:
                ad.bias.copy_((torch.randn(ad.bias.shape[0], generator=g, device="cuda") * b_scale).to(BF))
    return m


def gclose(name, got, ref, tol):
    got, ref = got.float().cpu(), ref.float().cpu()
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-20
    assert err <= tol * scale, f"{name}: max abs err {err:.4g} vs max |ref| {scale:.4g}"


def noise(step, B=2):
    g = torch.Generator().manual_seed(500 + step)
    return [torch.empty(B, TINY.audio_vocab).exponential_(1, generator=g) for _ in range(TINY.n_codebooks)]


def frames(m, tokens, mask, B=2, n=8, graph=True, use_cache=True, history=None, prompt=11):
    """n frames from a prompt of ``prompt`` positions with pinned noise; ``history`` teacher-forces the fed-back frames."""
    K = TINY.n_codebooks
    m.use_hip_graph, m.use_kv_cache = graph, use_cache
    m.setup_caches(B)
    m.reset_caches()
    cur_t, cur_m, cur_p = tokens[:B, :prompt], mask[:B, :prompt], torch.arange(prompt).unsqueeze(0).repeat(B, 1)
    out = []
    try:
        for step in range(n):
            f = m.generate_frame(cur_t, cur_m, cur_p, 0.8, 12, noise=noise(step, B)).cpu()
            out.append(f)
            nxt = history[step] if history is not None else f
            cur_t = torch.cat([nxt.long(), torch.zeros(B, 1, dtype=torch.long)], dim=1).unsqueeze(1)
            cur_m = torch.cat([torch.ones(B, K, dtype=torch.bool), torch.zeros(B, 1, dtype=torch.bool)], dim=1).unsqueeze(1)
            cur_p = cur_p[:, -1:] + 1
    finally:
        m.use_hip_graph, m.use_kv_cache = True, True
    return torch.stack(out)


# ----------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("K", [256, 1024, 2048, 8192])
def test_kext_gemv_and_projection_vs_fp32(dev, K):
    from csm.hip import ops
    g = torch.Generator().manual_seed(K)
    N = 512
    for kx in (32, 64):
        W = (torch.randn(N, K, generator=g) * 0.02).to(BF)
        W13 = (torch.randn(2 * N, K, generator=g) * 0.02).to(BF)
        At = (torch.randn(K, kx, generator=g) / K ** 0.5).to(BF)
        Bx = (torch.randn(N, kx, generator=g) * 0.05).to(BF)
        Bx13 = (torch.randn(2 * N, kx, generator=g) * 0.05).to(BF)
        bias, bias13 = (torch.randn(N, generator=g) * 0.1).to(BF), (torch.randn(2 * N, generator=g) * 0.1).to(BF)
        w = (1 + 0.1 * torch.randn(K, generator=g)).to(BF)
        s = 2.0
        for B in (1, 2, 3, 4):
            x = torch.randn(B, K, generator=g).to(BF)
            R = torch.randn(B, N, generator=g).to(BF)
            xd, Wd, Atd, Bxd, wd = x.to(dev), W.to(dev), At.to(dev), Bx.to(dev), w.to(dev)
            # projection, plain and with the norm prologue
            t = torch.empty(B, kx, dtype=BF, device=dev)
            ops.lora_project(xd, Atd, t, s)
            gclose("lora_project", t, s * (x.float() @ At.float()), 1e-2)
            tn = torch.empty(B, kx, dtype=BF, device=dev)
            ops.lora_project(xd, Atd, tn, s, norm_scale=wd, eps=1e-5)
            xn = O.rmsnorm(x, w, 1e-5)
            gclose("lora_project norm", tn, s * (xn.float() @ At.float()), 1e-2)
            # plain + residual, with bias
            y = torch.empty(B, N, dtype=BF, device=dev)
            ops.gemv_kext(xd, Wd, y, t, Bxd, residual=R.to(dev), bias=bias.to(dev))
            ref = x.float() @ W.float().t() + t.float().cpu() @ Bx.float().t() + bias.float() + R.float()
            gclose("kext residual bias", y, ref, 1.5e-2)
            # norm prologue, fp32 out
            yf = torch.empty(B, N, dtype=torch.float32, device=dev)
            ops.gemv_kext(xd, Wd, yf, tn, Bxd, norm_scale=wd, eps=1e-5)
            gclose("kext norm f32", yf, xn.float() @ W.float().t() + tn.float().cpu() @ Bx.float().t(), 1e-2)
            # norm prologue + SwiGLU (gate / up interleaved), with bias
            act = torch.empty(B, N, dtype=BF, device=dev)
            ops.gemv_kext(xd, W13.to(dev), act, tn, Bx13.to(dev), norm_scale=wd, eps=1e-5, swiglu=True, bias=bias13.to(dev))
            gu = (xn.float() @ W13.float().t() + tn.float().cpu() @ Bx13.float().t() + bias13.float()).to(BF).float()
            gclose("kext swiglu", act, torch.nn.functional.silu(gu[:, 0::2]) * gu[:, 1::2], 2e-2)
            # Bx = 0: bit-identical to the plain product
            z = torch.zeros(N, kx, dtype=BF, device=dev)
            for kw in ({"residual": R.to(dev)}, {"norm_scale": wd, "eps": 1e-5}):
                a = torch.empty(B, N, dtype=BF, device=dev)
                b = torch.empty(B, N, dtype=BF, device=dev)
                ops.gemv_ex(xd, Wd, a, **kw)
                ops.gemv_kext(xd, Wd, b, tn, z, **kw)
                assert torch.equal(a, b), ("Bx = 0 must leave the plain product's bits", B, K, kx, list(kw))
            a = torch.empty(B, N, dtype=BF, device=dev)
            b = torch.empty(B, N, dtype=BF, device=dev)
            ops.gemv_ex(xd, W13.to(dev), a, norm_scale=wd, eps=1e-5, swiglu=True)
            ops.gemv_kext(xd, W13.to(dev), b, tn, torch.zeros(2 * N, kx, dtype=BF, device=dev), norm_scale=wd, eps=1e-5, swiglu=True)
            assert torch.equal(a, b), ("Bx = 0, SwiGLU", B, K, kx)
            # row b of a B-row launch == the one-row launch on that row (projection and extended products)
            for r in range(B):
                t1 = torch.empty(1, kx, dtype=BF, device=dev)
                ops.lora_project(xd[r:r + 1], Atd, t1, s, norm_scale=wd, eps=1e-5)
                assert torch.equal(t1[0], tn[r]), ("projection row", B, r)
                y1 = torch.empty(1, N, dtype=BF, device=dev)
                ops.gemv_kext(xd[r:r + 1], Wd, y1, t[r:r + 1], Bxd, residual=R[r:r + 1].to(dev), bias=bias.to(dev))
                assert torch.equal(y1[0], y[r]), ("kext row", B, K, kx, r)
                a1 = torch.empty(1, N, dtype=BF, device=dev)
                ops.gemv_kext(xd[r:r + 1], W13.to(dev), a1, tn[r:r + 1], Bx13.to(dev), norm_scale=wd, eps=1e-5, swiglu=True,
                              bias=bias13.to(dev))
                assert torch.equal(a1[0], act[r]), ("kext swiglu row", B, K, kx, r)


def test_kext_at_csm1b_shapes(dev):
    """Config-3 adapters at CSM-1B's products: q|k|v (K = 2048, N = 3072, norm) and w2 (K = 8192, residual)."""
    from csm.hip import ops
    g = torch.Generator().manual_seed(3)
    for B in (1, 2):
        x = torch.randn(B, 2048, generator=g).to(BF)
        w = (1 + 0.1 * torch.randn(2048, generator=g)).to(BF)
        W = (torch.randn(3072, 2048, generator=g) * 0.02).to(BF)
        At = (torch.randn(2048, 32, generator=g) / 2048 ** 0.5).to(BF)
        Bx = (torch.randn(3072, 32, generator=g) * 0.05).to(BF)
        t = torch.empty(B, 32, dtype=BF, device=dev)
        ops.lora_project(x.to(dev), At.to(dev), t, 2.0, norm_scale=w.to(dev), eps=1e-5)
        xn = O.rmsnorm(x, w, 1e-5)
        y = torch.empty(B, 3072, dtype=BF, device=dev)
        ops.gemv_kext(x.to(dev), W.to(dev), y, t, Bx.to(dev), norm_scale=w.to(dev), eps=1e-5)
        gclose("qkv kext", y, xn.float() @ W.float().t() + 2.0 * (xn.float() @ At.float()) @ Bx.float().t(), 1.5e-2)
        a = (torch.randn(B, 8192, generator=g) * 0.5).to(BF)
        W2 = (torch.randn(2048, 8192, generator=g) * 0.02).to(BF)
        At2 = (torch.randn(8192, 32, generator=g) / 8192 ** 0.5).to(BF)
        Bx2 = (torch.randn(2048, 32, generator=g) * 0.05).to(BF)
        R = torch.randn(B, 2048, generator=g).to(BF)
        t2 = torch.empty(B, 32, dtype=BF, device=dev)
        ops.lora_project(a.to(dev), At2.to(dev), t2, 2.0)
        y2 = torch.empty(B, 2048, dtype=BF, device=dev)
        ops.gemv_kext(a.to(dev), W2.to(dev), y2, t2, Bx2.to(dev), residual=R.to(dev))
        gclose("w2 kext", y2, a.float() @ W2.float().t() + 2.0 * (a.float() @ At2.float()) @ Bx2.float().t() + R.float(), 1e-2)


# ----------------------------------------------------------------------------------------------------------- engine
def test_live_adapters_graph_eager_and_recompute(dev):
    """All seven target modules, non-zero B: eager == graph replay bit for bit; against the cache-free recompute path (training
    forward with the adapters) the prefill frame is identical and almost every code agrees."""
    m = lora_model(dev)
    tokens, mask, _ = O.synthetic_batch(TINY, 2, 20, seed=12)
    eager = frames(m, tokens, mask, graph=False)
    graph = frames(m, tokens, mask, graph=True)
    assert m._decode_state.graph is not None
    assert torch.equal(eager, graph), "graph replay must reproduce the eager frames with live adapters"
    rc = frames(m, tokens, mask, use_cache=False, history=eager)
    assert torch.equal(eager[0], rc[0]), "the prefill frame goes through the same kernels in both paths"
    agree = (eager == rc).float().mean().item()
    assert agree >= 0.9, f"KV-cache and recompute paths agree on only {agree:.1%} of the codes"
    # the adapters change the output (otherwise nothing above is tested)
    plain = tiny_model(dev)
    assert not torch.equal(frames(plain, tokens, mask, graph=False), eager)


def test_fresh_adapters_change_nothing(dev):
    """B = 0 straight after apply_lora_to_model: bit-identical to the model without adapters, eager and graph."""
    from csm.training.lora import apply_lora_to_model
    tokens, mask, _ = O.synthetic_batch(TINY, 2, 20, seed=13)
    plain = tiny_model(dev)
    ref = [frames(plain, tokens, mask, graph=gr) for gr in (False, True)]
    m = tiny_model(dev)
    apply_lora_to_model(m, r=8, target_modules=ALL7)
    for gr, r in zip((False, True), ref):
        assert torch.equal(frames(m, tokens, mask, graph=gr), r), gr


def test_live_vs_merged(dev):
    """Live adapters against the same adapters merged into the weights (different bf16 roundings): nearly every code agrees
    on a teacher-forced history; merging while the adapters stay attached gives exactly the merged frames (not applied twice)."""
    from csm.training.lora import merge_lora_weights
    tokens, mask, _ = O.synthetic_batch(TINY, 2, 20, seed=14)
    m = lora_model(dev, modules=["q_proj", "v_proj"])
    live = frames(m, tokens, mask, graph=False)
    m2 = lora_model(dev, modules=["q_proj", "v_proj"])
    merge_lora_weights(m2)
    attached = frames(m2, tokens, mask, history=live)
    lo = m2.lora
    m2.lora = None
    detached = frames(m2, tokens, mask, history=live)
    m2.lora = lo
    assert torch.equal(attached, detached), "merged adapters must not be applied a second time"
    agree = (live == detached).float().mean().item()
    assert agree >= 0.8, f"live and merged adapters agree on only {agree:.1%} of the codes"


def test_dropout_bias_batch_and_swap(dev):
    tokens, mask, _ = O.synthetic_batch(TINY, 2, 20, seed=15)
    # dropout > 0 while training: generation runs without it and leaves draws / training alone
    m0 = lora_model(dev, dropout=0.0)
    ref = frames(m0, tokens, mask)
    md = lora_model(dev, dropout=0.3)
    md.lora.training, md.lora.draws = True, 5
    got = frames(md, tokens, mask)
    assert torch.equal(got, ref)
    assert md.lora.training is True and md.lora.draws == 5
    # bias adapters against the recompute path
    mb = lora_model(dev, use_bias=True)
    kv = frames(mb, tokens, mask, graph=False)
    rc = frames(mb, tokens, mask, use_cache=False, history=kv)
    assert torch.equal(kv[0, :, 0], rc[0, :, 0])
    assert (kv == rc).float().mean().item() >= 0.9
    # ragged batch == single generation per row
    m = lora_model(dev)
    lens = [9, 13]
    tk = [tokens[b, :lens[b]] for b in range(2)]
    mk = [mask[b, :lens[b]] for b in range(2)]
    eng = m.engine
    K = TINY.n_codebooks
    amask = torch.cat([torch.ones(1, K, dtype=torch.bool), torch.zeros(1, 1, dtype=torch.bool)], 1).unsqueeze(1)

    def run(tl, ml, rows):
        B = len(tl)
        m.setup_caches(B)
        m.reset_caches()
        out = [eng.generate_first_frames(tl, ml, 0.8, 12, noise=[q[rows] for q in noise(0)]).cpu()]
        for step in range(1, 5):
            cur = torch.cat([out[-1].long(), torch.zeros(B, 1, dtype=torch.long)], 1).unsqueeze(1)
            out.append(m.generate_frame(cur, amask.repeat(B, 1, 1), torch.ones(B, 1, dtype=torch.long), 0.8, 12,
                                        noise=[q[rows] for q in noise(step)]).cpu())
        return torch.stack(out)

    both = run(tk, mk, slice(0, 2))
    for b in range(2):
        one = run(tk[b:b + 1], mk[b:b + 1], slice(b, b + 1))
        assert torch.equal(one[:, 0], both[:, b]), f"batch row {b} differs from its single generation"
    # new adapter values between two generations: the new state / graph picks them up
    a = frames(m, tokens, mask)
    with torch.no_grad():
        for ad in m.lora.adapters.values():
            ad.B.mul_(-1.0)
    b = frames(m, tokens, mask)
    assert not torch.equal(a, b)
    with torch.no_grad():
        for ad in m.lora.adapters.values():
            ad.B.mul_(-1.0)
    assert torch.equal(frames(m, tokens, mask), a)


def test_config3_adapters_at_csm1b_eager_vs_graph(dev):
    """CSM-1B stacks with config-3 adapters (q_proj, v_proj, r = 8; random init, B set non-zero): eager == graph."""
    from csm.models.model import Model, ModelArgs
    from csm.training.lora import apply_lora_to_model
    m = Model(ModelArgs("llama-1B", "llama-100M", 128256, 2051, 32), device="cuda", seed=0)
    apply_lora_to_model(m, r=8, alpha=16.0)
    with torch.no_grad():
        g = torch.Generator(device="cuda").manual_seed(1)
        for ad in m.lora.adapters.values():
            ad.B[:, :8].copy_((torch.randn(ad.B.shape[0], 8, generator=g, device="cuda") * 0.02).to(BF))
    K = 32
    g = torch.Generator().manual_seed(2)
    tokens = torch.zeros(1, 12, K + 1, dtype=torch.long)
    tokens[0, :, K] = torch.randint(0, 128256, (12,), generator=g)
    mask = torch.zeros(1, 12, K + 1, dtype=torch.bool)
    mask[0, :, K] = True
    amask = torch.cat([torch.ones(1, K, dtype=torch.bool), torch.zeros(1, 1, dtype=torch.bool)], 1).unsqueeze(1)

    def run(graph):
        m.use_hip_graph = graph
        m.reset_caches()
        out = []
        ct, cm, cp = tokens, mask, torch.arange(12).unsqueeze(0)
        for step in range(4):
            gq = torch.Generator().manual_seed(700 + step)
            q = [torch.empty(1, 2051).exponential_(1, generator=gq) for _ in range(K)]
            f = m.generate_frame(ct, cm, cp, 0.9, 50, noise=q).cpu()
            out.append(f)
            ct, cm, cp = torch.cat([f.long(), torch.zeros(1, 1, dtype=torch.long)], 1).unsqueeze(1), amask, cp[:, -1:] + 1
        m.use_hip_graph = True
        return torch.stack(out)

    m.setup_caches(1)
    assert torch.equal(run(False), run(True))


# ----------------------------------------------------------------------------------------------------------- API
class _Tok:
    def encode(self, text):
        return [1] + [3 + (b % 200) for b in text.encode()] + [2]


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


def _tiny32(seed=2):
    from csm.models.model import Model, ModelArgs
    return Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", 300, 2051, 32), device="cuda", seed=seed)


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    S, K = 16, 32
    tokens = torch.zeros(2, S, K + 1, dtype=torch.long)
    tokens[:, :, :K] = torch.randint(0, 2051, (2, S, K), generator=g)
    tokens[:, :, K] = torch.randint(0, 300, (2, S), generator=g)
    masks = torch.ones(2, S, K + 1, dtype=torch.bool)
    targets = torch.randint(0, 2051, (2, S, K), generator=g)
    return {"input_tokens": tokens, "input_masks": masks, "target_audio_tokens": targets}


def test_trainer_generate_sample_and_training_continues(dev, tmp_path):
    from csm.codec import MimiCodec
    from csm.training.lora_trainer import CSMLoRATrainer
    codec = MimiCodec(_hf_mimi(5).state_dict(), device="cuda")
    runs = []
    for with_sample in (True, False):
        tr = CSMLoRATrainer("", str(tmp_path / f"o{int(with_sample)}"), model=_tiny32(), device="cuda", lora_dropout=0.1,
                            target_modules=ALL7)
        tr.train_step(_batch(1))
        draws = tr.model.lora.draws
        if with_sample:
            path = tr.generate_sample("hello there", 0, str(tmp_path / "s" / "sample.wav"), text_tokenizer=_Tok(),
                                      audio_tokenizer=codec, max_audio_length_ms=400)
            with wave.open(path) as w:
                assert w.getframerate() == codec.sample_rate and w.getnframes() > 0
            assert tr.model.lora.training is True and tr.model.lora.draws == draws
        loss = tr.train_step(_batch(2))
        runs.append((float(loss), tr.model.lora.arena.clone()))
    assert runs[0][0] == runs[1][0], "the loss after a sample must be the loss without it"
    assert torch.equal(runs[0][1], runs[1][1]), "the adapters after a sample must be those without it"


def test_cli_finetune_lora_generate_samples(dev, tmp_path, monkeypatch):
    from csm.cli import finetune_lora as cli
    from csm.codec import MimiCodec
    from csm.models.model import ModelArgs
    from csm.training import trainer as trainer_mod
    monkeypatch.setattr(trainer_mod, "csm_1b_args", lambda: ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", 128256, 2051, 32))
    codec = MimiCodec(_hf_mimi(5).state_dict(), device="cuda")
    monkeypatch.setattr(cli, "sample_tokenizers", lambda args, device: (_Tok(), codec))
    from csm.training.lora_trainer import CSMLoRATrainer
    orig = CSMLoRATrainer.generate_sample             # the tiny stacks hold 128 positions: 5 frames instead of the default 10 s
    monkeypatch.setattr(CSMLoRATrainer, "generate_sample", lambda self, *a, **k: orig(self, *a, max_audio_length_ms=400, **k))
    out = tmp_path / "out"
    rc = cli.main(["--model-path", "", "--output-dir", str(out), "--synthetic", "4", "--max-seq-len", "16", "--epochs", "1",
                   "--batch-size", "2", "--val-split", "0", "--generate-samples", "--sample-prompt", "hi"])
    assert rc == 0
    assert (out / "sample.wav").exists()
