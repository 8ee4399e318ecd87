"""Several speakers' LoRA adapters trained in one batch (``LoRAState(n_adapters > 1)``, ``compute_loss(adapter_ids=...)``,
``MultiSpeakerLoRATrainer``) on the tiny model of tests/test_e2e_gpu.py at B = 4, S = 24, acoustic mode "all": against the oracle
run example by example with each example's own adapter, against the single-adapter path, for independence of the adapters from
each other, on packed batches, through the trainer to files a ``LoRABank`` reads, and every refusal."""
import pytest
import torch

from oracle import csm_oracle as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TINY = O.tiny_cfg()
SEVEN = ["q_proj", "k_proj", "v_proj", "output_proj", "w1", "w2", "w3"]
IDS = [0, 2, -1, 1]
_memo = {}


def tiny_model(dev, seed=11):
    from csm.models.model import Model, ModelArgs
    m = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", TINY.text_vocab, TINY.audio_vocab, TINY.n_codebooks), device="cuda")
    p32 = O.init_params(TINY, seed=seed)
    m.load_state_dict(p32)
    m.acoustic_mode = "all"
    return m, {k: v.to(BF).float() for k, v in p32.items()}


def rel(a, b):
    return abs(float(a) - float(b)) / max(1e-12, abs(float(b)))


def gclose(name, got, ref, tol=5e-2):
    got, ref = got.float().cpu(), ref.float().cpu()
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-20
    assert err <= tol * scale, f"{name}: max abs err {err:.4g} vs max |ref| {scale:.4g}"


def batch():
    if "b" not in _memo:
        _memo["b"] = O.synthetic_batch(TINY, 4, 24, seed=6)
    return _memo["b"]


def stacked(dev, mods, r, alpha, A=3, seed=1, b_seed=2):
    """The tiny model with a stack of A adapter sets, every B non-zero."""
    from csm.training.lora import apply_lora_to_model
    m, pq = tiny_model(dev)
    apply_lora_to_model(m, r=r, alpha=alpha, target_modules=mods, seed=seed, n_adapters=A)
    fill_B(m.lora, b_seed)
    return m, pq


def fill_B(lo, b_seed, only=None, scale=0.05):
    with torch.no_grad():
        g = torch.Generator(device="cuda").manual_seed(b_seed)
        for a in range(lo.n_adapters):
            for k, t in lo.named_tensors(adapter=a):
                if k.endswith("lora_B"):
                    v = (torch.randn(t.shape, generator=g, device="cuda") * scale).to(BF)
                    if only is None or a in only:
                        t.copy_(v)


def grads_of(lo, a):
    """{name: gradient view} of adapter set a, in the reference shapes."""
    r, out = lo.r, {}
    for ad in lo.adapter_sets[a].values():
        out[f"{ad.name}.lora_A"] = ad.gA[:r]
        out[f"{ad.name}.lora_B"] = ad.gB[:, :r]
    return out


# ------------------------------------------------------------------------------------------------------------ oracle parity
@pytest.mark.parametrize("mods,r,alpha", [(["q_proj", "v_proj", "w2"], 8, 16.0), (SEVEN, 4, 8.0)])
def test_loss_and_every_adapters_gradients_match_the_oracle_example_by_example(dev, mods, r, alpha):
    from csm.training.utils import compute_loss
    m, pq = stacked(dev, mods, r, alpha)
    lo = m.lora
    tokens, mask, targets = batch()
    total, det = compute_loss(m, tokens, mask, targets, adapter_ids=IDS)
    total.backward()
    # the oracle: every example alone, with its own adapter set (none for -1); the batch loss is their mean (equal row counts)
    sets = [{k: v.detach().float().cpu().requires_grad_(True) for k, v in lo.named_tensors(adapter=a)} for a in range(3)]
    per = []
    for b, a in enumerate(IDS):
        kw = dict(lora=sets[a], lora_scaling=alpha / r) if a >= 0 else {}
        rt, _ = O.compute_loss(pq, TINY, tokens[b:b + 1], mask[b:b + 1], targets[b:b + 1], acoustic_rows=None, **kw)
        per.append(rt)
    ref = torch.stack(per).mean()
    ref.backward()
    print(f"MULTI total {float(total):.6f} oracle {float(ref):.6f} rel {rel(total, ref):.2e}")
    assert rel(total, ref) < 1e-3, (float(total), float(ref))
    for a in range(3):
        for k, gv in grads_of(lo, a).items():
            gclose(f"adapter {a} {k} grad", gv, sets[a][k].grad, 5e-2)
    assert m.grad_arena is None or float(m.grad_arena.abs().max()) == 0.0, "base weights are frozen"
    # rank padding and the entries of Bx outside every adapter's own block: exactly zero
    for G in lo.groups.values():
        if G.mask is not None:
            assert float((G.gBx.float() * (1 - G.mask.float())).abs().max()) == 0.0, G.name
        used = 3 * G.blk
        if used < G.kx:
            assert float(G.gAt[:, used:].abs().max()) == 0.0 and float(G.gBx[:, used:].abs().max()) == 0.0
    if r < lo.r_pad:
        for a in range(3):
            for ad in lo.adapter_sets[a].values():
                assert float(ad.gA[r:].abs().max()) == 0.0 and float(ad.gB[:, r:].abs().max()) == 0.0, "rank padding"


def test_an_example_without_adapter_is_the_base_models(dev):
    from csm.training.utils import compute_loss
    m, pq = stacked(dev, ["q_proj", "v_proj", "w2"], 8, 16.0)
    tokens, mask, targets = batch()
    total, _ = compute_loss(m, tokens, mask, targets, adapter_ids=[-1, -1, -1, -1])
    total.backward()
    assert float(m.lora.grad_arena.abs().max()) == 0.0          # no row names an adapter: every gradient is exactly zero
    ref, _ = O.compute_loss(pq, TINY, tokens, mask, targets, acoustic_rows=None)
    assert rel(total, ref) < 1e-3
    stack, m.lora = m.lora, None
    with torch.no_grad():
        base, _ = compute_loss(m, tokens, mask, targets)
    m.lora = stack
    assert rel(total, base) < 1e-3, (float(total), float(base))


# ------------------------------------------------------------------------------------------------------------ single-adapter parity
@pytest.mark.parametrize("a", [0, 1, 2])
def test_one_adapter_for_every_example_is_the_single_adapter_path(dev, a):
    """All ids = a against a single-adapter LoRAState holding adapter a's weights.  a = 0: the block keeps its place in the first
    k-step of the extension and the other blocks add exact zeros, so the loss is the same number; the other ids move the block to
    another place of a k-step (how the bf16 MFMA sums inside one is not documented): the oracle-parity tolerance."""
    from csm.training.lora import LoRAState
    from csm.training.utils import compute_loss
    m, _ = stacked(dev, ["q_proj", "v_proj", "w2"], 8, 16.0)
    tokens, mask, targets = batch()
    stack = m.lora
    with torch.no_grad():
        multi, _ = compute_loss(m, tokens, mask, targets, adapter_ids=[a] * 4)
    single = LoRAState(m, 8, 16.0, 0.0, ["q_proj", "v_proj", "w2"], None, False, seed=1 + a)
    want = dict(stack.named_tensors(adapter=a))
    with torch.no_grad():
        for k, t in single.named_tensors():
            if k.endswith("lora_A"):
                assert torch.equal(t, want[k]), k                  # set a starts as seed + a alone would
            t.copy_(want[k])
    m.lora = single
    with torch.no_grad():
        alone, _ = compute_loss(m, tokens, mask, targets)
    print(f"SINGLE a={a} multi {float(multi):.8f} alone {float(alone):.8f}")
    if a == 0:
        assert torch.equal(multi, alone), (float(multi), float(alone))
    else:
        assert rel(multi, alone) < 1e-3, (float(multi), float(alone))


# ------------------------------------------------------------------------------------------------------------ neighbour invariance
def test_adapters_do_not_see_each_other(dev):
    """Two runs of three optimiser steps (no clipping) that differ only in adapter 1's initial weights: adapters 0 and 2 end
    bit-equal; adapter 3, which no example names, has a gradient of exactly zero."""
    from csm.training.optim import FusedAdamW
    from csm.training.utils import compute_loss
    tokens, mask, targets = batch()
    ends = []
    for run in range(2):
        m, _ = stacked(dev, ["q_proj", "v_proj", "w2"], 8, 16.0, A=4)
        if run:
            fill_B(m.lora, 99, only=(1,), scale=0.08)
            with torch.no_grad():
                for k, t in m.lora.named_tensors(adapter=1):
                    if k.endswith("lora_A"):
                        t.mul_(0.5)
        opt = FusedAdamW(m, {}, lora_lr=1e-3, lora_weight_decay=0.0)
        for step in range(3):
            total, _ = compute_loss(m, tokens, mask, targets, adapter_ids=[[0, 1, 2, 1], [2, 0, 1, -1], [1, 1, 0, 2]][step])
            total.backward()
            if step == 0:
                lo = m.lora
                for ad in lo.adapter_sets[3].values():
                    assert float(ad.gA.abs().max()) == 0.0 and float(ad.gB.abs().max()) == 0.0, "an adapter no example names"
                assert any(float(ad.gB.abs().max()) > 0 for ad in lo.adapter_sets[0].values())
                for G in lo.groups.values():
                    if G.mask is not None:
                        assert float((G.gBx.float() * (1 - G.mask.float())).abs().max()) == 0.0, G.name
            opt.step(zero_grad=True)
        ends.append({a: {k: t.detach().clone() for k, t in m.lora.named_tensors(adapter=a)} for a in range(4)})
    for a in (0, 2):
        for k in ends[0][a]:
            assert torch.equal(ends[0][a][k], ends[1][a][k]), f"adapter {a} {k} moved with adapter 1"
    assert any(not torch.equal(ends[0][1][k], ends[1][1][k]) for k in ends[0][1])
    moved = [k for k in ends[0][0] if k.endswith("lora_B")]
    assert moved


# ------------------------------------------------------------------------------------------------------------ packed
def test_packed_batch_with_per_segment_ids_matches_the_padded_one(dev):
    """The same five examples padded (ids [B]) and packed (ids [R, n_max] beside segment_lengths), within the bounds of
    tests/test_packed_train_gpu.py: loss rel 1e-3, gradients 5e-2 of the largest."""
    from csm.data import collate_packed, collate_variable_length
    from csm.data.training_data import IGNORE_INDEX
    from csm.training.utils import compute_loss
    items = []
    for i, (S, a) in enumerate(zip((50, 31, 40, 17, 33), (0, 2, -1, 1, 0))):
        tk, mk, tg = O.synthetic_batch(TINY, 1, S, seed=40 + i)
        items.append({"input_tokens": tk[0], "input_masks": mk[0], "target_audio_tokens": tg[0, :S - 1], "adapter": a})
    packed = collate_packed(items, max_seq_len=128)
    padded = collate_variable_length(items, target_pad=IGNORE_INDEX)
    assert packed["segment_lengths"].tolist() == [[50, 40, 33], [31, 17, 0]] and packed["adapter_ids"].tolist() == [[0, -1, 0], [2, 1, -1]]
    assert padded["adapter_ids"].tolist() == [0, 2, -1, 1, 0]
    res = {}
    for name, b in (("padded", padded), ("packed", packed)):
        m, _ = stacked(dev, ["q_proj", "v_proj", "w2"], 8, 16.0)
        m.target_ignore_index = IGNORE_INDEX
        total, _ = compute_loss(m, b["input_tokens"], b["input_masks"], b["target_audio_tokens"], segment_lengths=b.get("segment_lengths"),
                                adapter_ids=b["adapter_ids"])
        total.backward()
        res[name] = (float(total), {a: {k: v.float().clone() for k, v in grads_of(m.lora, a).items()} for a in range(3)})
    print(f"PACKED multi {res['packed'][0]:.6f} padded {res['padded'][0]:.6f}")
    assert rel(res["packed"][0], res["padded"][0]) < 1e-3, (res["packed"][0], res["padded"][0])
    for a in range(3):
        for k, gv in res["packed"][1][a].items():
            gclose(f"adapter {a} {k} grad", gv, res["padded"][1][a][k], 5e-2)


# ------------------------------------------------------------------------------------------------------------ the full loop
def test_trainer_two_steps_files_bank_and_generation(dev, tmp_path):
    from test_lora_bank_gpu import _Tok, _hf_mimi, _tiny32
    from csm.codec import MimiCodec
    from csm.data import SyntheticCSMDataset
    from csm.generator import Generator
    from csm.lora_bank import LoRABank
    from csm.training.lora_trainer import CSMLoRATrainer
    from csm.training.multi_speaker_lora import MultiSpeakerLoRATrainer
    with pytest.raises(NotImplementedError, match="share"):
        MultiSpeakerLoRATrainer("", str(tmp_path / "x"), [1, 2], share_backbone=True, model=_tiny32())
    m = _tiny32()
    m.acoustic_mode = "all"                                            # (the depth decoder's adapters train only with the acoustic term)
    speakers = [7, 3, 9]
    tr = MultiSpeakerLoRATrainer("", str(tmp_path / "o"), speakers, learning_rate=5e-3, model=m, device="cuda")
    tr.logger.setLevel(40)
    assert m.lora.n_adapters == 3 and tr.index == {7: 0, 3: 1, 9: 2}
    sets = {sid: (SyntheticCSMDataset(2, 16, 300, 2051, 32, seed=10 + sid), SyntheticCSMDataset(3, 16, 300, 2051, 32, seed=20 + sid))
            for sid in speakers}
    seen = []
    step = tr.train_step

    def spy(b):
        seen.append(b["adapter_ids"].tolist())
        return step(b)

    tr.train_step = spy
    best = tr.train(sets, batch_size=3, epochs=1, val_every=2, save_every=100, max_grad_norm=1.0)
    assert seen == [[0, 1, 2], [0, 1, 2]] and tr.global_step == 2       # two steps, the speakers in rotation
    assert set(best) == set(speakers) and all(0 < v < float("inf") for v in best.values())
    lo = m.lora
    assert all(float(t.abs().max()) > 0 for a in range(3) for k, t in lo.named_tensors(adapter=a) if k.endswith("lora_B")), "every set trained"
    stack, m.lora = lo, None
    try:
        bank = LoRABank(m)
        for sid in speakers:
            path = tmp_path / "o" / f"speaker_{sid}" / f"speaker_{sid}_lora.safetensors"
            assert path.exists() and (tmp_path / "o" / f"speaker_{sid}" / f"speaker_{sid}_lora_metadata.json").exists()
            st = bank.load(f"s{sid}", str(path))
            want = dict(stack.named_tensors(adapter=tr.index[sid]))
            got = dict(st.named_tensors())
            assert list(got) == list(want)
            for k in got:
                assert torch.equal(got[k], want[k]), (sid, k)
        # the files are what the single-adapter trainer reads, too
        one = CSMLoRATrainer("", str(tmp_path / "one"), model=_tiny32(), device="cuda")
        one.logger.setLevel(40)
        one.load_lora_weights(str(tmp_path / "o" / "speaker_3" / "speaker_3_lora.safetensors"))
        for k, t in one.model.lora.named_tensors():
            assert torch.equal(t, dict(stack.named_tensors(adapter=1))[k]), k
        gen = Generator(m, text_tokenizer=_Tok(), audio_tokenizer=MimiCodec(_hf_mimi(5).state_dict(), device="cuda"))
        for sid in speakers:
            gen.load_adapter(f"s{sid}", str(tmp_path / "o" / f"speaker_{sid}" / f"speaker_{sid}_lora.safetensors"))
        torch.manual_seed(3)
        outs = gen.generate_batch(["hello", "hello", "hello"], [0, 0, 0], [[], [], []], max_audio_length_ms=240, adapters=["s7", None, "s9"])
        assert len(outs) == 3 and all(o.dim() == 1 for o in outs)
    finally:
        m.reset_caches()
        m.lora = stack
    # a sample with one speaker's adapters goes through an exported copy; the stack stays attached
    wav = tr.generate_sample("hello", 9, str(tmp_path / "s9.wav"), text_tokenizer=_Tok(),
                             audio_tokenizer=MimiCodec(_hf_mimi(5).state_dict(), device="cuda"), max_audio_length_ms=160)
    assert (tmp_path / "s9.wav").exists() and wav.endswith("s9.wav") and m.lora is stack
    # load_speaker_model writes one speaker's set back
    before = {k: t.clone() for k, t in stack.named_tensors(adapter=0)}
    master = tr.optimizer.master("lora").clone()
    tr.load_speaker_model(7, str(tmp_path / "o" / "speaker_9" / "speaker_9_lora.safetensors"))
    # ... and re-seeds the optimiser's fp32 master for that set alone: the other speakers keep their low halves
    after = tr.optimizer.master("lora")
    moved = after != master
    assert bool(moved.any()) and bool((master != master.to(BF).float()).any()), "the masters carry low halves in this test"
    mine = torch.zeros(stack.arena.numel(), dtype=torch.bool, device="cuda")
    for k, t in stack.named_tensors(adapter=0):
        torch.as_strided(mine, t.size(), t.stride(), t.storage_offset() - stack.arena.storage_offset()).fill_(True)
    assert not bool((moved & ~mine).any()), "another speaker's master weights changed"
    assert torch.equal(after[mine], stack.arena.float()[mine])
    for k, t in stack.named_tensors(adapter=0):
        assert torch.equal(t, dict(stack.named_tensors(adapter=2))[k])
    assert any(not torch.equal(before[k], t) for k, t in stack.named_tensors(adapter=0))


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(dev, monkeypatch):
    import csm.engine as E
    from csm.training.lora import apply_lora_to_model, merge_lora_weights
    from csm.training.utils import compute_loss
    tokens, mask, targets = batch()
    m, _ = stacked(dev, ["q_proj", "v_proj"], 8, 16.0)
    stack = m.lora
    with pytest.raises(ValueError, match="adapter_ids"):                       # a stack without adapter_ids
        compute_loss(m, tokens, mask, targets)
    with pytest.raises(ValueError, match="out of range"):
        compute_loss(m, tokens, mask, targets, adapter_ids=[0, 1, 2, 3])
    with pytest.raises(ValueError, match="shape"):
        compute_loss(m, tokens, mask, targets, adapter_ids=[0, 1])
    m.lora = None                                                              # adapter_ids without a stack
    with pytest.raises(ValueError, match="stack"):
        compute_loss(m, tokens, mask, targets, adapter_ids=IDS)
    apply_lora_to_model(m, r=8, alpha=16.0, target_modules=["q_proj", "v_proj"], seed=1)
    with pytest.raises(ValueError, match="stack"):
        compute_loss(m, tokens, mask, targets, adapter_ids=[0, 0, 0, 0])
    m.lora = stack
    monkeypatch.setattr(E, "LORA_FUSE", False)                                 # a stack with LORA_FUSE off
    with pytest.raises(NotImplementedError, match="CSM_LORA_FUSE"):
        compute_loss(m, tokens, mask, targets, adapter_ids=IDS)
    monkeypatch.setattr(E, "LORA_FUSE", True)
    # a stack under an active process group
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="process group"):
        compute_loss(m, tokens, mask, targets, adapter_ids=IDS)
    monkeypatch.undo()
    # a stack reaching a generation path: export an adapter first
    with pytest.raises(ValueError, match="export"):
        with E.generation_lora(m):
            pass
    m.setup_caches(1)
    try:
        with pytest.raises(ValueError, match="export"):
            m.generate_frame(tokens[:1, :9], mask[:1, :9], torch.arange(9).unsqueeze(0), 0.9, 10)
        with pytest.raises(ValueError, match="export"):
            E._DecodeStack.attach_lora(object.__new__(E._DecodeStack), stack)
    finally:
        m.reset_caches()
    with pytest.raises(ValueError, match="export"):
        merge_lora_weights(m)
    # the exported set is what those paths take
    one = stack.export(2)
    with E.row_lora(m, one) as lo:
        assert lo is one
    assert m.lora is stack
    with torch.no_grad():                                                      # and the stack still trains after all of that
        total, _ = compute_loss(m, tokens, mask, targets, adapter_ids=IDS)
    assert torch.isfinite(total)
