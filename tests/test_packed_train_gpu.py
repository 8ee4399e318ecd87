"""Training on packed batches (several examples per row: ``csm.data.collate_packed``, ``Engine.forward_loss(segment_lengths=)``, the
segment-masked attention kernels and segment-local RoPE) against the CPU oracle run on the SAME examples in the padded form.  Tiny
model: a backbone of 4 / 2 heads x 64, max_seq_len 128.

Tolerances are the project's own (tests/test_e2e_gpu.py): losses within 1e-3 relative, gradients by gclose(..., 5e-2)."""
import math

import pytest
import torch

from oracle import csm_oracle as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TINY = O.tiny_cfg()
LENGTHS = (40, 31, 33, 17, 50)
GRADS = ("codebook0_head.weight", "backbone.layers.0.attn.q_proj.weight", "decoder.layers.1.mlp.w2.weight", "projection.weight",
         "audio_embeddings.weight")
_memo = {}


def tiny_model(dev, seed=11):
    from csm.models.model import Model, ModelArgs
    m = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", TINY.text_vocab, TINY.audio_vocab, TINY.n_codebooks), device="cuda")
    p32 = O.init_params(TINY, seed=seed)
    m.load_state_dict(p32)
    return m, {k: v.to(BF).float() for k, v in p32.items()}


def rel(a, b):
    return abs(float(a) - float(b)) / max(1e-12, abs(float(b)))


def gclose(name, got, ref, tol=3e-2):
    got, ref = got.float().cpu(), ref.float().cpu()
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-20
    assert err <= tol * scale, f"{name}: max abs err {err:.4g} vs max |ref| {scale:.4g}"


def _batches():
    """The five examples (T_i = S_i - 1), packed into 2 rows of 128 and padded to the batch maximum; computed once."""
    if not _memo:
        from csm.data import collate_packed, collate_variable_length
        from csm.data.training_data import IGNORE_INDEX
        items = []
        for i, S in enumerate(LENGTHS):
            tk, mk, tg = O.synthetic_batch(TINY, 1, S, seed=40 + i)
            items.append({"input_tokens": tk[0], "input_masks": mk[0], "target_audio_tokens": tg[0, :S - 1]})
        packed = collate_packed(items, max_seq_len=128)
        assert packed["input_tokens"].shape[:2] == (2, 128) and packed["segment_lengths"].tolist() == [[50, 40, 33], [31, 17, 0]]
        padded = collate_variable_length(items, target_pad=IGNORE_INDEX)
        _memo.update(packed=packed, padded=padded, ign=IGNORE_INDEX)
    return _memo["packed"], _memo["padded"], _memo["ign"]


def _oracle(pq, padded, **kw):
    """O.compute_loss plus autograd on the padded form, the depth decoder on the labelled rows."""
    tk, mk, tg = padded["input_tokens"], padded["input_masks"], padded["target_audio_tokens"]
    S = tk.shape[1]
    valid = (tg[:, :S - 1, 0] >= 0).reshape(-1).nonzero().squeeze(1)
    pr = {k: v.clone().requires_grad_(True) for k, v in pq.items()}
    rt, rdet = O.compute_loss(pr, TINY, tk, mk, tg, acoustic_rows=valid, **kw)
    rt.backward()
    return rt, rdet, pr


def test_packed_step_matches_the_oracle_on_the_padded_examples(dev):
    from csm.training.utils import compute_loss
    packed, padded, ign = _batches()
    m, pq = tiny_model(dev)
    m.acoustic_mode = "all"
    with pytest.raises(ValueError, match="target_ignore_index"):
        compute_loss(m, packed["input_tokens"], packed["input_masks"], packed["target_audio_tokens"], segment_lengths=packed["segment_lengths"])
    m.target_ignore_index = ign
    m.ensure_grads()
    total, det = compute_loss(m, packed["input_tokens"], packed["input_masks"], packed["target_audio_tokens"], segment_lengths=packed["segment_lengths"])
    total.backward()
    rt, rdet, pr = _oracle(pq, padded)
    print(f"PACKED total {float(total):.6f} oracle {float(rt):.6f} rel {rel(total, rt):.2e}")
    assert rel(total, rt) < 1e-3, (float(total), float(rt))
    assert rel(det["semantic_loss"], rdet["semantic_loss"]) < 1e-3 and rel(det["acoustic_loss"], rdet["acoustic_loss"]) < 1e-3
    grads = dict(m.named_parameters())
    for k in GRADS:
        gclose(k, grads[k].grad, pr[k].grad, 5e-2)
    # the same five examples through the HIP padded path
    with torch.no_grad():
        pad_total, _ = compute_loss(m, padded["input_tokens"], padded["input_masks"], padded["target_audio_tokens"])
    assert rel(total, pad_total) < 1e-3, (float(total), float(pad_total))
    # without the descriptor the packed rows are ordinary sequences whose examples see each other: a different loss
    with torch.no_grad():
        leak, _ = compute_loss(m, packed["input_tokens"], packed["input_masks"], packed["target_audio_tokens"])
    assert rel(leak, total) > 1e-3


def test_segment_lengths_are_validated(dev):
    from csm.training.utils import compute_loss
    packed, _, ign = _batches()
    m, _ = tiny_model(dev)
    m.target_ignore_index = ign
    args = (m, packed["input_tokens"], packed["input_masks"], packed["target_audio_tokens"])
    for bad in ([[50, 40, 39], [31, 17, 0]], [[50, 0, 33], [31, 17, 0]], [[50, 40, -1], [31, 17, 0]], [[50, 40, 33]]):
        with pytest.raises(ValueError, match="segment_lengths"):
            compute_loss(*args, segment_lengths=torch.tensor(bad))


def test_packed_lora_step_matches_the_oracle(dev):
    from csm.training.lora import apply_lora_to_model
    from csm.training.utils import compute_loss
    packed, padded, ign = _batches()
    m, pq = tiny_model(dev)
    m.acoustic_mode = "all"
    m.target_ignore_index = ign
    apply_lora_to_model(m, r=8, alpha=16.0, target_modules=["q_proj", "v_proj"], seed=1)
    with torch.no_grad():   # make B non-zero so that every gradient path is exercised
        g = torch.Generator(device=dev).manual_seed(2)
        for ad in m.lora.adapters.values():
            ad.B.copy_((torch.randn(ad.B.shape, generator=g, device=dev) * 0.05).to(BF))
    total, _ = compute_loss(m, packed["input_tokens"], packed["input_masks"], packed["target_audio_tokens"], segment_lengths=packed["segment_lengths"])
    total.backward()
    lora = {k: v.detach().float().cpu().requires_grad_(True) for k, v in m.get_lora_params().items()}
    rt, _, _ = _oracle(pq, padded, lora=lora, lora_scaling=2.0)
    assert rel(total, rt) < 1e-3, (float(total), float(rt))
    for ad in m.lora.adapters.values():
        gclose(f"{ad.name}.lora_A grad", ad.gA, lora[f"{ad.name}.lora_A"].grad, 5e-2)
        gclose(f"{ad.name}.lora_B grad", ad.gB, lora[f"{ad.name}.lora_B"].grad, 5e-2)


def test_trainer_epoch_with_pack_sequences(dev, tmp_path):
    from csm.data import SyntheticCSMDataset
    from csm.training.trainer import CSMTrainer
    m, _ = tiny_model(dev)
    m.acoustic_mode = "all"
    tr = CSMTrainer("", str(tmp_path), device=str(dev))
    tr.logger.setLevel(40)
    tr.model = m
    tr.num_workers = 0
    tr.pack_sequences, tr.max_seq_len = True, 128
    tr.prepare_optimizer()
    seen, step = [], tr.train_step

    def spy(batch, *a, **k):
        out = step(batch, *a, **k)
        seen.append((tuple(batch["input_tokens"].shape[:2]), batch["segment_lengths"].tolist(), float(out[0])))
        return out

    tr.train_step = spy
    ds = SyntheticCSMDataset(6, 40, TINY.text_vocab, TINY.audio_vocab, TINY.n_codebooks, seed=2)
    tr.train(ds, batch_size=6, accumulation_steps=1, epochs=1, val_every=1000, save_every=1000)
    assert m.target_ignore_index is not None
    assert len(seen) == 1 and seen[0][0] == (2, 128) and seen[0][1] == [[40, 40, 40], [40, 40, 40]] and math.isfinite(seen[0][2])
