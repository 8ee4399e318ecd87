"""The next-frame training objective on the GPU (``csm.data.to_next_frame`` items through the train step as it is): loss and
gradients against the CPU oracle, packed against padded, learning that reaches ``generate()``, and the trainers.  Tiny model of
tests/test_e2e_gpu.py (backbone 2 layers of 4 / 2 heads x 64, K = 4 codebooks of 67 codes, max_seq_len 128)."""
import math
from functools import partial

import pytest
import torch

from oracle import csm_oracle as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TINY = O.tiny_cfg()
K, V = TINY.n_codebooks, TINY.audio_vocab
# tests/test_packed_train_gpu.py: the tensors whose gradients it compares, one per group and both sides of the depth decoder
GRADS = ("codebook0_head.weight", "backbone.layers.0.attn.q_proj.weight", "decoder.layers.1.mlp.w2.weight", "projection.weight",
         "audio_embeddings.weight")
# learning reaches generation: the budget chosen on the GPU (see test_learning_reaches_generation)
STEPS, LR = 80, 1e-3
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


def gclose(name, got, ref, tol):
    got, ref = got.float().cpu(), ref.float().cpu()
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-20
    print(f"GRAD {name}: max abs err {err:.4g} of max |ref| {scale:.4g} = {err / scale:.3g}")
    assert err <= tol * scale, f"{name}: max abs err {err:.4g} vs max |ref| {scale:.4g}"


def reference_item(n_ctx, n_text, T, seed):
    """An item of the reference form: context turns of n_text text ids + 3 frames + EOS, the target's text; T target frames."""
    g = torch.Generator().manual_seed(seed)
    toks, masks = [], []
    for c in range(n_ctx + 1):
        t, m = torch.zeros(n_text, K + 1, dtype=torch.long), torch.zeros(n_text, K + 1, dtype=torch.bool)
        t[:, K] = torch.randint(0, TINY.text_vocab, (n_text,), generator=g)
        m[:, K] = True
        toks.append(t)
        masks.append(m)
        if c < n_ctx:
            t, m = torch.zeros(4, K + 1, dtype=torch.long), torch.zeros(4, K + 1, dtype=torch.bool)
            t[:3, :K] = torch.randint(0, V - 3, (3, K), generator=g)
            m[:, :K] = True
            toks.append(t)
            masks.append(m)
    return {"input_tokens": torch.cat(toks), "input_masks": torch.cat(masks), "target_audio_tokens": torch.randint(0, V - 3, (T, K), generator=g)}


def _items():
    """Two next-frame items of 12 and 19 positions: target only (4 text + 7 frames + EOS), and one context turn with every
    segment trained (3 text + 3 frames + EOS, 4 text + 7 frames + EOS)."""
    from csm.data import to_next_frame
    a = to_next_frame(reference_item(0, 4, 7, seed=1), "target")
    b = reference_item(1, 3, 7, seed=2)
    extra = torch.zeros(1, K + 1, dtype=torch.long)
    extra[0, K] = 17
    b["input_tokens"] = torch.cat([b["input_tokens"], extra])                  # a fourth text id for the target
    b["input_masks"] = torch.cat([b["input_masks"], b["input_masks"][-1:]])
    b = to_next_frame(b, "all")
    assert [a["input_tokens"].shape[0], b["input_tokens"].shape[0]] == [12, 19]
    return [a, b]


def _padded_step(dev):
    """The padded batch through compute_loss(return_rows=True) and backward, once: (batch, total, losses, {name: grad})."""
    if "padded" not in _memo:
        from csm.data import collate_variable_length
        from csm.data.training_data import IGNORE_INDEX
        from csm.training.utils import compute_loss
        batch = collate_variable_length(_items(), target_pad=IGNORE_INDEX)
        m, pq = tiny_model(dev)
        with pytest.raises(ValueError, match="target_ignore_index"):               # the message says what to set
            compute_loss(m, batch["input_tokens"], batch["input_masks"], batch["target_audio_tokens"])
        m.target_ignore_index = IGNORE_INDEX
        m.ensure_grads()
        total, det = compute_loss(m, batch["input_tokens"], batch["input_masks"], batch["target_audio_tokens"], return_rows=True)
        saved = {"sem_logits": m.engine.saved["logits"].clone(), "sem_t": m.engine.saved["t0"].clone(),
                 "ac_logits": m.engine.saved["dec"]["logits"].clone(), "ac_t": m.engine.saved["dec"]["tgt"].clone()}
        total.backward()
        grads = {k: p.grad.float().cpu().clone() for k, p in m.named_parameters()}
        _memo["padded"] = (batch, float(total.detach()), {k: v.detach().cpu() for k, v in det.items()}, grads, pq, saved)
    return _memo["padded"]


# ------------------------------------------------------------------------------------------------------------ 1. oracle
def test_loss_and_gradients_match_the_oracle(dev):
    """Tolerances of tests/test_e2e_gpu.py::test_ignore_index_padding (the same setting: an ignore index, acoustic mode "all", the
    oracle's depth decoder on the labelled rows): losses within 1e-3 relative, gradients by gclose(..., 5e-2) - here for every
    parameter, not four of them."""
    batch, total, det, grads, pq, _ = _padded_step(dev)
    tk, mk, tg = batch["input_tokens"], batch["input_masks"], batch["target_audio_tokens"]
    S = tk.shape[1]
    assert tk.shape[:2] == (2, 19) and tg.shape == (2, 19, K)
    valid = (tg[:, :S - 1, 0] >= 0).reshape(-1).nonzero().squeeze(1)
    assert valid.numel() == 8 + 12                                   # the positions before a frame: 7 + EOS, and 3 + EOS + 7 + EOS
    pr = {k: v.clone().requires_grad_(True) for k, v in pq.items()}
    rt, rdet = O.compute_loss(pr, TINY, tk, mk, tg, acoustic_rows=valid)
    rt.backward()
    print(f"NEXT-FRAME total {total:.6f} oracle {float(rt):.6f} rel {rel(total, rt):.2e}; semantic rel "
          f"{rel(det['semantic_loss'], rdet['semantic_loss']):.2e} acoustic rel {rel(det['acoustic_loss'], rdet['acoustic_loss']):.2e}")
    assert rel(total, rt) < 1e-3, (total, float(rt))
    assert rel(det["semantic_loss"], rdet["semantic_loss"]) < 1e-3 and rel(det["acoustic_loss"], rdet["acoustic_loss"]) < 1e-3
    assert sorted(grads) == sorted(pr)
    for k, p in pr.items():
        gclose(f"grad {k}", grads[k], p.grad, 5e-2)


def test_return_rows_are_what_the_means_are_taken_over(dev):
    """``semantic_rows`` / ``acoustic_rows`` sum to the two scalar losses to fp32 rounding: n positive fp32 terms summed in two
    orders differ by at most 2 (n - 1) 2^-24 relative, the scaling by 1 / n adds one rounding on either side: 2 n 2^-24."""
    batch, _, det, _, _, saved = _padded_step(dev)
    tg = batch["target_audio_tokens"]
    B, S = tg.shape[:2]
    lab = tg[:, :, 0] >= 0
    lab[:, S - 1] = False
    n = int(lab.sum())
    sr, ar, idx = det["semantic_rows"], det["acoustic_rows"], det["acoustic_row_index"]
    assert sr.shape == (B, S) and sr.dtype == torch.float32 and ar.shape == (n, K - 1) and ar.dtype == torch.float32
    assert idx.dtype == torch.int64 and idx.tolist() == lab.reshape(-1).nonzero().flatten().tolist()
    assert bool((sr[~lab] == 0).all()) and bool((sr[lab] > 0).all()) and bool((ar > 0).all())
    d_sem = rel(sr.double().sum() / n, det["semantic_loss"])
    d_ac = rel(ar.double().sum() / (n * (K - 1)), det["acoustic_loss"])
    print(f"ROWS n {n}: semantic rel {d_sem:.2e} (bound {2 * n * 2.0 ** -24:.2e}), acoustic rel {d_ac:.2e} (bound {2 * n * (K - 1) * 2.0 ** -24:.2e})")
    assert d_sem <= 2 * n * 2.0 ** -24 and d_ac <= 2 * n * (K - 1) * 2.0 ** -24
    # every entry is the CE of its own position and codebook: torch's CE over the logits the step itself produced (fp32 on both
    # sides; 1e-4 is far below the spread between rows, so a row or codebook out of place shows)
    F = torch.nn.functional
    want = F.cross_entropy(saved["sem_logits"][:, :V].cpu(), saved["sem_t"].cpu().clamp(min=0), reduction="none").view(B, S) * lab
    assert float((sr - want).abs().max()) < 1e-4
    wa = F.cross_entropy(saved["ac_logits"].reshape(-1, saved["ac_logits"].shape[-1])[:, :V].cpu(), saved["ac_t"].cpu(), reduction="none")
    assert float((ar - wa.view(K - 1, n).t()).abs().max()) < 1e-4
    assert float((ar[0] - ar[1]).abs().max()) > 1e-3 and float((ar[:, 0] - ar[:, 1]).abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------------------ 2. packed
def test_packed_equals_padded(dev):
    """The same two examples through ``collate_packed`` (one row of 128: 19 | 12) and through padding.  Bounds of
    tests/test_packed_train_gpu.py::test_packed_step_matches_the_oracle_on_the_padded_examples: losses within 1e-3 relative (its
    packed-against-padded comparison), gradients by gclose(..., 5e-2) on its GRADS."""
    from csm.data import collate_packed
    from csm.training.utils import compute_loss
    batch, total, det, grads, _, _ = _padded_step(dev)
    packed = collate_packed(_items(), max_seq_len=128)
    assert packed["segment_lengths"].tolist() == [[19, 12]] and packed["input_tokens"].shape[:2] == (1, 128)
    assert int((packed["target_audio_tokens"][:, :, 0] >= 0).sum()) == int((batch["target_audio_tokens"][:, :, 0] >= 0).sum()) == 20
    m, _ = tiny_model(dev)
    m.target_ignore_index = -100
    m.ensure_grads()
    pt, pdet = compute_loss(m, packed["input_tokens"], packed["input_masks"], packed["target_audio_tokens"],
                            segment_lengths=packed["segment_lengths"])
    pt.backward()
    print(f"PACKED total {float(pt):.6f} padded {total:.6f} rel {rel(pt, total):.2e}")
    assert rel(pt, total) < 1e-3
    assert rel(pdet["semantic_loss"], det["semantic_loss"]) < 1e-3 and rel(pdet["acoustic_loss"], det["acoustic_loss"]) < 1e-3
    got = dict(m.named_parameters())
    for k in GRADS:
        gclose(f"packed grad {k}", got[k].grad, grads[k], 5e-2)


# ------------------------------------------------------------------------------------------------------------ 3. generation
TEXT_IDS = [5, 171, 42, 260]


class _Text:
    def encode(self, text):
        return list(TEXT_IDS)


class _Codes:
    """Stands where the Mimi codec stands in ``Generator``: hands the generated codes back instead of audio."""
    sample_rate = 24000

    def decode(self, codes):                      # [1, K, T] -> [1, 1, K * T]
        return codes.float().reshape(1, 1, -1)


def _utterance():
    g = torch.Generator().manual_seed(123)
    codes = torch.randint(0, V - 3, (6, K), generator=g)
    assert bool((codes != 0).any(dim=1).all()), "no real frame may look like EOS"
    tokens = torch.zeros(4, K + 1, dtype=torch.long)
    tokens[:, K] = torch.tensor(TEXT_IDS)
    mask = torch.zeros(4, K + 1, dtype=torch.bool)
    mask[:, K] = True
    return {"input_tokens": tokens, "input_masks": mask, "target_audio_tokens": codes}


def train_on_utterance(dev, objective, steps=STEPS, lr=LR, trace=None):
    """Full-parameter training of the tiny model (seed 11) on the one utterance, acoustic mode "all", the trainers' loss weights
    and clipping (100 / 1, norm 1.0).  Returns (model, worst per-token CE of the last step's forward)."""
    from csm.data import collate_variable_length, to_next_frame
    from csm.data.training_data import IGNORE_INDEX
    from csm.training.optim import FusedAdamW
    from csm.training.utils import compute_loss
    torch.manual_seed(0)
    m, _ = tiny_model(dev)
    item = _utterance()
    if objective == "next_frame":
        item = to_next_frame(item)
        m.target_ignore_index = IGNORE_INDEX
        batch = collate_variable_length([item], target_pad=IGNORE_INDEX)
    else:
        batch = collate_variable_length([item])
    opt = FusedAdamW(m, {"backbone": lr, "decoder": lr, "embeddings": lr, "other": lr}, weight_decay=0.0)
    worst = float("inf")
    for step in range(steps):
        total, det = compute_loss(m, batch["input_tokens"], batch["input_masks"], batch["target_audio_tokens"], 100.0, 1.0,
                                  return_rows=True)
        total.backward()
        opt.clip_grad_norm(1.0)
        opt.step(zero_grad=True)
        if trace is not None or step == steps - 1:
            worst = max(float(det["semantic_rows"].max()), float(det["acoustic_rows"].max()))
            if trace is not None:
                trace.append(worst)
    return m, worst


def generate_frames(m, max_frames=12):
    """``Generator.generate`` (KV caches, the captured decode graph) with topk = 1 from the text prompt -> the frames [T, K] up to
    the EOS frame; ``max_frames`` when none came."""
    from csm.generator import Generator
    assert m.use_kv_cache
    gen = Generator(m, text_tokenizer=_Text(), audio_tokenizer=_Codes())
    try:
        out = gen.generate("the utterance", 0, [], max_audio_length_ms=80 * max_frames, topk=1)
    finally:
        m.reset_caches()
    return out.reshape(K, -1).t().long().cpu()


def test_learning_reaches_generation(dev):
    """One utterance (4 text ids, 6 frames, EOS) trained as a next-frame item for STEPS = 80 steps of AdamW at LR = 1e-3 (full
    parameters, no weight decay, weights 100 / 1, clip 1.0): every labelled token's CE must be below 0.1 in the last step's
    forward - below ln 2 the label is the argmax already; 0.1 (p > 0.9, a logit gap of at least 2.2) leaves room for the bf16
    differences between the training forward and the decode kernels.  Then greedy generation from the text prompt returns
    exactly the 6 frames and stops at EOS.

    Measured on an MI355X: the worst per-token CE is below 0.1 from step 44 on (0.018 at step 50) and 0.0012 after the 80 steps;
    at LR = 3e-3 it never got below 0.7 in 100 steps."""
    from csm.data.training_data import IGNORE_INDEX
    m, worst = train_on_utterance(dev, "next_frame")
    print(f"LEARN next_frame: worst per-token CE after {STEPS} steps at lr {LR}: {worst:.4f}")
    assert m.target_ignore_index == IGNORE_INDEX
    assert worst < 0.1, f"worst per-token CE {worst:.4f} after {STEPS} steps"
    frames = generate_frames(m)
    want = _utterance()["target_audio_tokens"]
    assert frames.shape == want.shape and torch.equal(frames, want), (frames.tolist(), want.tolist())


def test_the_reference_pairing_does_not_teach_generation(dev):
    """The same utterance, budget and optimiser under ``objective="reference"`` (text position p labelled with frame p; the
    audio is never an input and the position generation starts from is unlabelled): its loss goes down as well, and greedy
    generation does not reproduce the frames.  This is why the next-frame objective exists."""
    m, worst = train_on_utterance(dev, "reference")
    print(f"LEARN reference: worst per-token CE after {STEPS} steps: {worst:.4f}")
    assert math.isfinite(worst)
    frames = generate_frames(m)
    want = _utterance()["target_audio_tokens"]
    print(f"LEARN reference: generated {frames.shape[0]} frames, first {frames[:1].tolist()}, wanted {want[:1].tolist()}")
    assert not (frames.shape == want.shape and torch.equal(frames, want))


# ------------------------------------------------------------------------------------------------------------ 4. trainers
def _tiny32(seed=2):
    from csm.models.model import Model, ModelArgs
    m = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", 300, 2051, 32), device="cuda", seed=seed)
    m.acoustic_mode = "all"                       # (the depth decoder's adapters train only with the acoustic term)
    return m


def _synthetic(n, seed):
    from csm.data import SyntheticCSMDataset
    return SyntheticCSMDataset(n, 24, 300, 2051, 32, seed=seed, objective="next_frame")


def _check_batch(b, pack):
    from csm.data.training_data import IGNORE_INDEX
    tg = torch.as_tensor(b["target_audio_tokens"])
    assert bool((tg == IGNORE_INDEX).any()) and bool((tg >= 0).any())
    assert ("segment_lengths" in b) == pack
    if pack:
        assert tuple(tg.shape[:2]) == (1, 128) and torch.as_tensor(b["segment_lengths"]).tolist() == [[24, 24, 24, 24]]
    else:
        assert tuple(tg.shape[:2]) == (4, 24)


def _adapters_moved_and_nothing_else(m, arena_before):
    lo = m.lora
    n_sets = getattr(lo, "n_adapters", 1)
    sets = [lo.named_tensors(adapter=a) for a in range(n_sets)] if n_sets > 1 else [lo.named_tensors()]
    for tensors in sets:
        assert all(float(t.abs().max()) > 0 for k, t in tensors if k.endswith("lora_B")), "every lora_B started at zero and moved"
    assert m.grad_arena is None or float(m.grad_arena.abs().max()) == 0.0, "the base weights are frozen: no gradient outside the adapters"
    assert torch.equal(m.arena, arena_before)


@pytest.mark.parametrize("pack", [False, True], ids=["padded", "packed"])
def test_lora_trainer_two_steps(dev, tmp_path, pack):
    from csm.data import collate_packed
    from csm.data.training_data import IGNORE_INDEX
    from csm.training.lora_trainer import CSMLoRATrainer
    m = _tiny32()
    tr = CSMLoRATrainer("", str(tmp_path), learning_rate=5e-3, model=m, device="cuda", objective="next_frame")
    tr.logger.setLevel(40)
    assert m.target_ignore_index == IGNORE_INDEX and tr.objective == "next_frame"
    train, val = _synthetic(8, 3), _synthetic(4, 4)
    if pack:                                                           # what --pack-sequences does in the command line
        train.collate = val.collate = partial(collate_packed, max_seq_len=128)
    before = m.arena.clone()
    losses, step = [], tr.train_step

    def spy(b):
        _check_batch(b, pack)
        losses.append(float(step(b)))
        return torch.tensor(losses[-1])

    tr.train_step = spy
    best = tr.train(train, val, batch_size=4, epochs=1, val_every=2, save_every=100)
    assert len(losses) == 2 and all(math.isfinite(x) and x > 0 for x in losses) and math.isfinite(best)
    if not pack:
        assert isinstance(train.collate, partial) and train.collate.keywords == {"target_pad": IGNORE_INDEX} and isinstance(val.collate, partial)
    _adapters_moved_and_nothing_else(m, before)


@pytest.mark.parametrize("pack", [False, True], ids=["padded", "packed"])
def test_multi_speaker_trainer_two_steps(dev, tmp_path, pack):
    from csm.data import collate_packed
    from csm.data.training_data import IGNORE_INDEX
    from csm.training.multi_speaker_lora import MultiSpeakerLoRATrainer
    m = _tiny32()
    tr = MultiSpeakerLoRATrainer("", str(tmp_path), [7, 3], learning_rate=5e-3, model=m, device="cuda", pack_sequences=pack,
                                 max_seq_len=128, objective="next_frame")
    tr.logger.setLevel(40)
    assert m.target_ignore_index == IGNORE_INDEX and m.lora.n_adapters == 2
    sets = {sid: (_synthetic(4, 10 + sid), _synthetic(4, 20 + sid)) for sid in (7, 3)}
    if pack:                                                           # the validation sets collate themselves (the command line)
        for _, val in sets.values():
            val.collate = partial(collate_packed, max_seq_len=128)
    before = m.arena.clone()
    losses, step = [], tr.train_step

    def spy(b):
        _check_batch(b, pack)
        assert torch.as_tensor(b["adapter_ids"]).reshape(-1).tolist() == [0, 1, 0, 1]
        losses.append(float(step(b)))
        return torch.tensor(losses[-1])

    tr.train_step = spy
    best = tr.train(sets, batch_size=4, epochs=1, val_every=2, save_every=100)
    assert len(losses) == 2 and all(math.isfinite(x) and x > 0 for x in losses)
    assert set(best) == {7, 3} and all(0 < v < float("inf") for v in best.values()), "validation ran on next-frame batches"
    _adapters_moved_and_nothing_else(m, before)


def test_full_trainer_epoch(dev, tmp_path):
    """``CSMTrainer`` with ``objective = "next_frame"`` (what ``csm-train --objective next-frame`` sets): the ignore index and the
    IGNORE_INDEX padding without ``ignore_padding`` being named."""
    from csm.data.training_data import IGNORE_INDEX
    from csm.training.trainer import CSMTrainer
    m, _ = tiny_model(dev)
    tr = CSMTrainer("", str(tmp_path), device=str(dev))
    tr.logger.setLevel(40)
    tr.model = m
    tr.num_workers = 0
    tr.objective = "next_frame"
    tr.prepare_optimizer()
    from csm.data import SyntheticCSMDataset
    ds = SyntheticCSMDataset(4, 24, TINY.text_vocab, V, K, seed=2, objective="next_frame")
    seen, step = [], tr.train_step

    def spy(batch, *a, **k):
        out = step(batch, *a, **k)
        seen.append((bool((batch["target_audio_tokens"] == IGNORE_INDEX).any()), float(out[0])))
        return out

    tr.train_step = spy
    tr.train(ds, ds, batch_size=2, accumulation_steps=1, epochs=1, val_every=2, save_every=1000)
    assert m.target_ignore_index == IGNORE_INDEX
    assert len(seen) == 2 and all(ign and math.isfinite(x) for ign, x in seen) and math.isfinite(tr.best_loss)
