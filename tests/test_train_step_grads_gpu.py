"""The train step's gradients (``Engine.forward_loss`` / ``Engine.backward``, the two stacks' backward, the depth-decoder wiring, the
embedding backward and the gradient-buffer states) against the float64 reference of tests/train_step_ref.py, row by row, on the
tiny model of tests/test_e2e_gpu.py (head dims 64 / 128).

Every case of ``train_step_ref.CASES``: EVERY tensor - all 43 of the model, and every adapter tensor - is judged by
``train_step_ref.judge`` against grads64 with the nearest-even emulation as the noise scale: each live row's ratio <= L, each dead
row exactly zero.  The three losses: |loss - loss64| <= L max over eight stochastic draws |loss_draw - loss64|.  L is measured on
the reference alone (train_step_ref.L, proven by test_train_step_ref_cpu.py) and is not fitted to what runs here."""
import pytest
import torch

import train_step_ref as T
from oracle import csm_oracle as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SINGLE = [n for n, c in T.CASES.items() if c.prev is None]


def build(case, dev):
    """The tiny model as ``case`` wants it (ignore index, frozen groups, adapters holding ``make_lora``'s values)."""
    from csm.models.model import Model, ModelArgs
    m = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", T.TINY.text_vocab, T.TINY.audio_vocab, T.TINY.n_codebooks), device="cuda")
    m.load_state_dict(O.init_params(T.TINY, seed=T.PARAM_SEED))
    m.acoustic_mode = "all"
    if case.ign is not None:
        m.target_ignore_index = case.ign
    lora = None
    if case.lora is not None:
        from csm.training.lora import apply_lora_to_model
        sp = case.lora
        assert sp.decoder, "the engine attaches adapters to both stacks"
        apply_lora_to_model(m, r=sp.r, alpha=sp.alpha, target_modules=list(sp.modules), seed=sp.seed, n_adapters=sp.n_adapters)
        lora = T.make_lora(case)
        with torch.no_grad():
            for a, values in enumerate(lora):
                named = dict(m.lora.named_tensors(adapter=a))
                assert sorted(named) == sorted(values)
                for k, t in named.items():
                    t.copy_(values[k].to(BF))
    else:
        m.trainable.update({g: False for g in case.frozen})
    return m, lora


def run(m, case):
    """forward + backward of every micro-batch -> [(total, semantic, acoustic)]."""
    from csm.training.utils import compute_loss
    losses = []
    for seed, scale in case.micros():
        bt = T.batch(case, seed)
        total, det = compute_loss(m, bt["tokens"], bt["mask"], bt["targets"], case.sw, case.aw, acoustic_rows=bt["rows"],
                                  segment_lengths=bt["segment_lengths"], adapter_ids=bt["adapter_ids"])
        (total * scale).backward()
        losses.append((float(total.detach()), float(det["semantic_loss"]), float(det["acoustic_loss"])))
    return losses


def gradients(m, case):
    """Every gradient under the reference's names; a tensor nothing wrote (no arena, no .grad) counts as zeros."""
    out = {}
    for k, p in m.named_parameters():
        out[k] = (p.grad if p.grad is not None else torch.zeros_like(p)).detach().double().cpu()
    if case.lora is not None:
        lo = m.lora
        for a in range(lo.n_adapters):
            for ad in lo.adapter_sets[a].values():
                out[f"adapter{a}.{ad.name}.lora_A"] = ad.gA[:lo.r].detach().double().cpu()
                out[f"adapter{a}.{ad.name}.lora_B"] = ad.gB[:, :lo.r].detach().double().cpu()
    return out


def check(case, m, lora, losses, params=None):
    g64, emu = T.grads64(case, params, lora), T.grads_emulated(case, None, params, lora)
    v = T.judge(gradients(m, case), g64.grads, emu.grads, case.name)
    tensor = max(v.ratios, key=v.ratios.get)
    print(f"WORST {case.name} {v.worst:.3f} ({tensor}; L = {T.L}); {v.n_live} live rows, {v.n_dead} dead, {len(v.dead_nonzero)} dead but non-zero")
    ref, dev = T.loss_noise(case, params, lora)
    for got, r, d in zip(losses, ref, dev):
        print(f"LOSS {case.name} got {got} float64 {r} draws' max deviation {d}")
    assert not v.dead_nonzero, v.dead_nonzero[:8]
    assert v.worst <= T.L, (tensor, v.worst)
    assert len(losses) == len(ref)
    for got, r, d in zip(losses, ref, dev):
        for j in range(3):
            assert abs(got[j] - r[j]) <= T.L * d[j], (case.name, j, got, r, d)


@pytest.mark.parametrize("name", SINGLE)
def test_gradients_row_by_row(dev, name):
    case = T.CASES[name]
    m, lora = build(case, dev)
    check(case, m, lora, run(m, case))


def test_gradients_after_lazy_optimizer_steps(dev):
    """A full step, ``step(zero_grad="lazy")`` (dense groups stale, embeddings zero), then a backward at (1, 0) on new data: the
    decoder's stale buffer must be cleared (dead) and every other group must hold a fresh gradient, not old + new.  Then a further
    lazy step and a backward at (100, 1): the decoder group, zero by now, is accumulated into; the others are overwritten.  The
    references run on the weights the model holds after each step."""
    from csm.training.optim import FusedAdamW
    c2 = T.CASES["lazy_100_1"]
    c1 = c2.prev
    m, _ = build(c1.prev, dev)
    opt = FusedAdamW(m, {g: 1e-3 for g in T.GROUPS})
    run(m, c1.prev)
    for case in (c1, c2):
        opt.step(zero_grad="lazy")
        params = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
        m.acoustic_mode = "all"
        check(case, m, None, run(m, case), params=params)
    assert m.grad_state == {g: "live" for g in T.GROUPS}
