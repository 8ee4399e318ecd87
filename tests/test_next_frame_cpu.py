"""The next-frame training objective on the CPU (``csm.data.next_frame_labels`` / ``to_next_frame``, ``CSMDataset(objective=)``,
``SyntheticCSMDataset(objective=)``, the ``--objective`` / ``--loss-on`` flags): the structure of the items, that the loss over them
is the likelihood ``generate_frame`` evaluates prefix by prefix (fp32 oracle on both sides), that both collate functions keep every
label where it was put, and that nothing changes while the flags are absent."""
import argparse
import hashlib
import json
import logging
import math

import pytest
import torch
import torch.nn.functional as F

from csm.data import (CSMDataset, ContextualExampleGenerator, SyntheticCSMDataset, TrainingExample, collate_packed,
                      collate_variable_length, is_next_frame, next_frame_labels, to_next_frame)
from csm.data.training_data import IGNORE_INDEX
from oracle import csm_oracle as O

TINY = O.tiny_cfg()
K, V = TINY.n_codebooks, TINY.audio_vocab
CTX_FRAMES = 3                      # real frames of every hand-built context turn (an EOS frame follows them)


def make_item(n_ctx, n_text, T, seed=0, k=K):
    """An item of the reference form, built by hand: ``n_ctx`` context turns of ``n_text`` text ids + CTX_FRAMES frames + EOS,
    then the target's ``n_text`` text ids; ``target_audio_tokens`` = T frames of codes in [1, V - 3)."""
    g = torch.Generator().manual_seed(seed)
    toks, masks = [], []

    def text():
        t, m = torch.zeros(n_text, k + 1, dtype=torch.long), torch.zeros(n_text, k + 1, dtype=torch.bool)
        t[:, k] = torch.randint(0, TINY.text_vocab, (n_text,), generator=g)
        m[:, k] = True
        toks.append(t)
        masks.append(m)

    for _ in range(n_ctx):
        text()
        t, m = torch.zeros(CTX_FRAMES + 1, k + 1, dtype=torch.long), torch.zeros(CTX_FRAMES + 1, k + 1, dtype=torch.bool)
        t[:CTX_FRAMES, :k] = torch.randint(1, V - 3, (CTX_FRAMES, k), generator=g)
        m[:, :k] = True
        toks.append(t)
        masks.append(m)
    text()
    return {"input_tokens": torch.cat(toks), "input_masks": torch.cat(masks),
            "target_audio_tokens": torch.randint(1, V - 3, (T, k), generator=g)}


def labelled(targets):
    return (targets[:, 0] != IGNORE_INDEX).nonzero().flatten().tolist()


def expected_positions(n_ctx, n_text, T, loss_on):
    """By the definition: the position before every trained audio frame."""
    turn = n_text + CTX_FRAMES + 1
    s_old = n_ctx * turn + n_text
    out = list(range(s_old - 1, s_old + T))                        # last target text position .. last real target frame
    if loss_on == "all":
        for c in range(n_ctx):
            o = c * turn
            out += list(range(o + n_text - 1, o + n_text + CTX_FRAMES))
    return sorted(out)


# ------------------------------------------------------------------------------------------------------------ 1. structure
def test_smallest_case_by_hand():
    """No context, one text id, one frame: [text] [frame] [EOS]; position 0 is labelled with the frame, position 1 with EOS,
    position 2 (the EOS frame, the end of the sequence) with nothing - under either ``loss_on``."""
    it = make_item(0, 1, 1, seed=3)
    for loss_on in ("target", "all"):
        nf = to_next_frame(it, loss_on)
        tk, mk, tg = nf["input_tokens"], nf["input_masks"], nf["target_audio_tokens"]
        assert tk.shape == (3, K + 1) and tg.shape == (3, K)
        assert mk.tolist() == [[False] * K + [True], [True] * K + [False], [True] * K + [False]]
        assert torch.equal(tk[1, :K], it["target_audio_tokens"][0]) and int(tk[2].abs().sum()) == 0
        assert labelled(tg) == [0, 1]
        assert torch.equal(tg[0], it["target_audio_tokens"][0])
        assert tg[1].tolist() == [0] * K
        assert tg[2].tolist() == [IGNORE_INDEX] * K


@pytest.mark.parametrize("loss_on", ["target", "all"])
@pytest.mark.parametrize("T", [1, 7])
@pytest.mark.parametrize("n_text", [1, 5])
@pytest.mark.parametrize("n_ctx", [0, 1, 2])
def test_to_next_frame_structure(n_ctx, n_text, T, loss_on):
    it = make_item(n_ctx, n_text, T, seed=10 * n_ctx + n_text + T)
    before = {k_: v.clone() for k_, v in it.items()}
    nf = to_next_frame(it, loss_on)
    assert all(torch.equal(it[k_], before[k_]) for k_ in it), "the item handed in is left alone"
    tk, mk, tg = nf["input_tokens"], nf["input_masks"], nf["target_audio_tokens"]
    s_old = it["input_tokens"].shape[0]
    assert sorted(nf) == sorted(it) and all(nf[k_].dtype == it[k_].dtype for k_ in it)
    assert tk.shape == (s_old + T + 1, K + 1) and mk.shape == tk.shape and tg.shape == (s_old + T + 1, K)
    # the old input is a prefix; the target's frames and one all-zero EOS frame follow under the audio mask
    assert torch.equal(tk[:s_old], it["input_tokens"]) and torch.equal(mk[:s_old], it["input_masks"])
    assert torch.equal(tk[s_old:s_old + T, :K], it["target_audio_tokens"]) and int(tk[s_old:, K].abs().sum()) == 0
    assert int(tk[-1].abs().sum()) == 0
    assert bool(mk[s_old:, :K].all()) and not bool(mk[s_old:, K].any())
    rows = labelled(tg)
    assert rows == expected_positions(n_ctx, n_text, T, loss_on)
    for p in rows:
        assert torch.equal(tg[p], tk[p + 1, :K]) and bool(mk[p + 1, :K].all())
    unl = sorted(set(range(tg.shape[0])) - set(rows))
    assert bool((tg[unl] == IGNORE_INDEX).all()), "a row is labelled whole or not at all"
    assert tg[s_old + T - 1].tolist() == [0] * K, "the last real frame is labelled with EOS"
    assert s_old + T not in rows and tg.shape[0] - 1 == s_old + T, "the last row (the EOS position) is unlabelled"
    assert is_next_frame(nf) and not is_next_frame(it)
    # the same labels from the definition
    assert torch.equal(tg, next_frame_labels(tk, mk, s_old if loss_on == "target" else 0))
    if loss_on == "all":
        turn = n_text + CTX_FRAMES + 1
        for c in range(n_ctx):
            eos = c * turn + turn - 1
            assert eos not in rows, "a context turn's EOS position is followed by text: unlabelled"
            assert tg[eos - 1].tolist() == [0] * K


def test_to_next_frame_refusals():
    it = make_item(1, 2, 3)
    with pytest.raises(ValueError, match="loss_on"):
        to_next_frame(it, "everything")
    with pytest.raises(ValueError, match="columns"):
        to_next_frame(dict(it, target_audio_tokens=it["target_audio_tokens"][:, :K - 1]))
    with pytest.raises(ValueError, match="reference form"):
        to_next_frame(to_next_frame(it))


class _Text:
    def encode(self, text):
        return [1] + [3 + (ord(c) % 50) for c in text] + [2]


class _Audio:                                   # Mimi's protocol: [1, 1, N] -> [1, 32, ceil(N / 1920)], codes 1..2047
    def encode(self, wav):
        t = math.ceil(wav.shape[-1] / 1920)
        return 1 + (torch.arange(t)[None, None, :] * 7 + torch.arange(32)[None, :, None] + int(wav.shape[-1]) % 11) % 2047


def _conversation(n, sr=24000):
    return [TrainingExample(f"turn {i} says this", torch.zeros(sr * (1 + i % 2) // 4), i % 2) for i in range(n)]


def test_dataset_next_frame_and_over_length_rule():
    conv = _conversation(4)
    ctx = ContextualExampleGenerator(max_context_turns=3).create_contextual_examples(conv)
    tt, at = _Text(), _Audio()
    ref = CSMDataset(ctx, tt, at, max_seq_len=2048)
    assert ref.objective == "reference" and ref.truncate == "reference"
    for loss_on in ("target", "all"):
        ds = CSMDataset(ctx, tt, at, max_seq_len=2048, objective="next_frame", loss_on=loss_on)
        for i in range(4):
            want = to_next_frame(ref[i], loss_on)
            got = ds[i]
            assert all(torch.equal(got[k_], want[k_]) for k_ in want)
            assert got["input_tokens"].shape[1] == 33 and got["target_audio_tokens"].shape[1] == 32
        assert ds.lengths() == [ds[i]["input_tokens"].shape[0] for i in range(4)]
    # over-length: whole oldest turns go, the target's text, frames and EOS stay
    seg = [len(tt.encode(f"[{c.speaker_id}]{c.text}")) + math.ceil(c.audio.numel() / 1920) + 1 for c in conv]
    full = CSMDataset(ctx, tt, at, max_seq_len=2048, objective="next_frame", loss_on="all")[3]
    assert full["input_tokens"].shape[0] == sum(seg)
    for keep in (3, 2, 1, 0):                                          # context turns that still fit
        limit = sum(seg[3 - keep:])
        for max_len in (limit, limit + (seg[3 - keep - 1] - 1 if keep < 3 else 5)):     # exactly, and one short of one more turn
            it = CSMDataset(ctx, tt, at, max_seq_len=max_len, objective="next_frame", loss_on="all")[3]
            n = it["input_tokens"].shape[0]
            assert n == limit, (keep, max_len, n)
            assert torch.equal(it["input_tokens"], full["input_tokens"][-n:]) and torch.equal(it["input_masks"], full["input_masks"][-n:])
            assert torch.equal(it["target_audio_tokens"], full["target_audio_tokens"][-n:])
            assert bool(it["input_masks"][0, 32]), "an item starts with a turn's text"
    with pytest.raises(ValueError, match=r"example 3.*" + str(seg[3])):
        CSMDataset(ctx, tt, at, max_seq_len=seg[3] - 1, objective="next_frame")[3]
    for truncate in ("reference", "keep_context"):
        with pytest.raises(ValueError, match="truncate"):
            CSMDataset(ctx, tt, at, objective="next_frame", truncate=truncate)
    with pytest.raises(ValueError, match="objective"):
        CSMDataset(ctx, tt, at, objective="next")
    assert CSMDataset(ctx, tt, at, objective="next-frame").objective == "next_frame"


def test_synthetic_dataset_same_tokens_under_both_objectives():
    a = SyntheticCSMDataset(3, 40, TINY.text_vocab, V, K, seed=9)
    b = SyntheticCSMDataset(3, 40, TINY.text_vocab, V, K, seed=9, objective="next_frame")
    for i in range(3):
        x, y = a[i], b[i]
        assert torch.equal(x["input_tokens"], y["input_tokens"]) and torch.equal(x["input_masks"], y["input_masks"])
        assert x["target_audio_tokens"].shape == y["target_audio_tokens"].shape and x["target_audio_tokens"].dtype == y["target_audio_tokens"].dtype
        assert int(x["target_audio_tokens"].min()) >= 0
        assert torch.equal(y["target_audio_tokens"], next_frame_labels(y["input_tokens"], y["input_masks"]))
        audio = y["input_masks"][:, :K].all(1)
        assert labelled(y["target_audio_tokens"]) == (audio[1:].nonzero().flatten()).tolist() and is_next_frame(y)


# ------------------------------------------------------------------------------------------------------------ 2. alignment
def _prefix_likelihood(params, tokens, mask, targets):
    """What ``oracle.generate_frame`` computes for every labelled prefix, with the teacher's codes in place of samples: the
    codebook-0 logits at the prefix's last position, then the depth decoder grown one code at a time."""
    dec_params = {k_: v for k_, v in params.items() if k_.startswith("decoder.")}
    sem, ac = [], []
    for p in labelled(targets):
        code = targets[p]
        last_h = O.backbone_hidden(params, TINY, tokens[None, :p + 1], mask[None, :p + 1])[:, -1, :]
        c0 = last_h @ params["codebook0_head.weight"].t().float()
        sem.append(-F.log_softmax(c0, dim=-1)[0, code[0]])
        seq = [last_h.unsqueeze(1), params["audio_embeddings.weight"][code[0] + 0 * V].float()[None, None]]
        for i in range(1, K):
            x = torch.cat(seq, dim=1) @ params["projection.weight"].t().float()
            pos = torch.arange(x.shape[1]).unsqueeze(0)
            dec = O.transformer(dec_params, "decoder", TINY.decoder, x, pos)
            logits = dec[:, -1, :] @ params["audio_head"][i - 1].float()
            ac.append(-F.log_softmax(logits, dim=-1)[0, code[i]])
            seq.append(params["audio_embeddings.weight"][code[i] + i * V].float()[None, None])
    return torch.stack(sem).mean(), torch.stack(ac).mean()


def test_the_objective_is_the_likelihood_generation_samples_from():
    """One next-frame item (one context turn, 3 text ids, 5 target frames, every segment trained: 10 labelled positions of 16):
    the mean over the labelled positions of the negative log-likelihood that ``generate_frame`` assigns to the next frame given the
    prefix - evaluated prefix by prefix, the depth decoder one code at a time - equals ``oracle.semantic_loss`` /
    ``oracle.acoustic_loss(rows=labelled)`` on the whole sequence.  Both sides are the same fp32 oracle at two sequence lengths.

    Measured relative differences, seeds 0 / 1 / 2: semantic 2.17e-07 / 0 / 0, acoustic 0 / 0 / 0 (the one that is not zero is
    two fp32 roundings of a mean near 4.4).  Asserted: ten times the largest, 2.17e-06, which is below 1e-4."""
    bound = 10 * 2.17e-07
    assert bound < 1e-4
    nf = to_next_frame(make_item(1, 3, 5, seed=21), "all")
    tokens, mask, targets = nf["input_tokens"], nf["input_masks"], nf["target_audio_tokens"]
    rows = torch.tensor(labelled(targets))
    assert len(rows) == 10 and tokens.shape[0] == 16
    for seed in (0, 1, 2):
        params = O.init_params(TINY, seed)
        hidden = O.backbone_hidden(params, TINY, tokens[None], mask[None])
        sem = O.semantic_loss(params, hidden, targets[None])
        ac = O.acoustic_loss(params, TINY, hidden, targets[None], rows=rows)     # B = 1: the flat row of position p is p
        psem, pac = _prefix_likelihood(params, tokens, mask, targets)
        ds, da = abs(float(psem) - float(sem)) / float(sem), abs(float(pac) - float(ac)) / float(ac)
        print(f"ALIGN seed {seed}: semantic {float(sem):.6f} rel {ds:.2e}; acoustic {float(ac):.6f} rel {da:.2e}")
        assert ds <= bound and da <= bound, (seed, ds, da)
    # the reference pairing of the same utterance (position p with frame p) is another number altogether
    it = make_item(1, 3, 5, seed=21)
    hid = O.backbone_hidden(params, TINY, it["input_tokens"][None], it["input_masks"][None])
    n = min(it["input_tokens"].shape[0] - 1, 5)
    other = F.cross_entropy(hid[0, :n] @ params["codebook0_head.weight"].t(), it["target_audio_tokens"][:n, 0])
    assert abs(float(other) - float(sem)) > 1e-4


# ------------------------------------------------------------------------------------------------------------ 3. collation
def _three_items():
    """Next-frame items of 9, 14 and 23 positions, every segment trained."""
    def turn(n_text, frames, g):
        t = torch.zeros(n_text + frames + 1, K + 1, dtype=torch.long)
        m = torch.zeros(n_text + frames + 1, K + 1, dtype=torch.bool)
        t[:n_text, K] = torch.randint(0, TINY.text_vocab, (n_text,), generator=g)
        m[:n_text, K] = True
        t[n_text:n_text + frames, :K] = torch.randint(1, V - 3, (frames, K), generator=g)
        m[n_text:, :K] = True
        return t, m

    g = torch.Generator().manual_seed(5)
    items = []
    for turns in ([(3, 5)], [(2, 2), (3, 5)], [(2, 2), (3, 2), (4, 7)]):
        parts = [turn(n, f, g) for n, f in turns]
        tk, mk = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        items.append({"input_tokens": tk, "input_masks": mk, "target_audio_tokens": next_frame_labels(tk, mk)})
    assert [it["input_tokens"].shape[0] for it in items] == [9, 14, 23]
    return items


def test_collation_keeps_every_label_where_it_was_put():
    items = _three_items()
    n_lab = [len(labelled(it["target_audio_tokens"])) for it in items]
    assert n_lab == [6, 9, 14]
    b = collate_variable_length(items, target_pad=IGNORE_INDEX)
    assert b["target_audio_tokens"].shape == (3, 23, K)
    for i, it in enumerate(items):
        n = it["input_tokens"].shape[0]
        assert torch.equal(b["target_audio_tokens"][i, :n], it["target_audio_tokens"])
        assert bool((b["target_audio_tokens"][i, n:] == IGNORE_INDEX).all())
        assert torch.equal(b["input_tokens"][i, :n], it["input_tokens"])
    assert int((b["target_audio_tokens"][:, :, 0] != IGNORE_INDEX).sum()) == sum(n_lab)
    # packed: first fit by decreasing length puts all three into one row, 23 | 14 | 9; collate_packed keeps the first n - 1
    # labels of an example, and the n-th - its last position's - is unlabelled in this form anyway
    pk = collate_packed(items, max_seq_len=128)
    assert pk["segment_lengths"].tolist() == [[23, 14, 9]] and pk["target_audio_tokens"].shape == (1, 128, K)
    want = torch.full((128, K), IGNORE_INDEX, dtype=torch.long)
    o = 0
    for i in (2, 1, 0):
        n = items[i]["input_tokens"].shape[0]
        want[o:o + n] = items[i]["target_audio_tokens"]
        assert torch.equal(pk["input_tokens"][0, o:o + n], items[i]["input_tokens"])
        assert pk["target_audio_tokens"][0, o + n - 1].tolist() == [IGNORE_INDEX] * K, "a segment's last position is unlabelled"
        o += n
    assert torch.equal(pk["target_audio_tokens"][0], want)
    # every label still names the frame at the next position of its own segment
    tk, tg = pk["input_tokens"][0], pk["target_audio_tokens"][0]
    for p in labelled(tg):
        assert torch.equal(tg[p], tk[p + 1, :K])


# ------------------------------------------------------------------------------------------------------------ 4. command lines
def _digest(item):
    h = hashlib.sha256()
    for k_ in ("input_tokens", "input_masks", "target_audio_tokens"):
        h.update(item[k_].numpy().tobytes())
    return h.hexdigest()


def test_flags_parse_in_the_three_clis(tmp_path):
    from csm.cli import finetune_lora, finetune_lora_multi, train
    from csm.cli.common import objective_of
    cfg = tmp_path / "speakers.json"
    cfg.write_text(json.dumps([{"name": "a", "speaker_id": 1, "synthetic": 8}]))
    base = {train: ["--model-path", ""], finetune_lora: ["--model-path", ""],
            finetune_lora_multi: ["--model-path", "", "--output-dir", str(tmp_path), "--speakers-config", str(cfg)]}
    for cli, argv in base.items():
        a = cli.parse_args(argv)
        assert (a.objective, a.loss_on) == ("reference", "target") and objective_of(a) == ("reference", "target")
        a = cli.parse_args(argv + ["--objective", "next-frame"])
        assert (a.objective, a.loss_on) == ("next-frame", "target") and objective_of(a) == ("next_frame", "target")
        a = cli.parse_args(argv + ["--objective", "next-frame", "--loss-on", "all"])
        assert objective_of(a) == ("next_frame", "all")
        for bad in (["--objective", "next_frame"], ["--loss-on", "context"]):
            with pytest.raises(SystemExit):
                cli.parse_args(argv + bad)
    assert objective_of(argparse.Namespace()) == ("reference", "target"), "arguments from before the flags"


def test_load_datasets_default_is_unchanged_and_next_frame_applies(tmp_path, caplog):
    from csm.cli import train
    from csm.cli.common import load_datasets
    argv = ["--model-path", "", "--synthetic", "8", "--max-seq-len", "48"]
    tr, va = load_datasets(train.parse_args(argv))
    assert len(tr) == 7 and len(va) == 1 and tr.objective == "reference"
    # the bytes of the item this command line gave before the flags existed (recorded from the parent commit)
    assert _digest(tr[0]) == DEFAULT_SYNTHETIC_ITEM_SHA256
    plain = SyntheticCSMDataset(7, 48, seed=1234)[0]
    assert all(torch.equal(tr[0][k_], plain[k_]) for k_ in plain)
    tr2, va2 = load_datasets(train.parse_args(argv + ["--objective", "next-frame"]))
    assert tr2.objective == va2.objective == "next_frame"
    assert torch.equal(tr2[0]["input_tokens"], tr[0]["input_tokens"]) and is_next_frame(tr2[0]) and not is_next_frame(tr[0])
    # a token file: items of the reference form are converted, items already in the new form pass through, an item that
    # does not fit is skipped and counted
    old = [make_item(1, 2, 4, seed=s, k=32) for s in range(3)]
    long_one = make_item(2, 5, 30, seed=9, k=32)
    path = tmp_path / "items.pt"
    torch.save(old[:2] + [to_next_frame(old[2], "all"), long_one], str(path))
    args = train.parse_args(["--model-path", "", "--token-file", str(path), "--max-seq-len", "40", "--val-split", "0",
                             "--objective", "next-frame"])
    with caplog.at_level(logging.WARNING, logger="csm.cli.common"):
        ds, val = load_datasets(args)
    assert val is None and len(ds) == 3 and "skipped 1 of 4" in caplog.text
    for i in range(2):
        want = to_next_frame(old[i], "target")
        assert all(torch.equal(ds[i][k_], want[k_]) for k_ in want)
    want = to_next_frame(old[2], "all")
    assert all(torch.equal(ds[2][k_], want[k_]) for k_ in want), "an item in the new form passes through (its own loss_on stays)"
    # without the flag the same file loads as it always did: every tensor cut to --max-seq-len, nothing converted
    args = train.parse_args(["--model-path", "", "--token-file", str(path), "--max-seq-len", "40", "--val-split", "0"])
    ds, _ = load_datasets(args)
    assert len(ds) == 4 and torch.equal(ds[0]["target_audio_tokens"], old[0]["target_audio_tokens"])
    assert torch.equal(ds[3]["input_tokens"], long_one["input_tokens"]) and ds[2]["target_audio_tokens"].shape[0] == 13


def test_multi_cli_applies_the_flags_per_speaker():
    from csm.cli.finetune_lora_multi import run_objective, speaker_datasets_of
    args = argparse.Namespace(max_seq_len=32, val_split=0.25, mimi_weights=None, text_tokenizer=None, context_turns=2,
                              objective="reference", loss_on="target")
    configs = [{"name": "a", "speaker_id": 1, "synthetic": 8}, {"name": "b", "speaker_id": 2, "synthetic": 8, "objective": "next-frame"}]
    sets = speaker_datasets_of(configs, args)
    assert not is_next_frame(sets[1][0][0]) and is_next_frame(sets[2][0][0]) and is_next_frame(sets[2][1][0])
    assert run_objective(configs, args) == "next_frame" and run_objective(configs[:1], args) == "reference"
    args.objective = "next-frame"
    sets = speaker_datasets_of(configs[:1], args)
    assert is_next_frame(sets[1][0][0]) and run_objective(configs[:1], args) == "next_frame"
    with pytest.raises(ValueError, match="objective"):
        run_objective([{"name": "c", "speaker_id": 3, "synthetic": 8, "objective": "next"}], args)


DEFAULT_SYNTHETIC_ITEM_SHA256 = "776f3ddada381138fd28b131459bc100efeae575ad457b3498a54ac88bcf0fbf"
