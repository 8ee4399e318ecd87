"""Data front end of CSM training: audio loading, segmentation, contextual examples, frame tokenisation, collation.

Mirrors reference ``src/csm/data/training_data.py`` (classes, signatures and results) without torchaudio, which this
image does not have: WAV files are read with ``scipy.io.wavfile`` and resampled by the windowed-sinc interpolation
``torchaudio.functional.resample`` documents (Hann window, ``lowpass_filter_width=6``, ``rolloff=0.99``), restated
below.  Audio tokenisation goes through any object with Mimi's ``encode([1,1,N]) -> [1,K,T]`` protocol - on the GPU box
that is ``csm.codec.MimiCodec`` (HIP kernels); nothing here touches the GPU by itself, so the module imports on CPU.

Frame layout (reference ``generator.py:77-145`` = ``training_data.py:304-335``): a text token occupies column 32 of a
33-wide frame, an audio frame columns 0..31, and every audio segment ends in one all-zero EOS frame.
"""
import json
import math
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, Iterator, List, Optional, Sequence, Union

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset, Sampler

IGNORE_INDEX = -100
OBJECTIVES = ("reference", "next_frame")
LOSS_ON = ("target", "all")


def check_objective(objective: str, loss_on: str = "target") -> str:
    """``objective`` spelled as the data layer spells it (the command lines write ``next-frame``); anything else raises."""
    objective = str(objective).replace("-", "_")
    if objective not in OBJECTIVES:
        raise ValueError(f"objective must be one of {OBJECTIVES}, got {objective!r}")
    if loss_on not in LOSS_ON:
        raise ValueError(f"loss_on must be one of {LOSS_ON}, got {loss_on!r}")
    return objective


# ------------------------------------------------------------------------------------------------ next-frame objective
def next_frame_labels(tokens: torch.Tensor, mask: torch.Tensor, loss_from: int = 0) -> torch.Tensor:
    """Labels ``[S, K]`` int64 of the objective that ``generate()`` samples from, for one interleaved sequence ``tokens`` /
    ``mask`` ``[S, K+1]``: ``targets[p] = tokens[p+1, :K]`` where position p+1 is an audio frame (``mask[p+1, :K]`` all true)
    and ``p + 1 >= loss_from``; every other row, the last one included, is ``IGNORE_INDEX``.

    Position p's codebook-0 logits and the depth decoder fed ``hidden[p]`` then predict the frame that generation would
    feed back at position p+1 (``Model.generate_frame``).  It follows that
    * the last text position of a segment is labelled with that segment's first frame;
    * the position holding the last real frame is labelled with the EOS frame, all K codes 0 - which is what ends an
      utterance in ``generate()``;
    * the EOS position itself is unlabelled when the next position is text or the end of the sequence.
    ``loss_from`` leaves the frames before it (a conversation's context turns) out of the loss."""
    S, K = tokens.shape[0], tokens.shape[1] - 1
    targets = torch.full((S, K), IGNORE_INDEX, dtype=torch.long)
    if S > 1:
        nxt = mask[1:, :K].bool().all(dim=1) & (torch.arange(1, S) >= int(loss_from))
        targets[:-1][nxt] = tokens[1:, :K][nxt].to(torch.long)
    return targets


def is_next_frame(item: Dict[str, torch.Tensor]) -> bool:
    """An item already in the next-frame form: one label row per input position, at least one of them ``IGNORE_INDEX``
    (the last row always is)."""
    tg = item["target_audio_tokens"]
    return tg.shape[0] == item["input_tokens"].shape[0] and bool((tg == IGNORE_INDEX).any())


def to_next_frame(item: Dict[str, torch.Tensor], loss_on: str = "target") -> Dict[str, torch.Tensor]:
    """An item of the reference form (``input_tokens`` = context segments + the target's text frames, ``target_audio_tokens``
    = the target's codes ``[T, K]``) in the next-frame form: the target's T frames and one all-zero EOS frame are appended
    to the input under the audio mask, exactly as ``CSMDataset._tokenize_audio`` does for a context turn, and
    ``target_audio_tokens`` becomes ``next_frame_labels`` of the result, ``[S + T + 1, K]``.

    ``loss_on="target"`` labels the target utterance only (``loss_from`` = its first audio position: the last text position
    predicts frame 0, the last frame predicts EOS); ``loss_on="all"`` labels every segment's audio.  Keys and dtypes stay
    those of the reference form, so the collate functions, token files and ``TokenFileDataset`` take the result as it is -
    with ``target_pad=IGNORE_INDEX`` and ``model.target_ignore_index`` set."""
    check_objective("next_frame", loss_on)
    tokens, mask, codes = item["input_tokens"], item["input_masks"], item["target_audio_tokens"]
    S, (T, K) = tokens.shape[0], codes.shape
    if tokens.shape[1] != K + 1:
        raise ValueError(f"input_tokens has {tokens.shape[1]} columns and target_audio_tokens {K}: expected K + 1 and K")
    if bool((codes < 0).any()):
        raise ValueError("target_audio_tokens holds negative codes: the item is not in the reference form")
    frames = torch.zeros(T + 1, K + 1, dtype=tokens.dtype)
    frames[:T, :K] = codes.to(tokens.dtype)                                              # + EOS frame
    fmask = torch.zeros(T + 1, K + 1, dtype=mask.dtype)
    fmask[:, :-1] = True
    tokens, mask = torch.cat([tokens, frames], 0), torch.cat([mask, fmask], 0)
    out = dict(item)
    out.update(input_tokens=tokens, input_masks=mask,
               target_audio_tokens=next_frame_labels(tokens, mask, S if loss_on == "target" else 0))
    return out


def pad_with_ignore_index(dataset):
    """A dataset of the ``get_batch`` protocol collates itself (``dataset.collate``): have the padded collation pad the labels
    with ``IGNORE_INDEX``, which a next-frame batch needs.  Another collate function (``collate_packed``) is left alone."""
    if dataset is not None and getattr(dataset, "collate", None) is collate_variable_length:
        from functools import partial
        dataset.collate = partial(collate_variable_length, target_pad=IGNORE_INDEX)
    return dataset


# ------------------------------------------------------------------------------------------------ audio I/O
def resample(wav: torch.Tensor, orig_sr: int, new_sr: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> torch.Tensor:
    """Band-limited resampling of ``[..., N]`` by windowed-sinc interpolation (the algorithm of
    ``torchaudio.functional.resample`` with its default ``sinc_interp_hann`` kernel, which the reference calls at
    training_data.py:60)."""
    if orig_sr == new_sr:
        return wav
    g = math.gcd(int(orig_sr), int(new_sr))
    o, n = int(orig_sr) // g, int(new_sr) // g
    base = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / base)
    idx = torch.arange(-width, width + o, dtype=torch.float64) / o
    t = (torch.arange(0, -n, -1, dtype=torch.float64)[:, None] / n + idx[None, :]) * base
    t = t.clamp(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kernel = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window * (base / o)      # [n, 2*width + o]
    shape = wav.shape
    x = wav.reshape(-1, 1, shape[-1]).to(torch.float64)
    x = torch.nn.functional.pad(x, (width, width + o))
    y = torch.nn.functional.conv1d(x, kernel[:, None, :], stride=o)                                 # [B, n, frames]
    y = y.transpose(1, 2).reshape(x.shape[0], -1)
    length = math.ceil(n * shape[-1] / o)
    return y[:, :length].reshape(shape[:-1] + (length,)).to(wav.dtype)


def load_audio(path: Union[str, Path]):
    """``(waveform [channels, N] float32 in [-1, 1], sample_rate)`` of a WAV file (what ``torchaudio.load`` returns)."""
    from scipy.io import wavfile
    sr, data = wavfile.read(str(path))
    if data.ndim == 1:
        data = data[:, None]
    if data.dtype == np.uint8:
        x = (data.astype(np.float32) - 128.0) / 128.0
    elif np.issubdtype(data.dtype, np.integer):
        x = data.astype(np.float32) / float(2 ** (8 * data.dtype.itemsize - 1))
    else:
        x = data.astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(x.T)), int(sr)


@dataclass
class TrainingExample:
    """One utterance: transcript, mono waveform at the processor's sample rate, speaker id (training_data.py:16-23)."""
    text: str
    audio: torch.Tensor
    speaker_id: int
    metadata: Optional[Dict] = None


# ------------------------------------------------------------------------------------------------ segmentation
class CSMDataProcessor:
    """Cuts a recording + transcript into training utterances (reference training_data.py:26-176)."""

    def __init__(self, sample_rate: int = 24000, segment_duration_ms: int = 10000, overlap_ms: int = 2000):
        self.sample_rate = sample_rate
        self.segment_duration_samples = int(segment_duration_ms * sample_rate / 1000)
        self.overlap_samples = int(overlap_ms * sample_rate / 1000)

    def prepare_from_audio_file(self, audio_path, transcript_path, speaker_id: int, alignment_path=None) -> List[TrainingExample]:
        audio, sr = load_audio(audio_path)
        if sr != self.sample_rate:
            audio = resample(audio, sr, self.sample_rate)
        if audio.size(0) > 1:
            audio = audio.mean(dim=0, keepdim=True)
        audio = audio.squeeze(0)
        transcript = Path(transcript_path).read_text().strip()
        if alignment_path:
            return self._segment_with_alignments(audio, transcript, speaker_id, self._load_alignments(alignment_path))
        return self._segment_basic(audio, transcript, speaker_id)

    def _keep(self, text: str, n_samples: int) -> bool:
        return len(text) >= 10 and n_samples >= self.sample_rate       # at least 10 characters and one second

    def _segment_basic(self, audio: torch.Tensor, transcript: str, speaker_id: int) -> List[TrainingExample]:
        """Overlapping fixed-length windows; the text of a window is the proportional slice of the transcript
        (characters per sample), reference training_data.py:81-114."""
        n = audio.size(0)
        cps = len(transcript) / n
        out = []
        for s in range(0, n, self.segment_duration_samples - self.overlap_samples):
            e = min(s + self.segment_duration_samples, n)
            text = transcript[int(s * cps):int(e * cps)]
            if self._keep(text.strip(), e - s):
                out.append(TrainingExample(text, audio[s:e], speaker_id, {"start_sample": s, "end_sample": e}))
        return out

    @staticmethod
    def _load_alignments(path) -> Dict:
        with open(path, "r") as f:
            return json.load(f)

    def _segment_with_alignments(self, audio, transcript, speaker_id, alignments) -> List[TrainingExample]:
        """Greedy grouping of aligned words into windows no longer than the segment duration, measured from the
        window's first word (the initial window is anchored at sample 0); reference training_data.py:121-176."""
        words = alignments.get("words", [])
        if not words:
            return self._segment_basic(audio, transcript, speaker_id)
        spans, start, end, text = [], 0, 0, ""
        for w in words:
            ws, we = int(w["start"] * self.sample_rate), int(w["end"] * self.sample_rate)
            if we - start > self.segment_duration_samples:
                if text:
                    spans.append((start, end, text))
                start, end, text = ws, we, w["word"] + " "
            else:
                end, text = we, text + w["word"] + " "
        if text:
            spans.append((start, end, text))
        out = []
        for s, e, text in spans:
            text = text.strip()
            if self._keep(text, e - s):
                out.append(TrainingExample(text, audio[s:e], speaker_id, {"start_sample": s, "end_sample": e}))
        return out


class ContextualExampleGenerator:
    """Turn i of a conversation becomes a target with up to ``max_context_turns`` preceding turns as context
    (reference training_data.py:179-224)."""

    def __init__(self, max_context_turns: int = 3, include_audio_context: bool = True):
        self.max_context_turns = max_context_turns
        self.include_audio_context = include_audio_context

    def create_contextual_examples(self, conversation: Sequence[TrainingExample]) -> List[Dict]:
        return [{"context": list(conversation[max(0, i - self.max_context_turns):i]), "target": conversation[i]}
                for i in range(len(conversation))]


# ------------------------------------------------------------------------------------------------ dataset
class CSMDataset(Dataset):
    """Tokenised contextual examples (reference training_data.py:227-358): input = context segments (text + audio
    frames) followed by the target's text frames; ``target_audio_tokens`` = the target's Mimi codes ``[T, K]``.

    ``truncate="reference"`` (the default) reproduces the reference's over-length rule literally (only the target's text
    frames survive, lines 289-295); ``truncate="keep_context"`` keeps the last ``max_seq_len`` frames instead.

    ``objective="reference"`` is that form: ``forward_loss`` pairs input position p with target frame p - the reference's
    pairing, kept for parity and the benchmark.  ``objective="next_frame"`` returns ``to_next_frame(item, loss_on)``: the
    target's frames and EOS are part of the input and every label is the next position's frame, the likelihood
    ``generate()`` samples from.  Its over-length rule: the target's text, frames and EOS survive whole and whole oldest
    context turns are dropped until the item fits ``max_seq_len``; a target that does not fit alone raises ``ValueError``
    (``truncate=`` has no meaning there and is refused)."""

    def __init__(self, examples: List[Dict], text_tokenizer, audio_tokenizer, max_seq_len: int = 2048,
                 truncate: Optional[str] = None, objective: str = "reference", loss_on: str = "target"):
        objective = check_objective(objective, loss_on)
        if objective == "next_frame" and truncate is not None:
            raise ValueError("truncate= cuts frames off an item; objective='next_frame' drops whole oldest context turns "
                             "instead: give one or the other")
        truncate = "reference" if truncate is None else truncate
        if truncate not in ("reference", "keep_context"):
            raise ValueError("truncate must be 'reference' or 'keep_context'")
        for name, tok in (("text_tokenizer", text_tokenizer), ("audio_tokenizer", audio_tokenizer)):
            if not hasattr(tok, "encode"):
                raise TypeError(f"{name} needs an encode() method")
        self.examples, self.text_tokenizer, self.audio_tokenizer = examples, text_tokenizer, audio_tokenizer
        self.max_seq_len, self.truncate = max_seq_len, truncate
        self.objective, self.loss_on = objective, loss_on

    def __len__(self):
        return len(self.examples)

    def _codes(self, audio: torch.Tensor) -> torch.Tensor:
        """Mimi codes ``[K, T]`` int64 (on the CPU) of a mono waveform."""
        codes = self.audio_tokenizer.encode(audio.reshape(1, 1, -1))
        if isinstance(codes, (list, tuple)):
            codes = codes[0]
        if codes.dim() == 3:
            codes = codes[0]
        return codes.detach().to("cpu", torch.long)

    def _tokenize_text_segment(self, text: str, speaker: int):
        ids = self.text_tokenizer.encode(f"[{speaker}]{text}")
        frame = torch.zeros(len(ids), 33, dtype=torch.long)
        mask = torch.zeros(len(ids), 33, dtype=torch.bool)
        frame[:, -1] = torch.as_tensor(ids, dtype=torch.long)
        mask[:, -1] = True
        return frame, mask

    def _tokenize_audio(self, audio: torch.Tensor):
        codes = self._codes(audio)                                                      # [K, T]
        codes = torch.cat([codes, torch.zeros(codes.size(0), 1, dtype=torch.long)], 1)   # + EOS frame
        frame = torch.zeros(codes.size(1), 33, dtype=torch.long)
        mask = torch.zeros(codes.size(1), 33, dtype=torch.bool)
        frame[:, :codes.size(0)] = codes.t()
        mask[:, :-1] = True
        return frame, mask

    def _tokenize_segment(self, text: str, speaker: int, audio: torch.Tensor):
        tt, tm = self._tokenize_text_segment(text, speaker)
        at, am = self._tokenize_audio(audio)
        return torch.cat([tt, at], 0), torch.cat([tm, am], 0)

    def _tokenize_audio_for_target(self, audio: torch.Tensor) -> torch.Tensor:
        return self._codes(audio).t().contiguous()                                       # [T, K]

    def __getitem__(self, idx):
        ex = self.examples[idx]
        toks, masks = [], []
        for ctx in ex.get("context", []):
            t, m = self._tokenize_segment(ctx.text, ctx.speaker_id, ctx.audio)
            toks.append(t)
            masks.append(m)
        target = ex["target"]
        tt, tm = self._tokenize_text_segment(target.text, target.speaker_id)
        toks.append(tt)
        masks.append(tm)
        codes = self._tokenize_audio_for_target(target.audio)
        if self.objective == "next_frame":
            need = tt.size(0) + codes.size(0) + 1
            if need > self.max_seq_len:
                raise ValueError(f"example {idx}: its target alone takes {need} positions ({tt.size(0)} text, {codes.size(0)} "
                                 f"frames, 1 EOS), more than max_seq_len = {self.max_seq_len}")
            while sum(t.size(0) for t in toks) + codes.size(0) + 1 > self.max_seq_len:
                toks.pop(0)                                                              # the oldest context turn, whole
                masks.pop(0)
            return to_next_frame({"input_tokens": torch.cat(toks, 0), "input_masks": torch.cat(masks, 0),
                                  "target_audio_tokens": codes}, self.loss_on)
        tokens, mask = torch.cat(toks, 0), torch.cat(masks, 0)
        if tokens.size(0) > self.max_seq_len:
            keep = min(self.max_seq_len, tt.size(0)) if self.truncate == "reference" else self.max_seq_len
            tokens, mask = tokens[tokens.size(0) - keep:], mask[mask.size(0) - keep:]
        return {"input_tokens": tokens, "input_masks": mask, "target_audio_tokens": codes}

    def lengths(self) -> List[int]:
        """Input length of every item without running the audio tokenizer twice: frames = text ids + ceil(N/1920)+1
        per context turn, and for the target too under ``next_frame`` (an estimate used only for bucketing)."""
        out = []
        for ex in self.examples:
            n = len(self.text_tokenizer.encode(f"[{ex['target'].speaker_id}]{ex['target'].text}"))
            if self.objective == "next_frame":
                n += math.ceil(ex["target"].audio.numel() / 1920) + 1
            for c in ex.get("context", []):
                n += len(self.text_tokenizer.encode(f"[{c.speaker_id}]{c.text}")) + math.ceil(c.audio.numel() / 1920) + 1
            out.append(min(n, self.max_seq_len))
        return out


# ------------------------------------------------------------------------------------------------ collation
def collate_variable_length(batch: List[Dict[str, torch.Tensor]], target_pad: int = 0) -> Dict[str, torch.Tensor]:
    """Zero-pad ``input_tokens`` [S,33] / ``input_masks`` [S,33] / ``target_audio_tokens`` [T,K] to the batch max
    (reference training_data.py:379-408).  ``target_pad=IGNORE_INDEX`` pads the targets with -100 instead, which the
    HIP cross-entropy skips (rows with a negative target contribute neither loss nor gradient and are left out of the
    mean) - the reference's zero padding trains padded rows towards the EOS class."""
    max_s = max(b["input_tokens"].shape[0] for b in batch)
    max_t = max(b["target_audio_tokens"].shape[0] for b in batch)
    n = len(batch)
    k1 = batch[0]["input_tokens"].shape[1]
    k = batch[0]["target_audio_tokens"].shape[1]
    tokens = torch.zeros(n, max_s, k1, dtype=torch.long)
    masks = torch.zeros(n, max_s, k1, dtype=torch.bool)
    targets = torch.full((n, max_t, k), target_pad, dtype=torch.long)
    for i, b in enumerate(batch):
        s, t = b["input_tokens"].shape[0], b["target_audio_tokens"].shape[0]
        tokens[i, :s] = b["input_tokens"]
        masks[i, :s] = b["input_masks"]
        targets[i, :t] = b["target_audio_tokens"]
    out = {"input_tokens": tokens, "input_masks": masks, "target_audio_tokens": targets}
    if any("adapter" in b for b in batch):
        # the adapter set every example trains (multi-speaker LoRA, compute_loss(adapter_ids=...)); an example without one: -1
        out["adapter_ids"] = torch.tensor([int(b.get("adapter", -1)) for b in batch], dtype=torch.long)
    return out


def collate_packed(batch: List[Dict[str, torch.Tensor]], max_seq_len: int = 2048, target_pad: int = IGNORE_INDEX) -> Dict[str, torch.Tensor]:
    """Sequence packing: several examples share one row, each attends only to itself and has RoPE positions of its own (the
    engine's ``segment_lengths`` path), so no position is spent on padding up to the batch maximum.

    First-fit over the examples sorted by decreasing input length (ties keep the batch order: deterministic); rows are opened as
    needed; the row length S is the longest row rounded up to a multiple of 128, capped at ``max_seq_len``.  An example longer than
    ``max_seq_len`` raises.  Returns ``input_tokens`` [R, S, K+1], ``input_masks``, ``target_audio_tokens`` [R, S, K] and
    ``segment_lengths`` [R, n_max] (a row's segment lengths in order, zero-padded) - and, when an example carries an
    ``"adapter"`` (its adapter set, multi-speaker LoRA), ``adapter_ids`` [R, n_max] beside it (-1 where there is no segment).

    Targets follow the position-indexed label convention of ``forward_loss`` (position p is labelled by ``targets[p]``, the last
    position of a sequence by nothing), applied per segment: for example i of input length S_i with T_i target frames at row
    offset o_i, positions o_i + p, p < min(S_i - 1, T_i), carry ``targets_i[p]`` and every other position - each segment's last one
    and the row padding included - carries ``target_pad`` (IGNORE_INDEX: ``model.target_ignore_index`` must be set)."""
    lens = [int(b["input_tokens"].shape[0]) for b in batch]
    for i, n in enumerate(lens):
        if n > max_seq_len:
            raise ValueError(f"example {i} has {n} positions, more than max_seq_len = {max_seq_len}")
        if n < 1:
            raise ValueError(f"example {i} is empty")
    rows: List[List[int]] = []
    room: List[int] = []
    for i in sorted(range(len(batch)), key=lambda i: -lens[i]):   # (sorted is stable: ties keep the batch order)
        r = next((r for r in range(len(rows)) if room[r] >= lens[i]), None)
        if r is None:
            rows.append([])
            room.append(max_seq_len)
            r = len(rows) - 1
        rows[r].append(i)
        room[r] -= lens[i]
    S = min(max_seq_len, -(-max(max_seq_len - x for x in room) // 128) * 128)
    k1 = batch[0]["input_tokens"].shape[1]
    k = batch[0]["target_audio_tokens"].shape[1]
    R = len(rows)
    tokens = torch.zeros(R, S, k1, dtype=torch.long)
    masks = torch.zeros(R, S, k1, dtype=torch.bool)
    targets = torch.full((R, S, k), target_pad, dtype=torch.long)
    seg = torch.zeros(R, max(len(r) for r in rows), dtype=torch.long)
    # per-segment adapter sets (multi-speaker LoRA), only when an example carries one; no segment, or no "adapter": -1
    ads = torch.full(tuple(seg.shape), -1, dtype=torch.long) if any("adapter" in b for b in batch) else None
    for r, members in enumerate(rows):
        o = 0
        for j, i in enumerate(members):
            b, n = batch[i], lens[i]
            t = min(n - 1, int(b["target_audio_tokens"].shape[0]))
            tokens[r, o:o + n] = b["input_tokens"]
            masks[r, o:o + n] = b["input_masks"]
            targets[r, o:o + t] = b["target_audio_tokens"][:t]
            seg[r, j] = n
            if ads is not None:
                ads[r, j] = int(b.get("adapter", -1))
            o += n
    out = {"input_tokens": tokens, "input_masks": masks, "target_audio_tokens": targets, "segment_lengths": seg}
    if ads is not None:
        out["adapter_ids"] = ads
    return out


class LengthBucketSampler(Sampler):
    """Batches of similar length: indices are sorted by length inside windows of ``bucket_batches`` batches, cut into
    batches, and the batches shuffled - so zero padding (and the work spent on it) stays small.  Deterministic per
    (seed, epoch); with ``world_size > 1`` every rank takes every ``world_size``-th batch."""

    def __init__(self, lengths: Sequence[int], batch_size: int, bucket_batches: int = 50, shuffle: bool = True, seed: int = 0,
                 drop_last: bool = False, rank: int = 0, world_size: int = 1):
        self.lengths, self.batch_size, self.bucket_batches = list(lengths), batch_size, bucket_batches
        self.shuffle, self.seed, self.drop_last, self.rank, self.world_size, self.epoch = shuffle, seed, drop_last, rank, world_size, 0

    def set_epoch(self, epoch: int):
        self.epoch = epoch

    def _batches(self) -> List[List[int]]:
        g = torch.Generator().manual_seed(self.seed + self.epoch)
        n = len(self.lengths)
        order = torch.randperm(n, generator=g).tolist() if self.shuffle else list(range(n))
        window = self.batch_size * self.bucket_batches
        batches = []
        for w in range(0, n, window):
            chunk = sorted(order[w:w + window], key=lambda i: self.lengths[i])
            batches += [chunk[i:i + self.batch_size] for i in range(0, len(chunk), self.batch_size)]
        if self.drop_last:
            batches = [b for b in batches if len(b) == self.batch_size]
        if self.shuffle:
            batches = [batches[i] for i in torch.randperm(len(batches), generator=g).tolist()]
        usable = len(batches) - len(batches) % self.world_size
        return batches[self.rank:usable:self.world_size] if self.world_size > 1 else batches

    def __iter__(self) -> Iterator[List[int]]:
        return iter(self._batches())

    def __len__(self):
        return len(self._batches())


def create_dataloader(dataset: Dataset, batch_size: int, shuffle: bool = True, num_workers: int = 2, pin_memory: bool = True,
                      bucket_by_length: bool = False, target_pad: int = 0, pack_sequences: bool = False,
                      max_seq_len: int = 2048) -> DataLoader:
    """Reference ``create_dataloader`` (training_data.py:361-376).  ``bucket_by_length`` swaps the plain shuffle for
    :class:`LengthBucketSampler` (needs ``dataset.lengths()``).  ``pack_sequences`` collates with :func:`collate_packed` into rows
    of at most ``max_seq_len`` positions (``batch_size`` stays the number of examples drawn per step)."""
    from functools import partial
    collate = collate_variable_length if target_pad == 0 else partial(collate_variable_length, target_pad=target_pad)
    if pack_sequences:
        collate = partial(collate_packed, max_seq_len=max_seq_len)
    if bucket_by_length:
        sampler = LengthBucketSampler(dataset.lengths(), batch_size, shuffle=shuffle)
        return DataLoader(dataset, batch_sampler=sampler, num_workers=num_workers, pin_memory=pin_memory, collate_fn=collate)
    return DataLoader(dataset, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers, pin_memory=pin_memory,
                      collate_fn=collate)
