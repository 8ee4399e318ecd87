"""``MultiSpeakerLoRATrainer`` - API of reference ``src/csm/training/multi_speaker_lora.py`` on MI355X.

The reference builds one ``CSMLoRATrainer`` per speaker and trains them one after the other (multi_speaker_lora.py:137-213,
281-300), so S speakers cost S LoRA runs and the frozen base model is walked S times.  A LoRA step's time is the frozen base
model's, and the rows of a batch never see each other - so here ONE model carries a stack of adapter sets
(``LoRAState(n_adapters=S)``, training/lora.py), every example of a step runs with its own speaker's set
(``compute_loss(adapter_ids=...)``) and the frozen GEMMs, the attention and the heads run once over all of them.

What is kept: the constructor arguments, ``prepare_optimizers``, ``train(speaker_datasets={id: (train, val)}) -> {id: best
validation loss}``, ``save_all_models`` (``speaker_{id}/speaker_{id}_lora.safetensors`` + ``_metadata.json``, the single-adapter
format: ``LoRABank.load`` / ``CSMLoRATrainer.load_lora_weights`` read them), ``load_speaker_model``, ``generate_sample``.

``objective="next_frame"`` (not in the reference): the speakers' examples are ``csm.data.to_next_frame`` items - the ignore
index is set and every padded batch, the validation sets' included, pads its labels with it.

What differs, on purpose:
* the loss of a step is the batch loss - the mean over the labelled rows of the whole batch, whichever speakers they belong to;
* gradient clipping takes ONE norm over the whole stack;
* a speaker absent from a step still takes its Adam step, on a zero gradient (its moments decay, the bias correction advances);
* ``share_backbone`` / ``share_decoder``: the reference's shared trainer is built and saved but never trained
  (multi_speaker_lora.py:147-176 - ``train`` only walks ``self.trainers``), so sharing is refused rather than imitated; both
  default to False.  ``merge_speaker_models`` (an interpolation with that untrained shared part) is not built.
"""
import json
import math
import os
import time
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import torch

from ..models.model import Model
from .dp import GradSync
from .lora import apply_lora_to_model
from .lora_trainer import _to_torch
from .optim import FusedAdamW
from .trainer import csm_1b_args
from .utils import compute_loss, setup_logger


def rotation_draws(sizes: List[int], step: int, batch_size: int) -> List[Tuple[int, int]]:
    """The (speaker index, example index) of every slot of optimiser step ``step``: draw g = step * batch_size + slot goes to
    speaker g mod n, and is that speaker's (g div n)-th draw, which walks its ``sizes[speaker]`` examples in order, wrapping.
    Speakers without examples are left out of the rotation."""
    live = [i for i, n in enumerate(sizes) if n > 0]
    if not live:
        raise ValueError("no speaker has a training example")
    out = []
    for slot in range(batch_size):
        g = step * batch_size + slot
        sp = live[g % len(live)]
        out.append((sp, (g // len(live)) % sizes[sp]))
    return out


class MultiSpeakerLoRATrainer:
    """Fine-tunes one LoRA adapter set per speaker in a single run (reference multi_speaker_lora.py:29)."""

    def __init__(self, model_path: str, output_dir: str, speaker_ids: List[int], log_file: Optional[str] = None,
                 learning_rate: float = 1e-4, semantic_weight: float = 100.0, acoustic_weight: float = 1.0,
                 weight_decay: float = 0.01, lora_r: int = 8, lora_alpha: float = 16.0, lora_dropout: float = 0.0,
                 share_backbone: bool = False, share_decoder: bool = False, target_modules: Optional[List[str]] = None,
                 target_backbone_layers: Optional[List[int]] = None, target_decoder_layers: Optional[List[int]] = None,
                 lora_use_bias: bool = False, device: str = "cuda", model: Optional[Model] = None,
                 pack_sequences: bool = False, max_seq_len: int = 2048, seed: int = 0, objective: str = "reference"):
        from ..data.training_data import check_objective
        self.objective = check_objective(objective)      # (not in the reference) "next_frame": data.to_next_frame items
        if share_backbone or share_decoder:
            raise NotImplementedError("share_backbone / share_decoder: the reference's shared adapters are created and saved but "
                                      "never trained; train every speaker's own adapters (the default here) instead")
        if target_decoder_layers is not None and target_decoder_layers != target_backbone_layers:
            raise NotImplementedError("one layer list serves both stacks (LoRAState.target_layers): give target_backbone_layers "
                                      "alone, or the same list twice")
        if len(set(speaker_ids)) != len(speaker_ids) or not speaker_ids:
            raise ValueError(f"speaker_ids must be distinct and non-empty, got {speaker_ids}")
        if GradSync.active():
            raise NotImplementedError("multi-speaker LoRA under a process group is not built: run it in one process")
        self.model_path = model_path
        self.output_dir = Path(output_dir)
        self.output_dir.mkdir(parents=True, exist_ok=True)
        self.speaker_ids = list(speaker_ids)
        self.index = {sid: a for a, sid in enumerate(self.speaker_ids)}      # speaker id -> adapter set of the stack
        self.logger = setup_logger("multi_speaker_lora_trainer", log_file or str(self.output_dir / "multi_speaker_training.log"))
        self.learning_rate, self.semantic_weight, self.acoustic_weight = learning_rate, semantic_weight, acoustic_weight
        self.weight_decay = weight_decay
        self.lora_r, self.lora_alpha, self.lora_dropout = lora_r, lora_alpha, lora_dropout
        self.target_modules = target_modules or ["q_proj", "v_proj"]
        self.target_backbone_layers, self.target_decoder_layers = target_backbone_layers, target_decoder_layers
        self.lora_use_bias = lora_use_bias
        self.share_backbone, self.share_decoder = False, False
        self.pack_sequences, self.max_seq_len = pack_sequences, max_seq_len
        self.device = device
        self.model = model
        if self.model is None:
            self.model = Model(csm_1b_args(), device=device)
            if model_path:
                if model_path.endswith(".safetensors"):
                    from safetensors.torch import load_file
                    sd = load_file(model_path)
                else:
                    sd = torch.load(model_path, map_location="cpu", weights_only=False)
                    if isinstance(sd, dict) and "model" in sd and isinstance(sd["model"], dict):
                        sd = sd["model"]
                self.model.load_state_dict(sd)
        # one stack; set a starts as a single-adapter run with seed + a would (LoRAState)
        apply_lora_to_model(self.model, r=lora_r, alpha=lora_alpha, dropout=lora_dropout, target_modules=self.target_modules,
                            target_layers=target_backbone_layers, use_bias=lora_use_bias, seed=seed,
                            n_adapters=len(self.speaker_ids))
        if pack_sequences or self.objective == "next_frame":   # unlabelled positions by construction: the ignore index
            from ..data.training_data import IGNORE_INDEX
            self.model.target_ignore_index = IGNORE_INDEX
        self.logger.info(f"{len(self.speaker_ids)} speakers {self.speaker_ids}: one stack of adapter sets, r={lora_r}, "
                         f"alpha={lora_alpha}, modules {self.target_modules}")
        self.optimizer = None
        self.max_grad_norm = 0.0
        self.epoch = 0
        self.global_step = 0
        self.best_loss = float("inf")
        self.best_losses: Dict[int, float] = {}

    # ------------------------------------------------------------------------------------------------ optimiser
    def prepare_optimizers(self):
        """One ``FusedAdamW`` over the stack's arena (reference: one Adam per speaker, multi_speaker_lora.py:215-223)."""
        if self.optimizer is None:
            self.optimizer = FusedAdamW(self.model, {}, lora_lr=self.learning_rate, lora_weight_decay=0.0)
            self.logger.info(f"Training {self.model.lora.num_params():,} LoRA parameters in {len(self.speaker_ids)} adapter sets")

    # ------------------------------------------------------------------------------------------------ batches
    def _collate(self, items):
        from ..data.training_data import IGNORE_INDEX, collate_packed, collate_variable_length
        if self.pack_sequences:
            return collate_packed(items, max_seq_len=min(self.max_seq_len, self.model.bb.max_seq_len))
        pad = IGNORE_INDEX if getattr(self.model, "target_ignore_index", None) is not None else 0
        return collate_variable_length(items, target_pad=pad)

    def draw_batch(self, train_sets, step: int, batch_size: int):
        """The batch of optimiser step ``step``: ``batch_size`` examples, the speakers in rotation (``rotation_draws``), each
        carrying its adapter set - padded to the longest, or packed under ``pack_sequences``."""
        items = []
        for sp, ex in rotation_draws([len(d) for d in train_sets], step, batch_size):
            it = dict(train_sets[sp][ex])
            it["adapter"] = sp
            items.append(it)
        return self._collate(items)

    def train_step(self, batch):
        """One ``compute_loss(adapter_ids=...)``, one backward, one clip over the whole stack, one Adam step."""
        self.prepare_optimizers()
        m = self.model
        loss, _ = compute_loss(m, _to_torch(batch["input_tokens"]), _to_torch(batch["input_masks"]),
                               _to_torch(batch["target_audio_tokens"]), self.semantic_weight, self.acoustic_weight,
                               segment_lengths=batch.get("segment_lengths"), adapter_ids=batch["adapter_ids"])
        m.engine.backward(1.0)
        if self.max_grad_norm and self.max_grad_norm > 0:
            self.optimizer.clip_grad_norm(self.max_grad_norm)
        self.optimizer.step(zero_grad=True)
        return loss.detach()

    def _validate(self, a: int, val_dataset, batch_size: int) -> float:
        """A speaker's validation loss: its own set, every example with its adapter set (at most 10 batches, as
        ``CSMLoRATrainer._validate``)."""
        n = min(10, len(val_dataset) // batch_size)
        total = 0.0
        with torch.no_grad():
            for i in range(n):
                b = val_dataset.get_batch(i, batch_size)
                seg = b.get("segment_lengths")
                if seg is not None:
                    seg_t = torch.as_tensor(seg)
                    ids = torch.where(seg_t > 0, torch.full_like(seg_t, a), torch.full_like(seg_t, -1))
                else:
                    ids = torch.full((_to_torch(b["input_tokens"]).shape[0],), a, dtype=torch.long)
                loss, _ = compute_loss(self.model, _to_torch(b["input_tokens"]), _to_torch(b["input_masks"]),
                                       _to_torch(b["target_audio_tokens"]), self.semantic_weight, self.acoustic_weight,
                                       segment_lengths=seg, adapter_ids=ids)
                total += float(loss)
        return total / max(1, n)

    # ------------------------------------------------------------------------------------------------ training
    def train(self, speaker_datasets: Dict[int, Tuple], batch_size: int = 2, epochs: int = 5, val_every: int = 100,
              save_every: int = 500, max_grad_norm: float = 1.0, resume_from: Optional[Dict[int, str]] = None) -> Dict[int, float]:
        """Reference multi_speaker_lora.py:225-314.  ``speaker_datasets`` = {speaker id: (train, val)}; a train set answers
        ``len`` and ``[i]`` (one tokenised example), a validation set ``len`` and ``get_batch(i, batch_size)`` (or is None).  An
        epoch is as many steps as the speakers' examples fill batches.  Returns {speaker id: best validation loss}."""
        for sid in self.speaker_ids:
            if sid not in speaker_datasets:
                self.logger.warning(f"No dataset provided for speaker {sid}")
        unknown = [sid for sid in speaker_datasets if sid not in self.index]
        if unknown:
            raise ValueError(f"datasets for speakers {unknown} that are not among speaker_ids {self.speaker_ids}")
        self.prepare_optimizers()
        self.max_grad_norm = max_grad_norm
        self.logger.info(f"Objective: {self.objective}")
        if self.objective == "next_frame":               # the validation sets collate themselves (get_batch): pad with the ignore index
            from ..data.training_data import pad_with_ignore_index
            for _, val in speaker_datasets.values():
                pad_with_ignore_index(val)
        for sid, path in (resume_from or {}).items():
            self.load_speaker_model(sid, path)

        class _Empty:
            def __len__(self):
                return 0

        train_sets = [speaker_datasets[sid][0] if sid in speaker_datasets else _Empty() for sid in self.speaker_ids]
        steps_per_epoch = sum(len(d) for d in train_sets) // batch_size
        for epoch in range(self.epoch, self.epoch + epochs):
            t0 = time.time()
            losses = []
            for _ in range(steps_per_epoch):
                losses.append(self.train_step(self.draw_batch(train_sets, self.global_step, batch_size)))
                self.global_step += 1
                if self.global_step % val_every == 0:
                    self._validate_all(speaker_datasets, batch_size)
                if self.global_step % save_every == 0:
                    for sid in self.speaker_ids:
                        self._save_adapter(sid, str(self.output_dir / f"speaker_{sid}" / f"checkpoint_step_{self.global_step}"))
            avg = float(torch.stack(losses).mean()) if losses else float("nan")
            if losses and not math.isfinite(avg):
                raise FloatingPointError(f"non-finite training loss in epoch {epoch + 1}")
            self.logger.info(f"Epoch {epoch + 1} completed in {time.time() - t0:.2f}s, Avg Loss: {avg:.6f}")
            self.epoch = epoch + 1
        self.save_all_models()
        return {sid: self.best_losses.get(sid, float("inf")) for sid in self.speaker_ids if sid in speaker_datasets}

    def _validate_all(self, speaker_datasets, batch_size):
        for sid, (_, val) in speaker_datasets.items():
            if val is None or len(val) < batch_size:
                continue
            v = self._validate(self.index[sid], val, batch_size)
            self.logger.info(f"Step {self.global_step}, speaker {sid} Val Loss: {v:.6f}")
            if v < self.best_losses.get(sid, float("inf")):
                self.best_losses[sid] = v
                self._save_adapter(sid, str(self.output_dir / f"speaker_{sid}" / "best"))
        if self.best_losses:
            self.best_loss = min(self.best_losses.values())

    # ------------------------------------------------------------------------------------------------ files
    def _save_adapter(self, speaker_id: int, path: str) -> str:
        """A speaker's adapter set in the single-adapter file format of ``CSMLoRATrainer.save_model(save_mode="lora")``."""
        from safetensors.torch import save_file
        lo = self.model.lora
        base = path[:-len(".safetensors")] if path.endswith(".safetensors") else path
        os.makedirs(os.path.dirname(base) or ".", exist_ok=True)
        tensors = {k: v.detach().cpu().contiguous() for k, v in lo.named_tensors(adapter=self.index[speaker_id])}
        save_file(tensors, base + ".safetensors")
        meta = {"lora_r": self.lora_r, "lora_alpha": self.lora_alpha, "lora_dropout": self.lora_dropout,
                "target_modules": lo.target_modules, "target_layers": self.target_backbone_layers,
                "lora_use_bias": self.lora_use_bias, "params_count": sum(t.numel() for t in tensors.values()),
                "speaker_id": speaker_id}
        with open(base + "_metadata.json", "w") as f:
            json.dump(meta, f, indent=2)
        return base + ".safetensors"

    def save_all_models(self) -> Dict[int, str]:
        """Reference multi_speaker_lora.py:316-330: ``speaker_{id}/speaker_{id}_lora.safetensors`` for every speaker."""
        out = {}
        for sid in self.speaker_ids:
            out[sid] = self._save_adapter(sid, str(self.output_dir / f"speaker_{sid}" / f"speaker_{sid}_lora.safetensors"))
            self.logger.info(f"Saved model for speaker {sid} to {out[sid]}")
        return out

    def load_speaker_model(self, speaker_id: int, checkpoint_path: str):
        """Reference multi_speaker_lora.py:332-345: a single-adapter file into the speaker's set of the stack."""
        from safetensors.torch import load_file
        if speaker_id not in self.index:
            raise ValueError(f"no adapter set for speaker {speaker_id} (speakers: {self.speaker_ids})")
        if not checkpoint_path.endswith(".safetensors"):
            checkpoint_path = checkpoint_path + ".safetensors"
        sd = load_file(checkpoint_path)
        names = dict(self.model.lora.named_tensors(adapter=self.index[speaker_id]))
        missing = [k for k in names if k not in sd]
        if missing:
            raise KeyError(f"LoRA file lacks {len(missing)} tensors, e.g. {missing[:3]}")
        lo, opt = self.model.lora, self.optimizer
        tracked = opt is not None and "lora" in opt.state
        with torch.no_grad():
            # the fp32 masters of the OTHER speakers keep their low halves: only the loaded set's elements are re-seeded
            master = opt.master("lora").clone() if tracked else None
            loaded = torch.zeros(lo.arena.numel(), dtype=torch.bool, device=lo.arena.device)
            for k, dst in names.items():
                dst.copy_(sd[k].to(device=dst.device, dtype=dst.dtype))
                torch.as_strided(loaded, dst.size(), dst.stride(), dst.storage_offset() - lo.arena.storage_offset()).fill_(True)
            if tracked:
                opt.set_master("lora", torch.where(loaded, lo.arena.float(), master))

    # ------------------------------------------------------------------------------------------------ samples
    def generate_sample(self, text: str, speaker_id: int, output_path: Optional[str] = None, *, text_tokenizer=None,
                        audio_tokenizer=None, max_audio_length_ms: float = 10_000, temperature: float = 0.9, topk: int = 50) -> str:
        """Reference multi_speaker_lora.py:347-376: speech with one speaker's adapters.  The set is exported (a copy) and spoken
        with as a bank entry, through the per-row adapter path (``row_lora``); the stack stays attached for training."""
        from ..generator import Generator
        if speaker_id not in self.index:
            raise ValueError(f"no adapter set for speaker {speaker_id} (speakers: {self.speaker_ids})")
        if output_path is None:
            output_path = str(self.output_dir / f"speaker_{speaker_id}" / f"sample_{int(time.time())}.wav")
        state = self.model.lora.export(self.index[speaker_id])
        stack = self.model.lora
        self.model.lora = None                    # generation with bank adapters wants no live adapters beside them
        try:
            gen = Generator(self.model, text_tokenizer=text_tokenizer, audio_tokenizer=audio_tokenizer)
            name = f"speaker_{speaker_id}"
            gen.add_adapter(name, state)
            audio = gen.generate(text=text, speaker=speaker_id, context=[], max_audio_length_ms=max_audio_length_ms,
                                 temperature=temperature, topk=topk, adapter=name)
        finally:
            self.model.reset_caches()
            self.model.lora = stack
        os.makedirs(os.path.dirname(output_path) or ".", exist_ok=True)
        gen.save_wav(output_path, audio)
        self.logger.info(f"Sample for speaker {speaker_id} written to {output_path}")
        return output_path
