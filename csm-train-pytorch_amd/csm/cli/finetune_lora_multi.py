"""``csm-finetune-lora-multi`` on MI355X: flag names and defaults of reference ``src/csm/cli/finetune_lora_multi.py:34-221``.

The reference walks the speakers of ``--speakers-config`` one after the other, a whole ``CSMLoRATrainer`` run each
(finetune_lora_multi.py:558-567).  Here all of them train in ONE run - one base model, a stack of adapter sets, every example
with its own speaker's set (``MultiSpeakerLoRATrainer``) - so the per-speaker overrides of the rank, the modules, the learning
rate and the epochs that the reference's config allows are refused: one stack has one layout and one optimiser.

``--speakers-config``: a JSON list of {"name", "speaker_id", and one data source: "audio_dir" + "transcript_dir"
(+ "alignment_dir"), "token_file", or "synthetic": N}; optionally "objective" ("reference" | "next-frame") and "loss_on"
("target" | "all") in place of the run's ``--objective`` / ``--loss-on``.
"""
import argparse
import json
import logging
import os
import time

from .common import add_objective_args, load_datasets, objective_of

PER_SPEAKER_REFUSED = ("lora_r", "lora_alpha", "lora_dropout", "learning_rate", "epochs", "target_modules", "batch_size", "save_mode")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Fine-tune CSM with one LoRA adapter set per speaker, in one run (MI355X)")
    p.add_argument("--model-path", type=str, required=True, help="checkpoint (.pt or .safetensors); '' = random init")
    p.add_argument("--output-dir", type=str, required=True)
    p.add_argument("--speakers-config", type=str, required=True, help="JSON list of speaker configurations")
    lo = p.add_argument_group("LoRA")
    lo.add_argument("--lora-r", type=int, default=8)
    lo.add_argument("--lora-alpha", type=float, default=16.0)
    lo.add_argument("--lora-dropout", type=float, default=0.0)
    lo.add_argument("--target-modules", type=str, nargs="+", default=None)
    lo.add_argument("--target-layers", type=int, nargs="+", default=None)
    lo.add_argument("--lora-bias", action="store_true")
    t = p.add_argument_group("Training")
    t.add_argument("--learning-rate", type=float, default=1e-4)
    t.add_argument("--semantic-weight", type=float, default=100.0)
    t.add_argument("--acoustic-weight", type=float, default=1.0)
    t.add_argument("--weight-decay", type=float, default=0.01,
                   help="kept for the reference's command lines; not applied: the adapters train without weight decay, as in csm-finetune-lora")
    t.add_argument("--batch-size", type=int, default=2, help="examples per optimiser step, the speakers in rotation")
    t.add_argument("--epochs", type=int, default=5)
    t.add_argument("--val-every", type=int, default=100)
    t.add_argument("--save-every", type=int, default=500)
    t.add_argument("--max-grad-norm", type=float, default=1.0)
    t.add_argument("--acoustic-mode", choices=["off", "all", "amortized"], default="off")
    d = p.add_argument_group("Data")
    d.add_argument("--val-split", type=float, default=0.1)
    d.add_argument("--max-seq-len", type=int, default=2048)
    d.add_argument("--context-turns", type=int, default=2)
    d.add_argument("--mimi-weights", type=str, default=None, help="local Mimi weights (for audio_dir speakers and samples)")
    d.add_argument("--text-tokenizer", type=str, default=None, help="local directory of the Llama-3.2 tokenizer files")
    d.add_argument("--pack-sequences", action="store_true", help="pack several examples (of any speakers) into each row")
    add_objective_args(d)                             # a speaker entry may override either one ("objective", "loss_on")
    p.add_argument("--save-mode", choices=["lora", "full", "both"], default="lora",
                   help="only 'lora' (one adapter file per speaker): a merged model is one speaker's - merge a speaker's file with "
                        "csm-finetune-lora --resume-from FILE --epochs 0 --save-mode full")
    p.add_argument("--log-level", type=str, choices=["debug", "info", "warning", "error", "critical"], default="info")
    p.add_argument("--generate-samples", action="store_true")
    p.add_argument("--sample-prompt", type=str, default="This is a test of the fine-tuned voice model.")
    p.add_argument("--debug", action="store_true")
    p.add_argument("--sample-speakers", type=int, default=None, help="train only the first N speakers of the config")
    return p.parse_args(argv)


def load_speaker_configs(path: str, sample_n=None):
    """Reference finetune_lora_multi.py:257-307 (the first N instead of a random N: a run is reproducible)."""
    with open(path) as f:
        configs = json.load(f)
    if not isinstance(configs, list) or not configs:
        raise ValueError(f"{path}: expected a non-empty JSON list of speaker configurations")
    for i, c in enumerate(configs):
        for field in ("name", "speaker_id"):
            if field not in c:
                raise ValueError(f"Speaker config {i} missing required field: {field}")
        if not (("audio_dir" in c and "transcript_dir" in c) or "token_file" in c or c.get("synthetic")):
            raise ValueError(f"Speaker config {i} ({c['name']}): give audio_dir + transcript_dir, token_file or synthetic")
        for field in ("audio_dir", "transcript_dir", "alignment_dir", "token_file"):
            if c.get(field) and not os.path.exists(c[field]):
                raise ValueError(f"Speaker config {i} ({c['name']}): {field} does not exist: {c[field]}")
        refused = [k for k in PER_SPEAKER_REFUSED if k in c]
        if refused:
            raise ValueError(f"Speaker config {i} ({c['name']}): per-speaker {refused} - the speakers share one stack of adapter "
                             "sets and one optimiser; set these for the whole run (flags), or run such a speaker alone with "
                             "csm-finetune-lora")
    if len({c["speaker_id"] for c in configs}) != len(configs):
        raise ValueError(f"{path}: speaker_id values must be distinct")
    return configs[:sample_n] if sample_n else configs


def speaker_datasets_of(configs, args):
    """{speaker id: (train, val)} through the data plumbing of the single-speaker CLIs (cli/common.py load_datasets)."""
    out = {}
    for c in configs:
        ns = argparse.Namespace(token_file=c.get("token_file"), synthetic=int(c.get("synthetic", 0)), max_seq_len=args.max_seq_len,
                                val_split=c.get("val_split", args.val_split), audio_dir=c.get("audio_dir"),
                                transcript_dir=c.get("transcript_dir"), alignment_dir=c.get("alignment_dir"),
                                speaker_id=c["speaker_id"], mimi_weights=args.mimi_weights, text_tokenizer=args.text_tokenizer,
                                context_turns=c.get("context_turns", args.context_turns), **speaker_objective(c, args))
        out[c["speaker_id"]] = load_datasets(ns)
    return out


def speaker_objective(c, args):
    """{"objective", "loss_on"} of a speaker entry: its own, else the run's flags."""
    return dict(objective=c.get("objective", getattr(args, "objective", "reference")),
                loss_on=c.get("loss_on", getattr(args, "loss_on", "target")))


def run_objective(configs, args):
    """What the trainer is told: ``next_frame`` as soon as one speaker's examples are in that form (the ignore index they need
    leaves the other speakers' losses as they are, up to the padding it takes out)."""
    objs = {objective_of(argparse.Namespace(**speaker_objective(c, args)))[0] for c in configs}
    return "next_frame" if "next_frame" in objs else "reference"


def main(argv=None):
    from ..training.multi_speaker_lora import MultiSpeakerLoRATrainer
    args = parse_args(argv)
    if args.save_mode != "lora":
        raise SystemExit(f"--save-mode {args.save_mode}: this run writes one adapter file per speaker and no merged model (a merged model "
                         "is one speaker's): merge a speaker's file afterwards with csm-finetune-lora --resume-from "
                         "OUTPUT_DIR/speaker_ID/speaker_ID_lora.safetensors --epochs 0 --save-mode full")
    configs = load_speaker_configs(args.speakers_config, args.sample_speakers)
    model = None
    if not args.model_path:
        from ..models.model import Model
        from ..training.trainer import csm_1b_args
        model = Model(csm_1b_args(), device="cuda:0", seed=0)
    trainer = MultiSpeakerLoRATrainer(model_path=args.model_path, output_dir=args.output_dir,
                                      speaker_ids=[c["speaker_id"] for c in configs], learning_rate=args.learning_rate,
                                      semantic_weight=args.semantic_weight, acoustic_weight=args.acoustic_weight,
                                      weight_decay=args.weight_decay, lora_r=args.lora_r, lora_alpha=args.lora_alpha,
                                      lora_dropout=args.lora_dropout, target_modules=args.target_modules,
                                      target_backbone_layers=args.target_layers, lora_use_bias=args.lora_bias, device="cuda:0",
                                      model=model, pack_sequences=args.pack_sequences, max_seq_len=args.max_seq_len,
                                      objective=run_objective(configs, args))
    trainer.logger.setLevel(logging.DEBUG if args.debug else getattr(logging, args.log_level.upper(), logging.INFO))
    trainer.model.acoustic_mode = args.acoustic_mode
    datasets = speaker_datasets_of(configs, args)
    if args.pack_sequences:                           # the validation sets collate themselves (get_batch)
        from functools import partial
        from ..data import collate_packed
        for _, val in datasets.values():
            if val is not None and hasattr(val, "collate"):
                val.collate = partial(collate_packed, max_seq_len=min(args.max_seq_len, trainer.model.bb.max_seq_len))
    t0 = time.time()
    best = trainer.train(datasets, batch_size=args.batch_size, epochs=args.epochs, val_every=args.val_every,
                         save_every=args.save_every, max_grad_norm=args.max_grad_norm)
    results = []
    tokenizers = None
    if args.generate_samples:
        try:
            from .finetune_lora import sample_tokenizers
            tokenizers = sample_tokenizers(args, "cuda:0")      # once: the text tokenizer and the Mimi codec serve every speaker
        except Exception as e:                        # noqa: BLE001 - a sample is a by-product of the run
            trainer.logger.error(f"Error loading the tokenizers for the samples: {e}")
    for c in configs:
        sid = c["speaker_id"]
        path = str(trainer.output_dir / f"speaker_{sid}" / f"speaker_{sid}_lora.safetensors")
        r = {"speaker_name": c["name"], "speaker_id": sid, "best_loss": float(best.get(sid, float("inf"))), "model_path": path,
             "success": True}
        if tokenizers is not None:
            try:
                text_tok, audio_tok = tokenizers
                r["sample"] = trainer.generate_sample(c.get("sample_prompt", args.sample_prompt), sid,
                                                      str(trainer.output_dir / f"speaker_{sid}" / f"{c['name']}_sample.wav"),
                                                      text_tokenizer=text_tok, audio_tokenizer=audio_tok)
            except Exception as e:                    # noqa: BLE001 - a sample is a by-product of the run
                trainer.logger.error(f"Error generating sample for speaker {sid}: {e}")
        results.append(r)
    with open(os.path.join(args.output_dir, "multi_speaker_results.json"), "w") as f:
        json.dump({"date": time.strftime("%Y-%m-%d %H:%M:%S"), "num_speakers": len(configs), "training_time": time.time() - t0,
                   "speaker_results": results, "args": vars(args)}, f, indent=2)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
