"""``csm-finetune-lora`` on MI355X: flag names and defaults of reference ``src/csm/cli/finetune_lora.py:32-237``."""
import argparse
import logging

from ..training.dp import init_distributed
from ..training.lora_trainer import CSMLoRATrainer
from .common import add_data_args, load_datasets, objective_of


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Fine-tune CSM with LoRA (MI355X)")
    p.add_argument("--model-path", type=str, required=True, help="checkpoint (.pt or .safetensors); '' = random init")
    p.add_argument("--output-dir", type=str, default="csm_lora")
    add_data_args(p, context_turns=2)   # reference default of csm-finetune-lora
    lo = p.add_argument_group("LoRA")
    lo.add_argument("--lora-r", type=int, default=8)
    lo.add_argument("--lora-alpha", type=float, default=16.0)
    lo.add_argument("--lora-dropout", type=float, default=0.0)
    lo.add_argument("--target-modules", type=str, nargs="+", default=["q_proj", "v_proj"])
    lo.add_argument("--target-layers", type=int, nargs="+", default=None)
    lo.add_argument("--lora-bias", action="store_true")
    t = p.add_argument_group("Training")
    t.add_argument("--learning-rate", type=float, default=1e-4)
    t.add_argument("--semantic-weight", type=float, default=100.0)
    t.add_argument("--acoustic-weight", type=float, default=1.0)
    t.add_argument("--weight-decay", type=float, default=0.01)
    t.add_argument("--batch-size", type=int, default=2)
    t.add_argument("--epochs", type=int, default=5)
    t.add_argument("--val-every", type=int, default=100)
    t.add_argument("--save-every", type=int, default=500)
    t.add_argument("--max-grad-norm", type=float, default=1.0)
    t.add_argument("--resume-from", type=str, default=None)
    t.add_argument("--save-mode", choices=["lora", "full", "both"], default="lora")
    t.add_argument("--acoustic-mode", choices=["off", "all", "amortized"], default="off")
    p.add_argument("--log-level", type=str, default="info")
    p.add_argument("--debug", action="store_true")
    p.add_argument("--generate-samples", action="store_true",
                   help="after saving, write {output-dir}/sample.wav from the trained adapters (needs --mimi-weights, --text-tokenizer)")
    p.add_argument("--sample-prompt", type=str, default="Hello, this is a test of the fine-tuned voice.")
    return p.parse_args(argv)


def sample_tokenizers(args, device):
    """(text tokenizer, Mimi codec) for ``--generate-samples``: the local files ``--text-tokenizer`` / ``--mimi-weights`` stand for
    what the reference downloads (cli/generate.py)."""
    from ..codec import load_mimi
    from ..generator import load_llama3_tokenizer
    text = load_llama3_tokenizer(args.text_tokenizer) if args.text_tokenizer else None
    audio = load_mimi(args.mimi_weights, device=device) if args.mimi_weights else None
    return text, audio


def generate_sample(trainer, args, device):
    """Reference finetune_lora.py:462-476: a sample from the final adapters; a failure is logged, the run still succeeds."""
    path = f"{args.output_dir}/sample.wav"
    try:
        text_tok, audio_tok = sample_tokenizers(args, device)
        trainer.generate_sample(args.sample_prompt, args.speaker_id, path, text_tokenizer=text_tok, audio_tokenizer=audio_tok)
        trainer.logger.info(f"Generated sample: {path}")
    except Exception as e:                         # noqa: BLE001 - a sample is a by-product of the run
        trainer.logger.error(f"Error generating sample: {e}")
        return None
    return path


def main(argv=None):
    args = parse_args(argv)
    rank, world, local = init_distributed()
    model = None
    if not args.model_path:
        from ..models.model import Model
        from ..training.trainer import csm_1b_args
        model = Model(csm_1b_args(), device=f"cuda:{local}", seed=0)
    trainer = CSMLoRATrainer(model_path=args.model_path, output_dir=args.output_dir, learning_rate=args.learning_rate,
                             semantic_weight=args.semantic_weight, acoustic_weight=args.acoustic_weight,
                             weight_decay=args.weight_decay, lora_r=args.lora_r, lora_alpha=args.lora_alpha,
                             lora_dropout=args.lora_dropout, target_modules=args.target_modules,
                             target_layers=args.target_layers, lora_use_bias=args.lora_bias, device=f"cuda:{local}", model=model,
                             objective=objective_of(args)[0])
    trainer.logger.setLevel(logging.DEBUG if args.debug else getattr(logging, args.log_level.upper(), logging.INFO))
    trainer.model.acoustic_mode = args.acoustic_mode
    train_ds, val_ds = load_datasets(args)
    if args.pack_sequences:                        # several examples per row (data.collate_packed); implies the ignore index
        from functools import partial
        from ..data import collate_packed
        from ..data.training_data import IGNORE_INDEX
        trainer.model.target_ignore_index = IGNORE_INDEX
        for ds in (train_ds, val_ds):
            if ds is not None:
                ds.collate = partial(collate_packed, max_seq_len=min(args.max_seq_len, trainer.model.bb.max_seq_len))
    trainer.prepare_optimizer()
    best = trainer.train(train_ds, val_ds, batch_size=args.batch_size, epochs=args.epochs, val_every=args.val_every,
                         save_every=args.save_every, max_grad_norm=args.max_grad_norm, resume_from=args.resume_from)
    if rank == 0:
        trainer.save_model(f"{args.output_dir}/final", args.save_mode)
        trainer.logger.info(f"best validation loss: {best}")
        if args.generate_samples:
            generate_sample(trainer, args, f"cuda:{local}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
