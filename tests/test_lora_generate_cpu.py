"""csm-finetune-lora: the sample-generation flags (reference finetune_lora.py) parse, and a sample failure is logged without
failing the run."""
import logging

from csm.cli import finetune_lora as cli


def test_generate_sample_flags_parse():
    a = cli.parse_args(["--model-path", "", "--generate-samples", "--sample-prompt", "hi there", "--speaker-id", "3",
                        "--mimi-weights", "m.safetensors", "--text-tokenizer", "tokdir"])
    assert a.generate_samples and a.sample_prompt == "hi there" and a.speaker_id == 3
    assert a.mimi_weights == "m.safetensors" and a.text_tokenizer == "tokdir"
    d = cli.parse_args(["--model-path", ""])
    assert not d.generate_samples and d.mimi_weights is None and d.text_tokenizer is None


def test_sample_failure_is_logged_not_raised(tmp_path, caplog):
    class Trainer:
        logger = logging.getLogger("lora_generate_cpu_test")

        def generate_sample(self, *a, **k):
            raise RuntimeError("no codec")

    args = cli.parse_args(["--model-path", "", "--output-dir", str(tmp_path), "--generate-samples"])
    with caplog.at_level(logging.ERROR, logger="lora_generate_cpu_test"):
        assert cli.generate_sample(Trainer(), args, "cpu") is None
    assert "no codec" in caplog.text
