"""Model.fp8_adapters and its command-line / loader spellings, without a GPU (the decode path itself: test_fp8_adapters_gpu.py)."""
import inspect

import pytest


def test_model_fp8_adapters_attribute():
    from csm.models.model import Model, ModelArgs
    m = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", 300, 2051, 4))
    assert m.fp8_adapters is False
    m._decode_state = object()
    m.fp8_adapters = False
    assert m._decode_state is not None, "setting the same value keeps the state"
    m.fp8_adapters = True
    assert m.fp8_adapters is True and m._decode_state is None, "changing the flag drops the decode state (and its graph)"
    assert m.decode_weights == "bf16", "the flag does not switch the mode on"
    assert "bf16 base" in type(m).fp8_adapters.__doc__ and "quantised base" in type(m).fp8_adapters.__doc__
    from csm.generator import load_csm_1b
    assert inspect.signature(load_csm_1b).parameters["fp8_adapters"].default is False


def test_cli_takes_fp8_adapters(capsys):
    from csm.cli.generate import parse_args
    with pytest.raises(SystemExit):
        parse_args(["--help"])
    assert "--fp8-adapters" in capsys.readouterr().out
    base = ["--model-path", "m.pt", "--text", "hi", "--mimi-weights", "w", "--text-tokenizer", "t"]
    assert parse_args(base).fp8_adapters is False
    a = parse_args(base + ["--decode-weights", "fp8", "--fp8-adapters", "--lora-adapter", "voice.safetensors"])
    assert a.fp8_adapters is True and a.decode_weights == "fp8" and a.lora_adapter == "voice.safetensors"
    with pytest.raises(SystemExit):
        parse_args(base + ["--fp8-adapters"])                   # only with --decode-weights fp8


def test_cli_passes_the_flag_to_the_loader(monkeypatch):
    from csm.cli import generate as cli
    seen = {}

    class Stop(Exception):
        pass

    def fake_load(*a, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(cli, "load_csm_1b", fake_load)
    base = ["--model-path", "m.pt", "--text", "hi", "--mimi-weights", "w", "--text-tokenizer", "t"]
    with pytest.raises(Stop):
        cli.main(base + ["--decode-weights", "fp8", "--fp8-adapters"])
    assert seen.get("decode_weights") == "fp8" and seen.get("fp8_adapters") is True
    seen.clear()
    with pytest.raises(Stop):
        cli.main(base + ["--decode-weights", "fp8"])
    assert seen.get("decode_weights") == "fp8" and "fp8_adapters" not in seen
