"""Per-utterance LoRA adapters, the host side: csm-generate's --lora-adapter flag and the bank's layout validation on plain
metadata dicts (what CSMLoRATrainer.save_model writes beside an adapter file)."""
import pytest

from csm.cli import generate as cli
from csm.lora_bank import LAYOUT_FIELDS, check_layout, layout_of, layout_of_metadata


def _args(*extra):
    return cli.parse_args(["--model-path", "m.pt", "--text", "hi", "--mimi-weights", "m.safetensors", "--text-tokenizer", "tok",
                           *extra])


def test_lora_adapter_flag_parses():
    a = _args("--lora-adapter", "out/adapter.safetensors", "--stream")
    assert a.lora_adapter == "out/adapter.safetensors" and a.stream
    assert _args().lora_adapter is None


def _meta(**kw):
    m = {"lora_r": 8, "lora_alpha": 16.0, "lora_dropout": 0.0, "target_modules": ["q_proj", "v_proj"], "target_layers": None,
         "lora_use_bias": False, "params_count": 1}
    m.update(kw)
    return m


def test_layout_from_metadata():
    lay = layout_of_metadata(_meta())
    assert set(lay) == set(LAYOUT_FIELDS)
    assert lay == {"target_modules": ["q_proj", "v_proj"], "target_layers": None, "use_bias": False, "r_pad": 8}
    # r and alpha may differ under one padded rank; module order does not matter
    same = [_meta(lora_r=5, lora_alpha=3.0), _meta(lora_r=1), _meta(target_modules=["v_proj", "q_proj"])]
    for m in same:
        check_layout(lay, layout_of_metadata(m))
    assert layout_of_metadata(_meta(lora_r=9))["r_pad"] == 16
    assert layout_of(["w2"], [1, 0], True, 16)["target_layers"] == [0, 1]


@pytest.mark.parametrize("field,meta", [
    ("target_modules", _meta(target_modules=["q_proj", "k_proj", "v_proj"])),
    ("target_layers", _meta(target_layers=[0])),
    ("use_bias", _meta(lora_use_bias=True)),
    ("r_pad", _meta(lora_r=12)),
])
def test_layout_mismatch_names_the_field(field, meta):
    with pytest.raises(ValueError, match=field):
        check_layout(layout_of_metadata(_meta()), layout_of_metadata(meta), "voice")
