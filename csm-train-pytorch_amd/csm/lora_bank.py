"""A bank of LoRA adapters for one base model: generation with a different adapter per utterance of a batch.

Each entry is a ``LoRAState`` (training/lora.py) - a trainer's live one (``add``) or one read from the ``.safetensors`` +
``_metadata.json`` pair that ``CSMLoRATrainer.save_model(save_mode="lora")`` writes (``load``, generation-only: no gradient
arena).  The decode kernels take the adapters of one call as per-row tables over a shared extension width, so every entry must
have the same layout: ``target_modules``, ``target_layers``, ``use_bias`` and ``r_pad`` (the rank padded to a multiple of 8).
``r`` and ``alpha`` may differ - the kernels take a per-adapter scale alpha / r.
"""
import json
from collections import OrderedDict
from typing import List, Optional

LAYOUT_FIELDS = ("target_modules", "target_layers", "use_bias", "r_pad")


def layout_of(target_modules, target_layers, use_bias, r) -> dict:
    """The fields that fix an adapter set's arena layout, normalised for comparison (module order does not matter: the groups
    order their members themselves)."""
    return {"target_modules": sorted(target_modules), "target_layers": None if target_layers is None else sorted(int(i) for i in target_layers),
            "use_bias": bool(use_bias), "r_pad": (int(r) + 7) // 8 * 8}


def layout_of_metadata(meta: dict) -> dict:
    """``layout_of`` for the ``_metadata.json`` of ``CSMLoRATrainer.save_model``."""
    return layout_of(meta.get("target_modules") or ["q_proj", "v_proj"], meta.get("target_layers"), meta.get("lora_use_bias", False),
                     meta["lora_r"])


def layout_of_state(state) -> dict:
    return layout_of(state.target_modules, state.target_layers, state.use_bias, state.r)


def check_layout(have: dict, new: dict, name: str = "adapter") -> None:
    """Raise a ValueError naming the first field in which ``new`` differs from the bank's ``have``."""
    for f in LAYOUT_FIELDS:
        if have[f] != new[f]:
            raise ValueError(f"LoRA adapter {name!r} does not fit the bank: {f} is {new[f]!r}, the bank's adapters have {have[f]!r} "
                             f"(all adapters of a bank share {', '.join(LAYOUT_FIELDS)})")


class LoRABank:
    """Named adapter sets for one base model (``Generator.add_adapter`` / ``load_adapter``)."""

    def __init__(self, model):
        self.model = model
        self.entries: "OrderedDict[str, object]" = OrderedDict()
        self.layout: Optional[dict] = None

    @property
    def names(self) -> List[str]:
        return list(self.entries)

    def _admit(self, name: str, layout: dict) -> None:
        if not isinstance(name, str) or not name:
            raise ValueError(f"adapter names are non-empty strings, got {name!r}")
        others = [n for n in self.entries if n != name]
        if others:
            check_layout(self.layout, layout, name)

    def add(self, name: str, state):
        """Register ``state`` (a ``LoRAState`` of this model, e.g. a trainer's live one - read in place: later writes to its
        weights are seen by later generations).  A name already present is replaced."""
        if state.merged:
            raise ValueError(f"LoRA adapter {name!r} is merged into the base weights: a bank entry must be un-merged")
        layout = layout_of_state(state)
        self._admit(name, layout)
        self.entries[name] = state
        self.layout = layout
        return state

    def load(self, name: str, path: str):
        """Read an adapter file written by ``CSMLoRATrainer.save_model(save_mode="lora")`` (``path`` with or without the
        ``.safetensors`` suffix; its ``_metadata.json`` beside it) into a generation-only ``LoRAState``."""
        from safetensors.torch import load_file
        from .training.lora import LoRAState
        if not path.endswith(".safetensors"):
            path = path + ".safetensors"
        with open(path[:-len(".safetensors")] + "_metadata.json") as f:
            meta = json.load(f)
        self._admit(name, layout_of_metadata(meta))
        state = LoRAState(self.model, int(meta["lora_r"]), float(meta["lora_alpha"]), 0.0,
                          meta.get("target_modules") or ["q_proj", "v_proj"], meta.get("target_layers"),
                          bool(meta.get("lora_use_bias", False)), grad=False)
        state.training = False
        sd = load_file(path)
        names = dict(state.named_tensors())
        missing = [k for k in names if k not in sd]
        if missing:
            raise ValueError(f"LoRA file {path} lacks {len(missing)} tensors, e.g. {missing[:3]}")
        import torch
        with torch.no_grad():
            for k, dst in names.items():
                if tuple(sd[k].shape) != tuple(dst.shape):
                    raise ValueError(f"LoRA file {path}: {k} has shape {tuple(sd[k].shape)}, expected {tuple(dst.shape)}")
                dst.copy_(sd[k].to(device=dst.device, dtype=dst.dtype))
        return self.add(name, state)

    def get(self, name: str):
        if name not in self.entries:
            raise ValueError(f"unknown LoRA adapter {name!r} (loaded: {self.names})")
        return self.entries[name]

    def resolve(self, names) -> list:
        """One ``LoRAState`` or None per name (None = no adapter)."""
        return [None if n is None else self.get(n) for n in names]
