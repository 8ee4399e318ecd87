from .model import Model, ModelArgs, sample_topk, sample_topk_rows  # noqa: F401
