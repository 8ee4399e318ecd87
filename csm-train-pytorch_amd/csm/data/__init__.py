"""Data loading and processing for CSM (mirror of reference ``src/csm/data/__init__.py``)."""
from .training_data import (
    TrainingExample,
    CSMDataProcessor,
    ContextualExampleGenerator,
    CSMDataset,
    LengthBucketSampler,
    create_dataloader,
    collate_variable_length,
    collate_packed,
    load_audio,
    resample,
    IGNORE_INDEX,
    next_frame_labels,
    to_next_frame,
    is_next_frame,
)
from .synthetic import SyntheticCSMDataset

__all__ = ["TrainingExample", "CSMDataProcessor", "ContextualExampleGenerator", "CSMDataset", "LengthBucketSampler",
           "create_dataloader", "collate_variable_length", "collate_packed", "load_audio", "resample", "SyntheticCSMDataset",
           "IGNORE_INDEX", "next_frame_labels", "to_next_frame", "is_next_frame"]
