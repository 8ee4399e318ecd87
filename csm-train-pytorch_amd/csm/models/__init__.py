from .model import (Model, ModelArgs, sample_filtered_rows, sample_processed_rows, sample_topk, sample_topk_rows,  # noqa: F401
                    sample_typical_rows)
