"""/root/reference/point_vs/preprocessing/data_loaders.py on this path: the sampling / batching side (:170-186
class-balancing sampler, :512-520 loader) and the parquet data-root dataset (:33-520), whose complexes are built on the
GPU from a resident pool (pointvs_amd/parquet_data.py)."""
from pointvs_amd.data_loaders import GraphLoader, RankWeightedSampler, class_balance_weights  # noqa: F401
from pointvs_amd.parquet_data import (PygPointCloudDataset, SynthPharmDataset, classification_types_to_lists,  # noqa: F401
                                      get_data_loader, regression_types_to_lists)

classifiaction_types_to_lists = classification_types_to_lists      # (the reference's spelling)
