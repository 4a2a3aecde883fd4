"""Drop-in mirrors of the reference `src/models` scoring surface (`src/models/__init__.py:3-15`)."""
from .lightgcn import LightGCN
from .matrix_factorization import MatrixFactorization
from .neural_cf import NeuralCF
from .popularity import PopularityBaseline
from .segment_popularity import SegmentPopularity, age_segments
from .base import UserHistory, UserSequence
from .item_cf import ItemCF, WeightedItemCF
from .content_knn import ContentKNN
from .sequential_cf import SequentialCF
from .implicit_als import ImplicitALS
from .wide_deep import WideDeep
from .ensemble import Ensemble
from .reranker import Reranker

__all__ = ["NeuralCF", "LightGCN", "WideDeep", "MatrixFactorization", "PopularityBaseline",
           "ItemCF", "WeightedItemCF", "ContentKNN", "ImplicitALS", "UserHistory", "Ensemble",
           "SegmentPopularity", "age_segments", "Reranker", "SequentialCF", "UserSequence"]
