"""MI355X-native top-N scoring path of hyunlord/hnm_recommendation.

Embedding lookup -> all-items scoring (NeuralCF / LightGCN / Wide&Deep / MF) -> top-K, and
the popularity baseline's fit and per-user top-K, and item-based collaborative filtering
(co-occurrence fit, per-user and per-basket top-K), and implicit-feedback ALS (Gram matrix
and per-row Cholesky solves: the fit, fold-in of a basket), and the fusion of several models'
top-K lists into one (an ensemble: reciprocal rank fusion, weighted scores, cascade), and
item-attribute nearest neighbours (a dense all-pairs fit: the answer for articles without purchases),
and popular lists per user segment (the answer for customers without purchases),
and two-stage serving (the recall models' candidates merged per user and re-scored by a neural
ranker),
and directed next-purchase transitions (a counting fit over the time-ordered purchase sequences),
as hand-written gfx950 HIP kernels behind the C ABI in include/hnm.h (libhnm_mi355x.so),
exposed through modules that mirror the reference's `src/models` surface.
"""
from .evaluation import RecommendationMetrics
from .models import (ContentKNN, Ensemble, ImplicitALS, ItemCF, LightGCN, MatrixFactorization, NeuralCF,
                     PopularityBaseline, Reranker, SegmentPopularity, SequentialCF, UserHistory,
                     UserSequence, WeightedItemCF, WideDeep, age_segments)

__all__ = ["NeuralCF", "LightGCN", "WideDeep", "MatrixFactorization", "PopularityBaseline",
           "ItemCF", "WeightedItemCF", "ContentKNN", "ImplicitALS", "Ensemble", "Reranker",
           "RecommendationMetrics", "UserHistory", "SegmentPopularity", "age_segments",
           "SequentialCF", "UserSequence"]
