"""keras_rs.layers surface of the hot path."""

from keras_rs_amd.layers.distributed_embedding import (Adagrad, Adam, DistributedEmbedding, Ftrl, RowwiseAdagrad,
                                                       SGD, concat_features)
from keras_rs_amd.layers.dense import Dense
from keras_rs_amd.layers.distributed_embedding_config import FeatureConfig, TableConfig
from keras_rs_amd.layers.dot_interaction import DotInteraction
from keras_rs_amd.layers.embed_reduce import EmbedReduce, Embedding, Ragged
from keras_rs_amd.layers.feature_cross import FeatureCross
from keras_rs_amd.layers.losses import (BinaryCrossentropy, CategoricalCrossentropy, Huber, MeanAbsoluteError,
                                        MeanSquaredError, SparseCategoricalCrossentropy, binary_crossentropy)
# (keras keeps the two MeanSquaredError / MeanAbsoluteError in keras.losses and keras.metrics; here the bare names are the
#  losses and the metrics carry a suffix -- keras_rs_amd.layers.metrics has them under keras' names)
from keras_rs_amd.layers.metrics import (AUC, BinaryAccuracy, BinaryMetricGroup, RegressionMetricGroup,
                                         RootMeanSquaredError, SparseTopKCategoricalAccuracy, auc_from_confusion)
from keras_rs_amd.layers.metrics import MeanAbsoluteError as MeanAbsoluteErrorMetric
from keras_rs_amd.layers.metrics import MeanSquaredError as MeanSquaredErrorMetric
from keras_rs_amd.layers.recurrent import GRU
from keras_rs_amd.layers.retrieval import (AsymmetricHashingRetrieval, BruteForceRetrieval, FactorizedTopK,
                                           HardNegativeMining, InBatchSoftmaxLoss, PartitionedRetrieval,
                                           RemoveAccidentalHits, Retrieval, SamplingProbabilityCorrection)
from keras_rs_amd.layers.sequence import LayerNormalization, MultiHeadAttention, TransformerDecoder

__all__ = ["AUC", "Adagrad", "Adam", "AsymmetricHashingRetrieval", "BinaryAccuracy", "BinaryCrossentropy", "BinaryMetricGroup", "auc_from_confusion", "binary_crossentropy", "BruteForceRetrieval", "CategoricalCrossentropy", "Dense", "DistributedEmbedding", "DotInteraction", "EmbedReduce", "Embedding", "FeatureConfig",
           "FactorizedTopK", "FeatureCross", "Ftrl", "GRU", "HardNegativeMining", "Huber", "MeanAbsoluteError", "MeanAbsoluteErrorMetric", "MeanSquaredError", "MeanSquaredErrorMetric", "RegressionMetricGroup", "RootMeanSquaredError", "InBatchSoftmaxLoss", "LayerNormalization", "MultiHeadAttention", "PartitionedRetrieval", "Ragged", "RemoveAccidentalHits", "Retrieval", "RowwiseAdagrad", "SGD", "SamplingProbabilityCorrection",
           "SparseCategoricalCrossentropy", "SparseTopKCategoricalAccuracy", "TableConfig", "TransformerDecoder", "concat_features"]
