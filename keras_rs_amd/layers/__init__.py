"""keras_rs.layers surface of the hot path."""

from keras_rs_amd.layers.distributed_embedding import (Adagrad, Adam, DistributedEmbedding, Ftrl, RowwiseAdagrad,
                                                       SGD, concat_features)
from keras_rs_amd.layers.dense import Dense
from keras_rs_amd.layers.distributed_embedding_config import FeatureConfig, TableConfig
from keras_rs_amd.layers.dot_interaction import DotInteraction
from keras_rs_amd.layers.embed_reduce import EmbedReduce, Embedding, Ragged
from keras_rs_amd.layers.feature_cross import FeatureCross
from keras_rs_amd.layers.losses import (BinaryCrossentropy, CategoricalCrossentropy, SparseCategoricalCrossentropy,
                                        binary_crossentropy)
from keras_rs_amd.layers.metrics import (AUC, BinaryAccuracy, BinaryMetricGroup, SparseTopKCategoricalAccuracy,
                                         auc_from_confusion)
from keras_rs_amd.layers.recurrent import GRU
from keras_rs_amd.layers.retrieval import (AsymmetricHashingRetrieval, BruteForceRetrieval, FactorizedTopK,
                                           HardNegativeMining, InBatchSoftmaxLoss, PartitionedRetrieval,
                                           RemoveAccidentalHits, Retrieval, SamplingProbabilityCorrection)
from keras_rs_amd.layers.sequence import LayerNormalization, MultiHeadAttention, TransformerDecoder

__all__ = ["AUC", "Adagrad", "Adam", "AsymmetricHashingRetrieval", "BinaryAccuracy", "BinaryCrossentropy", "BinaryMetricGroup", "auc_from_confusion", "binary_crossentropy", "BruteForceRetrieval", "CategoricalCrossentropy", "Dense", "DistributedEmbedding", "DotInteraction", "EmbedReduce", "Embedding", "FeatureConfig",
           "FactorizedTopK", "FeatureCross", "Ftrl", "GRU", "HardNegativeMining", "InBatchSoftmaxLoss", "LayerNormalization", "MultiHeadAttention", "PartitionedRetrieval", "Ragged", "RemoveAccidentalHits", "Retrieval", "RowwiseAdagrad", "SGD", "SamplingProbabilityCorrection",
           "SparseCategoricalCrossentropy", "SparseTopKCategoricalAccuracy", "TableConfig", "TransformerDecoder", "concat_features"]
