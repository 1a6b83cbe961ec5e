"""The reference's examples/multi_task.py from the MI355X layers: one user table and one movie table shared by two
tasks -- a rating tower trained with MeanSquaredError (K24) and in-batch retrieval trained with the softmax loss -- and
the reference's two loss weights, `ranking_loss_wt` and `retrieval_loss_wt`.

    python examples/multi_task.py               # the joint model on synthetic ratings (needs an MI355X)
    python examples/multi_task.py --stored      # the retrieval loss on the stored [B, B] score matrix, for A/B

The retrieval loss is InBatchSoftmaxLoss(reduction="sum") (K13: the scores are never stored); `--stored` is the
reference's formulation, CategoricalCrossentropy(from_logits=True, reduction="sum") on user @ movie^T with eye(B)
labels (K11).  RootMeanSquaredError is updated every step by the call that computes the rating loss.  Evaluation
retrieves the top 10 movies of each user with BruteForceRetrieval (K8) and feeds the ids to
SparseTopKCategoricalAccuracy(k=10, from_sorted_ids=True); as in the reference, rows rated 0.9 or less weigh 0.
"""

from __future__ import annotations

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import keras_rs_amd.layers as kl  # noqa: E402
from basic_ranking import synthetic_ratings  # noqa: E402
from keras_rs_amd.optim import Adagrad  # noqa: E402


class MultiTaskModel:
    """MultiTaskModel of the reference (examples/multi_task.py:112-290)."""

    def __init__(self, num_users: int, num_movies: int, embedding_dim: int = 32, layer_sizes=(256, 128),
                 ranking_loss_wt: float = 1.0, retrieval_loss_wt: float = 1.0, stored: bool = False, device=None):
        self.num_movies = num_movies
        self.user_embedding = kl.Embedding(num_users, embedding_dim, device=device)
        self.movie_embedding = kl.Embedding(num_movies, embedding_dim, device=device)
        self.rating_model = [kl.Dense(n, activation="relu", device=device) for n in layer_sizes] + \
                            [kl.Dense(1, device=device)]
        self.rmse_metric = kl.RootMeanSquaredError()
        self.ranking_loss_fn = kl.MeanSquaredError(metrics=self.rmse_metric)
        self.stored = stored
        self.retrieval_loss_fn = kl.CategoricalCrossentropy(from_logits=True, reduction="sum") if stored else \
            kl.InBatchSoftmaxLoss(reduction="sum")
        self.top_k_metric = kl.SparseTopKCategoricalAccuracy(k=10, from_sorted_ids=True)
        self.ranking_loss_wt, self.retrieval_loss_wt = ranking_loss_wt, retrieval_loss_wt
        self._device = device

    @property
    def weights(self) -> list:
        return self.user_embedding.weights + self.movie_embedding.weights + \
            [w for d in self.rating_model for w in d.weights]

    def __call__(self, user_id: torch.Tensor, movie_id: torch.Tensor):
        """(user embeddings [B, D], movie embeddings [B, D], predicted rating [B, 1])"""
        user, movie = self.user_embedding(user_id), self.movie_embedding(movie_id)
        x = torch.cat([user, movie], dim=-1)
        for layer in self.rating_model:
            x = layer(x)
        return user, movie, x

    def compute_loss(self, rating: torch.Tensor, outputs) -> dict:
        user, movie, pred = outputs
        if self.stored:
            scores = torch.matmul(user, movie.transpose(0, 1))
            labels = torch.eye(scores.shape[0], dtype=torch.float32, device=scores.device)
            retrieval = self.retrieval_loss_fn(labels, scores)
        else:
            retrieval = self.retrieval_loss_fn(user, movie)
        ranking = self.ranking_loss_fn(rating, pred)            # (updates rmse_metric from the same call)
        return {"retrieval": retrieval, "ranking": ranking,
                "total": self.retrieval_loss_wt * retrieval + self.ranking_loss_wt * ranking}

    @torch.no_grad()
    def evaluate(self, user_id: torch.Tensor, movie_id: torch.Tensor, rating: torch.Tensor) -> dict:
        """rmse over the rows and the top-10 accuracy of retrieving each well-rated row's movie"""
        self.rmse_metric.reset_state()
        self.top_k_metric.reset_state()
        all_movies = torch.arange(self.num_movies, device=user_id.device, dtype=torch.int32)
        index = kl.BruteForceRetrieval(self.movie_embedding(all_movies), all_movies, k=10, return_scores=False,
                                       device=self._device)
        user, _, pred = self(user_id, movie_id)
        self.rmse_metric.update_state(rating, pred)
        self.top_k_metric.update_state(movie_id.to(torch.int64), index(user), sample_weight=(rating > 0.9).float())
        return {"rmse": self.rmse_metric.result(), "top_10_accuracy": self.top_k_metric.result()}


def main(epochs: int = 3, rows: int = 8192, batch: int = 1024, num_users: int = 500, num_movies: int = 300,
         embedding_dim: int = 32, ranking_loss_wt: float = 1.0, retrieval_loss_wt: float = 1.0,
         learning_rate: float = 0.1, stored: bool = False, quiet: bool = False) -> dict:
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    user, movie, rating = synthetic_ratings(rows, num_users, num_movies, dev)
    model = MultiTaskModel(num_users, num_movies, embedding_dim, ranking_loss_wt=ranking_loss_wt,
                           retrieval_loss_wt=retrieval_loss_wt, stored=stored, device=dev)
    model(user[:2], movie[:2])                                  # (builds the layers)
    opt = Adagrad(model.weights, lr=learning_rate, initial_accumulator_value=0.1)   # (keras.optimizers.Adagrad's default)
    losses, recorded = [], []
    for epoch in range(epochs):
        model.rmse_metric.reset_state()
        for lo in range(0, rows - batch + 1, batch):
            sl = slice(lo, lo + batch)
            opt.zero_grad()
            outputs = model(user[sl], movie[sl])
            value = model.compute_loss(rating[sl], outputs)
            value["total"].backward()
            opt.step()
            losses.append({k: v.detach() for k, v in value.items()})
            recorded.append((epoch, rating[sl], outputs[2].detach()))
        if not quiet:
            last = losses[-1]
            print(f"epoch {epoch}: total {float(last['total']):.4f} ranking {float(last['ranking']):.4f} retrieval "
                  f"{float(last['retrieval']):.2f} rmse {float(model.rmse_metric.result()):.4f}")
    train_rmse = model.rmse_metric.result().clone()
    held = slice(0, min(rows, 2048))
    metrics = model.evaluate(user[held], movie[held], rating[held])
    if not quiet:
        print(f"evaluation: rmse {float(metrics['rmse']):.4f} top-10 accuracy {float(metrics['top_10_accuracy']):.4f}")
    return {"losses": losses, "recorded": recorded, "rmse": train_rmse, "last_epoch": epochs - 1, "evaluation": metrics,
            "model": model}


if __name__ == "__main__":
    main(stored="--stored" in sys.argv[1:])
