"""The reference's first tutorial, examples/basic_ranking.py, from the MI355X layers: a rating model
(two Embeddings -> concat -> Dense(256, relu) -> Dense(64, relu) -> Dense(1)) trained with
MeanSquaredError, RootMeanSquaredError as its metric and Adagrad(0.1), on synthetic ratings made in this file.

    python examples/basic_ranking.py            # a few epochs on synthetic (user, movie, rating) rows (needs an MI355X)

Loss, gradient and the metric update of a step are ONE krs_regression_fwd_bwd call (K24): the loss object carries the
metric (`metrics=`), so the predictions are read once.  The ratings are learnable: a user bias plus a movie bias,
squashed to [0, 1] as the reference normalises MovieLens ratings.
"""

from __future__ import annotations

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import keras_rs_amd.layers as kl  # noqa: E402
from keras_rs_amd.optim import Adagrad  # noqa: E402


class RankingModel:
    """RankingModel of the reference (examples/basic_ranking.py:120-160): rating = tower(concat(user, movie))."""

    def __init__(self, num_users: int, num_movies: int, embedding_dim: int = 32, device=None):
        self.user_embedding = kl.Embedding(num_users, embedding_dim, device=device)
        self.movie_embedding = kl.Embedding(num_movies, embedding_dim, device=device)
        self.ratings = [kl.Dense(256, activation="relu", device=device), kl.Dense(64, activation="relu", device=device),
                        kl.Dense(1, device=device)]

    def __call__(self, user_id: torch.Tensor, movie_id: torch.Tensor) -> torch.Tensor:
        """ids of one shape [...] -> ratings [..., 1]"""
        shape = tuple(user_id.shape)
        x = torch.cat([self.user_embedding(user_id.reshape(-1)), self.movie_embedding(movie_id.reshape(-1))], dim=-1)
        for layer in self.ratings:
            x = layer(x)
        return x.reshape(shape + (1,))

    @property
    def weights(self) -> list:
        return self.user_embedding.weights + self.movie_embedding.weights + [w for d in self.ratings for w in d.weights]


def synthetic_ratings(rows: int, num_users: int, num_movies: int, device, seed: int = 0):
    """(user_id [rows] int32, movie_id [rows] int32, rating [rows] fp32 in [0, 1]): sigmoid(user bias + movie bias)."""
    gen = torch.Generator().manual_seed(seed)
    user_bias, movie_bias = torch.randn(num_users, generator=gen), torch.randn(num_movies, generator=gen)
    user = torch.randint(0, num_users, (rows,), generator=gen)
    movie = torch.randint(0, num_movies, (rows,), generator=gen)
    rating = torch.sigmoid(user_bias[user] + movie_bias[movie])
    return user.to(device=device, dtype=torch.int32), movie.to(device=device, dtype=torch.int32), rating.to(device)


def main(epochs: int = 3, rows: int = 8192, batch: int = 1024, num_users: int = 500, num_movies: int = 300,
         embedding_dim: int = 32, learning_rate: float = 0.1, quiet: bool = False) -> dict:
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    user, movie, rating = synthetic_ratings(rows, num_users, num_movies, dev)
    model = RankingModel(num_users, num_movies, embedding_dim, device=dev)
    model(user[:2], movie[:2])                                  # (builds the layers)
    rmse = kl.RootMeanSquaredError()
    loss_fn = kl.MeanSquaredError(metrics=rmse)                 # loss + gradient + metric update: one kernel call
    opt = Adagrad(model.weights, lr=learning_rate, initial_accumulator_value=0.1)   # (keras.optimizers.Adagrad's default)
    losses, recorded = [], []
    for epoch in range(epochs):
        rmse.reset_state()
        for lo in range(0, rows - batch + 1, batch):
            sl = slice(lo, lo + batch)
            opt.zero_grad()
            pred = model(user[sl], movie[sl])
            value = loss_fn(rating[sl], pred)                   # y_true [B] with y_pred [B, 1]
            value.backward()
            opt.step()
            losses.append(value.detach())
            recorded.append((epoch, rating[sl], pred.detach()))
        if not quiet:
            print(f"epoch {epoch}: loss {float(losses[-1]):.4f} rmse {float(rmse.result()):.4f}")
    with torch.no_grad():
        sample = model(user[:5], movie[:5]).reshape(-1)
    if not quiet:
        print("predicted / true rating of the first rows:",
              [f"{float(a):.2f}/{float(b):.2f}" for a, b in zip(sample, rating[:5])])
    return {"losses": losses, "recorded": recorded, "rmse": rmse.result(), "last_epoch": epochs - 1, "loss_fn": loss_fn}


if __name__ == "__main__":
    main()
