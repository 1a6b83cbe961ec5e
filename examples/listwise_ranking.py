"""The reference's examples/listwise_ranking.py from the MI355X layers: the rating model of basic_ranking.py scores
lists of 5 movies per user, trained once pointwise with MeanSquaredError (K24) and once with the listwise
PairwiseHingeLoss (K9); both are evaluated with NDCG(k=5) (K10), the comparison the reference's file makes.

    python examples/listwise_ranking.py         # trains both models on synthetic lists (needs an MI355X)

y_true and y_pred are [batch, 5]: MeanSquaredError takes the mean over the list as its last axis, which is what Keras
does with the reference's lists.
"""

from __future__ import annotations

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import keras_rs_amd.layers as kl  # noqa: E402
from basic_ranking import RankingModel  # noqa: E402
from keras_rs_amd.losses import PairwiseHingeLoss  # noqa: E402
from keras_rs_amd.metrics import NDCG  # noqa: E402
from keras_rs_amd.optim import Adagrad  # noqa: E402

LIST = 5     # NUM_EXAMPLES_PER_LIST of the reference


def synthetic_lists(lists: int, num_users: int, num_movies: int, device, seed: int = 0):
    """(user_id [lists] int32, movie_id [lists, 5] int32, rating [lists, 5] fp32 in {0.5, 1, .., 5}): a user bias plus a
    movie bias plus a user x movie taste term, binned to half stars."""
    gen = torch.Generator().manual_seed(seed)
    user_bias, movie_bias = torch.randn(num_users, generator=gen), torch.randn(num_movies, generator=gen)
    taste_u, taste_m = torch.randn(num_users, 4, generator=gen), torch.randn(num_movies, 4, generator=gen)
    user = torch.randint(0, num_users, (lists,), generator=gen)
    movie = torch.randint(0, num_movies, (lists, LIST), generator=gen)
    raw = user_bias[user, None] + movie_bias[movie] + (taste_u[user, None, :] * taste_m[movie]).sum(-1) * 0.5
    rating = torch.clamp(torch.round((torch.sigmoid(raw) * 4.5 + 0.5) * 2) / 2, 0.5, 5.0)
    return user.to(device=device, dtype=torch.int32), movie.to(device=device, dtype=torch.int32), rating.to(device)


def score_lists(model: RankingModel, user: torch.Tensor, movie: torch.Tensor) -> torch.Tensor:
    """user [B], movie [B, 5] -> scores [B, 5]"""
    return model(user[:, None].expand_as(movie), movie).reshape(movie.shape)


def train(loss_fn, data, test, num_users, num_movies, embedding_dim, epochs, batch, learning_rate, dev, name, quiet):
    torch.manual_seed(0)                       # both models start from the same weights
    user, movie, rating = data
    model = RankingModel(num_users, num_movies, embedding_dim, device=dev)
    score_lists(model, user[:2], movie[:2])    # (builds the layers)
    opt = Adagrad(model.weights, lr=learning_rate, initial_accumulator_value=0.1)   # (keras.optimizers.Adagrad's default)
    losses, recorded = [], []
    for epoch in range(epochs):
        for lo in range(0, user.shape[0] - batch + 1, batch):
            sl = slice(lo, lo + batch)
            opt.zero_grad()
            pred = score_lists(model, user[sl], movie[sl])
            value = loss_fn(rating[sl], pred)
            value.backward()
            opt.step()
            losses.append(value.detach())
            recorded.append((rating[sl], pred.detach()))
    ndcg = NDCG(k=LIST, name="ndcg")
    with torch.no_grad():
        ndcg.update_state(test[2], score_lists(model, test[0], test[1]))
    if not quiet:
        print(f"{name}: loss {float(losses[0]):.4f} -> {float(losses[-1]):.4f}, test ndcg@{LIST} {float(ndcg.result()):.4f}")
    return {"losses": losses, "recorded": recorded, "ndcg": ndcg.result()}


def main(epochs: int = 3, lists: int = 4096, batch: int = 512, num_users: int = 300, num_movies: int = 200,
         embedding_dim: int = 32, learning_rate: float = 0.1, quiet: bool = False) -> dict:
    dev = torch.device("cuda", torch.cuda.current_device())
    held_out = max(batch, lists // 4)
    user, movie, rating = synthetic_lists(lists + held_out, num_users, num_movies, dev)
    data = (user[:lists], movie[:lists], rating[:lists])
    test = (user[lists:], movie[lists:], rating[lists:])       # other lists of the same users and movies
    args = (data, test, num_users, num_movies, embedding_dim, epochs, batch, learning_rate, dev)
    return {"mse": train(kl.MeanSquaredError(), *args, "MeanSquaredError", quiet),
            "hinge": train(PairwiseHingeLoss(), *args, "PairwiseHingeLoss", quiet)}


if __name__ == "__main__":
    main()
