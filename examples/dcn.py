"""The reference's examples/dcn.py from the MI355X layers: raw MovieLens-shaped features -> IntegerLookup /
StringLookup -> one Embedding per feature -> concat -> FeatureCross(projection_dim) stack -> Dense stack -> rating,
trained with MeanSquaredError, RootMeanSquaredError as its metric and Adagrad, on synthetic rows made in this file.

    python examples/dcn.py            # a few epochs (needs an MI355X)

The raw ids are deliberately NOT row numbers: user and movie ids are sparse int64 values, zip codes are strings.  The
vocabularies come from `adapt`, counted on the device (K26); a step's lookups are one krs_vocab_lookup each, in front of
the K1 gathers.
"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import keras_rs_amd.layers as kl  # noqa: E402
from keras_rs_amd.optim import Adagrad  # noqa: E402

INT_FEATURES, STR_FEATURES = ("user_id", "movie_id", "user_occupation"), ("user_zip_code",)


class DCN:
    """The reference's DCN: embeddings of every feature side by side, `cross_layers` low-rank cross layers, a Dense
    tower and a linear rating head."""

    def __init__(self, lookups: dict, embedding_dim: int = 16, projection_dim: int = 8, cross_layers: int = 2,
                 units=(64, 32), device=None):
        self.lookups = lookups
        self.embeddings = {k: kl.Embedding(v.vocabulary_size(), embedding_dim, device=device) for k, v in lookups.items()}
        self.cross = [kl.FeatureCross(projection_dim=projection_dim, device=device) for _ in range(cross_layers)]
        self.tower = [kl.Dense(u, activation="relu", device=device) for u in units] + [kl.Dense(1, device=device)]

    def indices(self, features: dict) -> dict:
        return {k: self.lookups[k](features[k]) for k in self.lookups}

    def __call__(self, features: dict) -> torch.Tensor:
        rows = self.indices(features)
        x0 = torch.cat([self.embeddings[k](rows[k].reshape(-1)) for k in self.lookups], dim=-1)
        x = x0
        for layer in self.cross:
            x = layer(x0, x)
        for layer in self.tower:
            x = layer(x)
        return x

    @property
    def weights(self) -> list:
        layers = list(self.embeddings.values()) + self.cross + self.tower
        return [w for layer in layers for w in layer.weights]


def synthetic_movielens(rows: int, num_users: int, num_movies: int, device, seed: int = 0):
    """({feature: raw values [rows]}, rating [rows] fp32 in [0, 1]).  Raw user / movie ids are random 40-bit numbers,
    occupations are 0..20, zip codes are 5-digit strings; the rating is sigmoid(user bias + movie bias)."""
    rng = np.random.default_rng(seed)
    raw_user = np.unique(rng.integers(1, 1 << 40, 2 * num_users))[:num_users]
    raw_movie = np.unique(rng.integers(1, 1 << 40, 2 * num_movies))[:num_movies]
    zips = np.array([f"{z:05d}" for z in rng.integers(0, 100000, max(2, num_users // 4))], dtype=object)
    user, movie = rng.integers(0, num_users, rows), rng.integers(0, num_movies, rows)
    rating = 1.0 / (1.0 + np.exp(-(rng.standard_normal(num_users)[user] + rng.standard_normal(num_movies)[movie])))
    features = {"user_id": torch.from_numpy(raw_user[user]).to(device),
                "movie_id": torch.from_numpy(raw_movie[movie]).to(device),
                "user_occupation": torch.from_numpy(user % 21).to(device),
                "user_zip_code": zips[user % len(zips)]}
    return features, torch.from_numpy(rating.astype(np.float32)).to(device)


def main(epochs: int = 3, rows: int = 8192, batch: int = 1024, num_users: int = 500, num_movies: int = 300,
         embedding_dim: int = 16, projection_dim: int = 8, learning_rate: float = 0.1, quiet: bool = False) -> dict:
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    features, rating = synthetic_movielens(rows, num_users, num_movies, dev)
    lookups = {k: kl.IntegerLookup(device=dev) for k in INT_FEATURES} | {k: kl.StringLookup(device=dev) for k in STR_FEATURES}
    for name, layer in lookups.items():
        layer.adapt(features[name])                             # counted on the device, ordered as Keras orders
    model = DCN(lookups, embedding_dim, projection_dim, device=dev)
    model({k: v[:2] for k, v in features.items()})              # (builds the layers)
    rmse = kl.RootMeanSquaredError()
    loss_fn = kl.MeanSquaredError(metrics=rmse)
    opt = Adagrad(model.weights, lr=learning_rate, initial_accumulator_value=0.1)
    losses = []
    for epoch in range(epochs):
        rmse.reset_state()
        for lo in range(0, rows - batch + 1, batch):
            opt.zero_grad()
            value = loss_fn(rating[lo:lo + batch], model({k: v[lo:lo + batch] for k, v in features.items()}))
            value.backward()
            opt.step()
            losses.append(value.detach())
        if not quiet:
            print(f"epoch {epoch}: loss {float(losses[-1]):.4f} rmse {float(rmse.result()):.4f}")
    return {"losses": losses, "model": model, "features": features, "rmse": rmse.result()}


if __name__ == "__main__":
    main()
