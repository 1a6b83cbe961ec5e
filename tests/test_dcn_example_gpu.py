"""examples/dcn.py at a toy size: it runs, it learns, and every looked-up index lies inside its embedding table."""

import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dcn_example_trains_on_raw_ids():
    spec = importlib.util.spec_from_file_location("dcn_example", os.path.join(ROOT, "examples", "dcn.py"))
    dcn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dcn)
    run = dcn.main(epochs=6, rows=2048, batch=256, num_users=60, num_movies=40, quiet=True)
    losses = [float(v) for v in run["losses"]]
    assert len(losses) == 48 and losses[-1] < losses[0]
    model = run["model"]
    for name, rows in model.indices(run["features"]).items():
        size = model.lookups[name].vocabulary_size()
        assert 0 <= int(rows.min()) and int(rows.max()) < size == model.embeddings[name].input_dim, name
        assert int(rows.min()) >= 1      # every training token is in its adapted vocabulary: none lands on the OOV slot
