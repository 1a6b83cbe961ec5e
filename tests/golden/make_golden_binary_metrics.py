"""Writes tests/golden/binary_metrics.json: the known answers of keras' own docstrings and tests for
keras.metrics.AUC (confusion_metrics.py, confusion_metrics_test.py) and keras.metrics.BinaryAccuracy
(accuracy_metrics.py).  Keras cannot be run here, so the numbers are typed in from its published examples; before
they are written, each is checked against the float64 restatement of the formulas (tests/binary_metric_restatement.py).

    python tests/golden/make_golden_binary_metrics.py
"""

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import binary_metric_restatement as BR  # noqa: E402

AUC_CASES = {
    "y_true": [0, 0, 1, 1], "y_pred": [0, 0.5, 0.3, 0.9], "num_thresholds": 3,
    "cases": [
        {"source": "confusion_metrics.py: AUC docstring", "weights": None,
         "state": {"tp": [2, 1, 0], "fp": [2, 0, 0], "tn": [0, 2, 2], "fn": [0, 1, 2]},
         "results": {"ROC/interpolation": 0.75}},
        {"source": "confusion_metrics.py: AUC docstring, sample_weight", "weights": [1, 0, 0, 1], "state": None,
         "results": {"ROC/interpolation": 1.0}},
        {"source": "confusion_metrics_test.py: AUCTest, weighted", "weights": [1, 2, 3, 4],
         "state": {"tp": [7, 4, 0], "fp": [3, 0, 0], "tn": [0, 3, 3], "fn": [0, 3, 7]},
         "results": {"ROC/interpolation": 0.785714, "ROC/minoring": 0.571429, "ROC/majoring": 1.0,
                     "PR/interpolation": 0.916613, "PR/minoring": 0.3, "PR/majoring": 1.0}},
    ],
}
ACCURACY_CASES = {
    "y_true": [[1], [1], [0], [0]], "y_pred": [[0.98], [1], [0], [0.6]], "threshold": 0.5,
    "cases": [
        {"source": "accuracy_metrics.py: BinaryAccuracy docstring", "weights": None, "result": 0.75},
        {"source": "accuracy_metrics.py: BinaryAccuracy docstring, sample_weight", "weights": [1, 0, 0, 1],
         "result": 0.5},
    ],
}


def main():
    a = AUC_CASES
    for c in a["cases"]:
        state = BR.confusion(a["y_true"], a["y_pred"], c["weights"], a["num_thresholds"])
        if c["state"] is not None:
            for got, key in zip(state, ("tp", "fp", "tn", "fn")):
                assert np.array_equal(got, np.asarray(c["state"][key], np.float64)), (c["source"], key, got)
        for key, expected in c["results"].items():
            got = BR.auc_from_confusion(*state, *key.split("/"))
            assert abs(got - expected) <= 1e-6 + 1e-6 * abs(expected), (c["source"], key, got, expected)
    b = ACCURACY_CASES
    for c in b["cases"]:
        total, count = BR.accuracy(b["y_true"], b["y_pred"], c["weights"], b["threshold"])
        assert abs(total / count - c["result"]) <= 1e-6, (c["source"], total, count)
    with open(os.path.join(HERE, "binary_metrics.json"), "w") as f:
        json.dump({"atol": 1e-6, "rtol": 1e-6, "auc": a, "binary_accuracy": b}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
