"""Writes tests/golden/ranking_losses.json: the expected values of the five ranking-loss test files of keras-rs
(keras_rs/src/losses/*_test.py), transcribed as data with the file and lines each comes from.

    python tests/golden/make_golden_ranking.py

Every case is one call of the reference loss on the shared inputs below; "expected" is what its test asserts
(atol 1e-5 for arrays, 5 decimal places for reduced scalars).  Cases the reference states as
`expected_output * sample_weight` are written out multiplied here.
"""
import json
import os

# setUp of every test file (e.g. pairwise_logistic_loss_test.py:14-22, list_mle_loss_test.py:14-27)
SCORES = [[1.0, 3.0, 2.0, 4.0, 0.8], [1.0, 1.8, 2.0, 3.0, 2.0]]
LABELS = [[1.0, 0.0, 1.0, 3.0, 2.0], [0.0, 1.0, 2.0, 3.0, 1.5]]
MASK = [[True, True, True, True, True], [True, True, True, False, False]]       # test_mask_input
ITEM_WEIGHT = [[1.0, 1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 0.0, 0.0]]           # test_itemwise_sample_weight_with_zeros
SCALAR_WEIGHT = 5.0                                                               # test_scalar_sample_weight

# loss -> (file, {what: (expected, lines)})
PAIRWISE = {
    "PairwiseHingeLoss": ("pairwise_hinge_loss_test.py", {
        "none": ([[3.0, 0.0, 2.0, 0.0, 6.6000004], [0.0, 0.20000005, 1.8, 0.0, 0.79999995]], "24-29"),
        "temperature": ([[5.0, 0.0, 3.0, 0.0, 10.200001], [0.0, 0.0, 1.5999999, 0.0, 0.5999999]], "43-53"),
        "sum_over_batch_size": (1.44, "62-65"),
        "mask": ([[3.0, 0.0, 2.0, 0.0, 6.6000004], [0.0, 0.20000005, 0.79999995, 0.0, 0.0]], "93-111"),
    }),
    "PairwiseLogisticLoss": ("pairwise_logistic_loss_test.py", {
        "none": ([[2.126928, 0.0, 1.313262, 0.52873, 4.566504], [0.0, 0.371101, 1.604548, 1.016734, 0.9114]],
                 "24-29"),
        "temperature": ([[4.01815, 0.0, 2.126928, 0.149214, 7.812055], [0.0, 0.183901, 1.333091, 0.358842, 0.639943]],
                        "43-53"),
        "sum_over_batch_size": (1.243921, "62-65"),
        "mask": ([[2.126928, 0.0, 1.313262, 0.52873, 4.566504], [0.0, 0.371101, 0.9114, 0.0, 0.0]], "93-111"),
    }),
    "PairwiseSoftZeroOneLoss": ("pairwise_soft_zero_one_loss_test.py", {
        "none": ([[0.880797, 0.0, 0.731059, 0.474736, 2.218608], [0.0, 0.310025, 1.219108, 0.888561, 0.719108]],
                 "26-31"),
        "temperature": ([[0.982014, 0.0, 0.880797, 0.141321, 2.503386], [0.0, 0.167982, 1.020515, 0.339565, 0.520515]],
                        "45-55"),
        "sum_over_batch_size": (0.744200, "64-67"),
        "mask": ([[0.880797, 0.0, 0.731059, 0.474736, 2.218608], [0.0, 0.310025, 0.719108, 0.0, 0.0]], "95-112"),
    }),
    # the temperature case expects the untempered values: the loss overrides compute_unreduced_loss
    "PairwiseMeanSquaredError": ("pairwise_mean_squared_error_test.py", {
        "none": ([[12.44, 34.64, 9.84, 9.84, 28.76], [2.29, 1.41, 1.89, 1.89, 0.84]], "26-28"),
        "temperature": ([[12.440001, 34.64, 9.84, 9.84, 28.759998], [2.29, 1.41, 1.89, 1.89, 0.84]], "42-52"),
        "sum_over_batch_size": (10.384, "61-64"),
        "mask": ([[12.440001, 34.64, 9.84, 9.84, 28.759998], [1.04, 0.68, 1.64, 0.0, 0.0]], "92-110"),
    }),
}
LISTMLE = ("list_mle_loss_test.py", {
    "none": ([6.865693, 3.088192], "28"),
    "temperature": ([10.969891, 2.1283305], "47-56"),
    "sum_over_batch_size": (4.9769425, "65-70"),
})


def _scale(x, w):
    if isinstance(w, list):
        return [[a * b for a, b in zip(r, s)] for r, s in zip(x, w)]
    return [[a * w for a in r] for r in x] if isinstance(x[0], list) else [a * w for a in x]


def cases():
    out = []
    for loss, (f, exp) in list(PAIRWISE.items()) + [("ListMLELoss", LISTMLE)]:
        none, lines = exp["none"]
        base = {"loss": loss, "temperature": 1.0, "reduction": "none", "sample_weight": None, "mask": None,
                "rank": 2}
        out.append(dict(base, case="unbatched", rank=1, expected=[none[0]],
                        source=f"{f}:{lines} (test_unbatched_input)"))
        out.append(dict(base, case="batched", expected=none, source=f"{f}:{lines} (test_batched_input)"))
        t, tl = exp["temperature"]
        out.append(dict(base, case="temperature", temperature=0.5, expected=t, source=f"{f}:{tl}"))
        r, rl = exp["sum_over_batch_size"]
        out.append(dict(base, case="sum_over_batch_size", reduction="sum_over_batch_size", expected=r,
                        source=f"{f}:{rl}"))
        out.append(dict(base, case="scalar_sample_weight", sample_weight=SCALAR_WEIGHT,
                        expected=_scale(none, SCALAR_WEIGHT), source=f"{f} test_scalar_sample_weight"))
        if loss != "ListMLELoss":
            out.append(dict(base, case="itemwise_sample_weight", sample_weight=ITEM_WEIGHT,
                            expected=_scale(none, ITEM_WEIGHT), source=f"{f} test_itemwise_sample_weight_with_zeros"))
            m, ml = exp["mask"]
            out.append(dict(base, case="mask", mask=MASK, expected=m, source=f"{f}:{ml}"))
    return out


def main():
    doc = {"about": "expected values of keras_rs/src/losses/*_test.py (keras-rs), see make_golden_ranking.py",
           "scores": SCORES, "labels": LABELS, "cases": cases()}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ranking_losses.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(path, len(doc["cases"]), "cases")


if __name__ == "__main__":
    main()
