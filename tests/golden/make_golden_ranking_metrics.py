"""Writes tests/golden/ranking_metrics.json: the inputs and expected values of the six ranking-metric test files of
keras-rs (keras_rs/src/metrics/*_test.py), transcribed as data with the file and lines each comes from.

    python tests/golden/make_golden_ranking_metrics.py

A case is a metric (class, k, gain / discount functions by name) and a list of updates; each update carries its
inputs and the value the reference's test asserts for result() after it, with that assertion's tolerance: keras'
assertAllClose default atol = rtol = 1e-6, or rtol = 1e-5 where the test says so.  "reset_expected" is the value
asserted after reset_state().  Values the reference states as sums of (2^label - 1) / log2(rank + 1) are written
through dcg() below; "linear" / "inverse" name the gain label -> label and the discount rank -> 1 / rank of
test_alternative_gain_rank_discount_fns.

Every case was checked (tests/test_ranking_metrics_host.py) to give the same value whichever way score ties are
broken; none had to be dropped.
"""
import json
import math
import os

ATOL = 1e-6


def dcg(labels, ranks):
    return sum((2.0 ** y - 1.0) / math.log2(r + 1.0) for y, r in zip(labels, ranks))


def update(y_true, y_pred, expected, sample_weight=None, mask=None, rtol=1e-6):
    return {"y_true": y_true, "mask": mask, "y_pred": y_pred, "sample_weight": sample_weight,
            "expected": expected, "atol": ATOL, "rtol": rtol}


def case(metric, name, source, updates, k=None, gain="default", discount="default", reset_expected=None):
    return {"metric": metric, "case": name, "source": source, "k": k, "gain": gain, "discount": discount,
            "updates": updates, "reset_expected": reset_expected}


# ---- dcg_test.py and ndcg_test.py share their inputs (setUp, lines 24-41 of both) --------------------------------
G_TRUE = [[0, 0, 1, 0], [1, 0, 3, 2], [0, 0, 0, 0], [2, 1, 0, 0]]
G_PRED = [[0.1, 0.2, 0.9, 0.3], [0.1, 0.8, 0.9, 0.7], [0.4, 0.3, 0.2, 0.1], [0.9, 0.7, 0.1, 0.2]]
G_DCG = [dcg([1], [1]), dcg([3, 2, 1], [1, 3, 4]), 0.0, dcg([2, 1], [1, 2])]
G_IDEAL = [dcg([1], [1]), dcg([3, 2, 1], [1, 2, 3]), 0.0, dcg([2, 1], [1, 2])]
G_NDCG = [a / b if b != 0.0 else 0.0 for a, b in zip(G_DCG, G_IDEAL)]
G_GENERAL_TRUE = [[0, 1, 0, 0, 2, 3], [1, 0, 0, 2, 0, 2]]
G_GENERAL_PRED = [[0.8, 0.7, 0.1, 0.2, 0.9, 0.5], [0.9, 0.1, 0.2, 0.3, 0.2, 0.3]]
G_GENERAL_W = [[0.5, 4.0, 1.0, 0.0, 1.0, 0.0], [0.0, 0.0, 3.0, 1.0, 2.0, 0.0]]
G_GENERAL_W_MASKED = [[0.5, 4.0, 1.0, 0.0, 1.0, 0.0], [0.0, 1.0, 3.0, 1.0, 2.0, 0.0]]
G_GENERAL_MASK = [[True, True, True, False, True, False], [True, False, True, True, True, False]]
GOOD = dcg([3, 2, 1], [1, 3, 4])
BEST = dcg([3, 2, 1], [1, 2, 3])
ALT_DCG = [1 / 1, 3 / 1 + 2 / 3 + 1 / 4, 0.0, 2 / 1 + 1 / 2]
ALT_IDEAL = [1 / 1, 3 / 1 + 2 / 2 + 1 / 3, 0.0, 2 / 1 + 1 / 2]

# name, y_true, y_pred, sample_weight, DCG expected, its lines, NDCG expected, its lines
GRADED_UNBATCHED = [
    ("binary_perfect_rank", [0, 0, 1, 0], [0.1, 0.2, 0.9, 0.3], None, dcg([1], [1]), "69-75", 1.0, "76-82"),
    ("binary_good_rank", [0, 0, 1, 0], [0.8, 0.1, 0.7, 0.2], None, dcg([1], [2]), "76-82",
     dcg([1], [2]) / dcg([1], [1]), "83-89"),
    ("binary_bad_rank", [0, 0, 1, 0], [0.4, 0.3, 0.2, 0.1], None, dcg([1], [3]), "83-89",
     dcg([1], [3]) / dcg([1], [1]), "90-96"),
    ("irrelevant", [0, 0, 0, 0], [0.1, 0.2, 0.9, 0.3], None, 0.0, "90-96", 0.0, "97-103"),
    ("graded_good_rank", [1, 0, 3, 2], [0.1, 0.8, 0.9, 0.7], None, GOOD, "97-103", GOOD / BEST, "104-111"),
    ("graded_mixed_rank", [1, 0, 3, 2], [0.9, 0.1, 0.7, 0.8], None, dcg([1, 2, 3], [1, 2, 3]), "104-110",
     dcg([1, 2, 3], [1, 2, 3]) / BEST, "112-119"),
    ("sample_weight_0", [0.0, 1.0, 2.0], [0.5, 0.8, 0.2], [0.0, 0.0, 0.0], 0.0, "111-117", 0.0, "120-126"),
    ("sample_weight_scalar", [1, 0, 3, 2], [0.1, 0.8, 0.9, 0.7], 5.0, GOOD, "118-124", GOOD / BEST, "127-134"),
    ("sample_weight_1d", [1, 0, 3, 2], [0.1, 0.8, 0.9, 0.7], [2.0, 1.0, 3.0, 0.0], 7.652174, "125-131", 0.988237,
     "135-141"),
]
# name, sample_weight, DCG expected, NDCG expected (dcg_test.py:147-160, ndcg_test.py:157-170)
GRADED_BATCHED_W = [("scalar_0.5", 0.5, 3.3904016, 0.73770034), ("scalar_0", 0, 0, 0),
                    ("1d", [1.0, 0.5, 2.0, 1.0], 2.7288804, 0.74262)]
# name, y_true, y_pred, sample_weight, DCG expected, lines, NDCG expected, lines (test_2d_sample_weight)
GRADED_2D = [
    ("mask_relevant_item", [[0, 1, 0]], [[0.5, 0.8, 0.2]], [[1.0, 0.0, 1.0]], 0.0, "163-169", 0.0, "173-179"),
    ("mask_highest_ranked_item", [[0, 1, 0]], [[0.5, 0.8, 0.2]], [[1.0, 0.0, 1.0]], 0.0, "170-176", 0.0, "180-186"),
    ("mask_lower_ranked_relevant", [[1, 0, 1]], [[0.8, 0.2, 0.6]], [[1.0, 1.0, 0.0]], dcg([1], [1]), "177-183", 1.0,
     "187-193"),
    ("mask_irrelevant_item", [[0, 1, 0]], [[0.5, 0.8, 0.2]], [[0.0, 1.0, 1.0]], dcg([1], [1]), "184-190", 1.0,
     "194-200"),
    ("general_case", G_GENERAL_TRUE, G_GENERAL_PRED, G_GENERAL_W, 2.909091, "191-215", 0.903588, "201-225"),
]
# name, labels, mask, y_pred, sample_weight, DCG expected, lines, NDCG expected, lines (test_masking)
GRADED_MASKING = [
    ("mask_relevant_items", [[0.0, 1.0, 0.0]], [[True, False, True]], [[0.5, 0.8, 0.2]], None, 0.0, "227-233", 0.0,
     "237-243"),
    ("mask_first_relevant_item", [[1, 0, 1]], [[False, True, True]], [[0.8, 0.2, 0.6]], None, 1.0, "234-240", 1.0,
     "244-250"),
    ("mask_irrelevant_item", [[0, 1, 0]], [[False, True, True]], [[0.5, 0.8, 0.2]], None, 1.0, "241-247", 1.0,
     "251-257"),
    ("general_case", G_GENERAL_TRUE, G_GENERAL_MASK, G_GENERAL_PRED, G_GENERAL_W_MASKED, 2.909091, "248-280",
     0.903588, "258-290"),
]
GRADED_K = {"DCG": ([2.75, 2.90773, 3.28273, 3.39040], "289-299"),
            "NDCG": ([0.75, 0.696789, 0.72623, 0.7377], "299-309")}


def graded_cases():
    out = []
    for metric, f, pick in (("DCG", "dcg_test.py", 0), ("NDCG", "ndcg_test.py", 1)):
        for name, y, s, w, e0, l0, e1, l1 in GRADED_UNBATCHED:
            out.append(case(metric, f"unbatched/{name}", f"{f}:{(l0, l1)[pick]}",
                            [update(y, s, (e0, e1)[pick], sample_weight=w)]))
        batched = sum((G_DCG, G_NDCG)[pick]) / 4
        out.append(case(metric, "batched", f"{f}:{('42-52, 141-145', '43-59, 151-155')[pick]}",
                        [update(G_TRUE, G_PRED, batched)]))
        for name, w, e0, e1 in GRADED_BATCHED_W:
            out.append(case(metric, f"batched_sample_weight/{name}", f"{f}:{('147-160', '157-170')[pick]}",
                            [update(G_TRUE, G_PRED, (e0, e1)[pick], sample_weight=w)]))
        for name, y, s, w, e0, l0, e1, l1 in GRADED_2D:
            out.append(case(metric, f"2d_sample_weight/{name}", f"{f}:{(l0, l1)[pick]}",
                            [update(y, s, (e0, e1)[pick], sample_weight=w)]))
        for name, y, m, s, w, e0, l0, e1, l1 in GRADED_MASKING:
            out.append(case(metric, f"masking/{name}", f"{f}:{(l0, l1)[pick]}",
                            [update(y, s, (e0, e1)[pick], sample_weight=w, mask=m)]))
        ks, lines = GRADED_K[metric]
        for k, e in zip((1, 2, 3, 4), ks):
            out.append(case(metric, f"k/{k}", f"{f}:{lines}", [update(G_TRUE, G_PRED, e, rtol=1e-5)], k=k))
        first = sum((G_DCG, G_NDCG)[pick][:2]) / 2
        out.append(case(metric, "statefulness", f"{f}:{('301-324', '311-336')[pick]}",
                        [update(G_TRUE[:2], G_PRED[:2], first), update(G_TRUE[2:], G_PRED[2:], batched)],
                        reset_expected=0.0))
        alt = (sum(ALT_DCG) / 4,
               sum(a / b if b != 0.0 else 0.0 for a, b in zip(ALT_DCG, ALT_IDEAL)) / 4)[pick]
        out.append(case(metric, "alternative_gain_rank_discount_fns", f"{f}:{('331-347', '343-359')[pick]}",
                        [update(G_TRUE, G_PRED, alt, rtol=1e-5)], gain="linear", discount="inverse"))
    return out


# ---- the four binary-relevance metrics ---------------------------------------------------------------------------
PRED_B = [[0.1, 0.2, 0.9, 0.3], [0.8, 0.7, 0.1, 0.2], [0.4, 0.3, 0.2, 0.1], [0.9, 0.2, 0.1, 0.3]]
GEN_TRUE = [[0, 1, 1, 0], [1, 0, 2, 1]]
GEN_PRED = [[0.8, 0.7, 0.1, 0.2], [0.9, 0.1, 0.2, 0.3]]
GEN_W = [[0.8, 1.0, 1.0, 0.0], [1.0, 1.0, 0.0, 0.0]]
GEN_MASK = [[True, True, True, False], [True, True, False, False]]
SIMPLE_MASKING = [   # name, labels, mask, y_pred: test_masking of MAP, MRR (expected 0, 1, 1) and P@k (0, 0.5, 0.5)
    ("mask_relevant_items", [[0.0, 1.0, 0.0]], [[True, False, True]], [[0.5, 0.8, 0.2]]),
    ("mask_first_relevant_item", [[1, 0, 1]], [[False, True, True]], [[0.8, 0.2, 0.6]]),
    ("mask_irrelevant_item", [[0, 1, 0]], [[False, True, True]], [[0.5, 0.8, 0.2]]),
]
SIMPLE_2D = [        # the same three through a [1, 3] sample weight (test_2d_sample_weight of MAP and MRR)
    ("mask_relevant_items", [[0.0, 1.0, 0.0]], [[0.5, 0.8, 0.2]], [[1.0, 0.0, 1.0]]),
    ("mask_first_relevant_item", [[1, 0, 1]], [[0.8, 0.2, 0.6]], [[0.0, 1.0, 1.0]]),
    ("mask_irrelevant_item", [[0, 1, 0]], [[0.5, 0.8, 0.2]], [[0.0, 1.0, 1.0]]),
]

BINARY = {
    "MeanAveragePrecision": {
        "file": "mean_average_precision_test.py", "k": None,
        "true": [[0, 0, 1, 0], [0, 3, 4, 0], [0, 0, 0, 0], [1, 0, 2, 0]], "pred": PRED_B,
        "unbatched": ("48-112", [
            ("perfect_rank", [0.0, 0.0, 1.0, 0.0], [0.1, 0.2, 0.9, 0.3], None, 1.0),
            ("second_rank", [0.0, 0.0, 1.0, 0.0], [0.8, 0.1, 0.7, 0.2], None, 1 / 2),
            ("third_rank", [0.0, 0.0, 1.0, 0.0], [0.4, 0.3, 0.2, 0.1], None, 1 / 3),
            ("irrelevant", [0.0, 0.0, 0.0, 0.0], [0.1, 0.2, 0.9, 0.3], None, 0.0),
            ("multiple_relevant_items", [1.0, 0.0, 2.0, 0.0], [0.9, 0.2, 0.1, 0.3], None, 0.75),
            ("sample_weight_0", [0.0, 1.0, 0.0], [0.5, 0.8, 0.2], [0.0, 0.0, 0.0], 0.0),
            ("sample_weight_scalar", [0.0, 0.0, 1.0, 0.0], [0.8, 0.1, 0.7, 0.2], 5.0, 1 / 2),
            ("sample_weight_1d", [1.0, 0.0, 1.0, 0.0], [0.9, 0.2, 0.1, 0.3], [2.0, 1.0, 3.0, 0.0], 0.8),
        ]),
        "batched": ("114-118", 0.5625),
        "batched_w": ("120-133", [("scalar_0.5", 0.5, 0.5625), ("scalar_0", 0, 0),
                                  ("1d", [1.0, 0.5, 2.0, 1.0], 0.6)]),
        "2d": ("135-172", None, [(n, y, s, w, e) for (n, y, s, w), e in zip(SIMPLE_2D, (0.0, 1.0, 1.0))]
               + [("general_case", GEN_TRUE, GEN_PRED, GEN_W, 0.791667)]),
        "masking": ("174-215", [(n, y, m, s, None, e) for (n, y, m, s), e in zip(SIMPLE_MASKING, (0.0, 1.0, 1.0))]
                    + [("general_case", GEN_TRUE, GEN_MASK, GEN_PRED,
                        [[0.8, 0.8, 1.0, 1.0], [0.0, 0.0, 1.0, 1.0]], 0.592593)]),
        "k_values": ("217-227", [0.375, 0.4375, 0.4375, 0.5625]),
        "state": ("229-248", 0.75, 0.5625),
        "extra": [("scalar_sample_weight/0.5", "250-262", 0.5, 0.5625), ("scalar_sample_weight/weight_0", "250-262",
                                                                         0.0, 0.0),
                  ("1d_sample_weight", "264-273", [1.0, 0.5, 2.0, 1.0], 0.6)],
    },
    "MeanReciprocalRank": {
        "file": "mean_reciprocal_rank_test.py", "k": None,
        "true": [[0, 0, 1, 0], [0, 3, 0, 0], [0, 0, 0, 0], [1, 0, 2, 0]],
        "pred": [[0.1, 0.2, 0.9, 0.3], [0.8, 0.7, 0.1, 0.2], [0.4, 0.3, 0.2, 0.1], [0.9, 0.2, 0.8, 0.3]],
        "unbatched": ("48-112", [
            ("perfect_rank", [0.0, 0.0, 1.0, 0.0], [0.1, 0.2, 0.9, 0.3], None, 1.0),
            ("second_rank", [0.0, 0.0, 1.0, 0.0], [0.8, 0.1, 0.7, 0.2], None, 1 / 2),
            ("third_rank", [0.0, 0.0, 1.0, 0.0], [0.4, 0.3, 0.2, 0.1], None, 1 / 3),
            ("irrelevant", [0.0, 0.0, 0.0, 0.0], [0.1, 0.2, 0.9, 0.3], None, 0.0),
            ("multiple_relevant_items", [1.0, 0.0, 1.0, 0.0], [0.9, 0.2, 0.8, 0.3], None, 1.0),
            ("sample_weight_0", [0.0, 1.0, 0.0], [0.5, 0.8, 0.2], [0.0, 0.0, 0.0], 0.0),
            ("sample_weight_scalar", [0.0, 0.0, 1.0, 0.0], [0.8, 0.1, 0.7, 0.2], 5.0, 1 / 2),
            ("sample_weight_1d", [1.0, 0.0, 1.0, 0.0], [0.9, 0.2, 0.8, 0.3], [2.0, 1.0, 3.0, 0.0], 1.0),
        ]),
        "batched": ("114-118", 0.625),
        "batched_w": ("120-133", [("scalar_0.5", 0.5, 0.625), ("scalar_0", 0, 0), ("1d", [1.0, 0.5, 2.0, 1.0], 0.675)]),
        "2d": ("135-172", None, [(n, y, s, w, e) for (n, y, s, w), e in zip(SIMPLE_2D, (0.0, 1.0, 1.0))]
               + [("general_case", [[0, 1, 0, 0], [1, 0, 0, 1]], GEN_PRED,
                   [[0.8, 0.8, 0.0, 0.0], [0.0, 0.0, 1.0, 1.0]], 0.777778)]),
        "masking": ("174-215", [(n, y, m, s, None, e) for (n, y, m, s), e in zip(SIMPLE_MASKING, (0.0, 1.0, 1.0))]
                    + [("general_case", [[0, 1, 0, 0], [1, 0, 0, 1]],
                        [[True, True, False, False], [False, False, True, True]], GEN_PRED,
                        [[0.8, 0.8, 1.0, 1.0], [0.0, 0.0, 1.0, 1.0]], 0.777778)]),
        "k_values": ("217-224", [0.5, 0.625, 0.625, 0.625]),
        "state": ("226-245", 0.75, 0.625),
        "extra": [],
    },
    "PrecisionAtK": {
        "file": "precision_at_k_test.py", "k": 3,
        "true": [[0, 0, 1, 0], [0, 1, 1, 1], [0, 0, 0, 0], [1, 0, 1, 0]], "pred": PRED_B,
        "unbatched": ("48-98", [
            ("one_relevant", [0.0, 0.0, 1.0, 0.0], [0.1, 0.2, 0.9, 0.3], None, 1 / 3),
            ("two_relevant", [1.0, 0.0, 1.0, 0.0], [0.8, 0.1, 0.7, 0.2], None, 2 / 3),
            ("irrelevant", [0.0, 0.0, 0.0, 0.0], [0.1, 0.2, 0.9, 0.3], None, 0.0),
            ("sample_weight_0", [1.0, 1.0, 0.0], [0.5, 0.8, 0.2], [0.0, 0.0, 0.0], 0.0),
            ("sample_weight_scalar", [1.0, 0.0, 1.0, 0.0], [0.8, 0.1, 0.7, 0.2], 5.0, 2 / 3),
            ("sample_weight_1d", [1.0, 0.0, 1.0, 0.0], [0.8, 0.1, 0.7, 0.2], [2.0, 1.0, 3.0, 0.0], 2 / 3),
        ]),
        "batched": ("100-104", 1 / 3),
        "batched_w": ("106-119", [("scalar_0.5", 0.5, 1 / 3), ("scalar_0", 0, 0), ("1d", [1.0, 0.5, 2.0, 1.0], 0.3)]),
        "2d": ("121-157", 3, [
            ("mask_relevant_items", [[0.0, 1.0, 1.0]], [[0.5, 0.8, 0.2]], [[1.0, 0.0, 0.0]], 0.0),
            ("mask_first_relevant_item", [[1, 0, 1]], [[0.8, 0.2, 0.6]], [[0.0, 1.0, 1.0]], 0.5),
            ("mask_irrelevant_item", [[0, 1, 0]], [[0.5, 0.8, 0.2]], [[0.0, 1.0, 1.0]], 0.5),
            ("general_case", GEN_TRUE, GEN_PRED, GEN_W, 0.583333)]),
        "masking": ("159-199", [
            ("mask_relevant_items", [[0.0, 1.0, 1.0]], [[True, False, False]], [[0.5, 0.8, 0.2]], None, 0.0),
            ("mask_first_relevant_item", [[1, 0, 1]], [[False, True, True]], [[0.8, 0.2, 0.6]], None, 0.5),
            ("mask_irrelevant_item", [[0, 1, 0]], [[False, True, True]], [[0.5, 0.8, 0.2]], None, 0.5),
            ("general_case", GEN_TRUE, GEN_MASK, GEN_PRED, GEN_W, 0.583333)]),
        "k_values": ("201-211", [0.5, 0.375, 0.333333, 0.375]),
        "state": ("213-225", 0.5, 1 / 3),
        "extra": [],
    },
    "RecallAtK": {
        "file": "recall_at_k_test.py", "k": 3,
        "true": [[0, 0, 1, 0], [0, 1, 1, 1], [0, 0, 0, 0], [1, 0, 1, 0]], "pred": PRED_B,
        "unbatched": ("48-98", [
            ("one_relevant", [0.0, 0.0, 1.0, 0.0], [0.1, 0.2, 0.9, 0.3], None, 1.0),
            ("two_relevant", [1.0, 1.0, 0.0, 0.0], [0.8, 0.1, 0.7, 0.2], None, 0.5),
            ("irrelevant", [0.0, 0.0, 0.0, 0.0], [0.1, 0.2, 0.9, 0.3], None, 0.0),
            ("sample_weight_0", [1.0, 1.0, 0.0], [0.5, 0.8, 0.2], [0.0, 0.0, 0.0], 0.0),
            ("sample_weight_scalar", [1.0, 1.0, 0.0, 0.0], [0.8, 0.1, 0.7, 0.2], 5.0, 0.5),
            ("sample_weight_1d", [1.0, 1.0, 0.0, 0.0], [0.8, 0.1, 0.7, 0.2], [2.0, 1.0, 3.0, 0.0], 1.0),
        ]),
        "batched": ("100-104", 0.541667),
        "batched_w": ("106-119", [("scalar_0.5", 0.5, 0.541667), ("scalar_0", 0, 0),
                                  ("1d", [1.0, 0.5, 2.0, 1.0], 0.55)]),
        "2d": ("121-157", 2, [
            ("mask_relevant_items", [[0.0, 1.0, 1.0, 0.0]], [[0.5, 0.8, 0.2, 0.1]], [[1.0, 0.0, 0.0, 1.0]], 0.0),
            ("mask_first_relevant_item", [[0, 0, 1, 1]], [[0.8, 0.2, 0.6, 0.1]], [[1.0, 1.0, 0.0, 1.0]], 0.0),
            ("mask_irrelevant_item", [[0, 1, 0, 1]], [[0.5, 0.8, 0.2, 0.1]], [[0.0, 1.0, 1.0, 1.0]], 0.5),
            ("general_case", GEN_TRUE, GEN_PRED, GEN_W, 0.75)]),
        "masking": ("159-202", [
            ("mask_relevant_items", [[0.0, 1.0, 1.0, 0.0]], [[True, False, False, True]], [[0.5, 0.8, 0.2, 0.1]],
             None, 0.0),
            ("mask_first_relevant_item", [[0, 0, 1, 1]], [[True, True, False, True]], [[0.8, 0.2, 0.6, 0.1]], None,
             0.0),
            ("mask_irrelevant_item", [[0, 1, 0, 1]], [[False, True, True, True]], [[0.5, 0.8, 0.2, 0.1]], None, 0.5),
            ("general_case", GEN_TRUE, GEN_MASK, GEN_PRED, GEN_W, 0.75)]),
        "k_values": ("204-214", [0.375, 0.458333, 0.541667, 0.75]),
        "state": ("216-228", 0.833333, 0.541667),
        "extra": [],
    },
}


def binary_cases():
    out = []
    for metric, t in BINARY.items():
        f, k, y, s = t["file"], t["k"], t["true"], t["pred"]
        lines, rows = t["unbatched"]
        for name, yy, ss, w, e in rows:
            out.append(case(metric, f"unbatched/{name}", f"{f}:{lines}", [update(yy, ss, e, sample_weight=w)], k=k))
        lines, e = t["batched"]
        out.append(case(metric, "batched", f"{f}:{lines}", [update(y, s, e)], k=k))
        lines, rows = t["batched_w"]
        for name, w, e in rows:
            out.append(case(metric, f"batched_sample_weight/{name}", f"{f}:{lines}",
                            [update(y, s, e, sample_weight=w)], k=k))
        lines, k_masking, rows = t["2d"]   # with the k of the 2-D weight and masking tests (recall_at_k_test.py: 2)
        for name, yy, ss, w, e in rows:
            out.append(case(metric, f"2d_sample_weight/{name}", f"{f}:{lines}", [update(yy, ss, e, sample_weight=w)],
                            k=k_masking))
        lines, rows = t["masking"]
        for name, yy, m, ss, w, e in rows:
            out.append(case(metric, f"masking/{name}", f"{f}:{lines}",
                            [update(yy, ss, e, sample_weight=w, mask=m)], k=k_masking))
        lines, es = t["k_values"]
        for kk, e in zip((1, 2, 3, 4), es):
            out.append(case(metric, f"k/{kk}", f"{f}:{lines}", [update(y, s, e)], k=kk))
        lines, e1, e2 = t["state"]
        out.append(case(metric, "statefulness", f"{f}:{lines}", [update(y[:2], s[:2], e1), update(y[2:], s[2:], e2)],
                        k=k, reset_expected=0.0))
        for name, lines, w, e in t["extra"]:
            out.append(case(metric, name, f"{f}:{lines}", [update(y, s, e, sample_weight=w)], k=k))
    return out


def main():
    doc = {"about": "inputs and expected values of keras_rs/src/metrics/*_test.py (keras-rs), see "
                    "make_golden_ranking_metrics.py",
           "cases": graded_cases() + binary_cases()}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ranking_metrics.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(path, len(doc["cases"]), "cases")


if __name__ == "__main__":
    main()
