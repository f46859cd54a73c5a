"""badslam_amd/surface_eval.py: the summary of a distance array and precision / recall / F-score, on constructed arrays.  No GPU."""
import math

import numpy as np

from badslam_amd import surface_eval as se

INF = np.inf


def test_distance_summary_with_hits_misses_and_an_exact_threshold():
    d = np.array([0.0, 0.01, 0.02, 0.03, 0.04, INF, INF, 0.05, 0.10, 0.05], np.float32)
    t = [np.float32(0.02), np.float32(0.05), 1.0]
    s = se.distance_summary(d, t)
    hits = np.sort(d[np.isfinite(d)].astype(np.float64))
    assert (s["count"], s["hits"]) == (10, 8)
    assert s["mean"] == hits.mean() and s["median"] == (hits[3] + hits[4]) / 2 and s["rmse"] == math.sqrt((hits ** 2).mean())
    assert s["p90"] == np.percentile(hits, 90) and s["p99"] == np.percentile(hits, 99) and hits[-2] <= s["p90"] <= s["p99"] <= hits[-1]
    # the shares are of all ten points, a value equal to the threshold is within, a miss is within nothing
    assert s["within"] == [3 / 10, 7 / 10, 8 / 10] and s["beyond"] == 2 / 10
    assert s["thresholds"] == [float(v) for v in t]


def test_all_misses_and_an_empty_input():
    s = se.distance_summary(np.full(4, INF, np.float32), [0.01])
    assert (s["count"], s["hits"], s["within"], s["beyond"]) == (4, 0, [0.0], 1.0)
    assert all(math.isnan(s[k]) for k in ("mean", "median", "rmse", "p90", "p99"))
    e = se.distance_summary(np.zeros(0, np.float32), [0.01, 0.02])
    assert (e["count"], e["hits"]) == (0, 0) and all(math.isnan(v) for v in e["within"]) and math.isnan(e["beyond"]) and math.isnan(e["mean"])
    assert se.format_summary("empty", e).startswith("empty: 0 of 0")


def test_precision_recall_f_score_by_hand():
    accuracy = se.distance_summary(np.array([0.005, 0.015, 0.2, INF], np.float32), [0.01, 0.1])      # 1 of 4, 2 of 4
    completeness = se.distance_summary(np.array([0.001, 0.002, 0.003, 0.05, INF], np.float32), [0.01, 0.1])   # 3 of 5, 4 of 5
    f = se.f_scores(accuracy, completeness)
    assert [(r["threshold"], r["precision"], r["recall"]) for r in f] == [(0.01, 0.25, 0.6), (0.1, 0.5, 0.8)]
    assert f[0]["f_score"] == 2 * 0.25 * 0.6 / (0.25 + 0.6) and f[1]["f_score"] == 2 * 0.5 * 0.8 / (0.5 + 0.8)
    nothing = se.distance_summary(np.full(3, INF, np.float32), [0.01])
    assert se.f_scores(nothing, nothing)[0]["f_score"] == 0.0


class FakeBA:
    """Stands in for DirectBA: the distance of a point is |x| of its first coordinate, a miss beyond max_distance."""

    def __init__(self):
        self.calls = []

    def PointMeshDistance(self, points, mesh, max_distance, cell_size=None):
        self.calls.append((len(points), len(mesh["positions"]), max_distance, cell_size))
        d = np.abs(np.asarray(points, np.float32)[:, 0])
        return dict(distance=np.where(d <= max_distance, d, np.float32(INF)).astype(np.float32), triangle=np.zeros(len(d), np.uint32), cell_size=0.5, grid_cells=8,
                    grid_entries=20)


def test_evaluate_measures_both_directions():
    ba = FakeBA()
    reconstruction = dict(positions=np.array([[0.0, 0, 0], [0.03, 0, 0], [5.0, 0, 0]], np.float32), triangles=np.zeros((1, 3), np.uint32))
    ground_truth = dict(positions=np.array([[0.01, 0, 0], [0.04, 0, 0]], np.float32))
    r = se.evaluate(ba, reconstruction, ground_truth, max_distance=0.1, thresholds=(0.02, 0.05))
    assert ba.calls == [(3, 2, 0.1, None), (2, 3, 0.1, None)]
    assert r["accuracy"]["within"] == [1 / 3, 2 / 3] and r["accuracy"]["beyond"] == 1 / 3
    assert r["completeness"]["within"] == [0.5, 1.0] and r["completeness"]["beyond"] == 0.0
    assert [x["precision"] for x in r["f_scores"]] == [1 / 3, 2 / 3] and [x["recall"] for x in r["f_scores"]] == [0.5, 1.0]
    assert r["accuracy_grid"] == dict(cell_size=0.5, grid_cells=8, grid_entries=20) and r["max_distance"] == 0.1
