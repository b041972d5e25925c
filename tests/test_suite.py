"""Trace suites: loading, the CPU-backend SuiteEvaluator, the suite aggregates and suite_search."""
import json
import statistics
from fractions import Fraction

import numpy as np
import pytest

from funsearch_kubernetes_simulator_amd.core import TraceParser, TraceSuite, Workload, load_suite, synthetic_workload
from funsearch_kubernetes_simulator_amd.engine import SuiteEvaluator
from funsearch_kubernetes_simulator_amd.models import families as fam
from funsearch_kubernetes_simulator_amd.ops import cpu_engine as ce
from funsearch_kubernetes_simulator_amd.simulator.metrics import suite_aggregate


def _prefix(w, n, name):
    return Workload(w.cluster, w.pods.subset(np.arange(n)), name)


@pytest.fixture(scope="module")
def small_suite(default_workload):
    cpu037 = TraceParser().load_workload(pod_file="openb_pod_list_cpu037.csv")
    return TraceSuite([_prefix(default_workload, 257, "A"), _prefix(default_workload, 600, "B"),
                       _prefix(cpu037, 1500, "C")])


@pytest.fixture(scope="module")
def evaluated(small_suite):
    """(weights, tables, agg) of 37 composite candidates on the CPU backend, computed once."""
    w = fam.sample_composite_linear(37, np.random.default_rng(1))
    tables, agg = SuiteEvaluator(small_suite, device="cpu").evaluate_family("composite_linear", w)
    for a in (w, tables, agg):
        a.setflags(write=False)
    return w, tables, agg


def test_openb_preset():
    suite = load_suite("openb")
    assert len(suite) == 14 and suite.names == sorted(suite.names)
    assert "default" in suite.names and not any(n.startswith(("gpuspec", "multigpu")) for n in suite.names)
    assert [w.pods.n_pods for w in suite][suite.names.index("default")] == 8152
    assert load_suite(["cpu037", "openb_pod_list_default.csv"]).names == ["cpu037", "default"]
    with pytest.raises(ValueError):
        load_suite("no_such_preset")
    with pytest.raises(KeyError):      # the multigpu files lack the time columns, as before
        load_suite(["multigpu20"])


def test_two_clusters_raise(default_workload):
    other = synthetic_workload(n_nodes=32, n_pods=64, seed=1, base=default_workload)
    with pytest.raises(ValueError):
        TraceSuite([default_workload, other])
    with pytest.raises(ValueError):
        SuiteEvaluator([default_workload, other], device="cpu")


def test_tables_equal_per_trace_oracle(small_suite, evaluated):
    w, tables, _ = evaluated
    assert tables.shape == (3, 37, 13)
    for t, wl in enumerate(small_suite):
        assert np.array_equal(tables[t], ce.simulate_builtin_batch(wl, "composite_linear", w))
    # the sub-traces force failed placements: the candidates do not all score alike
    assert all((tables[t, :, 7] > 0).sum() * 4 >= 37 for t in range(3))


def test_aggregates(evaluated):
    _, tables, agg = evaluated
    scores = tables[:, :, 0]
    T = scores.shape[0]
    for p in range(scores.shape[1]):
        want = float(sum(Fraction(float(s)) for s in scores[:, p]) / T)
        assert agg[p, 0] == want == statistics.mean(scores[:, p].tolist())
    assert np.array_equal(agg[:, 1], scores.min(axis=0))
    assert np.array_equal(agg[:, 2], scores.argmin(axis=0))
    assert not agg[:, 3].any()
    tie = np.zeros((3, 2, 13))
    tie[:, 0, 0] = (0.5, 0.25, 0.25)       # the first minimum wins
    tie[:, 1, 0] = (0.1, 0.1, 0.7)
    assert suite_aggregate(tie)[:, 2].tolist() == [1.0, 0.0]


def test_raising_trace_scores_zero(small_suite):
    w = fam.sample_composite_linear(5, np.random.default_rng(2))
    w[3, 3] = np.inf                      # int(inf) raises in the reference: exc != 0 on every trace
    tables, agg = SuiteEvaluator(small_suite, device="cpu").evaluate_family("composite_linear", w)
    assert (tables[:, 3, 10] != 0).all() and (tables[:, [0, 1, 2, 4], 10] == 0).all()
    assert agg[3].tolist()[:2] == [0.0, 0.0] and agg[3, 3] == 3 and not agg[[0, 1, 2, 4], 3].any()
    # a row that raised on one trace only: 0 in the mean, counted once
    mixed = tables[:, :1].copy()
    mixed[1, 0, 10], mixed[1, 0, 0] = 3.0, 0.9    # (a stale score must not leak into the mean)
    a = suite_aggregate(mixed)[0]
    assert a[0] == statistics.mean([float(mixed[0, 0, 0]), 0.0, float(mixed[2, 0, 0])])
    assert a[1] == 0.0 and a[2] == 1 and a[3] == 1


def test_submit_wait_and_programs(small_suite, evaluated):
    w, tables, agg = evaluated
    ev = SuiteEvaluator(small_suite, device="cpu")
    ev.submit_family(2, "composite_linear", w[:5])
    t2, a2 = ev.wait(2)
    assert np.array_equal(t2, tables[:, :5]) and np.array_equal(a2, agg[:5])
    code = fam.to_program("composite_linear", w[0])
    per_trace = ev.evaluate_programs([code])
    assert [r[0].score for r in per_trace] == tables[:, 0, 0].tolist()


def test_mixed_family_batch_and_slot_guard(small_suite, evaluated):
    w, tables, _ = evaluated
    ev = SuiteEvaluator(small_suite, device="cpu")
    names = ["first_fit", "composite_linear", "best_fit", "composite_linear"]
    W = np.zeros((4, 16))
    W[1, :w.shape[1]], W[3, :w.shape[1]] = w[1], w[3]
    got, agg = ev.evaluate_family(names, W)
    for t, wl in enumerate(small_suite):
        assert np.array_equal(got[t, 0], ce.simulate_builtin_batch(wl, "first_fit", np.zeros((1, 16)))[0])
        assert np.array_equal(got[t, 2], ce.simulate_builtin_batch(wl, "best_fit", np.zeros((1, 16)))[0])
    assert np.array_equal(got[:, [1, 3]], tables[:, [1, 3]]) and np.array_equal(agg, suite_aggregate(got))
    ev.submit_family(0, "composite_linear", w[:2])
    with pytest.raises(RuntimeError):
        ev.evaluate_family("composite_linear", w[:2])   # slot 0 holds a batch
    ev.wait(0)
    with pytest.raises(ValueError):
        ev.wait(0)


def test_suite_search_writes_champion(small_suite, tmp_path):
    from funsearch_kubernetes_simulator_amd.funsearch import suite_search
    suite = TraceSuite(small_suite.workloads[:2], small_suite.names[:2])
    out = tmp_path / "best.json"
    cfg = {"family": "composite_linear", "aggregate": "min", "candidates": 64, "generations": 2, "seed": 3,
           "save_best": str(out)}
    rec = suite_search.run(cfg, SuiteEvaluator(suite, device="cpu"), log=lambda *_: None)
    saved = json.loads(out.read_text())
    assert saved["suite"]["traces"] == ["A", "B"] and saved["suite"]["aggregate"] == "min"
    assert saved["score"] == saved["suite"]["min"] == rec["score"]
    assert saved["family"] == "composite_linear" and len(saved["weights"]) == len(fam.CHAMPION_COMPOSITE)
    assert "def priority_function" in saved["code"]
    # the saved rows are the champion's own: re-evaluating its weights reproduces them
    tables, agg = SuiteEvaluator(suite, device="cpu").evaluate_family("composite_linear",
                                                                      np.array([saved["weights"]]))
    assert agg[0, 1] == saved["suite"]["min"] and agg[0, 0] == saved["suite"]["mean"]
    assert [saved["suite"]["per_trace"][n]["score"] for n in ("A", "B")] == tables[:, 0, 0].tolist()
