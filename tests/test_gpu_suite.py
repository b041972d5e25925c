"""SuiteEvaluator on the MI355X (one resident DeviceEvaluator per trace) vs the CPU oracle, bit-exact.

Sub-traces on the shipped 16-node cluster with three different pod counts
(three LDS layouts and key bit widths), all of which force failed placements:
A = default[:257], B = default[:600], C = cpu037[:1500].
"""
import numpy as np
import pytest

from funsearch_kubernetes_simulator_amd.core import TraceParser, TraceSuite, Workload
from funsearch_kubernetes_simulator_amd.engine import SuiteEvaluator
from funsearch_kubernetes_simulator_amd.models import families as fam
from funsearch_kubernetes_simulator_amd.ops import cpu_engine as ce
from funsearch_kubernetes_simulator_amd.simulator.metrics import suite_aggregate

pytestmark = pytest.mark.gpu

P = 37
FAMILIES = ("composite_linear", "feature_linear", "random_linear")


def _prefix(w, n, name):
    return Workload(w.cluster, w.pods.subset(np.arange(n)), name)


@pytest.fixture(scope="module")
def traces(default_workload):
    cpu037 = TraceParser().load_workload(pod_file="openb_pod_list_cpu037.csv")
    cpu300 = TraceParser().load_workload(pod_file="openb_pod_list_cpu300.csv")
    return {"A": _prefix(default_workload, 257, "A"), "B": _prefix(default_workload, 600, "B"),
            "C": _prefix(cpu037, 1500, "C"), "default": default_workload, "cpu037": cpu037, "cpu300": cpu300}


def _gpu(traces, keys, options=None):
    from funsearch_kubernetes_simulator_amd.ops import hip_engine as he
    if not he.device_available():
        pytest.fail("GPU test collected but no HIP device is visible")
    ev = SuiteEvaluator(TraceSuite([traces[k] for k in keys], list(keys)), device="gpu", options=options)
    assert ev.backend == "hip"
    return ev


@pytest.fixture(scope="module")
def abc(traces):
    return _gpu(traces, "ABC")


@pytest.fixture(scope="module")
def cands():
    rng = np.random.default_rng(1)
    out = {f: fam.SAMPLERS[f](P, rng) for f in FAMILIES}
    # one mixed batch: first-fit, best-fit and members of the three weighted families
    order = ("first_fit", "best_fit") + FAMILIES
    names, W = [order[i % 5] for i in range(P)], np.zeros((P, 16))
    for i, f in enumerate(names):
        if f in FAMILIES:
            W[i, :out[f].shape[1]] = out[f][i]
    out["mixed"] = (names, W)
    return out


_oracle_cache = {}


def oracle1(traces, key, family, weights):
    """CPU-oracle table of one trace, computed once per (trace, batch)."""
    weights = np.asarray(weights, dtype=np.float64)
    ck = (key, family if isinstance(family, str) else tuple(family), weights.tobytes())
    if ck not in _oracle_cache:
        if isinstance(family, str):
            tab = ce.simulate_builtin_batch(traces[key], family, weights)
        else:
            tab = np.zeros((len(family), 13))
            for f in sorted(set(family)):
                idx = [i for i, g in enumerate(family) if g == f]
                tab[idx] = ce.simulate_builtin_batch(traces[key], f, weights[idx])
        tab.setflags(write=False)
        _oracle_cache[ck] = tab
    return _oracle_cache[ck]


def oracle(traces, keys, family, weights):
    return np.stack([oracle1(traces, k, family, weights) for k in keys])


def check(traces, keys, family, weights, got):
    tables, agg = got
    want = oracle(traces, keys, family, weights)
    assert tables.shape == want.shape
    for t, k in enumerate(keys):
        assert np.array_equal(tables[t], want[t]), (k, np.argwhere(tables[t] != want[t])[:8])
    assert np.array_equal(agg, suite_aggregate(want))


def test_subtraces_force_failed_placements(traces, cands):
    """Precondition (CPU oracle): on each sub-trace at least a quarter of the
    candidates of every family record fragmentation events."""
    for key in "ABC":
        for f in FAMILIES:
            n = int((oracle1(traces, key, f, cands[f])[:, 7] > 0).sum())
            assert n * 4 >= P, (key, f, n)


@pytest.mark.parametrize("batch", FAMILIES + ("mixed",))
def test_suite_matches_oracle(abc, traces, cands, batch):
    family, weights = cands[batch] if batch == "mixed" else (batch, cands[batch])
    check(traces, "ABC", family, weights, abc.evaluate_family(family, weights))


def test_suite_of_one_equals_single_workload(traces, cands):
    from funsearch_kubernetes_simulator_amd.ops import hip_engine as he
    w = cands["composite_linear"]
    tables, agg = _gpu(traces, "C").evaluate_family("composite_linear", w)
    plain = he.DeviceEvaluator(traces["C"]).evaluate_builtin("composite_linear", w)
    assert tables.shape == (1, P, 13) and np.array_equal(tables[0], plain)
    check(traces, "C", "composite_linear", w, (tables, agg))


@pytest.mark.parametrize("n", (1, 3))
def test_fewer_policies_than_rows(abc, traces, cands, n):
    w = cands["composite_linear"][:n]
    check(traces, "ABC", "composite_linear", w, abc.evaluate_family("composite_linear", w))


def test_repeated_traces(traces, cands):
    ev = _gpu(traces, "AACAB")
    for f in ("feature_linear", "composite_linear"):
        check(traces, "AACAB", f, cands[f], ev.evaluate_family(f, cands[f]))


def test_capped_to_one_wave(traces, cands):
    ev = _gpu(traces, "ABC", {"row_wave_share": 1e-6})   # cap = max(1, int(share * resident waves)) = 1
    assert all(d.info()["row_wave_share"] == 1e-6 and d.info()["row_kernel_ok"] for d in ev.devices)
    w = cands["composite_linear"]
    check(traces, "ABC", "composite_linear", w, ev.evaluate_family("composite_linear", w))


def test_slots_and_queue_counters(abc, traces, cands):
    """Two suite batches in flight, an ordinary single-trace batch on the same
    engine, a suite batch again: the row kernel's queue counter and qbase of
    every slot stay consistent."""
    a, b, c = cands["composite_linear"], cands["random_linear"], cands["feature_linear"]
    abc.submit_family(1, "composite_linear", a)
    abc.submit_family(2, "random_linear", b)
    with pytest.raises(RuntimeError):
        abc.submit_family(1, "random_linear", b)   # slot 1 still holds a batch
    check(traces, "ABC", "random_linear", b, abc.wait(2))
    check(traces, "ABC", "composite_linear", a, abc.wait(1))
    for slot in (1, 0):
        abc.devices[0].submit_builtin(slot, "feature_linear", c)
        assert np.array_equal(abc.devices[0].wait(slot), oracle1(traces, "A", "feature_linear", c))
    abc.submit_family(1, "feature_linear", c)
    check(traces, "ABC", "feature_linear", c, abc.wait(1))
    check(traces, "ABC", "composite_linear", a, abc.evaluate_family("composite_linear", a))


def test_non_finite_weight_is_an_exception_row(abc, traces, cands):
    w = cands["composite_linear"][:9].copy()
    w[4, 3] = np.inf
    want = oracle(traces, "ABC", "composite_linear", w)
    assert (want[:, 4, 10] != 0).all() and (np.delete(want, 4, axis=1)[:, :, 10] == 0).all()   # it alone raises
    tables, agg = abc.evaluate_family("composite_linear", w)
    check(traces, "ABC", "composite_linear", w, (tables, agg))
    assert agg[4].tolist() == [0.0, 0.0, 0.0, 3.0] and not np.delete(agg, 4, axis=0)[:, 3].any()


def test_full_length_traces(traces):
    keys = ("cpu037", "default", "cpu300")   # 7,336 / 8,152 / 10,094 pods
    w = fam.sample_composite_linear(8, np.random.default_rng(3))
    check(traces, keys, "composite_linear", w, _gpu(traces, keys).evaluate_family("composite_linear", w))


def test_without_row_kernel(traces, cands):
    ev = _gpu(traces, "AC", {"row_kernel": "off"})
    assert not any(d._eng.would_use_rows(9) for d in ev.devices)
    w = cands["composite_linear"][:9]
    check(traces, "AC", "composite_linear", w, ev.evaluate_family("composite_linear", w))
