"""Program batches on a trace suite in one device launch (DeviceSuite,
k_replay_native_duo_suite) against the CPU VM and the per-trace launches, bit
for bit; SuiteEvaluator's program interface on the MI355X.

Suite and corpus are those of tests/test_suite_programs.py: sub-traces
A = default[:257], B = default[:600], C = cpu037[:1500] of the 16-node cluster
(three LDS layouts, key widths and heap-area sizes) and the 60 compiled
programs of tests/program_corpus.py.
"""
import numpy as np
import pytest

from funsearch_kubernetes_simulator_amd.core import TraceParser
from funsearch_kubernetes_simulator_amd.core.traces import synthetic_workload
from funsearch_kubernetes_simulator_amd.engine import SuiteEvaluator
from funsearch_kubernetes_simulator_amd.models import families as fam
from funsearch_kubernetes_simulator_amd.models.library import reference_policies
from funsearch_kubernetes_simulator_amd.ops import cpu_engine as ce
from funsearch_kubernetes_simulator_amd.policy.bytecode import Exc
from funsearch_kubernetes_simulator_amd.policy.compiler import compile_policy
from funsearch_kubernetes_simulator_amd.simulator.metrics import suite_aggregate

from test_suite_programs import (DECLINED, codes, cpu_abc, cpu_results, expected_aggregate, progs,  # noqa: F401
                                 suite_of, traces, vm_table)

pytestmark = pytest.mark.gpu


def _he():
    from funsearch_kubernetes_simulator_amd.ops import hip_engine as he
    if not he.device_available():
        pytest.fail("GPU test collected but no HIP device is visible")
    return he


@pytest.fixture(scope="module")
def gpu_ev(traces):  # noqa: F811
    """SuiteEvaluator on the device over A, B, C: its per-trace DeviceEvaluators
    (default options) and its DeviceSuite serve every test below, so the corpus
    is JIT-compiled once."""
    _he()
    ev = SuiteEvaluator(suite_of(traces, "ABC"), device="gpu")
    assert ev.backend == "hip" and ev.device_suite is not None
    return ev


@pytest.fixture(scope="module")
def devs(gpu_ev):
    return dict(zip("ABC", gpu_ev.devices))


@pytest.fixture(scope="module")
def abc(gpu_ev):
    return gpu_ev.device_suite


@pytest.fixture(scope="module")
def fused(abc, progs):  # noqa: F811
    """The fused launch's [3, 60, 13] tables of the whole corpus, computed once."""
    tables = abc.evaluate_native(progs)
    tables.setflags(write=False)
    return tables


def check_vs_vm(traces, keys, progs, tables, lo=None, max_left_out=6):  # noqa: F811
    """Rows equal to the CPU VM's on all 13 columns; rows either engine declines
    are left out.  lo: `progs` are the corpus programs [lo, lo + len(progs)) and
    the traces sub-traces (the cached corpus tables); None: replayed here."""
    assert tables.shape == (len(keys), len(progs), 13)
    for t, k in enumerate(keys):
        vm = vm_table(traces, k, lo, lo + len(progs)) if lo is not None else \
            ce.simulate_program_batch(traces[k], progs, threads=16)
        left_out = []
        for i in range(len(progs)):
            if int(tables[t, i, 10]) in DECLINED or int(vm[i, 10]) in DECLINED:
                left_out.append((i, int(tables[t, i, 10]), int(vm[i, 10])))
                continue
            assert np.array_equal(tables[t, i], vm[i]), (k, i, progs[i].source[-300:], tables[t, i], vm[i])
            assert tables[t, i, 11] == 0, (k, i)
        assert len(left_out) <= max_left_out, (k, left_out)


def test_fused_table_equals_cpu_vm(traces, progs, fused, abc):  # noqa: F811
    check_vs_vm(traces, "ABC", progs, fused, lo=0)
    info = abc.info()
    assert info["T"] == 3 and info["grid"] % 3 == 0 and 3 * 54 <= info["grid"] <= 3 * len(progs)
    assert info["order"] == [2, 1, 0] and len(info["tops"]) == 3 and 0 < info["lds"] <= 160 * 1024
    assert info["per_cu"] >= 1


def test_fused_equals_per_trace_launch(devs, progs, fused):  # noqa: F811
    for t, k in enumerate("ABC"):
        plain = devs[k].evaluate_native(progs)
        assert np.array_equal(fused[t], plain), (k, np.argwhere(fused[t] != plain)[:8])


@pytest.mark.parametrize("n", (1, 3))
def test_small_grids(abc, traces, progs, n):  # noqa: F811
    check_vs_vm(traces, "ABC", progs[:n], abc.evaluate_native(progs[:n]), lo=0)
    assert abc.info()["grid"] == 3 * n


def test_suite_of_one_equals_single_workload(devs, traces, progs, fused):  # noqa: F811
    sub = progs[:24]
    tables = _he().DeviceSuite([devs["C"]]).evaluate_native(sub)
    assert tables.shape == (1, 24, 13)
    assert np.array_equal(tables[0], devs["C"].evaluate_native(sub)) and np.array_equal(tables[0], fused[2, :24])


def test_repeated_traces(devs, progs, fused):  # noqa: F811
    """Equal pod counts in the order table; table entries that share one trace's arrays."""
    keys = "AACAB"
    ds = _he().DeviceSuite([devs[k] for k in keys])
    sub = progs[:24]
    tables = ds.evaluate_native(sub)
    assert ds.info()["order"] == [2, 4, 0, 1, 3]
    for t, k in enumerate(keys):
        assert np.array_equal(tables[t], fused["ABC".index(k), :24]), (t, k)


@pytest.mark.parametrize("top", (63, 255))
def test_hbm_heap_areas(devs, abc, progs, fused, top):  # noqa: F811
    """A forced heap top below every trace's heap: the rest of each replay's
    heap lives in its trace's HBM area (three area sizes behind heap_off)."""
    for d in devs.values():
        d.set_options(native_duo_top=top)
    try:
        tables = abc.evaluate_native(progs)
        assert abc.info()["tops"] == [top, top, top]
    finally:
        for d in devs.values():
            d.set_options(native_duo_top=-1)
    assert np.array_equal(tables, fused), np.argwhere(tables != fused)[:8]


def test_event_cap(devs, abc, progs, fused):  # noqa: F811
    """max_events reaches the fused launch: replays past it end with EXC_EVENTS
    (on C only), every other row is the uncapped one.  The kernel tests the cap
    at events 1023, 2047, ...: the cap is set so that the first test at or
    past it lies beyond every replay of A, taken from the uncapped n_events."""
    point = 1023
    while point <= fused[0, :, 8].max() + 1:
        point += 1024
    assert (fused[2, :, 8] > point + 1).any(), "no replay of C passes the cap"
    for d in devs.values():
        d.set_options(max_events=point - 100)
    try:
        capped = abc.evaluate_native(progs)
    finally:
        for d in devs.values():
            d.set_options(max_events=0)
    n_capped = [0, 0, 0]
    for t in range(3):
        for i in range(len(progs)):
            want, got = fused[t, i], capped[t, i]
            if int(want[10]) == 0 and want[8] > point + 1:
                assert int(got[10]) == Exc.EVENTS, (t, i, got)
            elif int(want[10]) == 0 and want[8] < point:
                assert np.array_equal(got, want), (t, i, got, want)
            else:
                # a replay that ends at the test point itself, or a raising program (its
                # row carries no event count): the uncapped row, or capped before it raised
                assert np.array_equal(got, want) or (t > 0 and int(got[10]) == Exc.EVENTS), (t, i, got, want)
            n_capped[t] += int(got[10]) == Exc.EVENTS
    assert n_capped[0] == 0 and n_capped[2] > 0, n_capped


def test_slots_and_coexistence(gpu_ev, traces, progs, fused):  # noqa: F811
    """Two suite batches in flight, waited for in reverse order, an ordinary
    per-trace native batch between them, then a family batch on the same
    SuiteEvaluator."""
    ev, ds = gpu_ev, gpu_ev.device_suite
    a, b, c = progs[:20], progs[20:40], progs[40:52]
    ds.submit_native(1, a)
    ds.submit_native(2, b)
    with pytest.raises(RuntimeError):
        ds.submit_native(1, b)   # slot 1 still holds a batch
    ev.devices[0].submit_native(0, c)
    plain = ev.devices[0].wait(0)
    tb = ds.wait(2)
    ta = ds.wait(1)
    assert np.array_equal(ta, fused[:, :20]) and np.array_equal(tb, fused[:, 20:40])
    assert np.array_equal(plain, fused[0, 40:52])
    check_vs_vm(traces, "ABC", a, ta, lo=0)
    check_vs_vm(traces, "ABC", b, tb, lo=20)
    w = fam.sample_composite_linear(9, np.random.default_rng(1))
    ev.submit_family(1, "composite_linear", w)
    tables, agg = ev.wait(1)
    want = np.stack([ce.simulate_builtin_batch(traces[k], "composite_linear", w) for k in "ABC"])
    assert np.array_equal(tables, want) and np.array_equal(agg, suite_aggregate(want))
    assert np.array_equal(ds.evaluate_native(a), ta)


def test_suite_evaluator_programs(gpu_ev, codes, cpu_results):  # noqa: F811
    ev = gpu_ev
    got = ev.evaluate_programs(codes)
    assert len(got) == 3 and all(len(row) == len(codes) for row in got)
    for t in range(3):
        for i in range(len(codes)):
            assert got[t][i].score == cpu_results[t][i].score and got[t][i].exc == cpu_results[t][i].exc, (t, i)
        assert sum(r.engine == "hip-native" for r in got[t]) >= 54, [r.engine for r in got[t]]
    scores, agg = ev.score_programs(codes)
    want = np.array([[r.score for r in row] for row in cpu_results])
    raised = np.array([[r.exc != 0 for r in row] for row in cpu_results])
    assert np.array_equal(scores, want) and np.array_equal(agg, expected_aggregate(want, raised))
    ev.submit_programs(1, codes[:7])
    ev.submit_programs(2, codes[7:12])
    with pytest.raises(RuntimeError):
        ev.submit_programs(2, codes[:2])
    s2, a2 = ev.wait_programs(2)
    s1, a1 = ev.wait_programs(1)
    assert np.array_equal(s1, want[:, :7]) and np.array_equal(s2, want[:, 7:12])
    assert np.array_equal(a1, agg[:7]) and np.array_equal(a2, agg[7:12])


def test_full_length_traces(traces):  # noqa: F811
    he = _he()
    full = dict(traces, cpu300=TraceParser().load_workload(pod_file="openb_pod_list_cpu300.csv"))
    keys = ("cpu037", "default", "cpu300")   # 7,336 / 8,152 / 10,094 pods
    texts = list(reference_policies().values())[:5] + \
        [fam.to_program("feature_linear", w) for w in fam.sample_feature_linear(3, np.random.default_rng(5))]
    sub = [compile_policy(c) for c in texts]
    assert len(sub) == 8
    ds = he.DeviceSuite([he.DeviceEvaluator(full[k]) for k in keys])
    tables = ds.evaluate_native(sub)
    assert ds.info()["order"] == [2, 1, 0]
    check_vs_vm(full, keys, sub, tables, max_left_out=0)


def test_refused_suite_answers_from_the_cpu(traces, codes):  # noqa: F811
    """17 nodes: off the row layout, so the fused launch refuses the suite."""
    he = _he()
    wide = [synthetic_workload(17, n, seed=n, base=traces["default"]) for n in (300, 500)]
    with pytest.raises(ValueError):
        he.DeviceSuite([he.DeviceEvaluator(w) for w in wide])
    ev = SuiteEvaluator(wide, device="auto")
    assert ev.backend == "hip" and ev.device_suite is None
    sub = codes[:6]
    got = ev.evaluate_programs(sub)
    want = SuiteEvaluator(wide, device="cpu").evaluate_programs(sub)
    for t in range(2):
        assert [(r.score, r.exc, r.engine) for r in got[t]] == [(r.score, r.exc, r.engine) for r in want[t]]
    scores, agg = ev.score_programs(sub)
    assert np.array_equal(scores, [[r.score for r in row] for row in want])
