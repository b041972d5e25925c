"""Device time metrics vs the CPU oracle's: waits, makespan, busy time, histogram.

The time instances of the replay kernels (csrc/hip/launch.h) carry a few
lane-resident integer accumulators through the replay and write one 192-byte
record per policy beside the usual row.  Everything is an integer, so every
comparison here is `np.array_equal` on the raw arrays against
`ce.time_builtin_batch` / `ce.time_program_batch` (which
`tests/test_time_metrics.py` holds to the engine-independent derivation from a
schedule, to the object engine and to the reference's recorded schedules), and
the rows must be the default launch's bit for bit.  `tests/test_time_metrics.py`
shows on the CPU that these shapes carry past 2^32, leave pods unplaced, fill
17-20 buckets and tell the candidates apart, so nothing here passes on an
empty record.
"""
import numpy as np
import pytest

import device_shapes as ds
from funsearch_kubernetes_simulator_amd.core.time_metrics import TimeMetricsBatch
from funsearch_kubernetes_simulator_amd.ops import cpu_engine as ce
from funsearch_kubernetes_simulator_amd.policy.bytecode import Exc

pytestmark = pytest.mark.gpu

#: shape -> what it exercises (the row kernel where the host allows it, else the one-wave kernel)
FAMILY_SHAPES = {
    "sweep005": "row kernel; wait_sum past 2^32, pods left unplaced",
    "sweep015": "row kernel; 17-20 buckets",
    "sweep017": "one-wave NPASS 1; 17-20 buckets",
    "sweep065": "one-wave NPASS 2",
    "sweep129": "one-wave NPASS 4 with a one-node pass; candidates that never wait",
    "d_partly_used": "non-zero initial usage",
    "e_all_at_time_zero": "ties broken by rank only",
    "f_zero_durations": "one-wave NPASS 1, zero durations",
    "j_many_classes": "a <= 16-node shape the row kernel refuses: one-wave NPASS 1",
    "i_pods257": "the rank index across a 256 boundary",
}
FAMILY_BATCHES = ("mixed", "aborts_random_linear")   # 11 and 5 policies: an idle row in the last wave
PROGRAM_SHAPES = ("sweep005", "sweep015", "sweep033", "sweep065", "sweep129")   # two-wave x2, one-wave NPASS 1 / 2 / 4
MAX_DEFERRED = 2


def _he():
    from funsearch_kubernetes_simulator_amd.ops import hip_engine as he
    if not he.device_available():
        pytest.fail("GPU test collected but no HIP device is visible")
    return he


def _device(workload, **options):
    return _he().DeviceEvaluator(workload, options={"trace_hash": True, **options})


_oracle = {}


def _frozen(key, make):
    if key not in _oracle:
        tm = make()
        for f in tm.RAW + ("rows",):
            getattr(tm, f).setflags(write=False)
        _oracle[key] = tm
    return _oracle[key]


def family_oracle(name, family, weights, key):
    """The CPU oracle's time metrics, computed once per (shape, batch) and left unchanged."""
    return _frozen((name, key), lambda: ce.time_builtin_batch(ds.shape(name), family, weights))


def program_oracle(name):
    return _frozen((name, "programs"), lambda: ce.time_program_batch(ds.program_workload(name), ds.programs()[1]))


def _same_records(got, want, what, rows=None):
    for i in (range(len(want)) if rows is None else rows):
        for f in TimeMetricsBatch.RAW:
            g, w = getattr(got, f)[i], getattr(want, f)[i]
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, i, f, np.asarray(g).tolist(), np.asarray(w).tolist())


@pytest.mark.parametrize("name", list(FAMILY_SHAPES))
def test_family_records_match_oracle(name):
    w = ds.shape(name)
    dev = _device(w)
    assert dev.info()["npass"] == ds.expected_npass(w.cluster.n_nodes)
    for batch in FAMILY_BATCHES:
        family, weights = ds.candidates()[batch]
        rows_kernel = dev._eng.would_use_rows(len(weights))
        assert rows_kernel == ds.rows_expected(name), (name, batch)
        want = family_oracle(name, family, weights, batch)
        got = dev.time_builtin(family, weights)
        assert dev.info()["time_instance_last"] == ("rows_mixed" if rows_kernel else "wave_mixed")
        assert got.engine == ["hip"] * len(weights)
        assert np.array_equal(got.rows, want.rows), (name, batch, np.argwhere(got.rows != want.rows)[:8].tolist())
        rows = dev.evaluate_builtin(family, weights)   # the default launch: bit for bit the same rows
        assert np.array_equal(got.rows, rows), (name, batch, np.argwhere(got.rows != rows)[:8].tolist())
        _same_records(got, want, (name, batch))
        if batch in ds.ABORT_BATCHES:
            raised = got.rows[:, 10] != 0
            assert raised.tolist() == [False, True, True, True, True]
            for f in got.RAW:
                assert not getattr(got, f)[raised].any(), (name, f)
            assert got.n_placed[0] > 0 and got.busy[0].any() and got.hist[0].sum() == got.n_placed[0]   # the clean row, intact


@pytest.mark.parametrize("name", ("sweep005", "sweep015"))
def test_composite_instance(name):
    """A composite-only batch runs the composite time instance (the default launch's waves per SIMD)."""
    w = ds.shape(name)
    dev = _device(w)
    family, weights = ds.candidates()["composite_linear"]
    want = family_oracle(name, family, weights, "composite_linear")
    got = dev.time_builtin(family, weights)
    assert dev.info()["time_instance_last"] == "rows_composite"
    assert np.array_equal(got.rows, want.rows)
    assert np.array_equal(got.rows, dev.evaluate_builtin(family, weights))
    _same_records(got, want, (name, "composite_linear"))
    assert (got.n_placed > 0).any() and len(set(got.wait_sum.tolist())) > 1


def test_accumulators_reset_between_a_rows_replays():
    """One wave: each of its four rows chains nine or ten replays, every one from zeroed accumulators."""
    name = "sweep005"
    rng = np.random.default_rng(38)
    from funsearch_kubernetes_simulator_amd.models import families as fam
    weights = fam.pad_weights(fam.SAMPLERS["composite_linear"](38, rng))
    dev = _device(ds.shape(name), row_wave_share=1e-6)
    want = family_oracle(name, "composite_linear", weights, "composite38")
    got = dev.time_builtin("composite_linear", weights)
    assert dev.info()["time_instance_last"] == "rows_composite"
    assert np.array_equal(got.rows, want.rows)
    _same_records(got, want, (name, "composite38"))
    assert len(set(got.wait_sum.tolist())) >= 6 and (got.wait_sum > 2 ** 32).all()


def test_time_mode_refuses_the_invariant_checker():
    family, weights = ds.candidates()["mixed"]
    dev = _device(ds.shape("sweep017"), check_invariants=61)
    with pytest.raises(ValueError, match="check_invariants"):
        dev.time_builtin(family, weights)


@pytest.mark.parametrize("name", PROGRAM_SHAPES)
def test_program_records_match_cpu_vm(name):
    w = ds.program_workload(name)
    dev = _device(w)
    assert dev.info()["npass"] == ds.expected_npass(w.cluster.n_nodes)
    groups, progs = ds.programs()
    want = program_oracle(name)
    got = dev.time_native(progs)
    assert dev.info()["time_instance_last"] == ("duo_native" if w.cluster.n_nodes <= 16 else "wave_native")
    rows = dev.evaluate_native(progs)
    assert np.array_equal(got.rows, rows), (name, np.argwhere(got.rows != rows)[:8].tolist())
    deferred = []
    for i, (g, p) in enumerate(zip(groups, progs)):
        if int(got.rows[i, 10]) == Exc.UNSUPPORTED and int(want.rows[i, 10]) != Exc.UNSUPPORTED:
            deferred.append((i, g, p.source[-160:]))
            continue
        assert np.array_equal(got.rows[i], want.rows[i]), (name, i, g, got.rows[i].tolist(), want.rows[i].tolist())
        _same_records(got, want, name, [i])
    # as tests/test_gpu_schedule.py: only corpus programs may be deferred to the host, two at the most
    assert all(g == "corpus" for _, g, _ in deferred) and len(deferred) <= MAX_DEFERRED, (name, deferred)
    if deferred:
        from funsearch_kubernetes_simulator_amd.engine import Evaluator
        ev = Evaluator(w, device="gpu", options={"trace_hash": True})
        routed = ev.time_programs([progs[i].source for i, _, _ in deferred])
        for j, (i, _, src) in enumerate(deferred):
            print(f"deferred to the host: {name} program {i}: {src!r} -> {routed.engine[j]}")
            assert routed.engine[j] in ("cpu", "object")
            assert np.array_equal(routed.rows[j, :12], want.rows[i, :12])
            for f in routed.RAW:
                assert np.array_equal(getattr(routed, f)[j], getattr(want, f)[i]), (name, i, f)


def test_time_metrics_on_the_default_trace():
    """The only full-trace test: first-fit and best-fit as program texts through `engine.time_metrics`, one launch."""
    from funsearch_kubernetes_simulator_amd import engine
    from funsearch_kubernetes_simulator_amd.core import load_default_workload
    from funsearch_kubernetes_simulator_amd.models.library import reference_policies, reference_scores
    from funsearch_kubernetes_simulator_amd.policy.compiler import compile_policy
    codes = [reference_policies()["first_fit"], reference_policies()["best_fit"]]
    got = engine.time_metrics(codes, device="auto")
    assert got.engine == ["hip-native"] * 2
    want = ce.time_program_batch(load_default_workload(), [compile_policy(c) for c in codes])
    assert np.array_equal(got.rows[:, :12], want.rows[:, :12])
    assert got.rows[:, 0].tolist() == [reference_scores()["first_fit"], reference_scores()["best_fit"]]
    _same_records(got, want, "default trace")
    assert (got.n_placed == 8152).all() and (got.wait_sum > 0).all()
