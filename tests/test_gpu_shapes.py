"""Device engines vs the CPU oracle on the shape catalogue (tests/device_shapes.py):
partly filled rows and passes, the NPASS 2 build, every side of the host gates.

Every comparison is `np.array_equal` on whole 13-column tables (trace hash
included) against `ce.simulate_builtin_batch` / `ce.simulate_program_batch`;
`tests/test_device_shapes.py` shows on the CPU that those rows are the
reference's, that the candidates are told apart and that placements fail.
Cases are named `<shape>-<engine / layout>`.
"""
import numpy as np
import pytest

import device_shapes as ds
from funsearch_kubernetes_simulator_amd.core import TraceSuite, Workload
from funsearch_kubernetes_simulator_amd.ops import cpu_engine as ce
from funsearch_kubernetes_simulator_amd.policy.bytecode import Exc
from funsearch_kubernetes_simulator_amd.simulator.metrics import suite_aggregate

pytestmark = pytest.mark.gpu

BATCHES = ("first_fit", "best_fit") + ds.FAMILIES + ("mixed",) + ds.ABORT_BATCHES
#: one shape per NPASS also runs with the device invariant checker on
CHECKED = ("sweep033", "sweep100", "sweep193")
#: the NPASS 4 shape that runs both repush rules
BOTH_REPUSH = "sweep129"


def _he():
    from funsearch_kubernetes_simulator_amd.ops import hip_engine as he
    if not he.device_available():
        pytest.fail("GPU test collected but no HIP device is visible")
    return he


def _device(workload, options):
    return _he().DeviceEvaluator(workload, options={"trace_hash": True, **options})


# ---- CPU oracle, computed once per (workload, batch, repush rule) ------------------------

_oracle_cache = {}


def builtin_oracle(w, family, weights, repush="first"):
    weights = np.asarray(weights, dtype=np.float64)
    ck = (w.name, w.pods.n_pods, family if isinstance(family, str) else tuple(family), weights.tobytes(), repush)
    if ck not in _oracle_cache:
        opts = ce.SimOptions(repush=repush)
        if isinstance(family, str):
            tab = ce.simulate_builtin_batch(w, family, weights, opts)
        else:
            tab = np.zeros((len(family), 13))
            for f in sorted(set(family)):
                idx = [i for i, g in enumerate(family) if g == f]
                tab[idx] = ce.simulate_builtin_batch(w, f, weights[idx], opts)
        tab.setflags(write=False)
        _oracle_cache[ck] = tab
    return _oracle_cache[ck]


def _same(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:8].tolist())


# ---- built-in kernels ------------------------------------------------------------------

def builtin_layouts(name):
    """(layout id, options, row kernel expected) of every built-in launch path the shape can take."""
    n, rows = ds.n_nodes(name), ds.rows_expected(name)
    out = [("auto", {}, rows)]
    if rows:
        out += [("rows-top1", {"row_kernel": "on", "row_heap_top": 1}, True),
                ("rows-top63", {"row_kernel": "on", "row_heap_top": 63}, True)]
    wave = {"row_kernel": "off"}
    if ds.expected_npass(n) == 4:
        wave["wave_duo"] = False
        out += [("duo-hbm-top0", {"wave_duo": True, "heap_mode": "hbm", "heap_top": 0}, False),
                ("duo-hbm-top63", {"wave_duo": True, "heap_mode": "hbm", "heap_top": 63}, False)]
        if name == BOTH_REPUSH:
            out += [("duo-hbm-earliest", {"wave_duo": True, "heap_mode": "hbm", "repush": "earliest"}, False),
                    ("wave-hbm-earliest", {**wave, "heap_mode": "hbm", "repush": "earliest"}, False)]
    out += [("wave-lds", {**wave, "heap_mode": "lds"}, False),
            ("wave-hbm-top0", {**wave, "heap_mode": "hbm", "heap_top": 0}, False),
            ("wave-hbm-top63", {**wave, "heap_mode": "hbm", "heap_top": 63}, False)]
    if name in CHECKED:
        out += [("wave-lds-checked", {**wave, "heap_mode": "lds", "check_invariants": 61}, False)]
    return out


BUILTIN_CASES = [(name, lay) for name in ds.SHAPES for lay in builtin_layouts(name)]


@pytest.mark.parametrize("name,layout", BUILTIN_CASES, ids=[f"{n}-{lay[0]}" for n, lay in BUILTIN_CASES])
def test_builtin_kernels_match_oracle(name, layout):
    lid, options, rows = layout
    w = ds.shape(name)
    dev = _device(w, options)
    info = dev.info()
    for key, val in ds.expected_info(name).items():
        assert info[key] == val, (key, info[key])
    assert info["wave_duo"] == bool(options.get("wave_duo", False))
    cands = ds.candidates()
    for batch in BATCHES:
        family, weights = cands[batch]
        assert dev._eng.would_use_rows(len(weights)) == rows, batch
        got = dev.evaluate_builtin(family, weights)
        _same(got, builtin_oracle(w, family, weights, options.get("repush", "first")), (name, lid, batch))
        if "check_invariants" in options and batch not in ds.ABORT_BATCHES:
            assert not got[:, 10].any(), (batch, got[:, 10])   # no INVARIANT row: the accounting held


# ---- device VM and native programs -------------------------------------------------------

def program_layouts(name):
    """(layout id, engine, options): N <= 16 runs the native row kernel with one
    and four programs per wave, the two-wave kernel and the one-wave kernel;
    larger clusters the one-wave kernel with either heap."""
    out = [("vm-lds", "vm", {"heap_mode": "lds"}), ("vm-hbm", "vm", {"heap_mode": "hbm"})]
    if ds.rows_expected(name):
        out += [("native-rows1", "native", {"row_kernel": "on", "native_rows": 1, "native_duo": False}),
                ("native-rows4", "native", {"row_kernel": "on", "native_rows": 4}),
                ("native-duo", "native", {"row_kernel": "on", "native_rows": 1, "native_duo": True}),
                ("native-wave", "native", {"row_kernel": "off"})]
    else:
        out += [("native-wave-lds", "native", {"row_kernel": "off", "heap_mode": "lds"}),
                ("native-wave-hbm", "native", {"row_kernel": "off", "heap_mode": "hbm"})]
    return out


PROGRAM_CASES = [(name, lay) for name in ds.PROGRAM_SHAPES for lay in program_layouts(name)]
MAX_DEFERRED = 2
_routed = {}   # (shape, program index) -> the routed result equalled the CPU VM's


def _routed_equals_cpu_vm(name, i):
    """A program the device deferred, through the engine's own routing."""
    if (name, i) not in _routed:
        from funsearch_kubernetes_simulator_amd.engine import Evaluator
        res = Evaluator(ds.program_workload(name), device="gpu").evaluate_programs([ds.programs()[1][i].source])[0]
        want = ds.program_oracle(name)[i]
        _routed[(name, i)] = (res.score == want[0] and res.exc == int(want[10]), res.engine, res.score, want[0])
    return _routed[(name, i)]


def _check_programs(name, got, what):
    groups, progs = ds.programs()
    want = ds.program_oracle(name)
    assert got.shape == want.shape
    deferred = []
    for i, (g, p) in enumerate(zip(groups, progs)):
        if int(got[i, 10]) == Exc.UNSUPPORTED and int(want[i, 10]) != Exc.UNSUPPORTED:
            deferred.append((i, g, p.source[-160:]))
            continue
        assert np.array_equal(got[i], want[i]), (what, i, g, p.source[-300:], got[i].tolist(), want[i].tolist())
    # only corpus programs may be deferred to the host, two at the most, each named here
    assert all(g == "corpus" for _, g, _ in deferred) and len(deferred) <= MAX_DEFERRED, (what, deferred)
    for i, _, src in deferred:
        print(f"deferred to the host: {what} program {i}: {src!r}")
        ok = _routed_equals_cpu_vm(name, i)
        assert ok[0], (what, i, src, ok)


@pytest.mark.parametrize("name,layout", PROGRAM_CASES, ids=[f"{n}-{lay[0]}" for n, lay in PROGRAM_CASES])
def test_programs_match_cpu_vm(name, layout):
    lid, engine, options = layout
    w = ds.program_workload(name)
    dev = _device(w, options)
    info = dev.info()
    assert info["npass"] == ds.expected_npass(w.cluster.n_nodes)
    progs = ds.programs()[1]
    if engine == "vm":
        got = dev.evaluate_programs(progs)
    else:
        assert dev._eng.would_use_rows(len(progs)) == (options["row_kernel"] == "on")
        got = dev.evaluate_native(progs)
        if "native_rows" in options:
            assert dev.info()["native_rows_last"] == (0 if options.get("native_duo") else options["native_rows"])
    _check_programs(name, got, (name, lid))


def test_program_service_on_five_nodes():
    """64 programs in one batch through the resident service on the 5-node
    shape == the per-batch launch on the same evaluator == the CPU VM."""
    name = "sweep005"
    dev = _device(ds.program_workload(name), {})
    groups, progs = ds.programs()
    pick = [i % len(progs) for i in range(64)]
    batch = [progs[i] for i in pick]
    want = dev.evaluate_native(batch)
    info = dev.start_service(slots=64, share=0.25)
    try:
        assert info["blocks"] >= 1 and info["slots"] == 64
        got = dev.evaluate_native(batch)
        sv = dev.info()["service"]
        assert sv["running"] and sv["published"] >= 64 - 2 * MAX_DEFERRED
    finally:
        dev.stop_service()
    assert dev.service is None
    _same(got, want, "service vs batch launch")
    _check_programs(name, got[:len(progs)], (name, "service"))
    _same(got[len(progs):], got[:64 - len(progs)], "repeated programs")


# ---- routing ---------------------------------------------------------------------------

ROUTED = ("sweep015", "sweep100", "sweep193")   # NPASS 1 (row kernel), 2 and 4


@pytest.mark.parametrize("name", ROUTED)
def test_evaluator_routes_family_batches_to_the_device(name):
    from funsearch_kubernetes_simulator_amd.engine import Evaluator
    _he()
    w = ds.shape(name)
    ev = Evaluator(w, device="auto")
    assert ev.backend == "hip" and ev.device.info()["npass"] == ds.expected_npass(w.cluster.n_nodes)
    for f in ds.FAMILIES:
        weights = ds.candidates()[f][1]
        _same(ev.evaluate_family(f, weights), builtin_oracle(w, f, weights), (name, f))


def test_evaluator_keeps_a_refused_shape_on_the_cpu():
    """Shape (l) above 128 nodes: `device="auto"` falls through to the CPU
    engine, `device="gpu"` raises."""
    from funsearch_kubernetes_simulator_amd.engine import Evaluator
    he = _he()
    w = ds.wide_gpu_milli(130)
    weights = ds.candidates()["composite_linear"][1]
    ev = Evaluator(w, device="auto")
    assert ev.backend == "cpu"
    _same(ev.evaluate_family("composite_linear", weights), builtin_oracle(w, "composite_linear", weights), w.name)
    with pytest.raises(he.UnsupportedWorkload):
        Evaluator(w, device="gpu")


@pytest.mark.parametrize("name", ROUTED)
def test_suite_evaluator_on_each_npass(name):
    """A `TraceSuite` holds traces of one cluster, so the three NPASS values
    take three suites: the shape's trace, its first half and its first 257 pods."""
    from funsearch_kubernetes_simulator_amd.engine import SuiteEvaluator
    _he()
    w = ds.shape(name)
    traces = [w] + [Workload(w.cluster, w.pods.subset(np.arange(k)), f"{name}[:{k}]")
                    for k in (w.pods.n_pods // 2, 257)]
    ev = SuiteEvaluator(TraceSuite(traces), device="auto")
    assert ev.backend == "hip" and all(d.info()["npass"] == ds.expected_npass(w.cluster.n_nodes) for d in ev.devices)
    for batch in ("composite_linear", "mixed"):
        family, weights = ds.candidates()[batch]
        tables, agg = ev.evaluate_family(family, weights)
        want = np.stack([builtin_oracle(t, family, weights) for t in traces])
        for k, t in enumerate(traces):
            _same(tables[k], want[k], (t.name, batch))
        assert np.array_equal(agg, suite_aggregate(want))
