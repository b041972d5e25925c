"""SuiteEvaluator's program interface on the CPU backend: score_programs, the
submit / wait slots and tools/suite_report.py on a program policy.

The suite is that of tests/test_gpu_suite.py -- sub-traces of the shipped
16-node cluster with three pod counts, A = default[:257], B = default[:600],
C = cpu037[:1500] -- and the programs are the compiled corpus of
tests/program_corpus.py (60 programs), as program texts.  The GPU tests of
tests/test_gpu_suite_programs.py take both from here.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from funsearch_kubernetes_simulator_amd.core import TraceParser, TraceSuite, Workload
from funsearch_kubernetes_simulator_amd.engine import SuiteEvaluator
from funsearch_kubernetes_simulator_amd.models.library import reference_policies
from funsearch_kubernetes_simulator_amd.ops import cpu_engine as ce
from funsearch_kubernetes_simulator_amd.policy.bytecode import Exc
from funsearch_kubernetes_simulator_amd.simulator.metrics import exact_mean

from program_corpus import programs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLINED = (int(Exc.UNSUPPORTED), int(Exc.BUDGET))


def _prefix(w, n, name):
    return Workload(w.cluster, w.pods.subset(np.arange(n)), name)


@pytest.fixture(scope="session")
def traces(default_workload):
    cpu037 = TraceParser().load_workload(pod_file="openb_pod_list_cpu037.csv")
    return {"A": _prefix(default_workload, 257, "A"), "B": _prefix(default_workload, 600, "B"),
            "C": _prefix(cpu037, 1500, "C"), "default": default_workload, "cpu037": cpu037}


@pytest.fixture(scope="session")
def progs():
    out = programs()
    assert len(out) == 60
    return out


@pytest.fixture(scope="session")
def codes(progs):
    return [p.source for p in progs]


_vm_cache = {}


def vm_table(traces, key, lo=0, hi=None):
    """Rows [lo, hi) of the CPU VM's result table [60, 13] of the corpus on one
    trace; the table is computed once per trace."""
    if key not in _vm_cache:
        tab = ce.simulate_program_batch(traces[key], programs(), threads=16)
        tab.setflags(write=False)
        _vm_cache[key] = tab
    return _vm_cache[key][lo:hi]


def suite_of(traces, keys):
    return TraceSuite([traces[k] for k in keys], list(keys))


@pytest.fixture(scope="session")
def cpu_abc(traces):
    ev = SuiteEvaluator(suite_of(traces, "ABC"), device="cpu")
    assert ev.backend == "cpu"
    return ev


@pytest.fixture(scope="session")
def cpu_results(cpu_abc, codes):
    """evaluate_programs of the whole corpus on the CPU backend, once: [T][P] EvalResult."""
    return cpu_abc.evaluate_programs(codes)


def expected_aggregate(scores, raised):
    """The suite aggregate rule, written out: exact mean, minimum, first minimum, raising traces."""
    scores = np.where(raised, 0.0, scores)
    agg = np.zeros((scores.shape[1], 4))
    for p in range(scores.shape[1]):
        col = scores[:, p].tolist()
        agg[p] = [exact_mean(col), min(col), col.index(min(col)), int(raised[:, p].sum())]
    return agg


def test_subtraces_exercise_the_program_paths(traces, progs):
    """Preconditions (CPU VM), per sub-trace: fragmentation events, distinct
    scores, policy exceptions; at most one program declined."""
    for key in "ABC":
        tab = vm_table(traces, key)
        exc = tab[:, 10].astype(int)
        declined = np.isin(exc, DECLINED)
        assert int((tab[:, 7] > 0).sum()) * 4 >= len(progs), key
        assert len(set(tab[:, 0].tolist())) >= 20, key
        assert int(((exc != 0) & ~declined).sum()) >= 3, key
        assert int(declined.sum()) <= 1, key
        assert not tab[~declined, 11].any(), key


def test_score_programs_cpu(cpu_abc, cpu_results, codes):
    scores, agg = cpu_abc.score_programs(codes)
    assert scores.shape == (3, len(codes)) and agg.shape == (len(codes), 4)
    want = np.array([[r.score for r in row] for row in cpu_results])
    raised = np.array([[r.exc != 0 for r in row] for row in cpu_results])
    assert np.array_equal(scores, want)
    assert np.array_equal(agg, expected_aggregate(want, raised))
    assert np.array_equal(agg[:, 3], raised.sum(axis=0))
    assert raised.any() and (want[raised] == 0.0).all()


def test_program_slots_cpu(cpu_abc, cpu_results, codes):
    a, b = codes[:10], codes[10:22]
    want = np.array([[r.score for r in row] for row in cpu_results])
    raised = np.array([[r.exc != 0 for r in row] for row in cpu_results])
    cpu_abc.submit_programs(1, a)
    cpu_abc.submit_programs(2, b)
    with pytest.raises(RuntimeError):
        cpu_abc.submit_programs(1, b)   # slot 1 still holds a batch
    sb, ab = cpu_abc.wait_programs(2)
    sa, aa = cpu_abc.wait_programs(1)
    assert np.array_equal(sa, want[:, :10]) and np.array_equal(sb, want[:, 10:22])
    assert np.array_equal(aa, expected_aggregate(want[:, :10], raised[:, :10]))
    assert np.array_equal(ab, expected_aggregate(want[:, 10:22], raised[:, 10:22]))
    s2, a2 = cpu_abc.score_programs(a)   # the synchronous call, same answers
    assert np.array_equal(s2, sa) and np.array_equal(a2, aa)
    with pytest.raises(ValueError):
        cpu_abc.wait_programs(1)


def test_suite_report_on_a_program_policy(tmp_path):
    policy = tmp_path / "first_fit_program.json"
    policy.write_text(json.dumps({"score": None, "code": reference_policies()["first_fit"]}))
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "suite_report.py"), str(policy),
                          "--suite", "default,cpu037", "--device", "cpu"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0].startswith("# program policy") and "2 traces" in lines[0]
    rows = [ln.split() for ln in lines[2:4]]
    assert [r[0] for r in rows] == ["default", "cpu037"] and [r[1] for r in rows] == ["8152", "7336"]
    assert all(r[-1] == "cpu" and r[-2] == "0" for r in rows)
    assert lines[4].startswith("mean ") and "traces raised 0" in lines[4]
