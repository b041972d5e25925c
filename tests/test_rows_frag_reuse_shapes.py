"""CPU preconditions of tests/test_gpu_rows_frag_reuse.py.

The device tests can only catch a wrong reuse of the row kernel's stashed
fragmentation sample if the workloads of `frag_reuse_shapes` hold every event
order the reuse rule tells apart.  A recording subclass of the CPython object
engine's `KubernetesSimulator` counts them here, so a later edit cannot hollow
those tests out:

* failure directly after failure (the stash is reused);
* failure, deletion, failure and failure, placement, failure (it must not be);
* a GPU pod's first failure directly after a failure (the waiting histogram
  has just changed), on workload A also with a gpu_milli below every waiting
  pod's, which lowers the smallest waiting class.
"""
import numpy as np
import pytest

import frag_reuse_shapes as fr
from funsearch_kubernetes_simulator_amd.funsearch.scheduler import FunSearchScheduler
from funsearch_kubernetes_simulator_amd.models import families as fam
from funsearch_kubernetes_simulator_amd.ops import cpu_engine as ce
from funsearch_kubernetes_simulator_amd.simulator import DiscreteEventSimulator, KubernetesSimulator, SchedulingEvaluator

WORKLOADS = {"a": fr.workload_a, "b": fr.workload_b}


class RecordingSimulator(KubernetesSimulator):
    """Logs one letter per event: D deletion, P placement, F failed retry (or a
    first failure without a GPU), G a GPU pod's first failure, L such a first
    failure whose gpu_milli is below every waiting GPU pod's."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.log = []

    def _handle_deletion(self, event):
        super()._handle_deletion(event)
        self.log.append("D")

    def _handle_creation(self, event):
        pod = event.pod
        fresh = pod not in self.waiting_pods
        waiting = [p.gpu_milli for p in self.waiting_pods if p.num_gpu > 0]
        super()._handle_creation(event)
        if pod.assigned_node != "":
            self.log.append("P")
        elif fresh and pod.num_gpu > 0:
            self.log.append("L" if waiting and pod.gpu_milli < min(waiting) else "G")
        else:
            self.log.append("F")


def replay_log(workload, weights):
    """(event letters, the exception that ended the replay or None)"""
    cluster, pods = workload.to_objects()
    sim = RecordingSimulator(cluster, pods, DiscreteEventSimulator(pods),
                             FunSearchScheduler(fam.to_program("composite_linear", weights)),
                             evaluator=SchedulingEvaluator(cluster, enabled=True), track_max_nodes=False)
    try:
        sim.run_schedule()
    except Exception as exc:   # a policy exception aborts the replay
        return "".join(sim.log), exc
    return "".join(sim.log), None


def transitions(workload, weights) -> dict:
    log, exc = replay_log(workload, weights)
    assert exc is None
    fail = "FGL"
    pairs = list(zip(log, log[1:]))
    triples = list(zip(log, log[1:], log[2:]))
    return {"events": len(log),
            "fail_fail": sum(a in fail and b in fail for a, b in pairs),
            "fail_del_fail": sum(a in fail and b == "D" and c in fail for a, b, c in triples),
            "fail_place_fail": sum(a in fail and b == "P" and c in fail for a, b, c in triples),
            "fail_fresh_gpu": sum(a in fail and b in "GL" for a, b in pairs),
            "fail_fresh_gpu_lower": sum(a in fail and b == "L" for a, b in pairs)}


@pytest.mark.parametrize("name", list(WORKLOADS))
def test_oracle_replays_are_long_complete_and_told_apart(name):
    tab = ce.simulate_builtin_batch(WORKLOADS[name](), "composite_linear", fr.composite_candidates())
    assert not tab[:, 10].any() and not tab[:, 9].any()          # no exception, nothing unplaced
    # 300 / 360 pods replay 17.5-25.4k events: most events are failed retries
    assert (tab[:, 8] >= 15000).all(), tab[:, 8]
    assert (tab[:, 7] >= 10000).all(), tab[:, 7]                  # fragmentation events
    # the samples are not all 0 and differ between candidates (5 and 7 distinct
    # means): one reused where it should have been recomputed moves the mean
    frag = tab[:, 5]
    assert (frag > 0).all() and len(set(frag.tolist())) >= 4, frag


@pytest.mark.parametrize("name", list(WORKLOADS))
def test_every_event_order_of_the_reuse_rule_occurs(name):
    w = WORKLOADS[name]()
    oracle = ce.simulate_builtin_batch(w, "composite_linear", fr.composite_candidates()[:3])
    for i in range(3):
        t = transitions(w, fr.composite_candidates()[i])
        assert t["events"] == int(oracle[i, 8]), (i, t)          # the object engine replays what the oracle does
        assert t["fail_fail"] >= 10000, (i, t)
        assert t["fail_del_fail"] >= 100, (i, t)
        assert t["fail_place_fail"] >= 100, (i, t)
        assert t["fail_fresh_gpu"] >= 100, (i, t)
        if name == "a":
            assert t["fail_fresh_gpu_lower"] >= 3, (i, t)


class _ScoreOutOfRange(Exception):
    pass


def abort_point(workload, weights):
    """Where the oracle and the device end a replay whose scorer leaves the
    int64 range (CPython itself goes on with big integers): (events before,
    kind of the event before, the last fragmentation sample before)."""
    cluster, pods = workload.to_objects()
    ev = SchedulingEvaluator(cluster, enabled=True)
    sched = FunSearchScheduler(fam.to_program("composite_linear", weights))

    def guarded(pod, node):
        s = sched(pod, node)
        if abs(s) >= 2 ** 63:
            raise _ScoreOutOfRange()
        return s

    sim = RecordingSimulator(cluster, pods, DiscreteEventSimulator(pods), guarded, evaluator=ev, track_max_nodes=False)
    with pytest.raises(_ScoreOutOfRange):
        sim.run_schedule()
    return len(sim.log), sim.log[-1], ev.fragmentation_events[-1]


def test_cpu_hog_fails_first_and_marked_rows_abort_after_failures():
    """The policy-switch workload: the added pod's failure is the first event of
    every replay and adds no waiting class, so its sample is 0; the marked
    candidates abort mid-replay, and at least four of them right after a failed
    placement whose sample was above 0 -- what a row would hand to its next
    policy if the start of a replay did not drop it."""
    w = fr.workload_a_cpu_hog()
    assert w.pods.n_pods == fr.workload_a().pods.n_pods + 1
    weights, marked = fr.switch_batch()
    tab = ce.simulate_builtin_batch(w, "composite_linear", weights)
    assert (tab[marked, 10] != 0).all() and not tab[~marked, 10].any()
    assert (tab[~marked, 7] >= 1).all()
    log, exc = replay_log(w, weights[0])
    assert exc is None and log[0] == "F" and len(log) == int(tab[0, 8])
    stale = 0
    for i in np.flatnonzero(marked):
        n, before, sample = abort_point(w, weights[i])
        assert n >= 20, (i, n)
        stale += before in "FGL" and sample > 0
    assert stale >= 4, stale
