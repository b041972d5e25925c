"""CPU preconditions of tests/test_gpu_rows_scan_deletion.py.

The device tests can only catch a wrong first-pending-deletion scan if the
replays of `scan_deletion_shapes` put the first deletion in every position
the scan tells apart.  A recording subclass of the CPython object engine's
event queue notes, at every failed placement, the heap length n and the index
f of the first DELETION in array order (-1: none) -- the heap array is the one
the device keeps (CPython's heapq, move for move) -- and the tests assert:

* f = 0; f odd and f even (the two halves of a lane's pair);
* f in {31, 32, 33}: either side of the first 32-slot step;
* f = n - 1 (the last live slot), also with n = 32, 64 and 128: slot n - 1 is
  then the first slot of a 32-slot step and the only live one in it;
* f >= 64 and f >= 128: beyond an LDS heap top of 63 and of 127 slots;
* no deletion at all with n <= 2 and with n no multiple of 32.
"""
import numpy as np
import pytest

import scan_deletion_shapes as sd
from funsearch_kubernetes_simulator_amd.funsearch.scheduler import FunSearchScheduler
from funsearch_kubernetes_simulator_amd.models import families as fam
from funsearch_kubernetes_simulator_amd.ops import cpu_engine as ce
from funsearch_kubernetes_simulator_amd.simulator import (DiscreteEventSimulator, EventType, KubernetesSimulator,
                                                          SchedulingEvaluator)


class RecordingQueue(DiscreteEventSimulator):
    """Logs (n, f) whenever a failed placement looks for its anchor."""

    def __init__(self, pods):
        super().__init__(pods)
        self.scans = []

    def repush_creation_event(self, pod):
        heap = self.event_heap
        f = next((i for i, (_, ev) in enumerate(heap) if ev.event_type == EventType.DELETION), -1)
        self.scans.append((len(heap), f))
        return super().repush_creation_event(pod)


def scans(workload, program_text):
    """([failures, 2] array of (n, f), events processed)"""
    cluster, pods = workload.to_objects()
    queue = RecordingQueue(pods)
    sim = KubernetesSimulator(cluster, pods, queue, FunSearchScheduler(program_text),
                              evaluator=SchedulingEvaluator(cluster, enabled=True), track_max_nodes=False)
    sim.run_schedule()
    return np.array(queue.scans, dtype=np.int64).reshape(-1, 2), sim.events_processed


@pytest.mark.parametrize("i", (0, 1))
def test_composite_replays_put_the_first_deletion_everywhere(i):
    w = sd.workload()
    weights = sd.batches()["composite_linear"][1]
    oracle = ce.simulate_builtin_batch(w, "composite_linear", weights[i:i + 1])
    s, events = scans(w, fam.to_program("composite_linear", weights[i]))
    assert events == int(oracle[0, 8]) and not oracle[0, 10]      # the object engine replays what the oracle does
    assert int(oracle[0, 9]) == 4                                  # the four pods that fit nowhere are dropped
    n, f = s[:, 0], s[:, 1]
    hit = f >= 0
    assert len(s) >= 10000 and (f < n).all()
    assert (f == 0).sum() >= 100
    assert (f % 2 == 1).sum() >= 1000 and ((f % 2 == 0) & (f > 0)).sum() >= 1000
    for edge in (31, 32, 33):
        assert (f == edge).sum() >= 20, edge
    assert (hit & (f == n - 1) & (f >= 2)).sum() >= 5
    assert (f >= 64).sum() >= 1000 and (f >= 128).sum() >= 300
    none_n = sorted(n[~hit].tolist())
    assert none_n == [0, 1, 2, w.pods.n_pods - 1], none_n
    assert (w.pods.n_pods - 1) % 32 != 0


@pytest.mark.parametrize("waiting", list(sd.QUEUES))
def test_queue_replays_end_a_heap_of_32k_entries_on_its_only_deletion(waiting):
    w = sd.queue(waiting)
    weights = sd.batches()["composite_linear"][1]
    oracle = ce.simulate_builtin_batch(w, "composite_linear", weights[:1])
    s, events = scans(w, fam.to_program("composite_linear", weights[0]))
    assert events == int(oracle[0, 8]) and not oracle[0, 10] and not oracle[0, 9]
    n, f = s[:, 0], s[:, 1]
    assert (f >= 0).all()
    for full in sd.QUEUES[waiting]:
        assert ((n == full) & (f == full - 1)).sum() >= 1, full


def test_programs_that_turn_feasible_nodes_away():
    w = sd.workload()
    tab = ce.simulate_program_batch(w, sd.programs())
    assert not tab[:, 10].any()
    never, picky = sd.program_texts()[2:]
    s, events = scans(w, never)
    # nothing is placed: one failure per pod, no deletion ever, every heap length once
    assert events == w.pods.n_pods == int(tab[2, 8]) == int(tab[2, 9])
    assert (s[:, 1] == -1).all() and sorted(s[:, 0].tolist()) == list(range(w.pods.n_pods))
    s, events = scans(w, picky)
    assert events == int(tab[3, 8]) and events >= 2000
    assert (s[:, 1] >= 64).sum() >= 100 and (s[:, 1] == -1).sum() >= 1
