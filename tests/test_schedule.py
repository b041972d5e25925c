"""Schedules on the CPU: each pod's node, GPU set and start time.

* the CPU oracle's schedules (`ce.schedule_builtin_batch`, `ce.schedule_program_batch`)
  against what the object engine (`simulator/cluster_sim.py`) leaves on its pods;
* against the reference's own simulator, from ``tests/golden/reference_schedules.json``
  (the first four cases of ``reference_parity_scores.json``: same sub-traces, same
  program texts; per pod the node index, the GPU index list and the final
  ``creation_time`` the reference left);

      python tests/test_schedule.py <reference checkout>

  records the file again, like ``tests/test_reference_parity.py`` records its own;
* `Schedule.validate` accepts every oracle schedule and rejects seeded
  corruptions, each for its own reason;
* the preconditions of the shapes ``tests/test_gpu_schedule.py`` runs, so the
  device comparison cannot pass vacuously;
* the routing of `Evaluator.schedule_programs`.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = os.path.join(GOLDEN_DIR, "reference_schedules.json")
PARITY = os.path.join(GOLDEN_DIR, "reference_parity_scores.json")
N_GOLDEN = 4

ORACLE_SHAPES = ("sweep005", "d_partly_used", "e_all_at_time_zero", "f_zero_durations")
GPU_SHAPES = ("sweep005", "sweep015", "sweep017", "sweep065", "sweep129", "d_partly_used", "e_all_at_time_zero",
              "f_zero_durations", "j_many_classes", "i_pods257")

DRIVER = r'''
import enum, json, sys, copy
if not hasattr(enum, "StrEnum"):
    class StrEnum(str, enum.Enum):
        @staticmethod
        def _generate_next_value_(name, start, count, last_values):
            return name.lower()
    enum.StrEnum = StrEnum
sys.path.insert(0, sys.argv[1])
from benchmarks.parser import TraceParser
from simulator.event_simulator import DiscreteEventSimulator
from simulator.main import KubernetesSimulator
from simulator.evaluator import SchedulingEvaluator
job = json.load(open(sys.argv[2]))
parser = TraceParser(sys.argv[1] + "/benchmarks/traces")
cluster0, pods0 = parser.parse_workload()
by_id = {p.pod_id: p for p in pods0}
out = []
for case in job:
    cluster = copy.deepcopy(cluster0)
    index = {nid: i for i, nid in enumerate(cluster.nodes_dict)}
    pods = [copy.deepcopy(by_id[i]) for i in case["pods"]]
    env = {"__builtins__": __builtins__}
    exec(case["code"], env)
    fn = env["priority_function"]
    sched = lambda pod, node: int(max(0, fn(pod, node)))
    ev = SchedulingEvaluator(cluster, enabled=True)
    sim = KubernetesSimulator(cluster, pods, DiscreteEventSimulator(pods), sched, evaluator=ev)
    sim.run_schedule()
    out.append({"node": [index[p.assigned_node] if p.assigned_node != "" else -1 for p in pods],
                "gpus": [list(p.assigned_gpus) for p in pods],
                "creation_time": [p.creation_time for p in pods]})
print(json.dumps(out))
'''


def _parity_cases():
    with open(PARITY) as f:
        return json.load(f)["cases"][:N_GOLDEN]


def _record(ref: str) -> None:
    from funsearch_kubernetes_simulator_amd.core import load_default_workload
    w = load_default_workload()
    cases = _parity_cases()
    with tempfile.TemporaryDirectory() as tmp:
        job, drv = os.path.join(tmp, "job.json"), os.path.join(tmp, "drv.py")
        with open(job, "w") as f:
            json.dump([{"pods": w.pods.pod_ids[c["start"]:c["start"] + c["n_pods"]], "code": c["code"]} for c in cases], f)
        with open(drv, "w") as f:
            f.write(DRIVER)
        r = subprocess.run([sys.executable, drv, ref, job], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    with open(GOLDEN, "w") as f:
        json.dump({"cases": [{"start": c["start"], "n_pods": c["n_pods"], **g} for c, g in zip(cases, got)]}, f,
                  separators=(",", ":"))
        f.write("\n")


# ---- helpers ---------------------------------------------------------------------------

def _shapes():
    import device_shapes as ds
    return ds


_cache = {}


def mixed_oracle(name):
    """The oracle's schedules of the "mixed" batch on a shape, computed once and left unchanged."""
    if name not in _cache:
        from funsearch_kubernetes_simulator_amd.ops import cpu_engine as ce
        ds = _shapes()
        family, weights = ds.candidates()["mixed"]
        sb = ce.schedule_builtin_batch(ds.shape(name), family, weights)
        for a in (sb.node, sb.gpu_mask, sb.start, sb.rows):
            a.setflags(write=False)
        _cache[name] = sb
    return _cache[name]


def _object_schedule(w, code):
    """node index, GPU set and start per pod as the object engine leaves them (None: the replay raised)."""
    from funsearch_kubernetes_simulator_amd.funsearch.scheduler import FunSearchScheduler
    from funsearch_kubernetes_simulator_amd.simulator import DiscreteEventSimulator, KubernetesSimulator, SchedulingEvaluator
    cluster, pods = w.to_objects()
    sim = KubernetesSimulator(cluster, pods, DiscreteEventSimulator(pods), FunSearchScheduler(code),
                              evaluator=SchedulingEvaluator(cluster, enabled=True))
    sim.run_schedule()
    index = {nid: i for i, nid in enumerate(w.cluster.node_ids)}
    return ([index[p.assigned_node] if p.assigned_node != "" else -1 for p in pods],
            [frozenset(p.assigned_gpus) for p in pods], [p.creation_time for p in pods], pods)


def _assert_equals_objects(s, obj, what):
    node, gpus, ctime, _ = obj
    assert s.node.tolist() == node, what
    for i in range(s.n_pods):
        assert frozenset(s.gpus(i)) == gpus[i], (what, i)
        if node[i] >= 0:
            assert int(s.start[i]) == ctime[i], (what, i)
        else:
            assert int(s.start[i]) == -1 and int(s.gpu_mask[i]) == 0, (what, i)


# ---- 1. the oracle against the object engine -----------------------------------------------

@pytest.mark.parametrize("name", ORACLE_SHAPES)
def test_oracle_families_match_object_engine(name):
    from funsearch_kubernetes_simulator_amd.models import families as fam
    ds = _shapes()
    w = ds.shape(name)
    family, weights = ds.candidates()["mixed"]
    sb = mixed_oracle(name)
    assert not sb.rows[:, 10].any()
    from funsearch_kubernetes_simulator_amd.models.library import reference_policies
    for i, f in enumerate(family):
        code = fam.to_program(f, weights[i]) if f in ds.FAMILIES else reference_policies()[f]
        _assert_equals_objects(sb[i], _object_schedule(w, code), (name, i, f))


@pytest.mark.parametrize("name", ORACLE_SHAPES)
def test_oracle_programs_match_object_engine(name):
    """The reference policies as programs, through the CPU VM."""
    from funsearch_kubernetes_simulator_amd.models.library import reference_policies
    from funsearch_kubernetes_simulator_amd.ops import cpu_engine as ce
    from funsearch_kubernetes_simulator_amd.policy.compiler import compile_policy
    w = _shapes().shape(name)
    codes = reference_policies()
    sb = ce.schedule_program_batch(w, [compile_policy(c) for c in codes.values()])
    assert not sb.rows[:, 10].any()
    for i, (pname, code) in enumerate(codes.items()):
        obj = _object_schedule(w, code)
        _assert_equals_objects(sb[i], obj, (name, pname))
        # apply() leaves on fresh pods what the object engine's run left on its own
        fresh = w.pods.to_objects()
        sb[i].apply(fresh)
        for a, b in zip(fresh, obj[3]):
            assert (a.assigned_node, sorted(a.assigned_gpus)) == (b.assigned_node, sorted(b.assigned_gpus)), a.pod_id
            if b.assigned_node != "":   # (a pod never placed keeps its trace creation time: a schedule has no start for it)
                assert a.creation_time == b.creation_time, (name, pname, a.pod_id)


def test_single_replay_returns_gpus_and_start():
    """`record_placements` of a single replay: the existing `placement` key, and the two new ones beside it."""
    from funsearch_kubernetes_simulator_amd.ops import cpu_engine as ce
    ds = _shapes()
    w = ds.shape("sweep005")
    family, weights = ds.candidates()["mixed"]
    r = ce.simulate_builtin(w, family[1], weights[1], ce.SimOptions(record_placements=True))
    s = mixed_oracle("sweep005")[1]
    assert list(r["placement"]) == s.node.tolist()
    assert np.array_equal(np.asarray(r["placement_gpus"]), s.gpu_mask)
    assert np.array_equal(np.asarray(r["placement_start"]), s.start)
    assert "placement_gpus" not in ce.simulate_builtin(w, family[1], weights[1])


# ---- 2. the oracle against the reference itself ----------------------------------------------

def test_oracle_matches_reference_schedules():
    from funsearch_kubernetes_simulator_amd.core import load_default_workload
    from funsearch_kubernetes_simulator_amd.core.arrays import Workload
    from funsearch_kubernetes_simulator_amd.engine import Evaluator
    assert os.path.getsize(GOLDEN) < 100 * 1024
    with open(GOLDEN) as f:
        golden = json.load(f)["cases"]
    cases = _parity_cases()
    assert len(golden) == N_GOLDEN == len(cases)
    w = load_default_workload()
    for g, c in zip(golden, cases):
        assert (g["start"], g["n_pods"]) == (c["start"], c["n_pods"])
        sub = Workload(w.cluster, w.pods.subset(np.arange(g["start"], g["start"] + g["n_pods"])))
        sb = Evaluator(sub, device="cpu").schedule_programs([c["code"]])
        assert sb.engine == ["cpu"] and sb.rows[0, 10] == 0 and sb.rows[0, 0] == float(c["score"])
        s = sb[0]
        assert s.node.tolist() == g["node"]
        placed = s.node >= 0
        assert s.start[placed].tolist() == [t for t, n in zip(g["creation_time"], g["node"]) if n >= 0]
        assert (s.start[~placed] == -1).all()
        for i in range(s.n_pods):
            assert set(s.gpus(i)) == set(g["gpus"][i]), (g["start"], i)
        s.validate(sub)


# ---- 3. validate ---------------------------------------------------------------------------

def _events_before(w, s, i):
    """Pods holding resources when pod i's start event is processed: started
    before it and not yet ended, in the heap's (time, rank, kind) order."""
    p = w.pods
    me = (int(s.start[i]), int(p.pod_rank[i]), 0)
    out = []
    for j in range(s.n_pods):
        if j == i or s.node[j] < 0:
            continue
        begin = (int(s.start[j]), int(p.pod_rank[j]), 0)
        end = (int(s.start[j]) + int(p.pod_dur[j]), int(p.pod_rank[j]), 1)
        if begin < me < end:
            out.append(j)
    return out


def _copy(s):
    from funsearch_kubernetes_simulator_amd.core.schedule import Schedule
    return Schedule(s.node.copy(), s.gpu_mask.copy(), s.start.copy(), s.row.copy(), s.engine, s.node_ids)


@pytest.mark.parametrize("name", ORACLE_SHAPES)
def test_validate_accepts_oracle_schedules(name):
    w = _shapes().shape(name)
    sb = mixed_oracle(name)
    for i in range(len(sb)):
        counts = sb[i].validate(w)
        assert counts["placed"] + counts["unplaced"] == w.pods.n_pods and counts["unplaced"] == int(sb.rows[i, 9])


@pytest.mark.parametrize("name", ("sweep005", "d_partly_used"))
def test_validate_rejects_seeded_corruptions(name):
    """Each corruption is built from the workload and the schedule with plain
    loops (`_events_before`), not with the validator, and must be rejected
    for its own reason, naming the pod.  The last one, a placed pod marked
    never placed, leaves a count that no longer matches the row: the schedule
    alone cannot tell which pod it was, so that message holds the two counts."""
    from funsearch_kubernetes_simulator_amd.core.schedule import ScheduleError
    w = _shapes().shape(name)
    c, p = w.cluster, w.pods
    good = mixed_oracle(name)[1]   # (a composite_linear row)
    good.validate(w)

    def rejected(s, pod, pattern):
        with pytest.raises(ScheduleError, match=pattern) as e:
            s.validate(w)
        if pod is not None:
            assert e.value.pod == pod and p.pod_ids[pod] in str(e.value), str(e.value)
        return str(e.value)

    # a pod without GPUs moved to a node whose cpu is taken when the pod starts
    done = False
    for i in np.flatnonzero((good.node >= 0) & (p.pod_ngpu == 0)):
        held = _events_before(w, good, i)
        for m in range(c.n_nodes):
            free = int(c.node_cpu_left[m]) - sum(int(p.pod_cpu[j]) for j in held if good.node[j] == m)
            if m != good.node[i] and free < p.pod_cpu[i]:
                s = _copy(good)
                s.node[i] = m
                rejected(s, int(i), rf"node {m} has cpu -\d+ left, below zero")
                done = True
                break
        if done:
            break
    assert done, "no pod / full node pair on this shape"

    # a GPU bit moved to a GPU of the same node without room for the pod's milli
    done = False
    for i in np.flatnonzero((good.node >= 0) & (p.pod_ngpu > 0)):
        n, held = int(good.node[i]), _events_before(w, good, i)
        for j in range(int(c.node_ngpus[n])):
            if (good.gpu_mask[i] >> j) & 1:
                continue
            free = int(c.gpu_milli_left[c.gpu_start[n] + j]) - sum(
                int(p.pod_gmilli[q]) for q in held if good.node[q] == n and (good.gpu_mask[q] >> j) & 1)
            if free < p.pod_gmilli[i]:
                s = _copy(good)
                low = int(s.gpu_mask[i]) & -int(s.gpu_mask[i])
                s.gpu_mask[i] = (int(s.gpu_mask[i]) & ~low) | (1 << j)
                rejected(s, int(i), rf"GPU {j} of node {n} has milli -\d+ left, below zero")
                done = True
                break
        if done:
            break
    assert done, "no GPU without room on this shape"

    placed = np.flatnonzero(good.node >= 0)
    # a start one tick before creation
    i = int(placed[np.argmin(good.start[placed] - p.pod_ctime[placed])])
    s = _copy(good)
    s.start[i] = p.pod_ctime[i] - 1
    rejected(s, i, "before its creation time")

    # a mask with a bit past the node's GPU count
    i = int(next(q for q in placed if p.pod_ngpu[q] > 0 and c.node_ngpus[good.node[q]] < 8))
    s = _copy(good)
    low = int(s.gpu_mask[i]) & -int(s.gpu_mask[i])
    s.gpu_mask[i] = (int(s.gpu_mask[i]) & ~low) | (1 << int(c.node_ngpus[good.node[i]]))
    rejected(s, i, "has a bit past the GPU count")

    # a placed pod marked never placed while n_unplaced stays
    i = int(placed[-1])
    s = _copy(good)
    s.node[i], s.gpu_mask[i], s.start[i] = -1, 0, -1
    rejected(s, None, rf"{int(good.row[9]) + 1} pods at node -1, the row's n_unplaced is {int(good.row[9])}")


def test_first_difference_and_wait():
    w = _shapes().shape("sweep005")
    sb = mixed_oracle("sweep005")
    a = sb[1]
    assert a.first_difference(_copy(a), w) is None
    b = _copy(a)
    placed = np.flatnonzero(a.node >= 0)
    order = placed[np.lexsort((w.pods.pod_rank[placed], a.start[placed]))]
    late, early = int(order[-1]), int(order[3])
    b.node[late] = (b.node[late] + 1) % w.cluster.n_nodes
    assert a.first_difference(b, w) == late
    b.start[early] += 1
    assert a.first_difference(b, w) == early and b.first_difference(a, w) == early
    wait = a.wait(w)
    assert (wait[placed] >= 0).all() and (wait[a.node < 0] == -1).all() and wait.max() > 0


# ---- 4. preconditions of the GPU shapes ------------------------------------------------------

@pytest.mark.parametrize("name", GPU_SHAPES)
def test_gpu_shapes_tell_schedules_apart(name):
    w = _shapes().shape(name)
    sb = mixed_oracle(name)
    assert len(sb) == 11 and not sb.rows[:, 10].any()
    assert len({sb.node[i].tobytes() for i in range(11)}) >= 4
    delayed = [(sb.start[i] > w.pods.pod_ctime)[sb.node[i] >= 0].any() for i in range(11)]
    assert any(delayed)
    if name == "sweep005":
        assert (sb.node < 0).any(axis=1).any()
    multi = (w.pods.pod_ngpu >= 2)[None, :] & (sb.node >= 0)
    assert multi.any()
    bits = np.array([[bin(int(m)).count("1") for m in row] for row in sb.gpu_mask])
    assert (bits[multi] >= 2).all()


# ---- 5. routing ----------------------------------------------------------------------------

def test_evaluator_routes_every_program_to_a_schedule():
    from funsearch_kubernetes_simulator_amd.engine import Evaluator, schedule
    from funsearch_kubernetes_simulator_amd.models.library import reference_policies
    from funsearch_kubernetes_simulator_amd.policy.bytecode import Exc
    from funsearch_kubernetes_simulator_amd.policy.template import PolicyTemplate
    w = _shapes().program_workload("sweep005")
    raising = PolicyTemplate.fill_template("    score = 1000 / (node.cpu_milli_left - node.cpu_milli_left)")
    cpython_only = PolicyTemplate.fill_template(
        "    score = node.cpu_milli_left * node.memory_mib_left * node.cpu_milli_total * node.memory_mib_total\n"
        "    score = score * 1000000 / 10 ** 30")
    plain = reference_policies()["best_fit"]
    ev = Evaluator(w, device="cpu")
    sb = ev.schedule_programs([plain, raising, cpython_only])
    assert len(sb) == 3 and sb.engine == ["cpu", "cpu", "object"]
    assert sb.rows[0, 10] == 0 and sb.rows[2, 10] == 0
    assert sb.rows[1, 10] == int(Exc.ZERO_DIVISION)
    assert (sb.node[1] == -1).all() and (sb.gpu_mask[1] == 0).all() and (sb.start[1] == -1).all()
    for i in (0, 2):
        assert (sb.node[i] >= 0).any()
        assert sb[i].validate(w)["unplaced"] == int(sb.rows[i, 9])
    _assert_equals_objects(sb[2], _object_schedule(w, cpython_only), "object engine")
    scores = ev.scores([plain, raising, cpython_only])
    assert sb.rows[:, 0].tolist() == scores
    one = schedule(plain, device="cpu", workload=w)
    assert np.array_equal(one.node[0], sb.node[0]) and one.engine == ["cpu"]
    fam = Evaluator(w, device="cpu").schedule_family("best_fit", np.zeros((1, 16)))
    assert np.array_equal(fam.node[0], sb.node[0]) and np.array_equal(fam.start[0], sb.start[0])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _record(sys.argv[1])
