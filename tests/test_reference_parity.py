"""Differential test against the reference implementation itself.

The reference's own simulator was run on random sub-traces and random
policies; the scores it returned are stored in
``tests/golden/reference_parity_scores.json`` and the native engine must
reproduce them bit for bit.  The file holds each case (the sub-trace's first
pod and length, the policy program this project generated) next to the score
the reference gave it.

    python tests/test_reference_parity.py <reference checkout>

records the file again: it runs the reference (imported with a 3-line
``enum.StrEnum`` shim for Python 3.10) in a subprocess on the same cases.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_parity_scores.json")

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
    pods = [copy.deepcopy(by_id[i]) for i in case["pods"]]
    env = {"__builtins__": __builtins__}
    exec(case["code"], env)
    fn = env["priority_function"]
    sched = lambda pod, node: int(max(0, fn(pod, node)))
    ev = SchedulingEvaluator(cluster, enabled=True)
    sim = KubernetesSimulator(cluster, pods, DiscreteEventSimulator(pods), sched, evaluator=ev)
    try:
        sim.run_schedule()
        out.append(ev.get_policy_score(pods))
    except Exception:
        out.append(0)
print(json.dumps(out))
'''


def _cases(w):
    from funsearch_kubernetes_simulator_amd.models import families as fam
    rng = np.random.default_rng(2024)
    cases = []
    for k in range(8):
        n = int(rng.integers(200, 900))
        start = int(rng.integers(0, w.pods.n_pods - n))
        idx = np.arange(start, start + n)
        family = "random_linear" if k % 2 else "feature_linear"
        W = (fam.sample_random_linear if family == "random_linear" else fam.sample_feature_linear)(1, rng)[0]
        cases.append({"pods": [w.pods.pod_ids[i] for i in idx], "code": fam.to_program(family, W), "idx": idx})
    return cases


def _record(ref: str) -> None:
    from funsearch_kubernetes_simulator_amd.core import load_default_workload
    cases = _cases(load_default_workload())
    with tempfile.TemporaryDirectory() as tmp:
        job, drv = os.path.join(tmp, "job.json"), os.path.join(tmp, "drv.py")
        with open(job, "w") as f:
            json.dump([{"pods": c["pods"], "code": c["code"]} for c in cases], f)
        with open(drv, "w") as f:
            f.write(DRIVER)
        r = subprocess.run([sys.executable, drv, ref, job], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    scores = json.loads(r.stdout.strip().splitlines()[-1])
    with open(GOLDEN, "w") as f:
        json.dump({"seed": 2024,
                   "cases": [{"start": int(c["idx"][0]), "n_pods": len(c["idx"]), "code": c["code"],
                              "score": repr(float(s))} for c, s in zip(cases, scores)]}, f, indent=1)
        f.write("\n")


@pytest.mark.slow
def test_random_subtraces_random_policies_match_reference():
    from funsearch_kubernetes_simulator_amd.core import load_default_workload
    from funsearch_kubernetes_simulator_amd.core.arrays import Workload
    from funsearch_kubernetes_simulator_amd.engine import Evaluator
    w = load_default_workload()
    with open(GOLDEN) as f:
        golden = json.load(f)["cases"]
    assert len(golden) == 8
    for g in golden:
        sub = Workload(w.cluster, w.pods.subset(np.arange(g["start"], g["start"] + g["n_pods"])))
        got = Evaluator(sub, device="cpu").scores([g["code"]])[0]
        assert got == float(g["score"]), (got, g["score"])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _record(sys.argv[1])
