#!/usr/bin/env python3
"""What a saved policy does on the default trace: where its pods go and how long they wait.

    python tools/schedule_report.py POLICY.json [--device auto|cpu|gpu] [--against cpu]

POLICY.json is a results-JSON of `data/policies/discovered/`: a family policy
(`family` and `weights`) is replayed as that family, anything else as its
`code`.  Prints pods and GPU pods per node, the waiting time (start minus
trace creation time: mean, median, 95th percentile, maximum, in trace
seconds), the pods never placed and the counts of `Schedule.validate` (which
checks the schedule against the workload alone).  `--against cpu` also replays
the policy on the CPU oracle and prints the first pod, in (start, rank) order,
whose record differs -- `none` when the two schedules are the same.  Exit
status 1 if the schedule does not validate or differs.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def take_schedule(ev, rec):
    if rec.get("family") and rec.get("weights") is not None:
        from funsearch_kubernetes_simulator_amd.models import families as fam
        return ev.schedule_family(rec["family"], fam.pad_weights(np.asarray(rec["weights"], dtype=np.float64)[None]))
    return ev.schedule_programs([rec["code"]])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("policy")
    ap.add_argument("--device", default="auto", choices=["auto", "cpu", "gpu"])
    ap.add_argument("--against", default=None, choices=["cpu"])
    a = ap.parse_args()
    from funsearch_kubernetes_simulator_amd.core import ScheduleError, load_default_workload
    from funsearch_kubernetes_simulator_amd.engine import Evaluator
    w = load_default_workload()
    with open(a.policy) as f:
        rec = json.load(f)
    kind = f"{rec['family']} family" if rec.get("family") and rec.get("weights") is not None else "program"
    s = take_schedule(Evaluator(w, device=a.device), rec)[0]
    print(f"policy   {os.path.basename(a.policy)} ({kind}), recorded score {rec.get('score')}")
    print(f"engine   {s.engine}: score {s.row[0]!r}, exc {int(s.row[10])}, {int(s.row[8])} events")
    placed = s.node >= 0
    print(f"{'node':<28}{'pods':>7}{'GPU pods':>10}")
    for n, nid in enumerate(w.cluster.node_ids):
        here = s.node == n
        print(f"{nid:<28}{int(here.sum()):>7}{int((here & (w.pods.pod_ngpu > 0)).sum()):>10}")
    wait = s.wait(w)[placed]
    if wait.size:
        print(f"waiting  mean {wait.mean():.1f} s, median {np.median(wait):.1f} s, 95th percentile "
              f"{np.percentile(wait, 95):.1f} s, maximum {int(wait.max())} s over {int(wait.size)} placed pods "
              f"({int((wait > 0).sum())} waited)")
    print(f"never placed  {int((~placed).sum())} pods")
    ok = True
    try:
        print("validate ", json.dumps(s.validate(w)))
    except ScheduleError as e:
        ok = False
        print("validate  FAILED:", e)
    if a.against:
        o = take_schedule(Evaluator(w, device="cpu"), rec)[0]
        d = s.first_difference(o, w)
        rows = "rows equal" if np.array_equal(s.row[:12], o.row[:12]) else "rows DIFFER"
        if d is None:
            print(f"against the CPU oracle ({o.engine})  first difference: none ({rows})")
        else:
            ok = False
            print(f"against the CPU oracle ({o.engine})  first difference: pod {w.pods.pod_ids[d]} (trace index {d}): "
                  f"node {int(s.node[d])} GPUs {s.gpus(d)} start {int(s.start[d])} here, "
                  f"node {int(o.node[d])} GPUs {o.gpus(d)} start {int(o.start[d])} there ({rows})")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
