#!/usr/bin/env python
"""Per-trace report of a saved family or program policy on a trace suite.

    python tools/suite_report.py POLICY.json [--suite openb] [--device auto|cpu]

One line per trace (score, utilisations, fragmentation, events), then the
suite mean and minimum.  A family policy has "family" and "weights"; a program
policy (e.g. the program champions under data/policies/discovered/) has
"code" only, and its row says which engine scored it on each trace.  Uses the
MI355X if one is visible, else the CPU.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from funsearch_kubernetes_simulator_amd.core.traces import SUITE_PRESETS, load_suite  # noqa: E402
from funsearch_kubernetes_simulator_amd.engine import COLS, SuiteEvaluator  # noqa: E402
from funsearch_kubernetes_simulator_amd.simulator.metrics import suite_aggregate_scores  # noqa: E402


def report(policy: dict, suite_name, device="auto") -> str:
    suite = load_suite(suite_name if suite_name in SUITE_PRESETS else suite_name.split(","))
    if "family" not in policy or "weights" not in policy:
        if "code" not in policy:
            raise SystemExit("suite_report needs a saved family policy (\"family\" and \"weights\") "
                             "or a program policy (\"code\")")
        return report_program(policy, suite, suite_name, device)
    ev = SuiteEvaluator(suite, device)
    tables, agg = ev.evaluate_family(policy["family"], np.asarray(policy["weights"], dtype=np.float64)[None, :])
    lines = [f"# {policy['family']} policy, saved score {policy.get('score')!r}; suite {suite_name} "
             f"({len(suite)} traces), backend {ev.backend}",
             f"{'trace':<12} {'pods':>6} {'score':>9} {'cpu':>7} {'mem':>7} {'gpu_cnt':>7} {'gpu_milli':>9} "
             f"{'frag':>8} {'frag_ev':>8} {'events':>8} {'unplaced':>8} {'exc':>4}"]
    for name, w, row in zip(suite.names, suite, tables[:, 0]):
        lines.append(f"{name:<12} {w.pods.n_pods:>6} {row[COLS['score']]:>9.6f} {row[COLS['avg_cpu']]:>7.4f} "
                     f"{row[COLS['avg_mem']]:>7.4f} {row[COLS['avg_gpu_count']]:>7.4f} "
                     f"{row[COLS['avg_gpu_milli']]:>9.4f} {row[COLS['frag']]:>8.5f} "
                     f"{int(row[COLS['n_frag_events']]):>8} {int(row[COLS['n_events']]):>8} "
                     f"{int(row[COLS['n_unplaced']]):>8} {int(row[COLS['exc']]):>4}")
    lines.append(f"mean {float(agg[0, 0])!r}  min {float(agg[0, 1])!r} ({suite.names[int(agg[0, 2])]})  "
                 f"traces raised {int(agg[0, 3])}")
    return "\n".join(lines)


def report_program(policy: dict, suite, suite_name, device="auto") -> str:
    ev = SuiteEvaluator(suite, device)
    results = [row[0] for row in ev.evaluate_programs([policy["code"]])]
    agg = suite_aggregate_scores([[r.score] for r in results], [[r.exc != 0] for r in results])
    lines = [f"# program policy, saved score {policy.get('score')!r}; suite {suite_name} "
             f"({len(suite)} traces), backend {ev.backend}",
             f"{'trace':<12} {'pods':>6} {'score':>9} {'cpu':>7} {'mem':>7} {'gpu_cnt':>7} {'gpu_milli':>9} "
             f"{'frag':>8} {'frag_ev':>8} {'events':>8} {'unplaced':>8} {'exc':>4} {'engine':>10}"]
    for name, w, r in zip(suite.names, suite, results):
        m = r.results
        if m is None:
            lines.append(f"{name:<12} {w.pods.n_pods:>6} {r.score:>9.6f} {'-':>7} {'-':>7} {'-':>7} {'-':>9} {'-':>8} "
                         f"{'-':>8} {r.n_events:>8} {'-':>8} {r.exc:>4} {r.engine:>10}")
            continue
        unplaced = r.detail.get("n_unplaced")
        lines.append(f"{name:<12} {w.pods.n_pods:>6} {r.score:>9.6f} {m.avg_cpu_utilization:>7.4f} "
                     f"{m.avg_memory_utilization:>7.4f} {m.avg_gpu_count_utilization:>7.4f} "
                     f"{m.avg_gpu_memory_utilization:>9.4f} {m.gpu_fragmentation_score:>8.5f} "
                     f"{m.num_fragmentation_events:>8} {r.n_events:>8} "
                     f"{'-' if unplaced is None else int(unplaced):>8} {r.exc:>4} {r.engine:>10}")
    lines.append(f"mean {float(agg[0, 0])!r}  min {float(agg[0, 1])!r} ({suite.names[int(agg[0, 2])]})  "
                 f"traces raised {int(agg[0, 3])}")
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("policy")
    ap.add_argument("--suite", default="openb", help="preset name or comma-separated trace names")
    ap.add_argument("--device", default="auto")
    args = ap.parse_args()
    with open(args.policy) as fh:
        policy = json.load(fh)
    print(report(policy, args.suite, args.device))
    return 0


if __name__ == "__main__":
    sys.exit(main())
