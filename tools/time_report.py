#!/usr/bin/env python3
"""How long a saved policy's pods wait on the default trace, and how long its schedule takes.

    python tools/time_report.py POLICY.json [--device auto|cpu|gpu] [--against cpu]

POLICY.json is a results-JSON of `data/policies/discovered/`: a family policy
(`family` and `weights`) is replayed as that family, anything else as its
`code`.  Prints the policy's time record (`core/time_metrics.py`: integer sums
and maxima over the pods the replay placed), the derived figures (mean wait,
span, time-weighted utilisation, quantile bounds) and the histogram of waits by
bit length.  `--against cpu` also takes the record from the CPU oracle and
prints whether the two are equal.  Exit status 1 if they are not.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def take(ev, rec):
    if rec.get("family") and rec.get("weights") is not None:
        from funsearch_kubernetes_simulator_amd.models import families as fam
        return ev.time_family(rec["family"], fam.pad_weights(np.asarray(rec["weights"], dtype=np.float64)[None]))
    return ev.time_programs([rec["code"]])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("policy")
    ap.add_argument("--device", default="auto", choices=["auto", "cpu", "gpu"])
    ap.add_argument("--against", default=None, choices=["cpu"])
    a = ap.parse_args()
    from funsearch_kubernetes_simulator_amd.core import load_default_workload
    from funsearch_kubernetes_simulator_amd.core.time_metrics import BUSY_NAMES
    from funsearch_kubernetes_simulator_amd.engine import Evaluator
    w = load_default_workload()
    with open(a.policy) as f:
        rec = json.load(f)
    kind = f"{rec['family']} family" if rec.get("family") and rec.get("weights") is not None else "program"
    tm = take(Evaluator(w, device=a.device), rec)
    r = tm.record(0)
    print(f"policy   {os.path.basename(a.policy)} ({kind}), recorded score {rec.get('score')}")
    print(f"engine   {tm.engine[0]}: score {tm.rows[0, 0]!r}, exc {int(tm.rows[0, 10])}, {int(tm.rows[0, 8])} events, "
          f"{int(tm.rows[0, 9])} pods never placed")
    print(f"record   n_placed {r['n_placed']}, wait_sum {r['wait_sum']} s, wait_max {r['wait_max']} s, end_max {r['end_max']} s")
    for k, n in enumerate(BUSY_NAMES):
        print(f"         busy[{n}] {r['busy'][k]} (total {tm.totals[k]})")
    print(f"derived  mean wait {tm.mean_wait[0]:.3f} s, span {tm.span_int(0)} s (from t0 = {tm.t0}), "
          f"{100 * tm.frac_waited[0]:.2f} % of placed pods waited")
    print("         time-weighted utilisation " + ", ".join(f"{n} {tm.tw_util[0, k]:.6f}" for k, n in enumerate(BUSY_NAMES)))
    print("         wait quantile bounds " + ", ".join(f"q{int(100 * q)} <= {int(tm.wait_quantile_bound(q)[0])} s"
                                                       for q in (0.5, 0.9, 0.95, 0.99)))
    print(f"{'bucket':<8}{'waits (s)':<28}{'pods':>8}")
    for b, c in enumerate(r["hist"]):
        if c:
            span = "0" if b == 0 else f"{1 << (b - 1)} .. {(1 << b) - 1}" if b < 31 else f">= {1 << 30}"
            print(f"{b:<8}{span:<28}{c:>8}")
    ok = True
    if a.against:
        o = take(Evaluator(w, device="cpu"), rec)
        ok = tm.raw_equal(o)
        rows = "rows equal" if np.array_equal(tm.rows[0, :12], o.rows[0, :12]) else "rows DIFFER"
        print(f"against the CPU oracle ({o.engine[0]})  record {'equal' if ok else 'DIFFERS: ' + json.dumps(o.record(0))} ({rows})")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
