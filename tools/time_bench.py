#!/usr/bin/env python3
"""What time-metrics mode costs on the device: three routes to the same records.

    python tools/time_bench.py [--candidates 4096] [--programs 256] [--repeats 3]

On the default trace, alternating, `--repeats` times each: replays per second
of one synchronous call on slot 0 (staging, launch, copy back and the host's
share included) for

    evaluate_builtin / evaluate_native                       the scores alone (baseline)
    time_builtin / time_native                               time-metrics mode
    schedule_builtin / schedule_native + .time_metrics()     the records by way of schedule mode

and whether the three agree: rows bit for bit, records field for field.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rate(fn, n):
    t = time.perf_counter()
    out = fn()
    return n / (time.perf_counter() - t), out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--candidates", type=int, default=4096)
    ap.add_argument("--programs", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    from funsearch_kubernetes_simulator_amd.bench.programs import evolved_children
    from funsearch_kubernetes_simulator_amd.core import load_default_workload
    from funsearch_kubernetes_simulator_amd.models import families as fam
    from funsearch_kubernetes_simulator_amd.ops.hip_engine import DeviceEvaluator
    w = load_default_workload()
    dev = DeviceEvaluator(w)
    W = fam.pad_weights(fam.SAMPLERS["composite_linear"](a.candidates, np.random.default_rng(0)))
    routes = {"evaluate_builtin": lambda: dev.evaluate_builtin("composite_linear", W),
              "time_builtin": lambda: dev.time_builtin("composite_linear", W),
              "schedule_builtin+time_metrics": lambda: dev.schedule_builtin("composite_linear", W).time_metrics(w)}
    for fn in routes.values():
        fn()   # once, untimed
    got = {k: [] for k in routes}
    for _ in range(a.repeats):
        for k, fn in routes.items():
            r, out = rate(fn, a.candidates)
            got[k].append(r)
            if k == "evaluate_builtin":
                rows = out
            elif k == "time_builtin":
                tm = out
            else:
                via = out
    print(f"{a.candidates} composite_linear candidates, instance {dev.info()['time_instance_last']}")
    for k, v in got.items():
        print(f"  {k:<32}" + " / ".join(f"{x:,.1f}" for x in v) + " replays/s")
    print(f"  time / evaluate: {np.median(got['time_builtin']) / np.median(got['evaluate_builtin']):.3f}; rows equal bit for "
          f"bit: {np.array_equal(rows, tm.rows) and np.array_equal(rows, via.rows)}; records equal: {tm.raw_equal(via)}; "
          f"mean wait {tm.mean_wait.min():.0f} .. {tm.mean_wait.max():.0f} s, span {int(tm.span.min())} .. {int(tm.span.max())} s")
    progs = evolved_children(a.programs)
    routes = {"evaluate_native": lambda: dev.evaluate_native(progs), "time_native": lambda: dev.time_native(progs),
              "schedule_native+time_metrics": lambda: dev.schedule_native(progs).time_metrics(w)}
    for fn in routes.values():
        fn()
    got = {k: [] for k in routes}
    for _ in range(a.repeats):
        for k, fn in routes.items():
            r, out = rate(fn, len(progs))
            got[k].append(r)
            if k == "evaluate_native":
                rows = out
            elif k == "time_native":
                tm = out
            else:
                via = out
    print(f"{len(progs)} evolved programs, instance {dev.info()['time_instance_last']}")
    for k, v in got.items():
        print(f"  {k:<32}" + " / ".join(f"{x:,.1f}" for x in v) + " replays/s")
    print(f"  time / evaluate: {np.median(got['time_native']) / np.median(got['evaluate_native']):.3f}; rows equal bit for bit: "
          f"{np.array_equal(rows, tm.rows) and np.array_equal(rows, via.rows)}; records equal: {tm.raw_equal(via)}; "
          f"{int((tm.rows[:, 10] != 0).sum())} rows carry an exception code")
    return 0


if __name__ == "__main__":
    sys.exit(main())
