#!/usr/bin/env python
"""Suite evaluation throughput: SuiteEvaluator against back-to-back per-trace launches.

    python tools/suite_bench.py [--suite openb] [--candidates 4096] [--repeats 5]

Both sides replay the same composite candidates on every trace with the same
kernels, one resident engine per trace.  The baseline waits for each trace's
launch before it starts the next (`evaluate_builtin` in turn); the
SuiteEvaluator submits the batch to every engine before it waits for any, so
the launches overlap on their own streams, and then reduces on the host.
Prints (trace, policy) replays/s of each repeat and the spread.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from funsearch_kubernetes_simulator_amd.core.traces import load_suite  # noqa: E402
from funsearch_kubernetes_simulator_amd.engine import SuiteEvaluator  # noqa: E402
from funsearch_kubernetes_simulator_amd.models import families as fam  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--suite", default="openb")
    ap.add_argument("--candidates", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    suite = load_suite(args.suite)
    ev = SuiteEvaluator(suite, device="gpu")
    w = fam.sample_composite_linear(args.candidates, np.random.default_rng(0))
    n = len(suite) * args.candidates

    def per_trace():
        return np.stack([dev.evaluate_builtin("composite_linear", w) for dev in ev.devices])

    def overlapped():
        return ev.evaluate_family("composite_linear", w)

    def launches_only():
        for dev in ev.devices:
            dev.submit_builtin(0, "composite_linear", w)
        return np.stack([dev.wait(0) for dev in ev.devices])

    ref = per_trace()                      # warm-up of every engine, and the reference tables
    tables, _ = overlapped()
    assert np.array_equal(tables, ref)
    print(f"suite {args.suite}: {len(suite)} traces x {args.candidates} composite candidates, "
          f"{args.repeats} repeats each, interleaved")
    rates = {"per-trace, back to back": [], "SuiteEvaluator (overlapped + host reduce)": [],
             "overlapped launches, no reduce": []}
    fns = dict(zip(rates, (per_trace, overlapped, launches_only)))
    for _ in range(args.repeats):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            rates[name].append(n / (time.perf_counter() - t0))
    for name, r in rates.items():
        r = np.array(r)
        print(f"{name:<44} median {np.median(r):>10.0f} replays/s  min {r.min():>10.0f}  max {r.max():>10.0f}  "
              f"spread {(r.max() - r.min()) / np.median(r) * 100:.1f}%  [{', '.join(f'{x:.0f}' for x in r)}]")
    info = ev.devices[0].info()
    print(f"each trace's own k_replay_rows launch: {info['row_waves_per_cu']} resident waves per CU, heap top "
          f"{info['row_heap_top']}, {info['num_cus']} CUs ({info['arch']}); the residency of the {len(suite)} "
          f"overlapped launches together is not measured here")
    return 0


if __name__ == "__main__":
    sys.exit(main())
