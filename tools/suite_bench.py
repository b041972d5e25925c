#!/usr/bin/env python
"""Suite evaluation throughput: SuiteEvaluator against back-to-back per-trace launches.

    python tools/suite_bench.py [--suite openb] [--candidates 4096] [--repeats 5]
    python tools/suite_bench.py --programs 64 [--suite openb] [--repeats 5] [--cpu]

Both sides replay the same composite candidates on every trace with the same
kernels, one resident engine per trace.  The baseline waits for each trace's
launch before it starts the next (`evaluate_builtin` in turn); the
SuiteEvaluator submits the batch to every engine before it waits for any, so
the launches overlap on their own streams, and then reduces on the host.
Prints (trace, policy) replays/s of each repeat and the spread.

``--programs N`` measures program batches instead: the first N device-capable
programs of the evolved population `bench.py` uses, on every trace, as
(a) the fused launch (`DeviceSuite`, one grid of T * N workgroups),
(b) per-trace launches of the same compiled batch on the T engines, all
submitted before any is waited for, (c) the same launches back to back, and
with ``--cpu`` (d) the CPU VM with 16 threads.  Shapes are JIT-compiled in a
first pass, which is timed on its own (the figure with JIT time); the repeats
are interleaved.  The three device routes must return equal tables.
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


def _report(rates: dict) -> None:
    for name, r in rates.items():
        r = np.array(r)
        print(f"{name:<44} median {np.median(r):>10.0f} replays/s  min {r.min():>10.0f}  max {r.max():>10.0f}  "
              f"spread {(r.max() - r.min()) / np.median(r) * 100:.1f}%  [{', '.join(f'{x:.0f}' for x in r)}]")


def bench_programs(args) -> int:
    from funsearch_kubernetes_simulator_amd.bench.programs import EVOLVED_SET, evolved_children
    from funsearch_kubernetes_simulator_amd.ops import cpu_engine
    suite = load_suite(args.suite)
    ev = SuiteEvaluator(suite, device="gpu")
    ds = ev.device_suite
    if ds is None:
        raise SystemExit("the device path refuses this suite")
    progs = evolved_children(args.programs + 64, workers=1)[:args.programs]
    T, N = len(suite), len(progs)
    n = T * N
    # one JIT for all routes: the per-trace engines launch the suite compiler's code
    for dev in ev.devices[1:]:
        dev._jit = ds.native_compiler
    ev.devices[0].warm_native()   # first-use initialisation of the JIT, outside every figure

    def fused():
        return ds.evaluate_native(progs)

    def per_trace_overlapped():
        for dev in ev.devices:
            dev.submit_native(0, progs)
        return np.stack([dev.wait(0) for dev in ev.devices])

    def per_trace_back_to_back():
        return np.stack([dev.evaluate_native(progs) for dev in ev.devices])

    def cpu_vm():
        return np.stack([cpu_engine.simulate_program_batch(w, progs, threads=16) for w in suite])

    print(f"suite {args.suite}: {T} traces x {N} programs (data/populations/{EVOLVED_SET}), "
          f"{args.repeats} repeats each, interleaved")
    t0 = time.perf_counter()
    ref = fused()
    t_first = time.perf_counter() - t0
    print(f"first fused pass, JIT compile of the batch's shapes included: {t_first:.3f} s, "
          f"{n / t_first:.0f} replays/s")
    declined = int((ref[0, :, 10] == 100).sum())
    print(f"programs the JIT declined: {declined} of {N}; rows with an exception: {int((ref[:, :, 10] != 0).sum())} of {n}")
    assert np.array_equal(per_trace_overlapped(), ref), "per-trace launches differ from the fused launch"
    assert np.array_equal(per_trace_back_to_back(), ref)
    rates = {"(a) fused launch": [], "(b) per-trace launches, overlapped": [], "(c) per-trace launches, back to back": []}
    fns = dict(zip(rates, (fused, per_trace_overlapped, per_trace_back_to_back)))
    if args.cpu:
        rates["(d) CPU VM, 16 threads"] = []
        fns["(d) CPU VM, 16 threads"] = cpu_vm
    for _ in range(args.repeats):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            rates[name].append(n / (time.perf_counter() - t0))
    _report(rates)
    a, b = np.array(rates["(a) fused launch"]), np.array(rates["(b) per-trace launches, overlapped"])
    spread = max(a.max() - a.min(), b.max() - b.min())
    print(f"(a) - (b) medians: {np.median(a) - np.median(b):+.0f} replays/s; run-to-run spread {spread:.0f}")
    info = ds.info()
    print(f"fused launch: grid {info['grid']} workgroups, heap tops {info['tops']} (traces {list(suite.names)}), "
          f"LDS {info['lds']} B, {info['per_cu']} workgroups per CU at that LDS (register limit {info['reg_cap']}), "
          f"{info['num_cus']} CUs")
    one = ev.devices[0].info()
    print(f"per-trace launch of trace {suite.names[0]}: heap top {one['native_duo_top_last']}, "
          f"{one['native_duo_per_cu_last']} workgroups per CU")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--suite", default="openb")
    ap.add_argument("--candidates", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--programs", type=int, default=0, help="measure program batches of this size instead")
    ap.add_argument("--cpu", action="store_true", help="with --programs: also the CPU VM with 16 threads")
    args = ap.parse_args()
    if args.programs > 0:
        return bench_programs(args)
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
    _report(rates)
    info = ev.devices[0].info()
    print(f"each trace's own k_replay_rows launch: {info['row_waves_per_cu']} resident waves per CU, heap top "
          f"{info['row_heap_top']}, {info['num_cus']} CUs ({info['arch']}); the residency of the {len(suite)} "
          f"overlapped launches together is not measured here")
    return 0


if __name__ == "__main__":
    sys.exit(main())
