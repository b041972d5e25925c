"""`evaluate()`: score policy programs on the fastest exact engine available.

Routing per program (every path yields the reference's score bit-for-bit; the
device's `**`, math.exp / log / pow are glibc's own algorithms, so they return
CPython's bits -- csrc/hip/glibc_math.h, checked at start-up by
`hip_engine.glibc_math_ok`):

1. compile to bytecode (`policy.compiler`); programs outside the native
   subset go straight to the object engine (CPython ``exec``, step 4);
2. MI355X (`ops.hip_engine`): natively compiled programs first
   (`policy.native_codegen` -> `ops.jit`, one k_replay_native wave per program,
   any batch size; compiled shapes are cached), then the device bytecode VM for
   what the native backend declines, when the batch is large enough to fill
   the chip;
3. native CPU VM (`ops.cpu_engine`): for no-GPU hosts, for programs the device
   reports as EXC_UNSUPPORTED (bigint / complex / trig) or
   EXC_BUDGET (per-call instruction budget), and for results whose exact-mean
   accumulator flagged `inexact`;
4. object engine (`simulator.KubernetesSimulator` + ``exec``), which *is* the
   reference semantics, for whatever the native engines cannot express; it
   runs under a wall-clock budget (``object_timeout_s``, default 600 s).

Scores follow `evaluate_policy_standalone` (`funsearch/funsearch_integration.py:30-64`):
any exception during the replay gives score 0.  `EvalResult.exc` tells which
exception class it was; `EvalResult.engine` which engine produced it.
"""

from __future__ import annotations

import atexit
import copy
import os
import threading
import time
from concurrent.futures import ProcessPoolExecutor
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .core.arrays import Workload
from .core.traces import load_default_workload
from .policy.bytecode import Exc
from .policy.compiler import CompiledPolicy, try_compile
from .simulator.metrics import EvaluationResults

COLS = {name: i for i, name in enumerate(
    ("score", "avg_cpu", "avg_mem", "avg_gpu_count", "avg_gpu_milli", "frag", "n_snapshots",
     "n_frag_events", "n_events", "n_unplaced", "exc", "inexact", "trace_hash_hi"))}


@dataclass
class EvalResult:
    score: float
    exc: int = 0
    engine: str = ""
    results: Optional[EvaluationResults] = None
    n_events: int = 0
    detail: Dict[str, float] = field(default_factory=dict)
    #: device cycles of the replay (program service only; 0 elsewhere): what a
    #: program costs the search -- parent sampling and bloat control, never the score
    device_cycles: float = 0.0

    @property
    def ok(self) -> bool:
        return self.exc == 0


def _row_to_result(row: np.ndarray, engine: str) -> EvalResult:
    exc = int(row[COLS["exc"]])
    if exc:
        return EvalResult(0.0, exc, engine, n_events=int(row[COLS["n_events"]]))
    res = EvaluationResults(
        avg_cpu_utilization=float(row[COLS["avg_cpu"]]),
        avg_memory_utilization=float(row[COLS["avg_mem"]]),
        avg_gpu_count_utilization=float(row[COLS["avg_gpu_count"]]),
        avg_gpu_memory_utilization=float(row[COLS["avg_gpu_milli"]]),
        gpu_fragmentation_score=float(row[COLS["frag"]]),
        num_snapshots=int(row[COLS["n_snapshots"]]),
        num_fragmentation_events=int(row[COLS["n_frag_events"]]))
    return EvalResult(float(row[COLS["score"]]), 0, engine, res, int(row[COLS["n_events"]]),
                      {"n_unplaced": float(row[COLS["n_unplaced"]]), "trace_hash_hi": float(row[COLS["trace_hash_hi"]])})


# ---------------------------------------------------------------------------- object engine
class ReplayTimeout(Exception):
    """Raised inside an object-engine replay that exceeded its wall-clock budget."""


def object_engine_eval(code: str, workload: Workload, budget_s: float = 0.0) -> EvalResult:
    """Reference-semantics replay with CPython ``exec`` (the exact fallback).

    ``budget_s`` > 0 bounds the replay's wall-clock time with ``SIGALRM`` (as
    the reference's `SafeExecutor`, `funsearch/safe_execution.py:81-96`, does
    per call): a program that loops forever scores 0 with `Exc.BUDGET`
    instead of hanging the search.  Only effective in a process's main thread.
    """
    import signal
    import threading
    from .funsearch.scheduler import FunSearchScheduler
    from .simulator import DiscreteEventSimulator, KubernetesSimulator, SchedulingEvaluator
    armed = budget_s > 0 and threading.current_thread() is threading.main_thread()
    if armed:
        def _expire(signum, frame):
            raise ReplayTimeout(f"replay exceeded {budget_s} s")
        old = signal.signal(signal.SIGALRM, _expire)
        signal.setitimer(signal.ITIMER_REAL, budget_s)
    try:
        sched = FunSearchScheduler(code)
        cluster, pods = workload.to_objects()
        ev = SchedulingEvaluator(cluster, enabled=True)
        sim = KubernetesSimulator(cluster, pods, DiscreteEventSimulator(pods), sched, evaluator=ev)
        sim.run_schedule()
        res = ev.get_evaluation_results()
        return EvalResult(float(ev.get_policy_score(pods)), 0, "object", res, sim.events_processed)
    except Exception as exc:  # any exception aborts the replay -> score 0
        return EvalResult(0.0, _exc_code(exc), "object")
    finally:
        if armed:
            signal.setitimer(signal.ITIMER_REAL, 0)
            signal.signal(signal.SIGALRM, old)


def object_engine_schedule(code: str, workload: Workload, budget_s: float = 0.0):
    """The object engine's replay with what it left on the pods: (row [13],
    node [n_pods] int32, GPU mask uint8, start int64).  A replay that raises
    has its exception code in the row and every pod at -1 / 0 / -1."""
    import signal
    import threading
    from .funsearch.scheduler import FunSearchScheduler
    from .simulator import DiscreteEventSimulator, KubernetesSimulator, SchedulingEvaluator
    n = workload.pods.n_pods
    row = np.zeros(len(COLS))
    node, mask, start = np.full(n, -1, np.int32), np.zeros(n, np.uint8), np.full(n, -1, np.int64)
    armed = budget_s > 0 and threading.current_thread() is threading.main_thread()
    if armed:
        def _expire(signum, frame):
            raise ReplayTimeout(f"replay exceeded {budget_s} s")
        old = signal.signal(signal.SIGALRM, _expire)
        signal.setitimer(signal.ITIMER_REAL, budget_s)
    try:
        sched = FunSearchScheduler(code)
        cluster, pods = workload.to_objects()
        ev = SchedulingEvaluator(cluster, enabled=True)
        sim = KubernetesSimulator(cluster, pods, DiscreteEventSimulator(pods), sched, evaluator=ev)
        sim.run_schedule()
        res = ev.get_evaluation_results()
        score = float(ev.get_policy_score(pods))
    except Exception as exc:  # any exception aborts the replay: no schedule
        row[COLS["exc"]] = _exc_code(exc)
        return row, node, mask, start
    finally:
        if armed:
            signal.setitimer(signal.ITIMER_REAL, 0)
            signal.signal(signal.SIGALRM, old)
    index = {nid: i for i, nid in enumerate(workload.cluster.node_ids)}
    for i, pod in enumerate(pods):
        if pod.assigned_node == "":
            continue
        node[i] = index[pod.assigned_node]
        mask[i] = sum(1 << int(g) for g in pod.assigned_gpus)
        start[i] = pod.creation_time
    row[:9] = (score, res.avg_cpu_utilization, res.avg_memory_utilization, res.avg_gpu_count_utilization,
               res.avg_gpu_memory_utilization, res.gpu_fragmentation_score, res.num_snapshots,
               res.num_fragmentation_events, sim.events_processed)
    row[COLS["n_unplaced"]] = int((node < 0).sum())
    return row, node, mask, start


def _object_schedule_worker(args):
    code, workload, budget_s = args
    return object_engine_schedule(code, workload, budget_s)


def object_engine_time(code: str, workload: Workload, budget_s: float = 0.0):
    """The object engine's time metrics, derived from what its replay left on
    the pods (`object_engine_schedule`, then `Schedule.time_record`): (row
    [13], record [24] int64).  All zero if the replay raised."""
    from .core.schedule import Schedule
    row, node, mask, start = object_engine_schedule(code, workload, budget_s)
    return row, Schedule(node, mask, start, row, "object").time_record(workload)


def _object_time_worker(args):
    code, workload, budget_s = args
    return object_engine_time(code, workload, budget_s)


def _exc_code(exc: BaseException) -> int:
    if isinstance(exc, ReplayTimeout):
        return int(Exc.BUDGET)
    if isinstance(exc, ZeroDivisionError):
        return int(Exc.ZERO_DIVISION)
    if isinstance(exc, OverflowError):
        return int(Exc.OVERFLOW)
    if isinstance(exc, IndexError):
        return int(Exc.INDEX)
    if isinstance(exc, NameError):
        return int(Exc.NAME)
    if isinstance(exc, TypeError):
        return int(Exc.TYPE)
    return int(Exc.VALUE)


def _object_worker(args):
    code, workload, budget_s = args
    return object_engine_eval(code, workload, budget_s)


# ---------------------------------------------------------------------------- evaluator
#: exception codes of a native-program row that hand the program to the next
#: engine: UNSUPPORTED / BUDGET as for every engine, TIMEOUT -- the two-wave
#: kernel ends a replay with it when one wave stops hearing from the other (a
#: bounded spin, replay_duo.hip.h), which depends on timing, not on the
#: program -- and INVARIANT, a failed accounting check, i.e. a kernel bug: the
#: program is re-scored by the next engine (so the score stays exact) but the
#: row is counted in ``stats["native_invariant"]`` and logged, never hidden
NATIVE_DEFER = (int(Exc.UNSUPPORTED), int(Exc.BUDGET), int(Exc.TIMEOUT), int(Exc.INVARIANT))


def _native_deferred(row, bump) -> bool:
    """True: this native-program row goes to the next engine (counted through `bump`)."""
    exc = int(row[COLS["exc"]])
    if exc == Exc.TIMEOUT:
        bump("native_timeout")
    elif exc == Exc.EVENTS:
        bump("native_event_cap")   # final: past the caller's replay event budget, not scored
    elif exc == Exc.INVARIANT:
        bump("native_invariant")
        import warnings
        warnings.warn("native replay failed its invariant check (kernel bug?); program re-scored on the CPU VM",
                      RuntimeWarning, stacklevel=3)
    return exc in NATIVE_DEFER or bool(row[COLS["inexact"]])


class Evaluator:
    """Batched exact evaluator bound to one workload.

    ``device``: ``"auto"`` (MI355X if visible, else CPU), ``"gpu"``/``int``
    (HIP device index; fails loudly if unavailable), or ``"cpu"``.
    """

    def __init__(self, workload: Optional[Workload] = None, device="auto", options: Optional[dict] = None,
                 cpu_threads: int = 0, object_workers: int = 0, n_slots: int = 4):
        self.workload = workload or load_default_workload()
        self.options = dict(options or {})
        from .ops.cpu_engine import default_threads
        self.cpu_threads = cpu_threads or default_threads()
        self.object_workers = object_workers or min(8, self.cpu_threads)
        # below this many programs a batch runs faster on the CPU VM (one replay per
        # core, ~0.1 s each) than as a handful of latency-bound device waves
        self.device_min_batch = int(self.options.pop("device_min_batch", 128))
        # natively compiled programs on the device (any batch size)
        self.native = bool(self.options.pop("native", True))
        # fault-injection hook: fail this fraction of program
        # evaluations as if the replay had raised -> score 0, like the reference
        self.fault_rate = float(self.options.pop("fault_rate", 0.0) or 0.0)
        # bytecode compiles of program batches in worker processes: the compiler is
        # pure Python (~4 ms per program), and pipelined islands otherwise queue on
        # the GIL for it (0: in-process)
        self.compile_workers = int(self.options.pop("compile_workers", 0) or 0)
        self._compile_pool = None
        self._compile_lock = threading.Lock()
        # counters are bumped from the dispatcher and from the fallback worker
        # threads (`fallback_async`): every update goes through `_bump`
        self._stats_lock = threading.Lock()
        fault_seed = int(self.options.pop("fault_seed", 0))
        self._fault_rng = np.random.default_rng(fault_seed)
        # the fallback threads draw from their own generator (under the stats
        # lock), so the dispatcher's fault sequence stays deterministic
        self._fallback_fault_rng = np.random.default_rng(fault_seed + 1)
        self.device = None
        want_gpu = device not in ("cpu", None)
        if want_gpu:
            from .ops import hip_engine
            idx = device if isinstance(device, int) else int(os.environ.get("LOCAL_RANK", 0))
            available = hip_engine.device_available()
            if available and not isinstance(device, int):
                idx %= hip_engine.native().device_count()   # ranks > GPUs (gloo rehearsal) share the cards
            if not available and device != "auto":
                raise RuntimeError("HIP device requested but none is visible")
            if available:
                try:
                    self.device = hip_engine.DeviceEvaluator(self.workload, idx, self.options, n_slots)
                except hip_engine.UnsupportedWorkload:
                    if device != "auto":
                        raise
        self.stats = {"device": 0, "device_native": 0, "cpu_vm": 0, "object": 0, "compile_errors": 0,
                      "jit_s": 0.0, "jit_shapes": 0, "native_timeout": 0, "native_invariant": 0}
        self._done: Dict[int, np.ndarray] = {}   # CPU stand-in for in-flight slots

    def _bump(self, key: str, n=1) -> None:
        with self._stats_lock:
            self.stats[key] = self.stats.get(key, 0) + n

    @property
    def backend(self) -> str:
        return "hip" if self.device is not None else "cpu"

    # -- built-in parametric families -------------------------------------------
    def evaluate_family(self, family: str, weights: np.ndarray) -> np.ndarray:
        """[P, 13] result table for P members of a built-in family."""
        if self.device is not None:
            return self.device.evaluate_builtin(family, weights)
        from .ops import cpu_engine
        return cpu_engine.simulate_builtin_batch(self.workload, family, weights,
                                                 cpu_engine.SimOptions(**self._cpu_opts()), self.cpu_threads)

    # -- schedules: what each replay did (core/schedule.py) ------------------------------
    def schedule_family(self, family, weights: np.ndarray):
        """`ScheduleBatch` of a family batch (`family`: one name, or one per row):
        the rows of `evaluate_family` and each pod's node, GPUs and start time."""
        if self.device is not None:
            return self.device.schedule_builtin(family, weights)
        from .ops import cpu_engine
        return cpu_engine.schedule_builtin_batch(self.workload, family, weights,
                                                 cpu_engine.SimOptions(**self._cpu_opts()), self.cpu_threads)

    def schedule_programs(self, codes: Sequence[str]):
        """`ScheduleBatch` of program texts, routed as their scores are: the
        device's native kernels, then -- for programs the JIT declines and rows
        it defers -- the CPU VM, then the object engine.  Every program gets a
        schedule, and `engine[i]` says where it came from; a program that
        raises has its `exc` in its row and nothing placed."""
        from .core.schedule import ScheduleBatch
        from .ops import cpu_engine
        codes = list(codes)
        compiled = self.compile_batch(codes)
        n = len(codes)
        out = ScheduleBatch.empty(n, self.workload.pods.n_pods, list(self.workload.cluster.node_ids))
        done = [False] * n
        pending = [i for i, p in enumerate(compiled) if p is not None]
        if self.device is not None and self.native:
            exact = getattr(self.device, "math_exact", True)
            dev_idx = [i for i in pending if compiled[i].device_ok and (exact or not compiled[i].uses_libm)]
            if dev_idx:
                got = self.device.schedule_native([compiled[i] for i in dev_idx])
                for j, i in enumerate(dev_idx):
                    if not _native_deferred(got.rows[j], self._bump):
                        out.put([i], got, [j])
                        done[i] = True
                        self._bump("device_native", 1)
        cpu_idx = [i for i in pending if not done[i]]
        if cpu_idx:
            got = cpu_engine.schedule_program_batch(self.workload, [compiled[i] for i in cpu_idx],
                                                    cpu_engine.SimOptions(**self._cpu_opts()), self.cpu_threads)
            for j, i in enumerate(cpu_idx):
                row = got.rows[j]
                if int(row[COLS["exc"]]) in (Exc.UNSUPPORTED, Exc.BUDGET) or row[COLS["inexact"]]:
                    continue
                out.put([i], got, [j])
                done[i] = True
                self._bump("cpu_vm", 1)
        rest = [i for i in range(n) if not done[i]]
        if rest:
            if self._object_engine_ok():
                budget_s = float(self.options.get("object_timeout_s", 600.0))
                jobs = [(codes[i], self.workload, budget_s) for i in rest]
                if len(rest) > 1 and self.object_workers > 1:
                    with ProcessPoolExecutor(max_workers=min(self.object_workers, len(rest))) as ex:
                        results = list(ex.map(_object_schedule_worker, jobs))
                else:
                    results = [_object_schedule_worker(j) for j in jobs]
                for i, (row, node, mask, start) in zip(rest, results):
                    out.put([i], ScheduleBatch(node[None], mask[None], start[None], row[None], ["object"]))
                    self._bump("object", 1)
            else:
                for i in rest:
                    out.rows[i, COLS["exc"]] = int(Exc.UNSUPPORTED)
                    out.engine[i] = "none"
        return out

    # -- time metrics: waits, makespan, busy time (core/time_metrics.py) -------------------
    def time_family(self, family, weights: np.ndarray):
        """`TimeMetricsBatch` of a family batch (`family`: one name, or one per
        row): the rows of `evaluate_family` and each replay's time record."""
        if self.device is not None:
            return self.device.time_builtin(family, weights)
        from .ops import cpu_engine
        self._time_gate()
        return cpu_engine.time_builtin_batch(self.workload, family, weights,
                                             cpu_engine.SimOptions(**self._cpu_opts()), self.cpu_threads)

    def _time_gate(self) -> None:
        """Time mode refuses a workload on which one of its 64-bit sums could overflow."""
        from .core.time_metrics import overflow_gate
        from .ops.hip_engine import UnsupportedWorkload
        if not hasattr(self, "_time_gate_reason"):
            self._time_gate_reason = overflow_gate(self.workload, self.device.layout["time_bits"]
                                                   if self.device is not None else None)
        if self._time_gate_reason:
            raise UnsupportedWorkload(f"time mode: {self._time_gate_reason} (a 64-bit sum could overflow)")

    def time_programs(self, codes: Sequence[str]):
        """`TimeMetricsBatch` of program texts, routed as `schedule_programs`
        routes them: the device's native time kernels, then -- for programs the
        JIT declines and rows it defers -- the CPU VM, then the object engine.
        `engine[i]` says where record i came from; a program that raises has
        its `exc` in its row and an all-zero record."""
        from .core.time_metrics import TimeMetricsBatch
        from .ops import cpu_engine
        self._time_gate()
        codes = list(codes)
        compiled = self.compile_batch(codes)
        n = len(codes)
        out = TimeMetricsBatch.empty(n, self.workload)
        done = [False] * n
        pending = [i for i, p in enumerate(compiled) if p is not None]
        if self.device is not None and self.native:
            exact = getattr(self.device, "math_exact", True)
            dev_idx = [i for i in pending if compiled[i].device_ok and (exact or not compiled[i].uses_libm)]
            if dev_idx:
                got = self.device.time_native([compiled[i] for i in dev_idx])
                for j, i in enumerate(dev_idx):
                    if not _native_deferred(got.rows[j], self._bump):
                        out.put([i], got, [j])
                        done[i] = True
                        self._bump("device_native", 1)
        cpu_idx = [i for i in pending if not done[i]]
        if cpu_idx:
            got = cpu_engine.time_program_batch(self.workload, [compiled[i] for i in cpu_idx],
                                                cpu_engine.SimOptions(**self._cpu_opts()), self.cpu_threads)
            for j, i in enumerate(cpu_idx):
                row = got.rows[j]
                if int(row[COLS["exc"]]) in (Exc.UNSUPPORTED, Exc.BUDGET) or row[COLS["inexact"]]:
                    continue
                out.put([i], got, [j])
                done[i] = True
                self._bump("cpu_vm", 1)
        rest = [i for i in range(n) if not done[i]]
        if rest:
            if self._object_engine_ok():
                budget_s = float(self.options.get("object_timeout_s", 600.0))
                jobs = [(codes[i], self.workload, budget_s) for i in rest]
                if len(rest) > 1 and self.object_workers > 1:
                    with ProcessPoolExecutor(max_workers=min(self.object_workers, len(rest))) as ex:
                        results = list(ex.map(_object_time_worker, jobs))
                else:
                    results = [_object_time_worker(j) for j in jobs]
                for i, (row, rec) in zip(rest, results):
                    out.put([i], TimeMetricsBatch.from_records(row[None], rec[None], "object", self.workload))
                    self._bump("object", 1)
            else:
                for i in rest:
                    out.rows[i, COLS["exc"]] = int(Exc.UNSUPPORTED)
                    out.engine[i] = "none"
        return out

    # asynchronous form: several family batches in flight (one HIP stream per slot)
    def submit_family(self, slot: int, family: str, weights: np.ndarray) -> None:
        if self.device is not None:
            self.device.submit_builtin(slot, family, weights)
        else:
            self._done[slot] = self.evaluate_family(family, weights)

    def wait(self, slot: int) -> np.ndarray:
        return self.device.wait(slot) if self.device is not None else self._done.pop(slot)

    def _cpu_opts(self) -> dict:
        from .ops.cpu_engine import DEFAULT_CALL_BUDGET
        keep = ("repush", "gpu_alloc", "snapshot_interval", "budget")   # (object_timeout_s: object engine only)
        opts = {k: v for k, v in self.options.items() if k in keep}
        opts.setdefault("budget", DEFAULT_CALL_BUDGET)
        return opts

    # -- programs ---------------------------------------------------------------------
    def compile_batch(self, codes: Sequence[str]) -> List[Optional[CompiledPolicy]]:
        """Bytecode for every program text (None: rejected), in worker processes
        when ``compile_workers`` > 0 and the batch has more than one program."""
        codes = list(codes)
        if self.compile_workers > 0 and len(codes) > 1:
            with self._compile_lock:
                if self._compile_pool is None:
                    import multiprocessing
                    # spawn: the workers never inherit the parent's HIP state
                    self._compile_pool = ProcessPoolExecutor(max_workers=self.compile_workers,
                                                             mp_context=multiprocessing.get_context("spawn"))
                    atexit.register(self._compile_pool.shutdown, wait=False, cancel_futures=True)
            chunk = max(1, len(codes) // (2 * self.compile_workers))
            results = list(self._compile_pool.map(try_compile, codes, chunksize=chunk))
        else:
            results = [try_compile(c) for c in codes]
        out = []
        for prog, _ in results:
            if prog is None:
                self._bump("compile_errors", 1)
            out.append(prog)
        return out

    def evaluate_programs(self, codes: Sequence[str], slot: int = 0) -> List[EvalResult]:
        """Scores of program texts (synchronous; device work on HIP slot `slot`)."""
        compiled = self.compile_batch(codes)
        out = self._evaluate_compiled(list(codes), compiled, native=self.native, slot=slot)
        if self.fault_rate > 0:
            for i in range(len(out)):
                if self._fault_rng.random() < self.fault_rate:
                    out[i] = EvalResult(0.0, int(Exc.VALUE), "fault-injection")
                    self._bump("faults")
        return out

    def _evaluate_compiled(self, codes: Sequence[str], compiled: List[Optional[CompiledPolicy]],
                           native: bool, slot: int = 0, host_only: bool = False,
                           object_ok: bool = True) -> List[EvalResult]:
        n = len(codes)
        out: List[Optional[EvalResult]] = [None] * n
        # 1) device: native code, then the bytecode VM
        pending = [i for i, p in enumerate(compiled) if p is not None]
        if self.device is not None and not host_only:
            exact = getattr(self.device, "math_exact", True)
            dev_idx = [i for i in pending if compiled[i].device_ok and (exact or not compiled[i].uses_libm)]
            if dev_idx and native:
                self._absorb_native(dev_idx, compiled, out, slot)
            dev_idx = [i for i in dev_idx if out[i] is None]
            if len(dev_idx) >= self.device_min_batch:
                tab = self.device.evaluate_programs([compiled[i] for i in dev_idx], slot=slot)
                for row, i in zip(tab, dev_idx):
                    if int(row[COLS["exc"]]) in (Exc.UNSUPPORTED, Exc.BUDGET) or row[COLS["inexact"]]:
                        continue
                    out[i] = _row_to_result(row, "hip")
                    self._bump("device", 1)
        # 2) native CPU VM
        cpu_idx = [i for i in pending if out[i] is None]
        if cpu_idx:
            from .ops import cpu_engine
            tab = cpu_engine.simulate_program_batch(self.workload, [compiled[i] for i in cpu_idx],
                                                    cpu_engine.SimOptions(**self._cpu_opts()), self.cpu_threads)
            for row, i in zip(tab, cpu_idx):
                if int(row[COLS["exc"]]) in (Exc.UNSUPPORTED, Exc.BUDGET) or row[COLS["inexact"]]:
                    continue
                out[i] = _row_to_result(row, "cpu")
                self._bump("cpu_vm", 1)
        # 3) object engine (exact by construction)
        rest = [i for i in range(n) if out[i] is None]
        if rest and not object_ok:
            # the caller sheds what only CPython can score (bigint / complex
            # intermediates): engine "shed", never a score
            for i in rest:
                out[i] = EvalResult(0.0, int(Exc.UNSUPPORTED), "shed")
                self._bump("shed")
            rest = []
        if rest:
            if self._object_engine_ok():
                budget_s = float(self.options.get("object_timeout_s", 600.0))
                jobs = [(codes[i], self.workload, budget_s) for i in rest]
                if host_only:
                    # a worker thread (async fallback): the wall-clock budget needs a
                    # process main thread, so the replays run in the spawned object pool
                    results = list(self._object_pool().map(_object_worker, jobs))
                elif len(rest) > 1 and self.object_workers > 1:
                    with ProcessPoolExecutor(max_workers=min(self.object_workers, len(rest))) as ex:
                        results = list(ex.map(_object_worker, jobs))
                else:
                    results = [_object_worker(j) for j in jobs]
            else:
                results = [EvalResult(0.0, int(Exc.UNSUPPORTED), "none") for _ in rest]
            for i, r in zip(rest, results):
                out[i] = r
                self._bump("object", 1)
        return out  # type: ignore[return-value]

    def score_compiled(self, progs: Sequence[CompiledPolicy], slot: int = 0) -> np.ndarray:
        """Scores of already-compiled programs (e.g. constant variants of one
        shape, funsearch/polish.py): one native device launch when a device is
        attached (programs it declines fall back to the CPU VM), else the CPU VM."""
        out = np.zeros(len(progs))
        rest = list(range(len(progs)))
        if self.device is not None and self.native and progs:
            self.device.submit_native(slot, progs)
            tab = self.device.wait(slot)
            ok = np.array([not _native_deferred(row, self._bump) for row in tab], dtype=bool)
            out[ok] = tab[ok, COLS["score"]]
            rest = [i for i in range(len(progs)) if not ok[i]]
            self._bump("device_native", int(ok.sum()))
        if rest:
            from .ops import cpu_engine
            tab = cpu_engine.simulate_program_batch(self.workload, [progs[i] for i in rest],
                                                    cpu_engine.SimOptions(**self._cpu_opts()), self.cpu_threads)
            for row, i in zip(tab, rest):
                exc = int(row[COLS["exc"]])
                out[i] = 0.0 if exc else row[COLS["score"]]
            self._bump("cpu_vm", len(rest))
        return out

    # -- asynchronous program batches (pipelined islands) ------------------------------
    def submit_programs(self, codes: Sequence[str], slot: int) -> "PendingPrograms":
        """Start evaluating `codes` on device slot `slot` (its own HIP stream):
        compiles to bytecode and, on a device, JIT-compiles the native shapes and
        launches them; returns at once.  `ready` / `collect` finish the batch
        (programs the native backend declines run on the next engine at collect
        time).  Without a device everything happens at collect time."""
        return self.submit_compiled(codes, self.compile_batch(list(codes)), slot, count_errors=False)

    def submit_compiled(self, codes: Sequence[str], compiled: Sequence[Optional[CompiledPolicy]],
                        slot: int, count_errors: bool = True) -> "PendingPrograms":
        """`submit_programs` for programs whose bytecode was produced elsewhere
        (the steady-state search compiles in its producer processes)."""
        return self.launch_prepared(self.prepare_compiled(codes, compiled, count_errors), slot)

    def prepare_compiled(self, codes: Sequence[str], compiled: Sequence[Optional[CompiledPolicy]],
                         count_errors: bool = True) -> "PendingPrograms":
        """The compile half of `submit_compiled`, callable from a worker thread:
        JIT-compiles and loads the batch's native shapes (held until the batch
        is collected or `discard_prepared`).  `launch_prepared` starts it."""
        pend = PendingPrograms(list(codes), -1)
        pend.compiled = list(compiled)
        if count_errors:
            self._bump("compile_errors", sum(p is None for p in pend.compiled))
        if self.device is not None and self.native:
            idx = [i for i, p in enumerate(pend.compiled) if p is not None and p.device_ok]
            if idx:
                t0 = time.perf_counter()
                batch = self.device.prepare_native([pend.compiled[i] for i in idx])
                pend.prepared = batch
                pend.native_idx = idx
                pend.jit_s = batch.compile_s
                pend.new_shapes = batch.compiled
                pend.submit_s = time.perf_counter() - t0
                self._bump("jit_s", batch.compile_s)
                self._bump("jit_shapes", batch.compiled)
        return pend

    def launch_prepared(self, pend: "PendingPrograms", slot: int) -> "PendingPrograms":
        """Launch a `prepare_compiled` batch on device slot `slot` (main thread)."""
        pend.slot = slot
        if pend.native_idx:
            t0 = time.perf_counter()
            self.device.submit_native(slot, [pend.compiled[i] for i in pend.native_idx], pend.prepared)
            pend.prepared = None
            pend.t_launch = time.perf_counter()
            pend.submit_s += pend.t_launch - t0
        return pend

    def discard_prepared(self, pend: "PendingPrograms") -> None:
        """Give back the modules of a prepared batch that will not be launched."""
        if pend.prepared is not None:
            self.device.release_native(pend.prepared)
            pend.prepared = None

    def ready(self, pend) -> bool:
        """Slot index (family batches) or `PendingPrograms`: finished?"""
        if isinstance(pend, int):
            return self.device.ready(pend) if self.device is not None else True
        return not pend.native_idx or self.device.ready(pend.slot)

    def collect(self, pend: "PendingPrograms", defer_fallback: bool = False) -> List[Optional[EvalResult]]:
        """Results of a submitted batch.  Programs the device did not score
        (declined, deferred) run on the host engines here -- or, with
        `defer_fallback`, are left as None and listed in ``pend.fallback_idx``
        for `fallback_async` (the steady-state dispatcher must not block on a
        CPython replay)."""
        n = len(pend.codes)
        out: List[Optional[EvalResult]] = [None] * n
        if pend.native_idx:
            tab = self.device.wait(pend.slot)
            pend.t_done = time.perf_counter()
            for row, i in zip(tab, pend.native_idx):
                if _native_deferred(row, self._bump):
                    continue
                out[i] = _row_to_result(row, "hip-native")
                self._bump("device_native", 1)
        rest = [i for i in range(n) if out[i] is None]
        if rest and defer_fallback:
            pend.fallback_idx = rest
            if self.fault_rate > 0:
                for i in range(n):
                    if out[i] is not None and self._fault_rng.random() < self.fault_rate:
                        out[i] = EvalResult(0.0, int(Exc.VALUE), "fault-injection")
                        self._bump("faults")
            return out
        if rest:
            sub = self._evaluate_compiled([pend.codes[i] for i in rest], [pend.compiled[i] for i in rest],
                                          native=False, slot=pend.slot)
            for i, r in zip(rest, sub):
                out[i] = r
        if self.fault_rate > 0:
            for i in range(n):
                if self._fault_rng.random() < self.fault_rate:
                    out[i] = EvalResult(0.0, int(Exc.VALUE), "fault-injection")
                    self._bump("faults")
        return out  # type: ignore[return-value]

    def collect_partial(self, pend: "PendingPrograms") -> Tuple[List[Tuple[int, EvalResult]], bool]:
        """Streaming `collect` (device program service, `DeviceEvaluator.
        service_take`): the (index, result) pairs of the batch's programs that
        finished since the last call, and whether the batch is complete; on
        completion the programs the device did not score are listed in
        ``pend.fallback_idx`` (for `fallback_async`)."""
        got: List[Tuple[int, EvalResult]] = []
        complete = True
        if pend.native_idx:
            pos, rows, complete = self.device.service_take(pend.slot)
            for j, row in zip(pos, rows):
                i = pend.native_idx[int(j)]
                if _native_deferred(row, self._bump):
                    pend.deferred_idx.append(i)
                    continue
                r = _row_to_result(row, "hip-native")
                if len(row) > len(COLS):
                    r.device_cycles = float(row[len(COLS)])
                self._bump("device_native", 1)
                if self.fault_rate > 0 and self._fault_rng.random() < self.fault_rate:
                    r = EvalResult(0.0, int(Exc.VALUE), "fault-injection")
                    self._bump("faults")
                got.append((i, r))
        if complete:
            pend.t_done = time.perf_counter()
            native = set(pend.native_idx or ())
            pend.fallback_idx = sorted([i for i in range(len(pend.codes)) if i not in native] + pend.deferred_idx)
        return got, complete

    def fallback_async(self, pend: "PendingPrograms", object_ok: bool = True):
        """Score ``pend.fallback_idx`` on the host engines (CPU VM, then
        CPython unless `object_ok` is False) in a worker thread; the future
        yields (indices, results)."""
        idx = list(pend.fallback_idx)
        codes = [pend.codes[i] for i in idx]
        compiled = [pend.compiled[i] for i in idx]
        with self._compile_lock:
            if getattr(self, "_fallback_pool", None) is None:
                from concurrent.futures import ThreadPoolExecutor
                nice = int(getattr(self, "fallback_nice", 0))

                def lower_priority():
                    # a host fallback (a CPU-VM replay: seconds of a core for a large
                    # program) yields the cores to the threads that keep the GPU fed;
                    # nice is per thread on Linux and the VM's worker threads inherit it
                    if nice > 0 and hasattr(os, "setpriority") and hasattr(threading, "get_native_id"):
                        try:
                            os.setpriority(os.PRIO_PROCESS, threading.get_native_id(), nice)
                        except OSError:
                            pass
                self._fallback_pool = ThreadPoolExecutor(max_workers=2, thread_name_prefix="fks-fallback",
                                                         initializer=lower_priority)

        def job():
            res = self._evaluate_compiled(codes, compiled, native=False, host_only=True, object_ok=object_ok)
            if self.fault_rate > 0:
                for k in range(len(res)):
                    with self._stats_lock:
                        hit = self._fallback_fault_rng.random() < self.fault_rate
                    if hit:
                        res[k] = EvalResult(0.0, int(Exc.VALUE), "fault-injection")
            return idx, res
        return self._fallback_pool.submit(job)

    def _object_pool(self):
        """Persistent spawn pool for CPython replays started from worker threads."""
        with self._compile_lock:
            if getattr(self, "_obj_pool", None) is None:
                import multiprocessing
                self._obj_pool = ProcessPoolExecutor(max_workers=max(1, self.object_workers),
                                                     mp_context=multiprocessing.get_context("spawn"))
                atexit.register(self._obj_pool.shutdown, wait=False, cancel_futures=True)
        return self._obj_pool

    def _absorb_native(self, idx, compiled, out, slot: int) -> None:
        batch = self.device.submit_native(slot, [compiled[i] for i in idx])
        self._bump("jit_s", batch.compile_s)
        self._bump("jit_shapes", batch.compiled)
        tab = self.device.wait(slot)
        for row, i in zip(tab, idx):
            if _native_deferred(row, self._bump):
                continue
            out[i] = _row_to_result(row, "hip-native")
            self._bump("device_native", 1)

    def _object_engine_ok(self) -> bool:
        # the object engine implements only the reference's semantics
        return (self.options.get("repush", "first") == "first"
                and self.options.get("gpu_alloc", "best_fit") == "best_fit"
                and float(self.options.get("snapshot_interval", 0.05)) == 0.05)

    def scores(self, codes: Sequence[str]) -> List[float]:
        return [r.score for r in self.evaluate_programs(codes)]


@dataclass
class PendingPrograms:
    """A program batch in flight on one device slot (`Evaluator.submit_programs`)."""
    codes: List[str]
    slot: int
    compiled: List[Optional[CompiledPolicy]] = field(default_factory=list)
    native_idx: List[int] = field(default_factory=list)
    jit_s: float = 0.0
    submit_s: float = 0.0
    new_shapes: int = 0
    prepared: object = None          # NativeBatch compiled ahead, not launched yet
    t_launch: float = 0.0
    t_done: float = 0.0
    fallback_idx: List[int] = field(default_factory=list)
    deferred_idx: List[int] = field(default_factory=list)   # device rows deferred to the host (collect_partial)


class SuiteEvaluator:
    """Batched exact evaluator bound to a trace suite (`core.traces.load_suite`).

    Families go through the existing engines, one launch per trace; program
    batches through one fused device launch for the whole suite (`DeviceSuite`).

    ``evaluate_family`` / ``submit_family`` + ``wait`` return ``(tables, agg)``:
    the ``[T, P, 13]`` per-trace result tables and the ``[P, 4]`` suite
    aggregates (exact mean of the T scores, minimum, index of the first
    minimum, traces on which the policy raised; a raising trace scores 0).
    ``family`` is one family name or one name per policy (a mixed batch).
    On an MI355X every trace is resident on the device with a
    `DeviceEvaluator` of its own (``n_slots`` streams each, so T * n_slots
    streams in all) and a batch is submitted to all of them before any is
    waited for: one launch per trace, overlapping on the chip.  The CPU
    backend loops the native CPU engine over the traces.  Both reduce on the
    host with `exact_mean`.

    ``evaluate_family`` is the synchronous form on slot 0: it raises while a
    ``submit_family(0, ...)`` batch is still in flight.

    ``evaluate_programs`` returns, per trace, the `EvalResult` of every
    program text; ``score_programs`` the ``[T, P]`` scores and the same
    ``[P, 4]`` aggregates; ``submit_programs`` + ``wait_programs`` are its
    asynchronous form (slots of their own, not the family slots).  On an
    MI355X whose traces all fit the <= 16-node row layout, each text is
    compiled once and the batch runs as one grid of T * P two-wave workgroups
    (`ops.hip_engine.DeviceSuite`: one JIT for the suite, the longest traces
    first); rows the device declines or defers (UNSUPPORTED, BUDGET, TIMEOUT,
    inexact) are re-scored on that trace's CPU VM and then the object engine,
    so scores are the CPU backend's, and ``EvalResult.engine`` is
    ``"hip-native"`` on the rows taken from the device.  A suite the fused
    launch refuses, and the CPU backend, use one ``Evaluator(device="cpu")``
    per trace.

    ``device``: as for `Evaluator`.
    """

    def __init__(self, suite=None, device="auto", options: Optional[dict] = None, cpu_threads: int = 0,
                 n_slots: int = 4):
        from .core.traces import TraceSuite, load_suite
        if suite is None or isinstance(suite, str):
            suite = load_suite(suite or "openb")
        elif not isinstance(suite, TraceSuite):
            suite = TraceSuite(list(suite))
        self.suite = suite
        self.names = list(suite.names)
        self.options = dict(options or {})
        from .ops.cpu_engine import default_threads
        self.cpu_threads = cpu_threads or default_threads()
        self.devices = None   # one DeviceEvaluator per trace, or None (CPU backend)
        if device not in ("cpu", None):
            from .ops import hip_engine
            idx = device if isinstance(device, int) else int(os.environ.get("LOCAL_RANK", 0))
            available = hip_engine.device_available()
            if available and not isinstance(device, int):
                idx %= hip_engine.native().device_count()
            if not available and device != "auto":
                raise RuntimeError("HIP device requested but none is visible")
            if available:
                built = []   # dropped as a whole if one trace does not fit the device layout
                try:
                    for w in suite:
                        built.append(hip_engine.DeviceEvaluator(w, idx, self.options, n_slots))
                    self.devices = built
                except hip_engine.UnsupportedWorkload:
                    del built[:]
                    if device != "auto":
                        raise
        self._done: Dict[int, Tuple[np.ndarray, np.ndarray]] = {}   # CPU stand-in for in-flight slots
        self._in_flight: set = set()   # slots holding a submitted batch
        self._program_evaluators: Optional[List[Evaluator]] = None
        self.n_slots = n_slots
        self._device_suite = None      # hip_engine.DeviceSuite, built on first use (False: refused)
        self._programs_in_flight: Dict[int, tuple] = {}   # program slot -> pending batch
        self.stats = {"device_native": 0, "host": 0, "native_timeout": 0, "native_invariant": 0,
                      "jit_s": 0.0, "jit_shapes": 0}

    def __len__(self) -> int:
        return len(self.suite)

    @property
    def backend(self) -> str:
        return "hip" if self.devices is not None else "cpu"

    def _suite_cpu_opts(self) -> dict:
        from .ops.cpu_engine import DEFAULT_CALL_BUDGET
        keep = ("repush", "gpu_alloc", "snapshot_interval", "budget")
        opts = {k: v for k, v in self.options.items() if k in keep}
        opts.setdefault("budget", DEFAULT_CALL_BUDGET)
        return opts

    def _cpu_tables(self, family, weights) -> np.ndarray:
        from .ops import cpu_engine
        opts = cpu_engine.SimOptions(**self._suite_cpu_opts())
        if isinstance(family, str):
            return np.stack([cpu_engine.simulate_builtin_batch(w, family, weights, opts, self.cpu_threads)
                             for w in self.suite])
        # a mixed batch: the CPU engine takes one family per call
        family = list(family)
        wide = np.zeros((len(family), 16))
        if weights is not None:
            weights = np.asarray(weights, dtype=np.float64).reshape(len(family), -1)
            wide[:, :weights.shape[1]] = weights
        tables = np.zeros((len(self.suite), len(family), len(COLS)))
        for f in sorted(set(family)):
            idx = [i for i, g in enumerate(family) if g == f]
            for t, w in enumerate(self.suite):
                tables[t, idx] = cpu_engine.simulate_builtin_batch(w, f, wide[idx], opts, self.cpu_threads)
        return tables

    def evaluate_family(self, family, weights: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """(tables [T, P, 13], agg [P, 4]) for P members of a built-in family
        (or of the families named per policy).  Synchronous, on slot 0."""
        self.submit_family(0, family, weights)
        return self.wait(0)

    def submit_family(self, slot: int, family, weights: np.ndarray) -> None:
        if slot in self._in_flight:
            raise RuntimeError(f"suite slot {slot} busy: wait() for its batch first")
        if self.devices is not None:
            for dev in self.devices:
                dev.submit_builtin(slot, family, weights)
        else:
            from .simulator.metrics import suite_aggregate
            tables = self._cpu_tables(family, weights)
            self._done[slot] = (tables, suite_aggregate(tables))
        self._in_flight.add(slot)

    def wait(self, slot: int) -> Tuple[np.ndarray, np.ndarray]:
        if slot not in self._in_flight:
            raise ValueError(f"suite slot {slot} has no batch in flight")
        self._in_flight.discard(slot)
        if self.devices is None:
            return self._done.pop(slot)
        from .simulator.metrics import suite_aggregate
        tables = np.stack([dev.wait(slot) for dev in self.devices])
        return tables, suite_aggregate(tables)

    def _bump(self, key: str, n=1) -> None:
        self.stats[key] = self.stats.get(key, 0) + n

    def _cpu_evaluators(self) -> List[Evaluator]:
        if self._program_evaluators is None:
            self._program_evaluators = [Evaluator(w, "cpu", dict(self.options), self.cpu_threads) for w in self.suite]
        return self._program_evaluators

    @property
    def device_suite(self):
        """The suite's fused program launch (`hip_engine.DeviceSuite`), or None:
        CPU backend, ``native`` / fault injection options, or a suite the device
        path refuses (a trace off the <= 16-node row layout)."""
        if self._device_suite is None:
            self._device_suite = False
            if (self.devices is not None and self.options.get("native", True)
                    and not float(self.options.get("fault_rate", 0.0) or 0.0)):
                from .ops import hip_engine
                try:
                    self._device_suite = hip_engine.DeviceSuite(self.devices, self.n_slots)
                except ValueError:
                    pass
        return self._device_suite or None

    def _submit_programs(self, slot: int, codes: List[str]) -> tuple:
        ds = self.device_suite
        if ds is None:
            return (codes, None, None, [ev.evaluate_programs(codes) for ev in self._cpu_evaluators()])
        compiled = [try_compile(c)[0] for c in codes]   # once per text, for every trace
        dev_idx = [i for i, p in enumerate(compiled)
                   if p is not None and p.device_ok and (ds.math_exact or not p.uses_libm)]
        if dev_idx:
            batch = ds.submit_native(slot, [compiled[i] for i in dev_idx])
            self._bump("jit_s", batch.compile_s)
            self._bump("jit_shapes", batch.compiled)
        return (codes, compiled, dev_idx, None)

    def _collect_programs(self, slot: int, pend: tuple) -> List[List[EvalResult]]:
        codes, compiled, dev_idx, done = pend
        if done is not None:
            return done
        T, n = len(self.suite), len(codes)
        out: List[List[Optional[EvalResult]]] = [[None] * n for _ in range(T)]
        if dev_idx:
            tables = self.device_suite.wait(slot)
            for t in range(T):
                for row, i in zip(tables[t], dev_idx):
                    if _native_deferred(row, self._bump):
                        continue
                    out[t][i] = _row_to_result(row, "hip-native")
                    self._bump("device_native")
        # what the device did not take: that trace's CPU VM, then the object engine
        for t, ev in enumerate(self._cpu_evaluators()):
            rest = [i for i in range(n) if out[t][i] is None]
            if rest:
                for i in rest:
                    if compiled[i] is None:
                        ev._bump("compile_errors", 1)
                res = ev._evaluate_compiled([codes[i] for i in rest], [compiled[i] for i in rest], native=False)
                for i, r in zip(rest, res):
                    out[t][i] = r
                self._bump("host", len(rest))
        return out  # type: ignore[return-value]

    def evaluate_programs(self, codes: Sequence[str]) -> List[List[EvalResult]]:
        """Per trace, the results of the program texts.  Synchronous, on program slot 0."""
        if 0 in self._programs_in_flight:
            raise RuntimeError("suite program slot 0 busy: wait_programs() for its batch first")
        return self._collect_programs(0, self._submit_programs(0, list(codes)))

    @staticmethod
    def _scores_of(results: List[List[EvalResult]]) -> Tuple[np.ndarray, np.ndarray]:
        from .simulator.metrics import suite_aggregate_scores
        scores = np.array([[r.score for r in row] for row in results], dtype=np.float64).reshape(len(results), -1)
        raised = np.array([[r.exc != 0 for r in row] for row in results], dtype=bool).reshape(len(results), -1)
        return np.where(raised, 0.0, scores), suite_aggregate_scores(scores, raised)

    def score_programs(self, codes: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
        """(scores [T, P], agg [P, 4]) of the program texts: per-trace scores (a
        raising replay scores 0) and `suite_aggregate`'s aggregates of them."""
        return self._scores_of(self.evaluate_programs(codes))

    def submit_programs(self, slot: int, codes: Sequence[str]) -> None:
        """Start a program batch on program slot `slot` (on the device: one fused
        launch on the `DeviceSuite`'s slot); `wait_programs(slot)` returns what
        `score_programs` returns.  A slot still holding a batch raises."""
        if slot in self._programs_in_flight:
            raise RuntimeError(f"suite program slot {slot} busy: wait_programs() for its batch first")
        if not 0 <= slot < self.n_slots:
            raise IndexError(f"suite program slot {slot} outside [0, {self.n_slots})")
        self._programs_in_flight[slot] = self._submit_programs(slot, list(codes))

    def wait_programs(self, slot: int) -> Tuple[np.ndarray, np.ndarray]:
        if slot not in self._programs_in_flight:
            raise ValueError(f"suite program slot {slot} has no batch in flight")
        return self._scores_of(self._collect_programs(slot, self._programs_in_flight.pop(slot)))


_default: Dict[str, Evaluator] = {}


def evaluate(codes, device="auto", workload: Optional[Workload] = None, **options) -> List[float]:
    """Scores of policy programs (one program text or a list of them).

    Compatible with the reference's fitness: identical to running
    `evaluate_policy_standalone` on each program (exception -> 0)."""
    single = isinstance(codes, str)
    codes = [codes] if single else list(codes)
    if workload is None and not options:
        key = str(device)
        ev = _default.get(key)
        if ev is None:
            ev = _default[key] = Evaluator(None, device)
    else:
        ev = Evaluator(workload, device, options)
    scores = ev.scores(codes)
    return scores[0] if single else scores


def evaluate_detailed(codes: Sequence[str], device="auto", workload: Optional[Workload] = None,
                      **options) -> List[EvalResult]:
    return Evaluator(workload, device, options).evaluate_programs(list(codes))


def schedule(codes, device="auto", workload: Optional[Workload] = None, **options):
    """`ScheduleBatch` of policy programs (one program text or a list of them):
    each pod's node, GPUs and start time under every program, beside its row."""
    codes = [codes] if isinstance(codes, str) else list(codes)
    return Evaluator(workload, device, options).schedule_programs(codes)


def time_metrics(codes, device="auto", workload: Optional[Workload] = None, **options):
    """`TimeMetricsBatch` of policy programs (one program text or a list of
    them): waits, makespan and busy time of every program's replay, beside its row."""
    codes = [codes] if isinstance(codes, str) else list(codes)
    return Evaluator(workload, device, options).time_programs(codes)


def copy_workload(w: Workload) -> Workload:
    return copy.deepcopy(w)
