"""How long a replay's pods waited and how long its schedule took.

The 13-column row scores a policy in event-count space; a `TimeMetricsBatch`
holds, per policy, integer sums and maxima over the pods its replay *placed*
(the record, `RECORD_WORDS` 64-bit words, the same on every engine):

    wait_sum   sum of start - pod_ctime
    wait_max   max of the same (0 if none placed)
    end_max    max of start + dur (0 if none placed)
    busy[4]    sum of cpu*dur, mem*dur, ngpu*dur, ngpu*gmilli*dur
    n_placed   count
    hist[32]   hist[b] = pods with bit_length(wait) == b, clamped at 31

Every placed pod is later deleted (the event loop drains the heap), so
`busy[k]` is exactly the time integral of the cluster's usage of resource k.
Everything is an integer, so two engines agree bit for bit or not at all.  The
derived figures are computed here, on the host, from Python ints with one
correctly rounded division each.  A replay that raised (`exc != 0`) has an
all-zero record.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from .arrays import Workload

#: columns of the result rows used here (ops.cpu_engine.RESULT_COLUMNS)
_SCORE, _N_UNPLACED, _EXC = 0, 9, 10
#: the record as the engines return it: 8 int64 slots, then 32 uint32 buckets (16 words of two)
RECORD_WORDS = 24
BUSY_NAMES = ("cpu", "mem", "gpu_count", "gpu_milli")
#: names a `funsearch.time_search` objective may use
COLUMNS = ("score", "mean_wait", "wait_max", "span", "tw_cpu", "tw_mem", "tw_gpu_count", "tw_gpu_milli", "frac_waited")


def wait_bucket(wait: int) -> int:
    """Histogram bucket of a wait: its bit length, clamped at 31 (0: did not wait)."""
    return min(int(wait).bit_length(), 31)


def overflow_gate(workload: Workload, time_bits: Optional[int] = None) -> Optional[str]:
    """None if no 64-bit sum of time mode can overflow on this workload, else
    why it can: over *all* pods (a replay places at most all of them), the four
    products sum x*dur and n_pods * 2^time_bits (a bound on wait_sum: on the
    device every event time fits the packed key's `time_bits`) must stay below
    2^63, and no duration or demand may be negative.  Without `time_bits` (the
    host engines, whose times are plain int64) the bound on an event time is
    max(pod_ctime) + sum(dur) + n_pods: a start is a creation time or one past
    a deletion, and deletions chain through at most every pod's duration.
    Python ints throughout."""
    p = workload.pods
    cols = {"duration": p.pod_dur, "cpu": p.pod_cpu, "memory": p.pod_mem, "num_gpu": p.pod_ngpu, "gpu_milli": p.pod_gmilli}
    for name, a in cols.items():
        if len(a) and int(np.min(a)) < 0:
            return f"negative {name}"
    dur = [int(x) for x in p.pod_dur]
    ngpu = [int(x) for x in p.pod_ngpu]
    sums = {
        "cpu*dur": sum(int(x) * d for x, d in zip(p.pod_cpu, dur)),
        "mem*dur": sum(int(x) * d for x, d in zip(p.pod_mem, dur)),
        "ngpu*dur": sum(g * d for g, d in zip(ngpu, dur)),
        "ngpu*gmilli*dur": sum(g * int(m) * d for g, m, d in zip(ngpu, p.pod_gmilli, dur)),
    }
    if time_bits is not None:
        sums["n_pods * 2^time_bits"] = p.n_pods << int(time_bits)
    else:
        sums["n_pods * latest event time"] = p.n_pods * (int(np.max(p.pod_ctime, initial=0)) + sum(dur) + p.n_pods)
    for name, v in sums.items():
        if v >= 2 ** 63:
            return f"sum of {name} over all pods is {v.bit_length()} bits"
    return None


def _div(a: int, b: int) -> float:
    return a / b if b else 0.0   # int / int: correctly rounded


@dataclass
class TimeMetricsBatch:
    """The time metrics of a policy batch.  Raw integer arrays `[P]` (and
    `busy [P, 4]`, `hist [P, 32]`), the replays' `rows [P, 13]`, `engine[i]`
    naming the engine that gave record i, and the derived figures as
    properties (float64 arrays, each element one division of Python ints)."""

    wait_sum: np.ndarray   # int64 [P]
    wait_max: np.ndarray   # int64 [P]
    end_max: np.ndarray    # int64 [P]
    busy: np.ndarray       # int64 [P, 4]
    n_placed: np.ndarray   # int64 [P]
    hist: np.ndarray       # uint32 [P, 32]
    rows: np.ndarray       # float64 [P, 13]
    engine: List[str]
    t0: int = 0                       # min(pod_ctime) of the workload
    totals: Sequence[int] = (0, 0, 0, 0)   # the cluster's cpu, memory, GPU count, GPU milli totals

    RAW = ("wait_sum", "wait_max", "end_max", "busy", "n_placed", "hist")

    def __post_init__(self):
        for f in ("wait_sum", "wait_max", "end_max", "busy", "n_placed"):
            setattr(self, f, np.ascontiguousarray(getattr(self, f), dtype=np.int64))
        self.hist = np.ascontiguousarray(self.hist, dtype=np.uint32)
        self.rows = np.ascontiguousarray(self.rows, dtype=np.float64)
        self.totals = tuple(int(x) for x in self.totals)
        raised = np.flatnonzero(self.rows[:, _EXC] != 0) if len(self.rows) else []
        for i in raised:
            for f in self.RAW:
                getattr(self, f)[i] = 0

    def __len__(self) -> int:
        return len(self.rows)

    # -- construction ---------------------------------------------------------------------
    @staticmethod
    def workload_constants(workload: Workload):
        c, p = workload.cluster, workload.pods
        t0 = int(p.pod_ctime.min()) if p.n_pods else 0
        totals = (int(c.node_cpu_total.sum()), int(c.node_mem_total.sum()), int(c.node_ngpus.sum()),
                  int(c.gpu_milli_total.astype(np.int64).sum()))
        return t0, totals

    @classmethod
    def from_records(cls, rows: np.ndarray, rec: np.ndarray, engine, workload: Workload) -> "TimeMetricsBatch":
        """From the engines' records `rec` [P, RECORD_WORDS] int64."""
        rec = np.ascontiguousarray(rec, dtype=np.int64).reshape(-1, RECORD_WORDS)
        hist = rec[:, 8:].copy().view(np.uint32).reshape(len(rec), 32)
        engine = [engine] * len(rec) if isinstance(engine, str) else list(engine)
        t0, totals = cls.workload_constants(workload)
        return cls(rec[:, 0].copy(), rec[:, 1].copy(), rec[:, 2].copy(), rec[:, 3:7].copy(), rec[:, 7].copy(), hist,
                   np.array(rows, dtype=np.float64), engine, t0, totals)

    @classmethod
    def empty(cls, n: int, workload: Workload) -> "TimeMetricsBatch":
        """`n` all-zero records with zero rows, to be filled by `put`."""
        return cls.from_records(np.zeros((n, 13)), np.zeros((n, RECORD_WORDS), np.int64), [""] * n, workload)

    def put(self, idx, other: "TimeMetricsBatch", sel=None) -> None:
        """Copy `other`'s policies `sel` (default: all) to positions `idx`."""
        sel = list(range(len(other))) if sel is None else list(sel)
        for i, j in zip(idx, sel):
            for f in self.RAW + ("rows",):
                getattr(self, f)[i] = getattr(other, f)[j]
            self.engine[i] = other.engine[j]

    def raw_equal(self, other: "TimeMetricsBatch") -> bool:
        return all(np.array_equal(getattr(self, f), getattr(other, f)) for f in self.RAW)

    def record(self, i: int) -> dict:
        """Record i as Python ints."""
        return {"wait_sum": int(self.wait_sum[i]), "wait_max": int(self.wait_max[i]), "end_max": int(self.end_max[i]),
                "busy": [int(x) for x in self.busy[i]], "n_placed": int(self.n_placed[i]),
                "hist": [int(x) for x in self.hist[i]]}

    # -- derived figures (host only) ------------------------------------------------------
    def _each(self, f) -> np.ndarray:
        return np.array([f(i) for i in range(len(self))], dtype=np.float64)

    def span_int(self, i: int) -> int:
        return int(self.end_max[i]) - self.t0 if int(self.n_placed[i]) else 0

    @property
    def mean_wait(self) -> np.ndarray:
        return self._each(lambda i: _div(int(self.wait_sum[i]), int(self.n_placed[i])))

    @property
    def span(self) -> np.ndarray:
        return self._each(lambda i: float(self.span_int(i)))

    @property
    def tw_util(self) -> np.ndarray:
        """[P, 4]: busy[k] / (tot[k] * span), 0 where a denominator is 0."""
        out = np.zeros((len(self), 4))
        for i in range(len(self)):
            for k in range(4):
                out[i, k] = _div(int(self.busy[i, k]), self.totals[k] * self.span_int(i))
        return out

    @property
    def frac_waited(self) -> np.ndarray:
        return self._each(lambda i: _div(int(self.n_placed[i]) - int(self.hist[i, 0]), int(self.n_placed[i])))

    def wait_quantile_bound(self, q: float) -> np.ndarray:
        """Per policy, the upper edge of the histogram bucket that holds the
        q-quantile of the waits (bucket b holds waits in [2^(b-1), 2^b - 1];
        bucket 0 only 0; bucket 31 is open: its edge is `wait_max`).  0 if
        nothing was placed."""
        if not 0.0 <= q <= 1.0:
            raise ValueError("q must be in [0, 1]")
        out = np.zeros(len(self), dtype=np.int64)
        for i in range(len(self)):
            n = int(self.n_placed[i])
            if n == 0:
                continue
            need = max(1, int(np.ceil(q * n)))
            seen = 0
            for b in range(32):
                seen += int(self.hist[i, b])
                if seen >= need:
                    out[i] = 0 if b == 0 else int(self.wait_max[i]) if b == 31 else (1 << b) - 1
                    break
        return out

    def column(self, name: str) -> np.ndarray:
        """One of `COLUMNS` as a float64 array [P]."""
        if name == "score":
            return self.rows[:, _SCORE].copy()
        if name == "wait_max":
            return self.wait_max.astype(np.float64)
        if name in ("mean_wait", "span", "frac_waited"):
            return getattr(self, name)
        if name.startswith("tw_") and name[3:] in BUSY_NAMES:
            return self.tw_util[:, BUSY_NAMES.index(name[3:])]
        raise KeyError(f"unknown time-metrics column {name!r} (one of {', '.join(COLUMNS)})")

    def block(self, i: int) -> dict:
        """Record i and its derived figures, as saved beside a champion."""
        d = self.record(i)
        tw = self.tw_util[i]
        d.update(engine=self.engine[i], mean_wait=float(self.mean_wait[i]), span=self.span_int(i),
                 frac_waited=float(self.frac_waited[i]), tw_util={n: float(tw[k]) for k, n in enumerate(BUSY_NAMES)},
                 wait_p50_bound=int(self.wait_quantile_bound(0.5)[i]), wait_p95_bound=int(self.wait_quantile_bound(0.95)[i]))
        return d
