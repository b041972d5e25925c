"""Family search on a trace suite: the `ParamIsland` loop with a suite aggregate as fitness.

Every generation's candidates are scored on every trace of the suite
(`engine.SuiteEvaluator`); an island's fitness is the exact mean of a
candidate's per-trace scores (``"aggregate": "mean"``) or its worst trace
(``"min"``), so the search cannot win by overfitting one trace.

    python -m funsearch_kubernetes_simulator_amd.funsearch.suite_search configs/suite_composite.json

The champion is saved in the policy JSON shape of the other searches (score,
generation, code, timestamp, family, weights) plus a ``suite`` block with its
per-trace result rows and both aggregates.
"""

from __future__ import annotations

import json
import os
import sys
import time
from datetime import datetime
from typing import Optional

import numpy as np

from ..engine import COLS, SuiteEvaluator
from ..models import families as fam
from .param_islands import make_islands

AGGREGATES = {"mean": 0, "min": 1}


def suite_block(names, tables_p: np.ndarray, agg_p: np.ndarray, aggregate: str) -> dict:
    """The ``suite`` block of a saved policy: one candidate's rows [T, 13] and aggregates [4]."""
    cols = list(COLS)
    return {"traces": list(names), "aggregate": aggregate, "mean": float(agg_p[0]), "min": float(agg_p[1]),
            "argmin": names[int(agg_p[2])], "raised": int(agg_p[3]),
            "per_trace": {n: {c: float(v) for c, v in zip(cols, row)} for n, row in zip(names, tables_p)}}


def run(config: dict, evaluator: Optional[SuiteEvaluator] = None, log=print) -> dict:
    """Run the search described by `config`; returns the saved champion record."""
    family = config.get("family", "composite_linear")
    aggregate = config.get("aggregate", "mean")
    if aggregate not in AGGREGATES:
        raise ValueError(f'"aggregate" must be one of {sorted(AGGREGATES)}')
    col = AGGREGATES[aggregate]
    if evaluator is None:
        from ..core.traces import load_suite
        suite = load_suite(config.get("suite", "openb"), config.get("traces_dir"))
        evaluator = SuiteEvaluator(suite, config.get("device", "auto"), config.get("options"))
    names = evaluator.names
    islands = make_islands(int(config.get("islands", 1)), family, int(config.get("candidates", 4096)),
                           int(config.get("elite_size", 32)), int(config.get("seed", 0)))
    for isl in islands:
        isl.sigma = float(config.get("sigma", isl.sigma))
    generations = int(config.get("generations", 50))
    best = {"score": float("-inf")}
    t0 = time.perf_counter()
    replays = 0
    for g in range(generations):
        for isl in islands:
            w = isl.propose()
            tables, agg = evaluator.evaluate_family(family, w)
            replays += tables.shape[0] * tables.shape[1]
            isl.update(w, agg[:, col], tables[:, :, COLS["n_events"]].max(axis=0))
            i = int(np.argmax(agg[:, col]))
            if agg[i, col] > best["score"]:
                best = {"score": float(agg[i, col]), "generation": g + 1, "weights": w[i].copy(),
                        "tables": tables[:, i].copy(), "agg": agg[i].copy()}
        log(f"[suite_search] gen {g + 1}/{generations}: best {aggregate} {best['score']:.6f} "
            f"(mean {best['agg'][0]:.6f}, min {best['agg'][1]:.6f}); "
            f"{replays / (time.perf_counter() - t0):.0f} (trace, policy) replays/s on {evaluator.backend}")
    record = {"score": best["score"], "generation": best["generation"],
              "code": fam.to_program(family, best["weights"]), "timestamp": datetime.now().isoformat(),
              "family": family, "weights": [float(x) for x in best["weights"]],
              "suite": suite_block(names, best["tables"], best["agg"], aggregate)}
    out = config.get("save_best")
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as fh:
            json.dump(record, fh, indent=2)
        log(f"[suite_search] champion saved to {out}")
    return record


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv:
        print(__doc__)
        return 2
    with open(argv[0]) as fh:
        config = json.load(fh)
    for kv in argv[1:]:   # key=value overrides (JSON values)
        k, _, v = kv.partition("=")
        try:
            config[k] = json.loads(v)
        except json.JSONDecodeError:
            config[k] = v
    run(config)
    return 0


if __name__ == "__main__":
    sys.exit(main())
