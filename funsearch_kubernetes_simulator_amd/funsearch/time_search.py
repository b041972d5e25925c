"""Family search with a time-aware fitness: the `ParamIsland` loop on the time-metrics mode.

The reference's score lives in event-count space: it never says how long pods
waited or how long the schedule took.  Here every generation's candidates are
replayed in time mode (`engine.Evaluator.time_family`: on the device the time
instances of the row kernel, one launch per generation) and an island's
fitness is a linear objective over named columns of the result
(`core.time_metrics.COLUMNS`), e.g. ``{"score": 1.0, "mean_wait": -2e-5}``:

    score, mean_wait, wait_max, span, tw_cpu, tw_mem, tw_gpu_count,
    tw_gpu_milli, frac_waited

A candidate whose replay raised or left pods unplaced has fitness -inf.

    python -m funsearch_kubernetes_simulator_amd.funsearch.time_search configs/time_composite.json

The champion is saved in the policy JSON shape of the other searches (score,
generation, code, timestamp, family, weights) plus ``fitness``, ``objective``
and a ``time_metrics`` block: its integer record and the derived figures.
"""

from __future__ import annotations

import json
import os
import sys
import time
from datetime import datetime
from typing import Dict, Optional

import numpy as np

from ..core.time_metrics import COLUMNS, TimeMetricsBatch
from ..engine import COLS, Evaluator
from ..models import families as fam
from .param_islands import make_islands


def fitness(tm: TimeMetricsBatch, objective: Dict[str, float]) -> np.ndarray:
    """The objective per candidate [P]; -inf where the replay raised or left pods unplaced."""
    f = np.zeros(len(tm))
    for name, coef in objective.items():
        f += float(coef) * tm.column(name)
    bad = (tm.rows[:, COLS["exc"]] != 0) | (tm.rows[:, COLS["n_unplaced"]] != 0)
    f[bad] = -np.inf
    return f


def run(config: dict, evaluator: Optional[Evaluator] = None, log=print) -> dict:
    """Run the search described by `config`; returns the saved champion record."""
    family = config.get("family", "composite_linear")
    objective = dict(config.get("objective", {"score": 1.0}))
    unknown = [k for k in objective if k not in COLUMNS]
    if unknown or not objective:
        raise ValueError(f'"objective" names must be among {", ".join(COLUMNS)} (got {unknown or "none"})')
    if evaluator is None:
        evaluator = Evaluator(None, config.get("device", "auto"), config.get("options"))
    islands = make_islands(int(config.get("islands", 1)), family, int(config.get("candidates", 4096)),
                           int(config.get("elite_size", 32)), int(config.get("seed", 0)))
    for isl in islands:
        isl.sigma = float(config.get("sigma", isl.sigma))
    generations = int(config.get("generations", 20))
    best = None
    t0 = time.perf_counter()
    replays = 0
    for g in range(generations):
        for isl in islands:
            w = isl.propose()
            tm = evaluator.time_family(family, w)
            replays += len(tm)
            f = fitness(tm, objective)
            isl.update(w, f, tm.rows[:, COLS["n_events"]])
            i = int(np.argmax(f))
            if best is None or f[i] > best["fitness"]:
                best = {"fitness": float(f[i]), "generation": g + 1, "weights": w[i].copy(),
                        "score": float(tm.rows[i, COLS["score"]]), "block": tm.block(i)}
        log(f"[time_search] gen {g + 1}/{generations}: best fitness {best['fitness']:.6f} (score {best['score']:.6f}, "
            f"mean wait {best['block']['mean_wait']:.1f} s, span {best['block']['span']} s); "
            f"{replays / (time.perf_counter() - t0):.0f} replays/s on {evaluator.backend}")
    record = {"score": best["score"], "generation": best["generation"],
              "code": fam.to_program(family, best["weights"]), "timestamp": datetime.now().isoformat(),
              "family": family, "weights": [float(x) for x in best["weights"]],
              "fitness": best["fitness"], "objective": objective, "time_metrics": best["block"]}
    out = config.get("save_best")
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as fh:
            json.dump(record, fh, indent=2)
        log(f"[time_search] champion saved to {out}")
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
