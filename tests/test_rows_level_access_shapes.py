"""CPU preconditions of tests/test_gpu_rows_level_access.py.

The device test can only catch a wrong access path of a pop round if the
replays reach that round.  On the CPU oracle and on the CPython object engine
(whose heap array is the one the device keeps, move for move) the large
workload of `level_access_shapes` must

* fit the row kernel: at most 16 nodes, at least 1,100 pods, so the heap starts
  above 1,024 entries and its pops walk rounds 0, 1 and 2;
* fail placements (`n_frag` > 0) in every replay, with no exception and no pod
  dropped, and tell the candidates apart;
* fail placements while the heap still holds more than 1,023 entries -- pops,
  pushes and scans then work on a heap whose last levels lie beyond every heap
  top the device test forces -- and at every depth on the way down: with 512
  to 1,023 entries, 32 to 511 and fewer than 32;
* drain the heap completely.
"""
import numpy as np

import level_access_shapes as la
from funsearch_kubernetes_simulator_amd.models import families as fam
from funsearch_kubernetes_simulator_amd.ops import cpu_engine as ce
from test_rows_scan_deletion_shapes import scans


def test_large_workload_fits_the_row_kernel_and_fails_placements():
    w = la.large()
    assert w.cluster.n_nodes <= 16 and w.pods.n_pods >= 1100
    assert w.pods.n_pods > max(la.TOPS) + 1
    for bname in ("composite_linear", "random_linear"):
        family, weights = la.batches()[bname]
        tab = ce.simulate_builtin_batch(w, family, weights)
        assert not tab[:, 10].any() and not tab[:, 11].any(), bname
        assert (tab[:, 7] > 0).all() and not tab[:, 9].any(), bname
        assert (tab[:, 8] > w.pods.n_pods).all(), bname
        assert len(set(tab[:, 0].tolist())) >= la.P // 2, bname


def test_large_workload_fails_placements_on_heaps_above_1023_entries():
    w = la.large()
    weights = la.batches()["composite_linear"][1]
    oracle = ce.simulate_builtin_batch(w, "composite_linear", weights[:1])
    s, events = scans(w, fam.to_program("composite_linear", weights[0]))
    assert events == int(oracle[0, 8]) and not oracle[0, 10]      # the object engine replays what the oracle does
    assert len(s) == int(oracle[0, 7]) > 0                         # one scan per failed placement
    n, f = s[:, 0], s[:, 1]
    assert (n > 1023).sum() >= 100
    assert ((n > 1023) & (f >= 0)).sum() >= 50                     # ... that find a deletion and push a retry
    assert ((n >= 512) & (n <= 1023)).sum() >= 100
    assert ((n >= 32) & (n < 512)).sum() >= 100
    assert (n < 32).sum() >= 1
    # a pop per event and one push per placement or anchored failure: the heap ends empty
    assert int(oracle[0, 9]) == 0 and (f < n).all()
