"""The phase-profiled kernel builds on the smallest catalogue shapes that reach them.

A profiled build replays exactly as its production kernel does, so every case
requires `np.array_equal` between the profiled launch's result table, the
table of the unprofiled launch on the same evaluator, and the CPU oracle (as
`tests/test_gpu_shapes.py` takes it), and checks the shape of the cycle array.

  k_replay_builtin_prof<false / true>   profile_builtin, 17 nodes, LDS / HBM heap
  k_replay_c5_prof                      profile_builtin("composite_linear"), 129 nodes, HBM heap
  k_replay_vm_prof<false / true>        profile_programs, 17 nodes, LDS / HBM heap
  k_replay_rows_prof<...>               profile_rows, 5 nodes: random_linear, composite_linear, mixed
  k_replay_rows_native_prof             profile_native, 5 nodes, one and four programs per wave

Not here: `profile_native` on the two-wave kernel (k_replay_native_duo_prof).
Its host side copies [2 P, 16] words back from a cycle buffer sized for the
[P, 2, 8] the kernel writes, so the case was left out instead of run.
"""
import numpy as np
import pytest

import device_shapes as ds
from funsearch_kubernetes_simulator_amd.policy.bytecode import Exc
from test_gpu_shapes import _check_programs, _device, _same, builtin_oracle

pytestmark = pytest.mark.gpu

HEAPS = ("lds", "hbm")
WAVE_SHAPE = "sweep017"    # NPASS 1, too wide for the row kernel
C5_SHAPE = "sweep129"      # NPASS 4
ROW_SHAPE = "sweep005"
ROW_PROF_WORDS = 16        # per wave: phase cycles [0, 8), wave-steps by kind [9, 16)


@pytest.mark.parametrize("heap", HEAPS)
def test_profiled_builtin_wave_kernel(heap):
    """The profiled build scores with the mixed-family scorer: every single-family batch."""
    w = ds.shape(WAVE_SHAPE)
    dev = _device(w, {"heap_mode": heap})
    assert dev.info()["npass"] == 1
    for batch in ("first_fit", "best_fit") + ds.FAMILIES:
        family, weights = ds.candidates()[batch]
        assert not dev._eng.would_use_rows(len(weights))
        assert dev._eng.would_use_hbm(len(weights)) == (heap == "hbm")
        tab, cycles = dev.profile_builtin(family, weights)
        assert cycles.shape == (len(weights), 8) and cycles.dtype == np.uint64
        _same(tab, dev.evaluate_builtin(family, weights), (batch, heap, "unprofiled"))
        _same(tab, builtin_oracle(w, family, weights), (batch, heap, "oracle"))


def test_profiled_composite_on_256_node_kernel():
    w = ds.shape(C5_SHAPE)
    dev = _device(w, {"heap_mode": "hbm"})
    info = dev.info()
    assert info["fast_div"] == 1 and info["npass"] == 4
    family, weights = ds.candidates()["composite_linear"]
    tab, cycles = dev.profile_builtin(family, weights)
    assert cycles.shape == (len(weights), 8) and cycles.dtype == np.uint64
    _same(tab, dev.evaluate_builtin(family, weights), "unprofiled")
    _same(tab, builtin_oracle(w, family, weights), "oracle")


@pytest.mark.parametrize("heap", HEAPS)
def test_profiled_device_vm(heap):
    dev = _device(ds.program_workload(WAVE_SHAPE), {"heap_mode": heap})
    progs = ds.programs()[1]
    assert dev._eng.would_use_hbm(len(progs)) == (heap == "hbm")
    tab, cycles = dev.profile_programs(progs)
    assert cycles.shape == (len(progs), 8) and cycles.dtype == np.uint64
    _same(tab, dev.evaluate_programs(progs), (heap, "unprofiled"))
    _check_programs(WAVE_SHAPE, tab, (WAVE_SHAPE, "vm-prof-" + heap))


@pytest.mark.parametrize("batch", ("random_linear", "composite_linear", "mixed"))
def test_profiled_row_kernel(batch):
    w = ds.shape(ROW_SHAPE)
    dev = _device(w, {})
    family, weights = ds.candidates()[batch]
    P = len(weights)
    assert dev._eng.would_use_rows(P)
    tab, cycles = dev.profile_rows(family, weights)
    assert cycles.shape == ((P + 3) // 4, ROW_PROF_WORDS) and cycles.dtype == np.uint64   # four policies per wave
    _same(tab, dev.evaluate_builtin(family, weights), (batch, "unprofiled"))
    _same(tab, builtin_oracle(w, family, weights), (batch, "oracle"))


@pytest.mark.parametrize("rows,options", [(1, {"native_rows": 1, "native_duo": False}), (4, {"native_rows": 4})],
                         ids=["rows1", "rows4"])
def test_profiled_native_row_kernel(rows, options):
    dev = _device(ds.program_workload(ROW_SHAPE), options)
    progs = ds.programs()[1]
    assert dev._eng.would_use_rows(len(progs))
    want = dev.evaluate_native(progs)
    assert dev.info()["native_rows_last"] == rows
    # the profiled launch takes natively compiled programs only: the rows of
    # programs the JIT declined stay EXC_UNSUPPORTED, as `wait` leaves them
    native = np.flatnonzero(want[:, 10] != Exc.UNSUPPORTED)
    got = np.zeros_like(want)
    got[:, 10] = Exc.UNSUPPORTED
    got[native], cycles = dev.profile_native([progs[i] for i in native])
    assert dev.info()["native_rows_last"] == rows
    assert cycles.shape == ((len(native) + rows - 1) // rows, ROW_PROF_WORDS) and cycles.dtype == np.uint64
    _same(got, want, (rows, "unprofiled"))
    _check_programs(ROW_SHAPE, got, (ROW_SHAPE, f"native-rows{rows}-prof"))
