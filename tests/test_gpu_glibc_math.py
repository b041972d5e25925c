"""The device build of glibc_math.h on the MI355X equals the host build (and
so CPython) bit for bit, and a pow / exp / log-heavy policy program replayed
natively on the device equals the CPU VM, which calls the host libm."""
import math
import sys

import numpy as np
import pytest

from funsearch_kubernetes_simulator_amd.ops import cpu_engine as ce
from funsearch_kubernetes_simulator_amd.policy.compiler import compile_policy

pytestmark = pytest.mark.gpu


def test_device_equals_host_build():
    from funsearch_kubernetes_simulator_amd.ops import hip_engine as he
    if not he.device_available():
        pytest.fail("GPU test collected but no HIP device is visible")
    m = he.native()
    rng = np.random.default_rng(3)
    n = 1 << 20
    xs = np.concatenate([rng.uniform(-745, 709.7, n // 2), rng.uniform(-2, 2, n // 2)])
    lx = np.concatenate([rng.uniform(0, 100, n // 2), 1 + rng.uniform(-0.07, 0.07, n // 2)])
    px = np.concatenate([rng.uniform(1e-3, 3, n // 2), rng.uniform(1, 1e4, n // 2)])
    py = np.concatenate([rng.uniform(-30, 30, n // 2), rng.uniform(-300, 300, n // 2)])
    for fn, x, y, host in ((0, xs, xs, lambda: m.gm_exp_batch(xs)), (1, lx, lx, lambda: m.gm_log_batch(lx)),
                           (2, px, py, lambda: m.gm_pow_batch(px, py))):
        dst, dout = m.gm_device_batch(fn, x, y, 0)
        hst, hout = host()
        assert np.array_equal(dst, hst), fn
        assert np.array_equal(dout.view(np.uint64), hout.view(np.uint64)), fn


def _device_and_host(m, fn, x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    dst, dout = m.gm_device_batch(fn, x, y, 0)
    hst, hout = m.gm_exp_batch(x) if fn == 0 else m.gm_log_batch(x) if fn == 1 else m.gm_pow_batch(x, y)
    return dst, dout, hst, hout


def test_device_takes_every_branch_of_the_self_check():
    """The arguments of the host self-check (`glibc_math_selfcheck`: tiny and
    huge exp arguments, subnormal log and pow arguments, |y| below 2^-65 and
    above 2^63, pow results over- and underflowing), 2^18 per function, through
    the device build: status and result bits of the host build."""
    from funsearch_kubernetes_simulator_amd.ops import hip_engine as he
    if not he.device_available():
        pytest.fail("GPU test collected but no HIP device is visible")
    m = he.native()
    n = 1 << 18
    ex, lx, px, py = m.glibc_math_selfcheck_args(n, 7)
    assert len(ex) == len(lx) == len(px) == len(py) == n
    # the draw reaches the branches the uniform draws of the test above never do
    assert (np.abs(ex) < 2.0 ** -54).any() and (np.abs(ex) >= 1024).any()
    assert (lx < 2.0 ** -1022).any() and (px < 2.0 ** -1022).any() and (lx > 0).all() and (px > 0).all()
    assert (np.abs(py) < 2.0 ** -65).any() and (np.abs(py) >= 2.0 ** 63).any() and (px != 1).all() and (py != 0).all()
    for fn, x, y in ((0, ex, ex), (1, lx, lx), (2, px, py)):
        dst, dout, hst, hout = _device_and_host(m, fn, x, y)
        assert np.array_equal(dst, hst), fn
        assert np.array_equal(dout.view(np.uint64), hout.view(np.uint64)), fn
        if fn != 1:   # over- and underflow happen
            assert (hst == 1).any() and (hout[hst == 0] == 0).any() and (np.abs(hout[hst == 0]) < 2.0 ** -1022).any(), fn


def _last_true(pred, lo, hi):
    """The largest double in [lo, hi) on which the monotone `pred` holds (pred(lo), not pred(hi))."""
    def key(x):
        b = int(np.float64(x).view(np.int64))
        return b if b >= 0 else -(b & 0x7FFFFFFFFFFFFFFF)

    def val(k):
        return float(np.int64(k if k >= 0 else -k | -(1 << 63)).view(np.float64))
    a, b = key(lo), key(hi)
    assert pred(lo) and not pred(hi)
    while b - a > 1:
        mid = (a + b) // 2
        a, b = (mid, b) if pred(val(mid)) else (a, mid)
    return val(a)


def _around(x, k=1):
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo, hi = math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf)
        out += [lo, hi]
    return out


def _finite(f, *a):
    try:
        return math.isfinite(f(*a))
    except OverflowError:
        return False


def branch_edge_arguments():
    """Hand list at the branch edges of exp / log / pow, inside their domains
    (exp: finite x; log: finite x > 0; pow: finite x > 0, x != 1, finite y != 0)."""
    dbl_max, tiny = sys.float_info.max, 2.0 ** -1022
    exp_x = []
    for s in (1.0, -1.0):
        exp_x += _around(s * 2.0 ** -54) + _around(s * 1024.0) + [s * 5e-324, s * dbl_max, s * 0.0]
    exp_x += _around(_last_true(lambda x: _finite(math.exp, x), 709.0, 710.0), 2)        # largest finite, successors
    exp_x += _around(_last_true(lambda x: math.exp(x) < tiny, -709.0, -708.0), 2)        # first subnormal result
    exp_x += _around(_last_true(lambda x: math.exp(x) == 0.0, -746.0, -745.0), 2)        # first zero result
    log_x = [5e-324, 1.0, dbl_max, math.nextafter(dbl_max, 0.0), math.nextafter(1.0, math.inf), math.nextafter(1.0, 0.0)]
    log_x += [tiny, math.nextafter(tiny, 0.0), math.nextafter(tiny, 1.0)]
    log_x += _around(1.0 - 2.0 ** -4, 2) + _around(1.0 + float.fromhex("0x1.09p-4"), 2)   # the near-1 window
    pw = []
    near_one = (0.5, 2.0, math.nextafter(1.0, 0.0), math.nextafter(1.0, 2.0), 0.999, 1.001, 1e-300, 1e300)
    for x in near_one:
        for s in (1.0, -1.0):
            pw += [(x, s * y) for y in _around(2.0 ** -65) + _around(2.0 ** 63) + [5e-324, dbl_max]]
    for x in (5e-324, 2.0 ** -1023, math.nextafter(tiny, 0.0), tiny):
        pw += [(x, y) for y in (0.5, -0.5, 2.0, -2.0, 1e-3, -1e-3, 1.0, -1.0, 1 / 3, 1e-310)]
    pw += [(2.0, y) for y in _around(1024.0, 2) + _around(-1022.0, 2) + _around(-1074.0, 2) + _around(-1075.0, 2)]
    pw += [(0.5, y) for y in _around(-1024.0, 2) + _around(1022.0, 2) + _around(1074.0, 2) + _around(1075.0, 2)]
    pw += [(10.0, y) for y in _around(_last_true(lambda y: _finite(pow, 10.0, y), 308.0, 309.0), 2)]
    pw += [(10.0, y) for y in _around(_last_true(lambda y: 10.0 ** y < tiny, -308.0, -307.0), 2)]
    pw += [(10.0, y) for y in _around(_last_true(lambda y: 10.0 ** y == 0.0, -324.0, -323.0), 2)]
    pw += [(0.1, y) for y in _around(_last_true(lambda y: 0.1 ** y > 0.0, 323.0, 324.0), 2)]
    return exp_x, log_x, pw


def test_device_at_the_branch_edges():
    """The hand list: device == host build (status and bits) == CPython's
    math.exp / math.log / ** (an OverflowError there is status 1)."""
    from funsearch_kubernetes_simulator_amd.ops import hip_engine as he
    if not he.device_available():
        pytest.fail("GPU test collected but no HIP device is visible")
    m = he.native()
    exp_x, log_x, pw = branch_edge_arguments()
    assert all(math.isfinite(x) for x in exp_x) and all(0 < x < math.inf for x in log_x)
    assert all(0 < x < math.inf and x != 1 and y != 0 and math.isfinite(y) for x, y in pw)

    def cpython(f, *a):
        try:
            return 0, f(*a)
        except OverflowError:
            return 1, None

    for fn, f, args in ((0, math.exp, [(x,) for x in exp_x]), (1, math.log, [(x,) for x in log_x]), (2, pow, pw)):
        x = [a[0] for a in args]
        y = [a[-1] for a in args]
        dst, dout, hst, hout = _device_and_host(m, fn, x, y)
        assert np.array_equal(dst, hst), fn
        assert np.array_equal(dout.view(np.uint64), hout.view(np.uint64)), fn
        for i, a in enumerate(args):
            st, want = cpython(f, *a)
            assert dst[i] == st, (fn, a, int(dst[i]), float(dout[i]))
            if st == 0:
                assert np.float64(want).view(np.uint64) == dout.view(np.uint64)[i], (fn, a, float(dout[i]), want)
        if fn != 1:   # the list reaches overflow, subnormal and zero results
            ok = dout[dst == 0]
            assert (dst == 1).any() and (ok == 0).any() and ((ok != 0) & (np.abs(ok) < 2.0 ** -1022)).any(), fn


def test_pow_heavy_program_native_equals_cpu_vm(default_workload):
    from funsearch_kubernetes_simulator_amd.ops import hip_engine as he
    dev = he.DeviceEvaluator(default_workload)
    from funsearch_kubernetes_simulator_amd.policy.template import PolicyTemplate
    body = PolicyTemplate.fill_template(
        "c = (node.cpu_milli_left / max(1, node.cpu_milli_total)) ** 1.37\n"
        "    m = math.exp(-node.memory_mib_left / max(1.0, node.memory_mib_total * 1.9))\n"
        "    g = math.log(1.0 + node.gpu_left + pod.cpu_milli / 997.0) ** 0.71\n"
        "    score = 1000 * (c + m) * g * 7.3 + math.pow(2.0, g) * 3.1")
    progs = [compile_policy(body.replace("1.37", str(1.37 + 0.013 * k))) for k in range(16)]
    nat = dev.evaluate_native(progs)
    vm = ce.simulate_program_batch(default_workload, progs, threads=16)
    assert (nat[:, 10] == 0).all(), nat[:, 10]          # nothing deferred: no EXC_UNSUPPORTED rows
    assert np.array_equal(nat, vm)
