"""Catalogue of inputs for the exact arithmetic under every device score.

Every engine's means come from a 128-bit fixed-point accumulator (96
fractional bits), a correctly rounded division of that word by the count, and
a finaliser that turns five means into a table row; the composite scorer and
the fragmentation sample divide through host-verified reciprocals.  Whole
replays only ever feed these ratios in [0, 1], counts of some 10^4 and no
rounding tie.  The cases here sit where such code goes wrong: carries between
the two words, band, grid and range edges, exact ties on both sides of the
64-bit quotient split, quotients below one unit, flagged inputs.

The references are plain Python (`fractions.Fraction`, `math`); nothing here
calls the code under test.  `tests/test_exact_arith_cases.py` holds the CPU
side (preconditions, the host twin, a Python model of the device routines with
seeded mutants) and `tests/test_gpu_exact_arith.py` runs the device on the
catalogue, bit for bit.

Four groups:

* (a) `acc_cases()`: sequences of doubles for the accumulators, with
  `acc_reference(seq, contract)` -> (sum * 2^96, count, inexact);
* (b) `div_cases()`: (label, A, n) for the division, with `div_reference`;
* (c) `finaliser_cases()`: accumulator states and replay counters, with
  `finaliser_row`;
* (d) `divisor_cases(layout)`: (d, hi, from_workload) for `div_by_recip`.
"""
import functools
import math
import random
from fractions import Fraction

F96 = 1 << 96
NEXT = math.nextafter

#: the `inexact` contracts, read from the code:
#: "lane"    LaneAcc::add (and the host twin fks::FixedAcc);
#: "row_add" RowAcc::add: the same, and any set sign bit flags;
#: "unit"    RowAcc::add_unit, and stash_unit + add_stash: only +0.0 and [2^-31, 2) pass
CONTRACTS = ("lane", "row_add", "unit")


# ---- (a) accumulator sequences -----------------------------------------------------------

def _sign_bit(v: float) -> bool:
    return math.copysign(1.0, v) < 0


def value_flags(v: float, contract: str) -> bool:
    """Whether adding `v` alone sets `inexact` (the value is then not added)."""
    if contract == "unit":
        return not ((v == 0.0 and not _sign_bit(v)) or 2.0 ** -31 <= v < 2.0)
    if not math.isfinite(v):
        return True
    if contract == "row_add" and _sign_bit(v):
        return True
    if v == 0.0:
        return False
    if abs(v) < 2.0 ** -1022 or abs(v) >= 2.0 ** 30:
        return True
    return (Fraction(v) * F96).denominator != 1


def acc_reference(seq, contract: str):
    """(exact sum of the accepted values * 2^96, count, inexact).  The sum is
    what the accumulator must hold whenever the flag is clear."""
    total, flag = 0, False
    for v in seq:
        if value_flags(v, contract):
            flag = True
            continue
        total += int(Fraction(v) * F96)
        if contract != "unit" and abs(total) >= (1 << 126):   # 2^30 of headroom, sticky
            flag = True
    return total, len(seq), flag


EDGE_VALUES = {
    # band edges of add_unit
    "2^-31": 2.0 ** -31, "below 2^-31": NEXT(2.0 ** -31, 0.0), "1": 1.0, "below 2": NEXT(2.0, 0.0), "2": 2.0,
    # grid edges
    "2^-96": 2.0 ** -96, "2^-97": 2.0 ** -97, "3*2^-96": 3 * 2.0 ** -96,
    "(2^53-1)*2^-96": (2.0 ** 53 - 1) * 2.0 ** -96, "(2^53-1)*2^-97": (2.0 ** 53 - 1) * 2.0 ** -97,
    # range edges
    "below 2^30": NEXT(2.0 ** 30, 0.0), "2^30": 2.0 ** 30,
    # never representable, or signed
    "5e-324": 5e-324, "2^-1022": 2.0 ** -1022, "inf": math.inf, "-inf": -math.inf, "nan": math.nan,
    "-1": -1.0, "-2^-96": -(2.0 ** -96), "-0.0": -0.0, "+0.0": 0.0,
}


@functools.lru_cache(maxsize=None)
def acc_cases():
    """name -> tuple of doubles.  Random k / T ratios first (in every
    contract), then each edge value alone and between two ordinary values,
    then headroom and cancellation sequences."""
    rng = random.Random(9601)
    out = {}
    lengths = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256] + [rng.randint(1, 256) for _ in range(70)]
    for i, n in enumerate(lengths):
        T = rng.choice([3, 7, 1000, 2 ** 31 - 1, rng.randint(1, 2 ** 31 - 1), rng.randint(1, 2 ** 31 - 1)])
        if i % 4 == 3:   # a divisor of its own per value
            seq = []
            for _ in range(n):
                t = rng.randint(1, 2 ** 31 - 1)
                seq.append(rng.randint(0, t) / t)
        elif i % 4 == 2:   # near 1: the low word overflows on about every other add
            seq = [rng.randint(T - T // 8, T) / T for _ in range(n)]
        else:
            seq = [rng.randint(0, T) / T for _ in range(n)]
        out[f"ratios{i:02d}_len{n}"] = tuple(seq)
    for n in (1, 3, 100, 256):
        out[f"thirds_len{n}"] = (1 / 3,) * n
    out["ones_len256"] = (1.0,) * 256
    out["empty"] = ()
    for name, v in EDGE_VALUES.items():
        out[f"edge[{name}]"] = (v,)
        out[f"edge[{name}] between"] = (0.75, v, 1 / 3)
    out["2^29 twice"] = (2.0 ** 29, 2.0 ** 29)
    out["2^29 + below 2^29"] = (2.0 ** 29, NEXT(2.0 ** 29, 0.0))
    out["below 2^30 + 2^-96"] = (NEXT(2.0 ** 30, 0.0), 2.0 ** -96)
    out["2^29 twice and back"] = (2.0 ** 29, 2.0 ** 29, -(2.0 ** 29))   # the flag is sticky
    out["-2^29 twice"] = (-(2.0 ** 29), -(2.0 ** 29))
    out["-2^29 - below 2^29"] = (-(2.0 ** 29), -NEXT(2.0 ** 29, 0.0))
    out["cancel to negative"] = (0.5, -0.75)
    out["cancel to zero"] = (0.375, 1 / 3, -0.375, -(1 / 3))
    out["cancel to -2^-96"] = (1 / 3, -(1 / 3), -(2.0 ** -96))
    out["borrow across the words"] = (2.0 ** -30, -(2.0 ** -96))   # 2^66 - 1: the low word borrows from the high
    for i in range(6):   # signed ratios
        T = rng.randint(1, 2 ** 31 - 1)
        out[f"signed{i}"] = tuple(rng.randint(-T, T) / T for _ in range(rng.randint(2, 200)))
    return out


def in_contract_share(contract: str) -> float:
    cases = acc_cases()
    return sum(not acc_reference(s, contract)[2] for s in cases.values()) / len(cases)


#: row programs: (op, accumulator, value) with the op names of `_fks_hip.TEST_ROW_OPS`
def stash_program(seq, salt: int = 0):
    """The row kernel's use of the fragmentation stash on `seq`: every value is
    stashed and added 1-3 times (a failure after a failure reuses the sample),
    the stash is dropped now and then, and accumulators 0-3 take snapshots in
    between.  Returns (ops, the sequence each accumulator 0-4 must hold)."""
    ops, held = [], [[], [], [], [], []]
    for i, v in enumerate(seq):
        ops.append(("stash_unit", 4, v))
        for _ in range(1 + (i + salt) % 3):
            ops.append(("add_stash", 4, 0.0))
            held[4].append(v)
        if (i + salt) % 2 == 0:
            ops.append(("stash_drop", 4, 0.0))
        if (i + salt) % 5 == 0:
            for k in range(4):
                u = (i + 1 + k) / (i + 7 + 2 * k)
                ops.append(("add_unit", k, u))
                held[k].append(u)
    return ops, held


# ---- (b) division -----------------------------------------------------------------------

DIV_N = (1, 2, 3, 7, 60, 9999, 2 ** 31 - 1, 2 ** 40 + 1, 2 ** 63 - 1)
TIE_SHIFTS = (0, 1, 10, 11, 12, 30, 60, 64, 70)   # the quotient (2m + 1) << s has 54 + s bits: 64 at s = 10


def div_reference(A: int, n: int) -> float:
    return float(Fraction(A, n << 96))


def div_branch(A: int, n: int) -> str:
    """Which way fixed_div_round takes the quotient to 64 bits."""
    q = abs(A) // n
    bits = q.bit_length()
    return "shift_right" if bits > 64 else "exact_64" if bits == 64 else "zero" if q == 0 else "shift_left"


@functools.lru_cache(maxsize=None)
def div_cases():
    """Tuple of (label, A, n), 0 < |A| < 2^126, 1 <= n < 2^63."""
    rng = random.Random(9602)
    out = []

    def add(label, A, n):
        if 0 < abs(A) < (1 << 126) and 1 <= n < (1 << 63):
            out.append((label, A, n))

    ms = [2 ** 52, 2 ** 52 + 1, 2 ** 53 - 2]
    ms += [rng.randrange(2 ** 52, 2 ** 53) & ~1 for _ in range(16)] + [rng.randrange(2 ** 52, 2 ** 53) | 1 for _ in range(17)]
    for s in TIE_SHIFTS:
        for n in DIV_N + (rng.randrange(1, 2 ** 8), rng.randrange(1, 2 ** 62)):
            for m in ms + [2 ** 53 - 1]:
                A = ((2 * m + 1) * n) << s
                if A >= (1 << 126) - 1:
                    continue
                kind = "carry" if m == 2 ** 53 - 1 else "tie_odd" if m & 1 else "tie_even"
                add(kind, A, n)
                add(kind + "_neg", -A, n)
                for d in (1, -1):   # off the tie by the remainder (or, n = 1, the last quotient bit) alone
                    add("tie_off", A + d, n)
                    add("tie_off_neg", -(A + d), n)
    for bits in (63, 64, 65):
        for n in DIV_N + tuple(rng.randrange(1, 2 ** 60) for _ in range(12)):
            for q in (1 << (bits - 1), (1 << bits) - 1, rng.getrandbits(bits - 1) | 1 << (bits - 1)):
                for r in {0, n - 1, rng.randrange(n)}:
                    add(f"q{bits}", q * n + r, n)
    add("below_one", 1, 2 ** 40)
    add("below_one", 1, 2 ** 63 - 1)
    add("below_one", -1, 2 ** 63 - 1)
    for n in DIV_N[1:] + tuple(rng.randrange(2, 2 ** 63) for _ in range(40)):
        add("below_one", n - 1, n)
        add("below_one", rng.randrange(1, n), n)
        add("below_one", -rng.randrange(1, n), n)
        add("below_one", (n + 1) // 2, n)
    for n in DIV_N:   # the means of a replay: ratios summed over n snapshots
        for _ in range(20):
            add("n_list", rng.randrange(1, min(n, 2 ** 29) * F96 + 1), n)
            add("n_list", rng.getrandbits(rng.randint(1, 125)) + 1, n)
    for _ in range(5000):
        A = rng.getrandbits(rng.randint(1, 126)) or 1
        add("random", -A if rng.random() < 0.3 else A, rng.getrandbits(rng.randint(1, 63)) or 1)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def div_references():
    return tuple(div_reference(A, n) for _, A, n in div_cases())


# ---- (c) finaliser rows -------------------------------------------------------------------

def mean_reference(total: int, count: int) -> float:
    return float(Fraction(total, count << 96)) if count > 0 else 0.0


def state_of(seq, contract: str = "unit"):
    return acc_reference(seq, contract)


def _const_state(v: float, count: int):
    """`count` adds of the on-grid double v."""
    return int(Fraction(v) * F96) * count, count, False


@functools.lru_cache(maxsize=None)
def finaliser_cases():
    """name -> dict(states = five (sum * 2^96, count, inexact), n_events,
    n_unplaced, exc, hash).  The counts of accumulators 0-3 are one number (the
    snapshots), as in every replay."""
    rng = random.Random(9603)

    def util(n, lo=0.2, hi=0.9):
        T = rng.randint(1000, 2 ** 31 - 1)
        return state_of([rng.randint(int(lo * T), int(hi * T)) / T for _ in range(n)])

    def case(states, n_events=12345, n_unplaced=0, exc=0, hsh=0x0123456789ABCDEF):
        return dict(states=tuple(states), n_events=n_events, n_unplaced=n_unplaced, exc=exc, hash=hsh)

    zero = (0, 0, False)
    out = {
        "plain": case([util(20), util(20), util(20), util(20), util(7, 0.0, 0.3)]),
        "no snapshots": case([zero, zero, zero, zero, util(3, 0.0, 0.3)]),
        "nothing at all": case([zero] * 5, n_events=0),
        "no fragmentation events": case([util(9), util(9), util(9), util(9), zero]),
        "unplaced pods": case([util(20), util(20), util(20), util(20), util(7, 0.0, 0.3)], n_unplaced=3),
        "exception": case([util(20), util(20), util(20), util(20), util(7, 0.0, 0.3)], exc=6),
        "exception, unsupported": case([util(4), util(4), util(4), util(4), zero], exc=100, n_unplaced=2),
        "frag below 0.1": case([util(5), util(5), util(5), util(5), _const_state(NEXT(0.1, 0.0), 3)]),
        "frag at 0.1": case([util(5), util(5), util(5), util(5), _const_state(0.1, 3)]),
        "frag above 0.1": case([util(5), util(5), util(5), util(5), _const_state(NEXT(0.1, 1.0), 3)]),
        "frag 0.25": case([util(5), util(5), util(5), util(5), _const_state(0.25, 11)]),
        "clamped to 0": case([util(6, 0.0, 0.02), util(6, 0.0, 0.02), util(6, 0.0, 0.02), util(6, 0.0, 0.02),
                              _const_state(0.5, 2)]),
        "means above 1": case([state_of([1.5, 1.25, 1.75], "row_add"), state_of([1.0, 1.5, 1.0], "row_add"),
                               state_of([1.25] * 3, "row_add"), state_of([1.0, 1.0, 1.75], "row_add"),
                               _const_state(0.0625, 4)]),
        "means of exactly 1": case([_const_state(1.0, 40)] * 4 + [zero]),
        "thirds": case([state_of([1 / 3] * 3)] * 4 + [state_of([1 / 3] * 7)]),
        "flagged utilisation": case([util(8), (util(8)[0], 8, True), util(8), util(8), util(2, 0.0, 0.3)]),
        "flagged fragmentation": case([util(8), util(8), util(8), util(8), (util(2, 0.0, 0.3)[0], 2, True)]),
        "hash with the top bits set": case([util(3), util(3), util(3), util(3), zero], hsh=0xFEDCBA9876543210),
        "hash of all ones": case([util(3), util(3), util(3), util(3), zero], hsh=2 ** 64 - 1),
        "mean below 2^-32": case([(1, 5, False), (F96 >> 40, 5, False), (3, 5, False), (F96 >> 33, 5, False),
                                  (7, 9999, False)]),
        "tie in a mean": case([(((2 * (2 ** 52 + 1) + 1) * 3) << 30, 3, False)] * 2 +
                              [(((2 * (2 ** 52 + 2) + 1) * 3) << 30, 3, False)] * 2 + [_const_state(0.03125, 1)]),
    }
    for i in range(7):   # random replays
        n, f = rng.randint(1, 400), rng.randint(0, 50)
        out[f"random{i}"] = case([util(n, 0.0, 1.0) for _ in range(4)] + [util(f, 0.0, 0.4) if f else zero],
                                 n_events=rng.randint(1, 10 ** 6), n_unplaced=rng.choice([0, 0, 0, 5]),
                                 hsh=rng.getrandbits(64))
    return out


def finaliser_row(c) -> list:
    """The 13 columns k_eval_reduce writes for a finished replay: score, five
    means, n_snap, n_frag, n_events, n_unplaced, exc, inexact, hash >> 11; an
    aborted replay (exc != 0) reports only its exception class."""
    if c["exc"] != 0:
        return [0.0] * 10 + [float(c["exc"])] + [0.0] * 2
    st = c["states"]
    n_snap, n_frag = st[0][1], st[4][1]
    avg = [mean_reference(st[k][0], n_snap if k < 4 else n_frag) for k in range(5)]
    score = 0.0
    if n_snap > 0 and c["n_unplaced"] == 0:   # combine_policy_score
        overall = (avg[0] + avg[1] + avg[2] + avg[3]) / 4.0
        penalty = min(0.1, avg[4])
        score = max(0.0, min(1.0, overall - penalty))
    return [score] + avg + [float(n_snap), float(n_frag), float(c["n_events"]), float(c["n_unplaced"]), 0.0,
                            float(any(s[2] for s in st)), float(c["hash"] >> 11)]


# ---- (d) divisors of div_by_recip ---------------------------------------------------------

GMAX = 8


def divisor_cases(layout):
    """(d, hi, from_workload) from `prepare_device_workload`'s layout of the
    default workload -- every reciprocal its upload verifies, over the numerators
    it verifies them on -- and the hand cases."""
    out = []

    def add(d, hi, wl):
        if (d, hi, wl) not in out:
            out.append((int(d), int(hi), wl))

    for key in ("cpu_total", "mem_total"):
        for t in sorted(set(int(x) for x in layout[key])):
            add(max(t, 1), t, True)
    for g in sorted(set(int(x) for x in layout["ngpus"])):
        add(max(g, 1), GMAX, True)
    n = layout["n_nodes"]
    caps = set(int(layout["gml_total"][i, 0]) for i in range(n) if layout["ngpus"][i] > 0)
    assert len(caps) == 1, "the default cluster has one per-GPU milli total"
    cap = caps.pop()
    for k in range(1, GMAX + 1):
        add(k * cap, GMAX * cap, True)
    tot = int(layout["tot_gmilli"])
    assert 0 < tot <= 2 ** 24, "the default workload's fragmentation divisor takes the reciprocal"
    add(tot, tot, True)
    add(1000, 2 ** 21 - 1, True)
    add(2 ** 24 - 3, 2 ** 24 - 3, False)
    add(3, 8, False)
    add(7, 8, False)
    return out
