"""Inputs of the star-by-star diagnostics tests (tests/test_gpu_metrics_stars.py) and the CPU checks of their
preconditions (tests/test_oracle_golden.py).

Lattice inputs: positions are multiples of 1/step in [-16, 16], masses multiples of 1/4 in [0.25, 2].  Every product
x * m is then a multiple of 1/(4 step) below 32 and every partial sum of n of them, in any order, is a multiple of that
unit below 32 n: exact in float32 while 32 n * 4 step <= 2^24 (step = 8: n <= 16 384; step = 2: n <= 65 536 -- the
larger case below is checked by value, not by this bound), exact in float64 far beyond.  The sums behind the centre of
mass and the enclosed masses then do not depend on the order in which a kernel adds them, and the reference value of
every per-star quantity is one fixed number.
"""
import numpy as np

from oracle import metrics_oracle as MO

SCAN_EB = 1024                     # sorted positions per block of the native enclosed-mass scan
PREP_SPAN = 256 * 256              # stars covered by one trip of the native per-star pass
BIG_N = PREP_SPAN + 300
SMALL_NS = (1, 2, 255, 256, 257, 1023, 1024, 1025, 2049)
LATTICE_CASES = [(n, d) for n in SMALL_NS + (BIG_N,) for d in (2, 3)]
RANDOM_N = 2049


def lattice_step(n):
    return 8 if n <= 2049 else 2


def lattice(n, dim, dtype, seed=0):
    """(positions, masses): lattice points drawn with repetition, unequal masses."""
    rng = np.random.default_rng(1000 * dim + n + seed)
    step = lattice_step(n)
    pos = (rng.integers(-16 * step, 16 * step + 1, size=(n, dim)) / step).astype(dtype)
    mass = (rng.integers(1, 9, size=n) / 4.0).astype(dtype)
    return pos, mass


def sums_round_trip_through_float32(pos, mass):
    """The precondition of exactness: sum |x m| per column and sum m, in float64, are float32 numbers."""
    p, m = pos.astype(np.float64), mass.astype(np.float64)
    s = np.concatenate([np.abs(p * m[:, None]).sum(axis=0), [m.sum()]])
    return bool(np.all(s.astype(np.float32).astype(np.float64) == s))


def _tree_scan(a):
    """Inclusive prefix sums with pairwise association (neighbours first, then pairs of pairs, ...)."""
    if a.shape[0] == 1:
        return a.copy()
    half = a.shape[0] // 2
    s = _tree_scan(a[0:2 * half:2] + a[1:2 * half:2])
    out = np.empty_like(a)
    out[0] = a[0]
    out[1::2] = s
    rest = out[2::2].shape[0]
    out[2::2] = s[:rest] + a[2::2]
    return out


def _blocks_reversed_scan(a):
    """Inclusive prefix sums: blocks of SCAN_EB in order, each prefix inside a block added from its own element
    back to the block's first."""
    out = np.empty_like(a)
    run = 0.0
    for b0 in range(0, a.shape[0], SCAN_EB):
        blk = a[b0:b0 + SCAN_EB]
        for k in range(blk.shape[0]):
            out[b0 + k] = run + np.cumsum(blk[k::-1])[-1]
        run = run + np.cumsum(blk[::-1])[-1]
    return out


def enclosed_three_ways(pos, mass):
    """The oracle's enclosed masses (in star order) under sequential, reversed-within-blocks and pairwise float64
    accumulation, each rounded once to the input dtype."""
    order = MO.stable_order(MO.com_radii(pos, mass))
    ms = mass[order].astype(np.float64)
    outs = []
    for scan in (np.cumsum, _blocks_reversed_scan, _tree_scan):
        e = np.empty_like(mass)
        e[order] = scan(ms).astype(mass.dtype)
        outs.append(e)
    return outs


def com_three_ways(pos, mass):
    """The oracle's centre of mass with its float64 sums taken sequentially, reversed within blocks, and pairwise."""
    dt = pos.dtype
    xm = (pos * mass[:, None]).astype(np.float64)
    cols = np.concatenate([xm, mass.astype(np.float64)[:, None]], axis=1)
    outs = []
    for scan in (np.cumsum, _blocks_reversed_scan, _tree_scan):
        tot = np.array([scan(np.ascontiguousarray(cols[:, k]))[-1] for k in range(cols.shape[1])]).astype(dt)
        outs.append((tot[:-1] / tot[-1]).astype(dt))
    return outs


def order_independent(pos, mass):
    e = enclosed_three_ways(pos, mass)
    c = com_three_ways(pos, mass)
    want_e, want_c = MO.enclosed_masses(pos, mass), MO.centre_of_mass(pos, mass)
    return (all(np.array_equal(x, want_e) for x in e) and all(np.array_equal(x, want_c) for x in c))


def random_mass_inputs(seed):
    rng = np.random.default_rng(seed)
    pos = (rng.standard_normal((RANDOM_N, 2)) * 3).astype(np.float32)
    mass = (0.5 + rng.random(RANDOM_N)).astype(np.float32)
    return pos, mass


_random_case = []


def random_mass_case():
    """The first seed <= 20 whose float32 enclosed masses and centre of mass come out the same under all three
    accumulation orders, with its inputs; (None, ...) if there is none.  A weak filter: float64 sums in different
    orders differ by about 1e-13 before their one rounding to float32, so only a value within that of a rounding
    boundary fails it and seed 0 is expected to pass."""
    if not _random_case:
        for seed in range(21):
            pos, mass = random_mass_inputs(seed)
            if order_independent(pos, mass):
                _random_case.append((seed, pos, mass))
                break
        else:
            _random_case.append((None,) + random_mass_inputs(0))
    return _random_case[0]
