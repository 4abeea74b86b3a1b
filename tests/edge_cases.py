"""Edge-value inputs for the pair kernels and the comparison that goes with them (no GPU needed to import).

make()     the clustered-core-plus-halo cloud of test_gpu_plan_shapes.inputs with one kind of edge value written in:
             nan-coord            coordinate 0 of one star is NaN
             inf-coord            coordinate D - 1 of one star is -inf
             runaway              coordinate 0 of one star is BIG: r2 overflows, the coordinate itself is finite
             runaway-pair         stars 10 and n - 1 at +BIG and -BIG
             runaway-same-side    stars 10 and n - 1 at +BIG and +BIG / 4: both beyond every staging limit on the same side,
                                  r2 between them overflows as well (two such stars must not land on one staged value)
             nearly               one star at NEARLY: r2 is still finite, r^3 is not
             massless             three stars of mass 0, all other masses distinct
             massless-else-equal  three stars of mass 0, all others equal
             all-massless         every mass 0
             nan-mass             one mass NaN
           BIG / NEARLY are 3e19 / 1e19 for fp32-typed state and 1e160 / 1e153 for fp64.  Edge stars sit at
           edge_indices(n) = (10, n // 2 + 3, n - 1): the first tile, a middle tile, the last real lane of the padded last
           tile; variants() lists the index choices a kind is run with.
compare()  classes first (NaN / +inf / -inf / finite must equal the oracle's), then the max-norm relative error over the
           elements finite in both, and a count of what was left out, so that a comparison cannot pass by skipping.
"""
import numpy as np

from test_gpu_plan_shapes import inputs

KINDS = ("nan-coord", "inf-coord", "runaway", "runaway-pair", "runaway-same-side", "nearly", "massless", "massless-else-equal",
         "all-massless", "nan-mass")
# run with distinct AND with equal masses
COORD_KINDS = ("nan-coord", "inf-coord", "runaway", "runaway-pair", "runaway-same-side", "nearly")
ONE_STAR_KINDS = ("nan-coord", "inf-coord", "runaway", "nearly", "nan-mass")      # edit one star: once per edge index
RUNAWAY_KINDS = ("runaway", "runaway-pair", "runaway-same-side")                  # r2 overflows: the star is decoupled
# a finite coordinate dwarfs the array maximum: the other stars are compared on their own as well
FAR_KINDS = RUNAWAY_KINDS + ("nearly",)

FINITE, NAN, PINF, NINF = 0, 1, 2, 3


def edge_indices(n):
    return (10, n // 2 + 3, n - 1)


def big(f64, nearly=False):
    if nearly:
        return 1e153 if f64 else 1e19
    return 1e160 if f64 else 3e19


def variants(kind, n, every_index=True):
    """The edge-star choices of a kind: one entry per edge index for the one-star kinds (only n - 1 without
    every_index), a single None for the kinds that place their own set of stars."""
    if kind in ONE_STAR_KINDS:
        return list(edge_indices(n)) if every_index else [n - 1]
    return [None]


def make(kind, n, dim, seed, f64, idx=None, uniform=False):
    """(pos, vel, mass, stars): the inputs of one case and the indices of the stars that carry the edge value.
    Velocities are of order 0.1.  uniform: equal masses (0.7) where the kind does not set them itself."""
    assert kind in KINDS, kind
    assert (idx is not None) == (kind in ONE_STAR_KINDS), (kind, idx)
    pos, vel, mass = inputs(n, dim, seed, f64, uniform or kind in ("massless-else-equal", "all-massless"))
    vel = (vel * 2).astype(vel.dtype)
    e = edge_indices(n)
    assert len(set(e)) == 3 and min(e) >= 0, f"n = {n} is too small for three distinct edge stars"
    if kind == "nan-coord":
        pos[idx, 0] = np.nan
        stars = (idx,)
    elif kind == "inf-coord":
        pos[idx, dim - 1] = -np.inf
        stars = (idx,)
    elif kind in ("runaway", "nearly"):
        pos[idx, 0] = big(f64, kind == "nearly")
        stars = (idx,)
    elif kind == "runaway-pair":
        pos[e[0], 0] = big(f64)
        pos[e[2], 0] = -big(f64)
        stars = (e[0], e[2])
    elif kind == "runaway-same-side":
        pos[e[0], 0] = big(f64)
        pos[e[2], 0] = big(f64) / 4
        stars = (e[0], e[2])
    elif kind in ("massless", "massless-else-equal"):
        mass[list(e)] = 0
        stars = e
    elif kind == "all-massless":
        mass[:] = 0
        stars = tuple(range(n))
    else:
        mass[idx] = np.nan
        stars = (idx,)
    assert np.isfinite(pos.dtype.type(big(f64)))      # BIG itself is finite in the state's dtype
    return pos, vel, mass, stars


def classes(a):
    a = np.asarray(a, np.float64)
    c = np.full(a.shape, FINITE, np.int8)
    c[np.isnan(a)] = NAN
    c[a == np.inf] = PINF
    c[a == -np.inf] = NINF
    return c


def compare(got, ref, bar, kind, what="", from_forces=False):
    """`got` (the engine) against `ref` (the oracle); returns the relative error it asserted.
    from_forces: the array is a force, or state integrated from forces -- the only place where kind inf-coord lets the
    engine hold NaN where the oracle is finite (a non-finite coordinate makes every force NaN)."""
    g = np.atleast_1d(np.asarray(got, np.float64))
    r = np.atleast_1d(np.asarray(ref, np.float64))
    assert g.shape == r.shape, (what, g.shape, r.shape)
    cg, cr = classes(g), classes(r)
    allowed = np.zeros(g.shape, bool)
    if kind == "inf-coord" and from_forces:
        allowed = (cg == NAN) & (cr == FINITE)
    wrong = (cg != cr) & ~allowed
    if wrong.any():
        at = tuple(int(v) for v in np.argwhere(wrong)[0])
        raise AssertionError(f"{what} [{kind}]: {int(wrong.sum())} elements of another class than the oracle's, "
                             f"first at {at}: got {g[at]!r}, oracle {r[at]!r}")
    both = (cg == FINITE) & (cr == FINITE)
    left_out = g.size - int(both.sum())
    expected_out = int((cr != FINITE).sum()) + int(allowed.sum())
    assert left_out == expected_out, \
        f"{what} [{kind}]: {left_out} elements left out of the comparison, {expected_out} accounted for"
    err = 0.0
    if both.any():
        err = float(np.abs(g[both] - r[both]).max() / max(np.abs(r[both]).max(), 1e-300))
    assert err < bar, f"{what} [{kind}]: relative error {err:.3e}, bar {bar:.1e}"
    return err
