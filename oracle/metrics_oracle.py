"""CPU restatement of the reference's galaxy diagnostics (metrics.py:25-156) in numpy.

TEST INFRASTRUCTURE ONLY (see nbody_oracle.c header): the checker for the native `nb_metrics` kernels; pinned
against the reference's own outputs in tests/golden/g6_galaxy_metrics.npz and g12_metric_flow.npz and, star by star,
against torch's CPU ops of the reference formulas (tests/test_oracle_golden.py).  Arithmetic is done in the dtype of
the inputs, op by op like the torch code.

Per-star functions first (one statement of each formula); the aggregates of the reference's four functions are built on
them.  Sums whose order torch does not fix (the masses, the mass-weighted positions, the bin means, the dispersion)
are accumulated in float64 and rounded once to the input dtype.
"""
import numpy as np


# --------------------------------------------------------------------------------------------- per star
def _norm(x):
    """sqrt(x0*x0 + x1*x1 [+ x2*x2]) in x's dtype, the squares added left to right."""
    s = x[:, 0] * x[:, 0]
    for k in range(1, x.shape[1]):
        s = s + x[:, k] * x[:, k]
    return np.sqrt(s)


def radii(positions):
    """r_i = |x_i| over all columns                                                       metrics.py:48 / :92"""
    with np.errstate(invalid="ignore", over="ignore"):
        return _norm(positions)


def speeds(velocities):
    """vm_i = |v_i|                                                                       metrics.py:140 / :155"""
    with np.errstate(invalid="ignore", over="ignore"):
        return _norm(velocities)


def tangential_speeds(positions, velocities):
    """vt_i = |x0 v1 - x1 v0| / clamp(r, min=0.1); a NaN radius stays NaN                 metrics.py:55-57"""
    dt = positions.dtype
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        cr = np.abs(positions[:, 0] * velocities[:, 1] - positions[:, 1] * velocities[:, 0])
        return (cr / np.maximum(radii(positions), dt.type(0.1))).astype(dt)


def centre_of_mass(positions, masses):
    """sum_i (x_i m_i) / sum_i m_i: products and the quotient in the input dtype          metrics.py:120-121"""
    dt = positions.dtype
    with np.errstate(invalid="ignore", over="ignore"):
        total = masses.sum(dtype=np.float64).astype(dt)
        return ((positions * masses[:, None]).sum(axis=0, dtype=np.float64).astype(dt) / total).astype(dt)


def com_radii(positions, masses):
    """r_com_i = |x_i - com|                                                              metrics.py:124"""
    with np.errstate(invalid="ignore", over="ignore"):
        return _norm(positions - centre_of_mass(positions, masses))


def stable_order(keys):
    """Indices that sort `keys` ascending, ties in index order, NaN last (torch.sort / argsort on ties: the native
    sort and this one both keep index order)."""
    return np.argsort(keys, kind="stable")


def enclosed_masses(positions, masses):
    """Mass inside r_com_i, own mass included: cumsum in r_com order mapped back          metrics.py:128-134"""
    order = stable_order(com_radii(positions, masses))
    enclosed = np.empty_like(masses)
    enclosed[order] = np.cumsum(masses[order].astype(np.float64)).astype(masses.dtype)
    return enclosed


def escape_speeds(positions, masses, G=0.001):
    """vesc_i = sqrt(2 G M_enc_i / clamp(r_com_i, min=0.1)); 2 G enters as a scalar of the input dtype  metrics.py:137"""
    dt = positions.dtype
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        rc = com_radii(positions, masses)
        return np.sqrt(dt.type(2 * G) * enclosed_masses(positions, masses) / np.maximum(rc, dt.type(0.1))).astype(dt)


def bound_flags(positions, velocities, masses, G=0.001):
    """|v_i| < vesc_i                                                                     metrics.py:143"""
    with np.errstate(invalid="ignore"):
        return speeds(velocities) < escape_speeds(positions, masses, G)


def bin_indices(r, edges):
    """Bin b with edge_b <= r < edge_b+1, or -1 (outside, NaN): the float32 edges compared in r's dtype  metrics.py:65"""
    e = np.asarray(edges, np.float32).astype(r.dtype)
    out = np.full(r.shape[0], -1, np.int64)
    with np.errstate(invalid="ignore"):
        for b in range(e.shape[0] - 1):
            out[(r >= e[b]) & (r < e[b + 1])] = b
    return out


def percentile_rank(n, percentile):
    """min(int(n * percentile / 100), n - 1)                                              metrics.py:93-95"""
    return min(int(n * percentile / 100), n - 1)


# --------------------------------------------------------------------------------------------- aggregates
def linspace_f32(max_radius, num_bins):
    """torch.linspace(0, max_radius, num_bins + 1) (float32, ATen's symmetric formulation: step * i below the middle,
    end - step * (steps - 1 - i) from it on).  The latter is taken as one fused multiply-subtract (the float64 product
    of two float32 numbers is exact, so rounding the float64 difference once is that fma): an empirical match of what
    torch's CPU build returns -- contraction by its compiler, not a promise of ATen's source -- held by
    tests/test_oracle_golden.py against torch.linspace itself."""
    steps = num_bins + 1
    end = np.float32(max_radius)
    step = end / np.float32(steps - 1)
    i = np.arange(steps)
    lo = (step * i.astype(np.float32)).astype(np.float32)
    hi = (np.float64(end) - np.float64(step) * (steps - 1 - i).astype(np.float64)).astype(np.float32)
    return np.where(i < steps // 2, lo, hi).astype(np.float32)


def rotation_curve(positions, velocities, num_bins=20, max_radius=None, edges=None):
    """metrics.py:25-78: per-bin masked means, NaN for empty bins."""
    r = radii(positions)
    if max_radius is None:
        max_radius = float(r.max()) if not np.isnan(r).any() else float("nan")
    dt = positions.dtype
    vt = tangential_speeds(positions, velocities)
    e = linspace_f32(max_radius, num_bins) if edges is None else np.asarray(edges, np.float32)
    which = bin_indices(r, e)
    means, counts = [], []
    for b in range(num_bins):
        mask = which == b
        counts.append(int(mask.sum()))
        with np.errstate(invalid="ignore"):
            means.append(float(vt[mask].astype(np.float64).mean().astype(dt)) if mask.any() else float("nan"))
    centres = ((e[:-1] + e[1:]) / np.float32(2)).astype(np.float32)
    return {"radii": centres, "velocities": np.array(means), "num_stars_per_bin": counts, "edges": e}


def galaxy_radius(positions, percentile=90):
    """metrics.py:81-95"""
    r = radii(positions)
    return float(np.sort(r)[percentile_rank(len(r), percentile)])


def bound_fraction(positions, velocities, masses, G=0.001):
    """metrics.py:98-145 (ties in r_com broken by index)"""
    flags = bound_flags(positions, velocities, masses, G)
    return float(np.float32(flags.sum()) / np.float32(len(masses)))


def velocity_dispersion(velocities):
    """metrics.py:148-156 (unbiased)"""
    with np.errstate(invalid="ignore"):
        return float(speeds(velocities).astype(np.float64).std(ddof=1).astype(velocities.dtype))
