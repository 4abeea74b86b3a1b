#!/usr/bin/env python3
"""Generator of g22_crash_points.npz: the reference's own detect_crash (crash_point_test.py:46-139) on a table of hand-built
tiny states.  Run by hand where the reference is available (like make_golden.py), never by the suite:

    python tests/golden/make_crash_golden.py <directory of the reference>      (or REFERENCE_DIR in the environment)

Every row holds the inputs -- N <= 4 stars, D = 2 or 3, float32 or float64: positions, velocities, previous positions, the
two energies and dt -- and what detect_crash returned: the code of its crash_type (0 .. 6, the order of
ensemble.CRASH_TYPES; 0: it returned None), its value and its severity.  The table covers every kind, every precedence pair
of neighbouring kinds and some further ones, both halves of the teleport `and`, both sides of the energy ratio with
prev_energy 0.0, -0.0, NaN and tiny, a maximum that sits in a negative component, -0.0 and subnormal values, and a
displacement whose float32 square overflows while no state value is infinite.  Rows at a threshold are built from exactly
representable roots (a speed of exactly 100 from (60, 80)).

For every row the generator asserts that torch's measures (the expressions of detect_crash) equal the numpy restatement of
ensemble.py's contract bit for bit: torch's CPU sqrt is not correctly rounded for every input, and a row where it differs
from numpy's would pin the tests to torch's rounding.  Such a row is to be replaced by hand, not kept.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_DIR")
if not REFERENCE:
    sys.exit(__doc__)
sys.path.insert(0, REFERENCE)
from crash_point_test import detect_crash          # noqa: E402

TYPES = ("", "NaN_EXPLOSION", "INFINITY_OVERFLOW", "TELEPORTATION", "VELOCITY_OVERFLOW", "ENERGY_SINGULARITY",
         "GALAXY_EXPLOSION")
NAN, INF = float("nan"), float("inf")
MAXN = 4
ROWS = []


def quiet(d):
    """A state that trips nothing, with exact roots: 3 stars, largest displacement 5 / 4096, speed 0.625, radius 10 / 13."""
    pos = [[3.0, 4.0, 12.0], [-6.0, 8.0, 0.0], [0.75, -1.0, 0.0]]
    vel = [[0.375, -0.5, 0.0], [0.125, 0.0, 0.0], [-0.25, 0.125, 0.5]]
    pos, vel = np.array(pos)[:, :d], np.array(vel)[:, :d]
    return pos, vel, pos - still(pos)


def still(pos):
    """What a row's positions moved by when it does not say: the first star by (3, 4) / 4096."""
    delta = np.zeros_like(pos)
    delta[0, :2] = (3.0 / 4096, 4.0 / 4096)
    return delta


def row(note, dtype, d, pos=None, vel=None, prev=None, energy=-1.0, prev_energy=-1.0, dt=0.01, edit=None):
    """One row from the quiet state of (dtype, d) with the given arrays replaced; edit(pos, vel, prev) changes single
    entries in place."""
    p, v, q = quiet(d)
    p = p if pos is None else np.array(pos, np.float64)
    v = v if vel is None else np.array(vel, np.float64)
    q = (p - still(p) if pos is not None else q) if prev is None else np.array(prev, np.float64)
    p, v, q = (np.array(a, np.float64) for a in (p, v, q))
    if edit:
        edit(p, v, q)
    assert p.shape == v.shape == q.shape and p.shape[1] == d and 1 <= p.shape[0] <= MAXN, note
    ROWS.append(dict(note=note, dtype=dtype, d=d, pos=p, vel=v, prev=q, energy=energy, prev_energy=prev_energy, dt=dt))


def both(note, d=None, **kw):
    """The row in float32 and float64 (and in D = 2 and 3 unless d is given)."""
    for dtype in ("float32", "float64"):
        for dd in ((2, 3) if d is None else (d,)):
            row(f"{note} [{dtype}, D={dd}]", dtype, dd, **kw)


def put(which, i, c, x):
    def edit(p, v, q):
        (p, v, q)[which][i, c] = x
    return edit


def chain(*edits):
    def edit(p, v, q):
        for e in edits:
            e(p, v, q)
    return edit


P, V, Q = 0, 1, 2
# ---- none
both("quiet")
both("quiet, a -0.0 and a subnormal", edit=chain(put(P, 2, 1, -0.0), put(Q, 2, 1, -0.0), put(V, 1, 1, 1e-45), put(V, 2, 0, -0.0)))
# ---- NaN, Inf and their precedence
both("NaN in the last position component", edit=lambda p, v, q: p.__setitem__((-1, -1), NAN))
both("NaN in one velocity", d=2, edit=put(V, 0, 1, NAN))
both("Inf in one position", d=3, edit=put(P, 1, 0, INF))
both("-Inf in one velocity, no NaN", d=2, edit=put(V, 2, 1, -INF))
both("NaN with Inf: NaN", d=2, edit=chain(put(V, 0, 0, INF), put(P, 2, 1, NAN)))
both("NaN with a teleport, an over-speed star, an energy jump and a huge radius: NaN", d=3,
     pos=[[3000.0, 0.0, 0.0], [NAN, 1.0, 1.0]], vel=[[300.0, 0.0, 0.0], [0.0, 0.0, 0.0]], prev=[[0.0, 0.0, 0.0], [0.0, 1.0, 1.0]],
     energy=-500.0)
both("Inf with a teleport: Inf", d=2, pos=[[5.0, 0.0], [INF, 1.0]], vel=[[0.125, 0.0], [0.0, 0.0]], prev=[[0.0, 0.0], [0.0, 1.0]])
both("Inf with an over-speed star and an energy jump: Inf", d=2, vel=[[300.0, 0.0], [-INF, 0.0], [0.0, 0.0]], energy=-500.0)
both("Inf with a huge radius: Inf", d=3, edit=chain(put(P, 1, 0, INF), put(P, 0, 2, 5000.0), put(Q, 0, 2, 5000.0)))
# ---- teleport: max_displacement >max_abs_velocity * dt * 10 and max_displacement > 1.0
for dtype in ("float32", "float64"):
    row(f"teleport: displacement 5 from (3, 4) [{dtype}, D=2]", dtype, 2, pos=[[3.0, 4.0], [-6.0, 8.0]],
        prev=[[0.0, 0.0], [-6.0, 8.0]], vel=[[0.25, 0.0], [0.0, -0.125]])
    row(f"teleport: displacement 7 from (2, 3, 6), in the last star [{dtype}, D=3]", dtype, 3,
        pos=[[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [2.0, 3.0, 6.0]], prev=[[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]],
        vel=[[0.25, 0.0, 0.0], [0.0, -0.125, 0.0], [0.0, 0.0, 0.0]])
    row(f"teleport, first half only: displacement 0.5 above the expected maximum, not above 1 [{dtype}, D=2]", dtype, 2,
        pos=[[0.5, 0.0], [-6.0, 8.0]], prev=[[0.0, 0.0], [-6.0, 8.0]], vel=[[0.25, 0.0], [0.0, -0.125]])
    row(f"teleport, first half only: displacement exactly 1 [{dtype}, D=2]", dtype, 2,
        pos=[[0.0, 1.0], [-6.0, 8.0]], prev=[[0.0, 0.0], [-6.0, 8.0]], vel=[[0.25, 0.0], [0.0, -0.125]])
    row(f"teleport, second half only: displacement 5 below the expected maximum 10 [{dtype}, D=2]", dtype, 2,
        pos=[[3.0, 4.0], [-6.0, 8.0]], prev=[[0.0, 0.0], [-6.0, 8.0]], vel=[[2.0, 0.0], [0.0, -0.125]], dt=0.5)
    row(f"teleport, second half only: displacement 5 equal to the expected maximum [{dtype}, D=2]", dtype, 2,
        pos=[[3.0, 4.0], [-6.0, 8.0]], prev=[[0.0, 0.0], [-6.0, 8.0]], vel=[[1.0, 0.0], [0.0, -0.125]], dt=0.5)
    row(f"no teleport because the largest |v| is a negative component: 3 against 40 * 0.01 * 10 [{dtype}, D=2]", dtype, 2,
        pos=[[3.0, 0.0], [-6.0, 8.0]], prev=[[0.0, 0.0], [-6.0, 8.0]], vel=[[1.0, 0.5], [-40.0, 1.0]])
    row(f"teleport with an over-speed star and a small dt: teleport [{dtype}, D=2]", dtype, 2,
        pos=[[3.0, 4.0], [-6.0, 8.0]], prev=[[0.0, 0.0], [-6.0, 8.0]], vel=[[200.0, 0.0], [0.0, -0.125]], dt=0.0001)
    row(f"displacement 5 with an over-speed star and dt 0.01: the expected maximum is 20, velocity [{dtype}, D=2]", dtype, 2,
        pos=[[3.0, 4.0], [-6.0, 8.0]], prev=[[0.0, 0.0], [-6.0, 8.0]], vel=[[200.0, 0.0], [0.0, -0.125]])
    row(f"teleport with an energy jump and a huge radius: teleport [{dtype}, D=3]", dtype, 3,
        pos=[[2000.0, 0.0, 0.0], [1.0, 1.0, 1.0]], prev=[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]],
        vel=[[0.25, 0.0, 0.0], [0.0, -0.125, 0.0]], energy=-500.0)
    row(f"displacement 3e19: its float32 square is inf, no state value is [{dtype}, D=2]", dtype, 2,
        pos=[[3e19, 0.0], [-6.0, 8.0]], prev=[[0.0, 0.0], [-6.0, 8.0]], vel=[[0.25, 0.0], [0.0, -0.125]])
    row(f"teleport of more than 100: severity capped [{dtype}, D=2]", dtype, 2,
        pos=[[300.0, 400.0], [-6.0, 8.0]], prev=[[0.0, 0.0], [-6.0, 8.0]], vel=[[0.25, 0.0], [0.0, -0.125]])
# ---- velocity: max_speed > 100.0
for dtype in ("float32", "float64"):
    row(f"speed exactly 100 from (60, 80): none [{dtype}, D=2]", dtype, 2, edit=chain(put(V, 1, 0, 60.0), put(V, 1, 1, -80.0)))
    row(f"speed exactly 100 from (0, 60, 80): none [{dtype}, D=3]", dtype, 3,
        edit=chain(put(V, 2, 0, 0.0), put(V, 2, 1, 60.0), put(V, 2, 2, 80.0)))
    row(f"speed just above 100, largest component negative [{dtype}, D=2]", dtype, 2,
        edit=chain(put(V, 1, 0, 60.0), put(V, 1, 1, -80.5)))
    row(f"speed 700 from (200, 300, 600) [{dtype}, D=3]", dtype, 3,
        edit=chain(put(V, 0, 0, -200.0), put(V, 0, 1, 300.0), put(V, 0, 2, -600.0)))
    row(f"speed above 1000: severity capped [{dtype}, D=2]", dtype, 2, edit=chain(put(V, 2, 0, 3000.0), put(V, 2, 1, 4000.0)))
    row(f"over-speed star with an energy jump: velocity [{dtype}, D=2]", dtype, 2, edit=put(V, 0, 0, 150.0), energy=-500.0)
    row(f"over-speed star with a huge radius: velocity [{dtype}, D=3]", dtype, 3,
        edit=chain(put(V, 0, 0, 150.0), put(P, 1, 2, 5000.0), put(Q, 1, 2, 5000.0)))
# ---- energy: prev_energy != 0 and (abs(energy / prev_energy) > 100 or < 0.01)
for i, (e, pe, note) in enumerate([
        (-183.0, -1.0, "ratio 183"), (-100.0, -1.0, "ratio exactly 100: none"), (-100.5, -1.0, "ratio 100.5"),
        (200.0, -1.0, "ratio 200 across a change of sign"), (0.01, 1.0, "ratio 0.01 as computed: none"),
        (-0.005, -1.0, "ratio 0.005"), (0.0, -1.0, "ratio 0: severity 1"), (-0.0, 2.0, "ratio 0 from -0.0"),
        (INF, -1.0, "ratio inf: severity 1"), (-1.0, 0.0, "prev_energy 0.0: skipped"), (-1.0, -0.0, "prev_energy -0.0: skipped"),
        (-1.0, NAN, "prev_energy NaN: the ratio is NaN, none"), (NAN, -1.0, "energy NaN: none"), (INF, INF, "inf / inf: none"),
        (-1.0, 1e-300, "tiny prev_energy: ratio 1e300, severity capped"), (1.0, 5e-324, "subnormal prev_energy: ratio inf"),
        (1e-3, 1e-9, "ratio 1e6: severity capped"), (-3.0, -1.0, "ratio 3: none"), (-1e-5, -1.0, "ratio 1e-5: severity 1 exactly"),
        (-0.5, 1e5, "ratio 5e-6: severity capped")]):
    row(f"energy: {note} [{('float32', 'float64')[i % 2]}, D={2 + i // 2 % 2}]", ("float32", "float64")[i % 2], 2 + i // 2 % 2,
        energy=e, prev_energy=pe)
both("energy jump with a huge radius: energy", d=2, edit=chain(put(P, 1, 0, 5000.0), put(Q, 1, 0, 5000.0)), energy=-500.0)
# ---- radius: max_radius > 1000
for dtype in ("float32", "float64"):
    row(f"radius exactly 1000 from (600, 800): none [{dtype}, D=2]", dtype, 2,
        edit=chain(put(P, 2, 0, 600.0), put(P, 2, 1, -800.0), put(Q, 2, 0, 600.0), put(Q, 2, 1, -800.0)))
    row(f"radius just above 1000 in the last star [{dtype}, D=2]", dtype, 2,
        edit=chain(put(P, 2, 0, 600.0), put(P, 2, 1, -801.0), put(Q, 2, 0, 600.0), put(Q, 2, 1, -801.0)))
    row(f"radius 7000 from (2000, 3000, 6000) [{dtype}, D=3]", dtype, 3,
        edit=chain(*[put(a, 0, c, x) for a in (P, Q) for c, x in enumerate((-2000.0, 3000.0, 6000.0))]))
    row(f"radius above 10000: severity capped [{dtype}, D=3]", dtype, 3, edit=chain(put(P, 1, 1, -3e4), put(Q, 1, 1, -3e4)))
    row(f"one star, radius 1300 from (500, 1200) [{dtype}, D=2]", dtype, 2, pos=[[500.0, -1200.0]], prev=[[500.0, -1200.0]],
        vel=[[0.0, 0.0]])


def torch_measures(p, v, q):
    """detect_crash's own expressions (:60-71, :83-85, :98-99, :126-127)."""
    return (bool(torch.isnan(p).any() or torch.isnan(v).any()), bool(torch.isinf(p).any() or torch.isinf(v).any()),
            torch.sqrt(((p - q) ** 2).sum(dim=-1)).max().item(), v.abs().max().item(),
            torch.sqrt((v ** 2).sum(dim=-1)).max().item(), torch.sqrt((p ** 2).sum(dim=-1)).max().item())


def numpy_measures(p, v, q):
    """The contract of ensemble.py in numpy: per star (c0*c0 + c1*c1) + c2*c2 in the state dtype, one correctly rounded root
    of the maximum."""
    def norm2(a):
        s = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]
        return s + a[:, 2] * a[:, 2] if a.shape[1] == 3 else s
    with np.errstate(all="ignore"):
        return (bool(np.isnan(p).any() or np.isnan(v).any()), bool(np.isinf(p).any() or np.isinf(v).any()),
                float(np.sqrt(norm2(p - q).max())), float(np.abs(v).max()), float(np.sqrt(norm2(v).max())),
                float(np.sqrt(norm2(p).max())))


def main():
    warnings.simplefilter("ignore")
    rows = [r for r in ROWS if r is not None]
    R = len(rows)
    out = dict(pos=np.zeros((R, MAXN, 3)), vel=np.zeros((R, MAXN, 3)), prev=np.zeros((R, MAXN, 3)), n=np.zeros(R, np.int64),
               d=np.zeros(R, np.int64), is_f64=np.zeros(R, bool), energy=np.zeros(R), prev_energy=np.zeros(R), dt=np.zeros(R),
               kind=np.zeros(R, np.int64), value=np.full(R, np.nan), severity=np.zeros(R), measures=np.zeros((R, 4)),
               note=np.array([r["note"] for r in rows]), crash_types=np.array(TYPES))
    for i, r in enumerate(rows):
        dt_np = np.float64 if r["dtype"] == "float64" else np.float32
        with np.errstate(all="ignore"):
            p, v, q = (r[k].astype(dt_np) for k in ("pos", "vel", "prev"))
        n, d = p.shape
        tm, nm = torch_measures(*(torch.from_numpy(a) for a in (p, v, q))), numpy_measures(p, v, q)
        if not (tm[0] or tm[1]):
            assert tm == nm, f"row {i} ({r['note']}): torch {tm} against numpy {nm}: replace the row"
        assert tm[:2] == nm[:2], r["note"]
        rep = detect_crash(torch.from_numpy(p), torch.from_numpy(v), torch.from_numpy(q), None, r["energy"], r["prev_energy"],
                           r["dt"], 0)
        for k, a in (("pos", p), ("vel", v), ("prev", q)):
            out[k][i, :n, :d] = a
        out["n"][i], out["d"][i], out["is_f64"][i] = n, d, r["dtype"] == "float64"
        out["energy"][i], out["prev_energy"][i], out["dt"][i] = r["energy"], r["prev_energy"], r["dt"]
        out["measures"][i] = tm[2:] if not (tm[0] or tm[1]) else np.nan
        if rep is not None:
            out["kind"][i], out["value"][i], out["severity"][i] = TYPES.index(rep.crash_type), rep.value, rep.severity
        print(f"{i:3d} {TYPES[out['kind'][i]] or 'none':20s} value {out['value'][i]:<12.6g} severity {out['severity'][i]:<8.4g} {r['note']}")
    kinds = set(out["kind"].tolist())
    assert kinds == set(range(7)), kinds
    assert R >= 60, R
    np.savez_compressed(os.path.join(HERE, "g22_crash_points.npz"), **out)
    print(f"{R} rows written")


if __name__ == "__main__":
    main()
