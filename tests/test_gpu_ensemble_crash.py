"""The crash-point detector on the GPU: crash_measures / run_crash_watched of GalaxyEnsemble and QuantizedEnsemble against the
numpy restatement of the measures' contract (test_ensemble_crash_api.numpy_measures), against the reference's torch
expressions, and against solo GalaxySimulations driven through the reference's loop (crash_point_test.py:186-215).

B = 7 members: the clustered-core-plus-halo inputs of test_gpu_plan_shapes with one seed per member, member 3 with uniform
masses, changed per member as MEMBERS says (velocities zeroed or scaled, a NaN velocity, and one hand-built member: two unit
masses at (+-1, 0) that swap places in one tick, the other stars of mass 1e-6 about 40 away).  Shapes: see CASES.

The per-member parameters (WATCH) were found on the CPU with the reference implementation under oracle/ driven through the
same loop; what is asserted first is that the SOLO values measured here keep 1 % away from both energy thresholds at every
check and show the variety the parameters were chosen for.  Figures of the solo loops are printed before anything is asserted
on them.  Per case ONE watched run and ONE set of solo loops are computed and shared by the tests.
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_plan_shapes import inputs
from test_gpu_ensemble import T, same, solo_state, snapshot
from test_ensemble_crash_api import numpy_measures

pytestmark = pytest.mark.gpu

B = 7
UNIFORM_MEMBER, NAN_MEMBER, TELEPORT_MEMBER = 3, 1, 6
LEVELS = [2, 16, 64, 100, 256, 8, 32]          # CUSTOM: per member
GRID = ("int8_sim", "int4_sim", "custom")
# (N, D, mode).  37: one partial wave of live threads; 257: a second pass of the stride loop for a single star; 1025: every
# thread in several passes plus one star; 300: a hook mode with fp32 state; int4_sim: the finish launch moves the positions in
# place; custom: positions ping-pong
CASES = [
    (37, 2, "float32"), (37, 3, "float64"),
    (257, 2, "float32"),
    (1025, 3, "float64"),
    (300, 2, "bfloat16"),
    (257, 3, "int4_sim"), (257, 2, "custom"),
]
IDS = [f"n{n}-d{d}-{m}" for n, d, m in CASES]
CAST37 = CASES[:2]
# what becomes of member b's generated velocities: kept, zeroed, or scaled
MEMBERS = ["kept", "kept", "kept", "zero", "zero", 400.0, "teleport"]
STABLE = (0.001, 0.1, 0.01)
# member b's (G, softening, dt).  What the reference implementation gave on the CPU for the two N = 37 cases (0-based tick
# of the check that fired):
#   (37, 2, float32)  2: VELOCITY at tick 0 (speed 111);  3: VELOCITY at tick 4 (speed 137);  4: ENERGY at tick 7 (ratio 134);
#                     5: RADIUS at tick 7 (radius 1096);  6: TELEPORT at tick 0 (1.99 against an expected 0.30)
#   (37, 3, float64)  2: VELOCITY at tick 0 (speed 624);  3: VELOCITY at tick 4 (speed 133);  4: ENERGY at tick 12 (ratio 122);
#                     5: RADIUS at tick 6 (radius 1090);  6: TELEPORT at tick 0
# members 0 and 1 are stable (member 1 gets a NaN velocity: NAN at tick 0).  The other cases take the first table: there only
# some halted and some not are asked for.
WATCH32 = [STABLE, STABLE, (5.0, 0.01, 0.1), (1.0, 0.01, 0.05), (0.01, 0.001, 0.05), (0.001, 0.1, 2.0), (4.0, 0.1, 2.0)]
WATCH = {(37, 3, "float64"): [STABLE, STABLE, (50.0, 0.01, 0.1), (0.05, 0.002, 0.1), (0.01, 0.002, 0.1), (0.001, 0.1, 2.0),
                              (4.0, 0.1, 2.0)]}
MAX_TICKS = {37: 20}                  # the budget of a case's shared run (else 8)


def budget(case):
    return MAX_TICKS.get(case[0], 8)


def params(case):
    return tuple([q[k] for q in WATCH.get(case, WATCH32)] for k in range(3))


@pytest.fixture(scope="module")
def nb():
    import nbody_cosmological_simulation_amd as pkg
    assert pkg._native.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return pkg


@functools.lru_cache(maxsize=None)
def members(case):
    """Initial (B, N, D) positions, velocities and (B, N) masses of a case (numpy, the mode's settled dtype; all finite)."""
    n, d, mode = case
    dtype = np.float64 if mode == "float64" else np.float32
    ms = []
    for b in range(B):
        p, v, m = inputs(n, d, 1000 + 17 * b, mode == "float64", uniform=(b == UNIFORM_MEMBER))
        if MEMBERS[b] == "zero":
            v = np.zeros_like(v)
        elif MEMBERS[b] == "teleport":
            p, v, m = np.zeros((n, d)), np.zeros((n, d)), np.full(n, 1e-6)
            p[:, 0], p[:, 1] = 30.0 + 0.25 * np.arange(n), 30.0
            p[:2], m[:2] = 0.0, 1.0
            p[0, 0], p[1, 0] = 1.0, -1.0
        elif MEMBERS[b] != "kept":
            v = v * MEMBERS[b]
        ms.append((p.astype(dtype), v.astype(dtype), m.astype(dtype)))
    return tuple(np.stack([m[k] for m in ms]) for k in range(3))


def nan_velocities(case):
    v = members(case)[1].copy()
    v[NAN_MEMBER, min(5, case[0] - 1), 0] = np.nan
    return v


def make_ens(nb, case, order=range(B)):
    p, v, m = members(case)
    idx = list(order)
    G, soft, dt = ([q[b] for b in idx] for q in params(case))
    kw = dict(precision_mode=nb.PrecisionMode(case[2]), G=G, softening=soft, dt=dt)
    if case[2] in GRID:
        lv = [LEVELS[b] for b in idx] if case[2] == "custom" else None
        return nb.QuantizedEnsemble(T(p[idx]), T(v[idx]), T(m[idx]), custom_levels=lv, **kw)
    return nb.GalaxyEnsemble(T(p[idx]), T(v[idx]), T(m[idx]), **kw)


def make_solo(nb, case, b, acc0, vel=None):
    p, v, m = members(case)
    G, soft, dt = (q[b] for q in params(case))
    s = nb.GalaxySimulation(T(p[b]), T(v[b]), T(m[b]), precision_mode=nb.PrecisionMode(case[2]),
                            custom_levels=LEVELS[b] if case[2] == "custom" else None, G=G, softening=soft, dt=dt)
    # the constructor's evaluation takes the tiled path and may differ in the last bit: start from the ensemble's
    s.accelerations = T(acc0[b]).clone()
    if vel is not None:
        s.velocities = T(vel).clone()
    return s


def measures_of(pos, vel, prev):
    """numpy_measures of every member: (flags (B, 2) bool, maxima (B, 4) float64)."""
    rows = [numpy_measures(pos[b], vel[b], None if prev is None else prev[b]) for b in range(len(pos))]
    return np.array([r[:2] for r in rows]), np.array([r[2:] for r in rows])


def solo_crash_loop(nb, s, ticks):
    """crash_point_test.py:186-215 on a solo GalaxySimulation with crash_kind on the numpy measures of the downloaded states.
    Returns (ticks_taken, kind, energy ratio per check, (flags, maxima, energy, prev_energy) of the last check or None)."""
    ratios, last = [], None
    for tick in range(ticks):
        prev_pos = s.positions.clone().numpy()
        prev_energy = s.get_total_energy()
        s.step()
        energy = s.get_total_energy()
        m = numpy_measures(s.positions.numpy(), s.velocities.numpy(), prev_pos)
        ratios.append(abs(energy / prev_energy) if prev_energy != 0 else float("nan"))
        last = (m[:2], m[2:], energy, prev_energy)
        kind = nb.crash_kind(*m, energy, prev_energy, s.dt)
        if kind:
            return tick + 1, kind, ratios, last
    return ticks, 0, ratios, last


def same_debug(case, got, b, want, what):
    for key in ("lmin", "lmax", "r2max", "fmin", "fmax", "fast_path"):
        if key in ("fmin", "fmax") and case[2] == "custom":
            assert np.isnan(got[key][b]), f"{what}: {key} of member {b} should be NaN under CUSTOM"
            continue
        g, w = got[key][b], want[key]
        assert (g == w) or (g != g and w != w), f"{what}: {key} of member {b}: ensemble {g!r}, solo {w!r}"


def eq(a, b):
    """Equal bit for bit as values (NaN equal to NaN; 0.0 and -0.0 do not occur where this is used on signed zeros)."""
    return a == b or (a != a and b != b)


def ulps_apart(a, b, dtype):
    """Distance in units in the last place between two non-negative values of `dtype` (0 for equal infinities)."""
    if a == b:
        return 0
    ints = np.int64 if dtype == np.float64 else np.int32
    return abs(int(np.array(a, dtype).view(ints)) - int(np.array(b, dtype).view(ints)))


_RUNS = {}


def watched_run(nb, case):
    """The shared run of a case: run_crash_watched(budget) on the B = 7 ensemble (member 1 with its NaN velocity) and the solo
    loops of its members.  Returns a dict: rep, got (final snapshot), dbg, acc0, launches, tick, member_ticks, solos
    [(ticks_taken, kind, ratios, last, final state, quant_debug or None)]."""
    if case not in _RUNS:
        e = make_ens(nb, case)
        acc0 = e.accelerations.numpy()
        vel = nan_velocities(case)
        e.set_state(velocities=T(vel))
        before = e.launches()
        rep = e.run_crash_watched(budget(case))
        out = dict(rep=rep, got=snapshot(e), dbg=e.quant_debug() if case[2] in GRID else None, acc0=acc0,
                   launches=e.launches() - before, tick=e.tick, member_ticks=e.member_ticks)
        e.close()
        solos = []
        for b in range(B):
            s = make_solo(nb, case, b, acc0, vel[b] if b == NAN_MEMBER else None)
            res = solo_crash_loop(nb, s, budget(case))
            solos.append(res + (solo_state(s), s.quant_debug() if out["dbg"] is not None else None))
            s.close()
        out["solos"] = solos
        for b, (ticks, kind, ratios, _, _, _) in enumerate(solos):
            print(f"{case} member {b}: solo loop takes {ticks} ticks, kind {kind}; |E / E_prev| per check "
                  + " ".join(f"{r:.4g}" for r in ratios) + f" | watch: {int(rep.ticks_taken[b])} ticks, kind {int(rep.kind[b])}")
        _RUNS[case] = out
    return _RUNS[case]


# ---- 1. the measures, element by element ---------------------------------------------------------------------------------------
def planted(case):
    """(positions, velocities, prev_positions) of the case with one feature per member (see the test)."""
    n, d, mode = case
    pos, vel, _ = (a.copy() for a in members(case))
    prev = pos.copy()
    prev[:, :, 0] -= pos.dtype.type(1.0 / 1024)                    # everybody moved a little
    star = [0, min(255, n - 1), min(256, n - 2), n - 1]
    for b in range(4):                                             # the largest displacement in this star of member b
        prev[b, star[b], :2] = pos[b, star[b], :2] - np.array([300.0, -400.0], pos.dtype) * (b + 1)
    if mode != "float64":
        prev[0, 0, 0] = -3e19                                      # its square is inf in float32, nothing in the state is
    vel[3, n // 2, :2] = (10.0, -70.0)                             # the largest speed, its largest component negative
    pos[4, n - 1] = 0.0
    pos[4, n - 1, :2] = (3000.0, -4000.0)                          # the largest radius in the last star
    prev[4, n - 1] = pos[4, n - 1]
    vel[4, 0, 0], vel[4, 1, 1] = -0.0, np.finfo(pos.dtype).smallest_subnormal
    pos[5, n - 1, d - 1] = np.nan                                  # a NaN only in the last position component
    prev[5, n - 1, d - 1] = 0.0
    vel[6, n // 3, 1] = -np.inf                                    # an Inf only in one velocity component, no NaN anywhere
    return pos, vel, prev


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_measures_element_by_element(nb, case):
    n, d, mode = case
    dtype = np.float64 if mode == "float64" else np.float32
    pos, vel, prev = planted(case)
    flags, maxima = measures_of(pos, vel, prev)
    assert flags.tolist() == [[False, False]] * 5 + [[True, False], [False, True]]
    if mode != "float64":
        assert np.isinf(maxima[0, 0]) and np.isfinite(pos[0]).all() and np.isfinite(prev[0]).all()
    assert maxima[3, 1] == 70.0 and maxima[4, 3] == 5000.0
    e = make_ens(nb, case)
    e.set_state(positions=T(pos), velocities=T(vel))
    before = snapshot(e), e.tick, e.launches(), e.member_ticks
    got = e.crash_measures(T(prev))
    assert isinstance(got, nb.CrashMeasures)
    fields = (got.max_displacement, got.max_abs_velocity, got.max_speed, got.max_radius)
    assert got.has_nan.dtype == np.bool_ and got.has_inf.dtype == np.bool_ and all(f.dtype == np.float64 for f in fields)
    assert got.has_nan.tolist() == flags[:, 0].tolist() and got.has_inf.tolist() == flags[:, 1].tolist()
    for b in range(5):                     # members with a NaN or an Inf are compared on flags only
        # (a) the numpy restatement, bit for bit
        assert [float(f[b]) for f in fields] == maxima[b].tolist(), f"member {b}: {[f[b] for f in fields]} against {maxima[b]}"
        # (b) the reference's torch expressions on the CPU, to one unit in the last place of the state dtype
        p, v, q = T(pos[b]), T(vel[b]), T(prev[b])
        ref = (torch.sqrt(((p - q) ** 2).sum(dim=-1)).max().item(), v.abs().max().item(),
               torch.sqrt((v ** 2).sum(dim=-1)).max().item(), torch.sqrt((p ** 2).sum(dim=-1)).max().item())
        for f, r in zip(fields, ref):
            assert ulps_apart(float(f[b]), r, dtype) <= 1, f"member {b}: {float(f[b])!r} against torch's {r!r}"
    # without previous positions the displacement is 0 and the rest is unchanged
    none = e.crash_measures()
    assert none.max_displacement.tolist() == [0.0] * B
    for b in range(5):
        assert [none.max_abs_velocity[b], none.max_speed[b], none.max_radius[b]] == maxima[b, 1:].tolist()
    assert none.has_nan.tolist() == flags[:, 0].tolist() and none.has_inf.tolist() == flags[:, 1].tolist()
    # previous positions on the device
    dev = e.crash_measures(T(prev).cuda())
    for a, c in zip(dev, got):
        assert np.array_equal(a[:5], c[:5]) and a.dtype == c.dtype
    assert dev.has_nan.tolist() == got.has_nan.tolist() and dev.has_inf.tolist() == got.has_inf.tolist()
    # nothing moved
    same(snapshot(e), before[0], "state after crash_measures")
    assert (e.tick, e.launches(), e.member_ticks) == before[1:]
    e.close()
    # members are independent: permuting them permutes the result
    perm = [3, 6, 0, 5, 1, 4, 2]
    e = make_ens(nb, case, perm)
    e.set_state(positions=T(pos[perm]), velocities=T(vel[perm]))
    other = e.crash_measures(T(prev[perm]))
    e.close()
    for a, c in zip(other, got):
        keep = [i for i, b in enumerate(perm) if b < 5]
        assert np.array_equal(a[keep], c[[perm[i] for i in keep]])
    assert other.has_nan.tolist() == got.has_nan[perm].tolist() and other.has_inf.tolist() == got.has_inf[perm].tolist()


# ---- 2. the watched run against the solo loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_watch_halts_members_where_the_reference_loop_stops_them(nb, case):
    run = watched_run(nb, case)
    rep, solos = run["rep"], run["solos"]
    # conditions on the inputs, from the solo values
    for b, (_, _, ratios, _, _, _) in enumerate(solos):
        for r in ratios:
            assert not abs(r / 100.0 - 1.0) <= 0.01 and not abs(r / 0.01 - 1.0) <= 0.01, f"member {b} sits on a threshold: change the inputs"
    halted = [b for b in range(B) if solos[b][1]]
    assert halted and len(halted) < B, "some members must be halted and some not: change the inputs"
    # the decisions
    assert run["launches"] == budget(case) and run["tick"] == budget(case)
    assert run["member_ticks"] == [int(t) for t in rep.ticks_taken]
    for b, (ticks, kind, _, _, state, dbg) in enumerate(solos):
        want = (ticks, ticks - 1 if kind else budget(case), kind, nb.ensemble.CRASH_TYPES[kind], kind != 0)
        assert (int(rep.ticks_taken[b]), int(rep.stable_ticks[b]), int(rep.kind[b]), rep.crash_type[b], bool(rep.crashed[b])) == want, f"member {b}"
        same([g[b] for g in run["got"]], state, f"member {b} against its solo run of {ticks} steps")
        if dbg is not None:
            same_debug(case, run["dbg"], b, dbg, f"member {b} after {ticks} ticks")
    assert int(rep.kind[NAN_MEMBER]) == nb.ensemble.CRASH_NAN and int(rep.ticks_taken[NAN_MEMBER]) == 1
    if case in CAST37:
        assert int(rep.kind[TELEPORT_MEMBER]) == nb.ensemble.CRASH_TELEPORT and int(rep.ticks_taken[TELEPORT_MEMBER]) == 1


def test_the_two_small_cases_show_every_kind_that_stepping_can_reach(nb):
    """INF cannot be reached by stepping (an infinite coordinate turns every force into NaN in the same tick): it is covered by
    test_measures_element_by_element and by g22."""
    E = nb.ensemble
    kinds, stops = set(), set()
    for case in CAST37:
        solos = watched_run(nb, case)["solos"]
        kinds |= {s[1] for s in solos}
        stops = {s[0] for s in solos}
        assert len(stops) >= 3, f"{case}: fewer than three distinct stop ticks: change the inputs"
        assert any(s[1] and s[0] == 1 for s in solos), f"{case}: no member crashes at its first check: change the inputs"
        assert any(s[1] and s[0] > 5 for s in solos), f"{case}: no member crashes after its fifth check: change the inputs"
    assert kinds == {E.CRASH_NONE, E.CRASH_NAN, E.CRASH_TELEPORT, E.CRASH_VELOCITY, E.CRASH_ENERGY, E.CRASH_RADIUS}, kinds


# ---- 3. the report against its own history ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_report_is_crash_kind_applied_to_its_own_history_and_measures(nb, case):
    run = watched_run(nb, case)
    rep, solos = run["rep"], run["solos"]
    total = rep.history.total.cpu().numpy()
    ke, pe = rep.history.kinetic.cpu().numpy(), rep.history.potential.cpu().numpy()
    S = budget(case) + 1
    assert rep.history.ticks == list(range(S)) and total.shape == (S, B)
    G, soft, dt = params(case)
    m = rep.measures
    for b in range(B):
        taken, kind = int(rep.ticks_taken[b]), int(rep.kind[b])
        # every earlier check found nothing: the flags are monotone (a NaN stays), and the other criteria held off until the
        # last check, whose measures the report has; so the earlier checks are judged on the energies, which is all of the
        # decision that is not bit-identical to the solo loop's
        flags, maxima, _, _ = solos[b][3]
        assert (bool(m.has_nan[b]), bool(m.has_inf[b])) == flags, f"member {b}"
        if not any(flags):
            assert [m.max_displacement[b], m.max_abs_velocity[b], m.max_speed[b], m.max_radius[b]] == list(maxima), f"member {b}"
        args = (m.has_nan[b], m.has_inf[b], m.max_displacement[b], m.max_abs_velocity[b], m.max_speed[b], m.max_radius[b])
        assert nb.crash_kind(*args, total[taken, b], total[taken - 1, b], dt[b]) == kind, f"member {b}"
        for s in range(1, taken):
            assert nb.crash_kind(False, False, 0.0, 0.0, 0.0, 0.0, total[s, b], total[s - 1, b], dt[b]) == 0, f"member {b} check {s}"
        if kind:
            value = nb.crash_value(kind, m.max_displacement[b], m.max_speed[b], m.max_radius[b], total[taken, b])
            sev = nb.crash_severity(kind, m.max_displacement[b], m.max_speed[b], m.max_radius[b], total[taken, b], total[taken - 1, b])
            assert eq(rep.value[b], value) and eq(rep.severity[b], sev), f"member {b}"
        else:
            assert np.isnan(rep.value[b]) and rep.severity[b] == 0.0
        # frozen: every later sample repeats the member's last one, bit for bit
        for s in range(taken, S):
            assert eq(ke[s, b], ke[taken, b]) and eq(pe[s, b], pe[taken, b]), f"member {b} sample {s}"
    assert rep.ticks_taken.dtype == np.int64 and rep.stable_ticks.dtype == np.int64 and rep.kind.dtype == np.int64
    assert rep.crashed.dtype == np.bool_ and rep.value.dtype == np.float64 and rep.severity.dtype == np.float64


# ---- 4. mechanics ------------------------------------------------------------------------------------------------------------------
MECH = [(37, 2, "float32"), (257, 3, "int4_sim"), (257, 2, "custom")]


def solo_members(nb, case, acc0, vel):
    return [make_solo(nb, case, b, acc0, vel[b] if b == NAN_MEMBER else None) for b in range(B)]


def check_against_solos(nb, case, e, rep, solos, budgets, what):
    """The solo loops with these budgets, on solos that go on from where they are; the ensemble must agree."""
    got = snapshot(e)
    dbg = e.quant_debug() if case[2] in GRID else None
    for b, s in enumerate(solos):
        ticks, kind, _, _ = solo_crash_loop(nb, s, budgets[b])
        assert (int(rep.ticks_taken[b]), int(rep.kind[b])) == (ticks, kind), f"{what}: member {b}"
        assert int(rep.stable_ticks[b]) == (ticks - 1 if kind else budgets[b]), f"{what}: member {b}"
        same([g[b] for g in got], solo_state(s), f"{what}: member {b} against its solo run")
        if dbg is not None and ticks:
            same_debug(case, dbg, b, s.quant_debug(), f"{what}: member {b}")


@pytest.mark.parametrize("case", MECH, ids=[f"n{n}-d{d}-{m}" for n, d, m in MECH])
def test_uneven_budgets_and_a_second_call_that_goes_on_from_the_first(nb, case):
    """Budgets of 0 and 1, a budget that ends one tick before the member would have crashed (member 3 of the N = 37 case
    crashes at its fifth check: with four ticks it is not halted), and a second call whose first check is against the
    positions at ITS entry."""
    shared = watched_run(nb, case)
    first = [0, 1, 3, 4, 2, 1, 0]
    if case == MECH[0]:
        assert shared["solos"][3][:2] == (5, nb.ensemble.CRASH_VELOCITY)
    e = make_ens(nb, case)
    vel = nan_velocities(case)
    e.set_state(velocities=T(vel))
    solos = solo_members(nb, case, shared["acc0"], vel)
    before = e.launches()
    rep = e.run_crash_watched(first)
    assert e.launches() - before == 4 and e.tick == 4
    check_against_solos(nb, case, e, rep, solos, first, "first call")
    if case == MECH[0]:
        assert not rep.crashed[3] and int(rep.ticks_taken[3]) == 4 and int(rep.stable_ticks[3]) == 4
    assert not rep.crashed[0] and int(rep.ticks_taken[0]) == 0 and not rep.crashed[6]
    assert rep.measures.max_radius[0] == 0.0 and not rep.measures.has_nan[0]              # never checked
    taken = [int(t) for t in rep.ticks_taken]
    assert e.member_ticks == taken
    second = [3, 2, 0, 2, 5, 1, 2]
    rep2 = e.run_crash_watched(second)
    check_against_solos(nb, case, e, rep2, solos, second, "second call")
    assert e.tick == 4 + 5 and e.launches() - before == 4 + 5
    assert e.member_ticks == [a + int(c) for a, c in zip(taken, rep2.ticks_taken)]
    assert rep2.history.ticks == list(range(4, 10))
    if case == MECH[0]:
        assert int(rep2.kind[3]) == nb.ensemble.CRASH_VELOCITY and int(rep2.ticks_taken[3]) == 1   # its fifth tick in all
        assert int(rep2.kind[6]) == nb.ensemble.CRASH_TELEPORT and int(rep2.ticks_taken[6]) == 1
    for s in solos:
        s.close()
    e.close()


@pytest.mark.parametrize("warm", [1, 3], ids=["after-run-1", "after-run-3"])
@pytest.mark.parametrize("case", MECH, ids=[f"n{n}-d{d}-{m}" for n, d, m in MECH])
def test_either_position_buffer_may_be_current_at_entry_and_later_calls_go_on(nb, case, warm):
    """run(1) / run(3) leave an odd / even number of buffer swaps behind; then a watched call, then run_members, run_recorded
    and run_watched, every member still bit-identical to its solo run."""
    shared = watched_run(nb, case)
    e = make_ens(nb, case)
    solos = solo_members(nb, case, shared["acc0"], members(case)[1])          # (no NaN here: the later calls step everybody)
    before = e.launches()
    e.run(warm)
    for s in solos:
        s.run(warm)
    budgets = [3, 0, 2, 3, 1, 3, 2]
    rep = e.run_crash_watched(budgets)
    check_against_solos(nb, case, e, rep, solos, budgets, f"watched call after run({warm})")
    assert e.launches() - before == warm + 3
    later = [2, 1, 0, 2, 1, 0, 2]
    e.run_members(later)
    h = e.run_recorded(2, every=1)
    w = e.run_watched(2, check_interval=1)
    assert h.ticks == [e.tick - 4, e.tick - 3, e.tick - 2]
    got = snapshot(e)
    for b, s in enumerate(solos):
        s.run(later[b] + 2 + int(w.stable_ticks[b]))
        same([g[b] for g in got], solo_state(s), f"member {b} after the later calls")
        s.close()
    assert e.launches() - before == warm + 3 + 2 + 2 + 2
    e.close()
