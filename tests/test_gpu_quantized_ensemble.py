"""QuantizedEnsemble on the GPU: every member bit-identical to the solo engine under INT8_SIM / INT4_SIM / CUSTOM, every
member's tables those of its solo run, members independent of each other, the suite's bars against the oracle, solo-equal
energies and a recorded run, and one force launch per tick.

The setup is test_gpu_ensemble's: B = 5 members, the clustered-core-plus-halo inputs of test_gpu_plan_shapes with one seed
per member, member 3 with uniform masses; G, softening and dt differ per member (two members have softening^2 below the
grid's floor of 0.01, three above it); dt changes after the second tick.  CUSTOM cases give every member its own number of
levels.  One five-tick trajectory per case is computed once by a B = 5 ensemble driven with step() and shared by the tests.

The tables after the constructor: a solo constructor evaluates on the TILED path, whose sums may differ from the one-launch
step's in the last bit (why every solo run here starts from the ensemble's accelerations) -- measured on an MI355X at
(1025, 3, int4_sim), member 0: fmax 0.815361499786377 (ensemble) against 0.8153613805770874 (solo constructor), one fp32
ulp.  lmin / lmax / r2max / fast_path do not depend on the path and are compared with the solo constructor's; all six
entries AND the initial accelerations are compared, exactly, with a solo run that evaluates the initial positions on the
one-launch path: zero velocities and zero accelerations make the first tick's kick + drift leave the positions as they are.
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_plan_shapes import inputs, relerr
from test_gpu_ensemble import B, TICKS, G_, SOFT, DT, DT2, UNIFORM_MEMBER, T, same, solo_state, snapshot, drive_steps

pytestmark = pytest.mark.gpu

LEVELS = [2, 3, 16, 64, 256]            # CUSTOM: per member
FIXED = {"int8_sim": 256, "int4_sim": 16}

# (N, D, mode): N = 37 fewer sources than one 256-entry stride of the pair loop, all padding, one partial workgroup; 700
# ordinary; 1025 one star past the 1024-source LDS tile; 2049 the workgroup switches 512 -> 256 and the solo path builds
# its tables in a launch of their own; 3072 the upper limit
CASES = [
    (37, 2, "int8_sim"), (37, 3, "custom"),
    (700, 3, "int4_sim"), (700, 2, "custom"),
    (1025, 2, "int8_sim"), (1025, 3, "int4_sim"),
    (2049, 3, "custom"), (2049, 2, "int8_sim"),
    (3072, 3, "int4_sim"),
]
# 16 / 32 lanes per target instead of the default 64 (NB_SMALL_LANES, read when a handle is created: ensemble and solo runs of
# a case share it), each in D = 2 and D = 3; N = 257 is one full 256-source stride plus one star, several workgroups
LANES = {(257, 2, "int8_sim"): 16, (257, 3, "custom"): 16, (257, 3, "int4_sim"): 32, (257, 2, "custom"): 32}
CASES += list(LANES)
IDS = [f"n{n}-d{d}-{m}" + (f"-lanes{LANES[n, d, m]}" if (n, d, m) in LANES else "") for n, d, m in CASES]


@pytest.fixture(autouse=True)
def lanes_knob(request, monkeypatch):
    case = request.node.callspec.params.get("case") if hasattr(request.node, "callspec") else None
    if case in LANES:
        monkeypatch.setenv("NB_SMALL_LANES", str(LANES[case]))
DEBUG_KEYS = ("lmin", "lmax", "r2max", "fmin", "fmax", "fast_path")


@pytest.fixture(scope="module")
def nb():
    import nbody_cosmological_simulation_amd as pkg
    assert pkg._native.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return pkg


def levels_of(case):
    return LEVELS if case[2] == "custom" else [FIXED[case[2]]] * B


@functools.lru_cache(maxsize=None)
def members(case):
    """Initial (B, N, D) positions, velocities and (B, N) masses of a case (numpy float32)."""
    n, d, _ = case
    ms = [inputs(n, d, 1000 + 17 * b, False, uniform=(b == UNIFORM_MEMBER)) for b in range(B)]
    return tuple(np.stack([m[k] for m in ms]) for k in range(3))


def make_ens(nb, case, order=range(B), pos=None):
    p, v, m = members(case)
    idx = list(order)
    p = p if pos is None else pos
    lv = [LEVELS[b] for b in idx] if case[2] == "custom" else None
    return nb.QuantizedEnsemble(T(p[idx]), T(v[idx]), T(m[idx]), precision_mode=nb.PrecisionMode(case[2]), custom_levels=lv,
                                G=[G_[b] for b in idx], softening=[SOFT[b] for b in idx], dt=[DT[b] for b in idx])


def make_solo(nb, case, b, acc0=None, pos=None):
    p, v, m = members(case)
    p = p if pos is None else pos
    s = nb.GalaxySimulation(T(p[b]), T(v[b]), T(m[b]), precision_mode=nb.PrecisionMode(case[2]),
                            custom_levels=LEVELS[b] if case[2] == "custom" else None, G=G_[b], softening=SOFT[b], dt=DT[b])
    if acc0 is not None:
        # the constructor's evaluation takes the tiled path and may differ in the last bit: start from the ensemble's
        s.accelerations = T(acc0[b]).clone()
    return s


def solo_at_rest(nb, case, b, pos=None):
    """(quant_debug(), accelerations) of member b's initial positions evaluated by the solo one-launch step: one tick from
    zero velocities and zero accelerations (x + 0 * dt == x)."""
    p, v, m = members(case)
    p = p if pos is None else pos
    s = nb.GalaxySimulation(T(p[b]), T(np.zeros_like(v[b])), T(m[b]), precision_mode=nb.PrecisionMode(case[2]),
                            custom_levels=LEVELS[b] if case[2] == "custom" else None, G=G_[b], softening=SOFT[b], dt=DT[b])
    s.accelerations = T(np.zeros_like(p[b]))
    s.step()
    assert s.force_kernel_name() == "small_step_kernel"
    assert np.array_equal(s.positions.numpy(), p[b], equal_nan=True), "the tick at rest moved the stars"
    out = s.quant_debug(), s.accelerations.numpy()
    s.close()
    return out


def same_initial(nb, case, b, dbg0, acc0, solo_dbg, pos=None):
    """Member b after the ensemble's constructor: the path-independent entries against the solo constructor's, everything
    (and the accelerations) against the solo one-launch evaluation of the same positions."""
    same_debug(case, dbg0, b, solo_dbg, "after the constructor", keys=("lmin", "lmax", "r2max", "fast_path"))
    rest_dbg, rest_acc = solo_at_rest(nb, case, b, pos)
    same_debug(case, dbg0, b, rest_dbg, "after the constructor (solo one-launch evaluation)")
    assert rest_acc.dtype == acc0.dtype and np.array_equal(rest_acc, acc0[b], equal_nan=True), f"initial accelerations of member {b}"


def same_debug(case, got, b, want, what, keys=DEBUG_KEYS):
    """Member b of the ensemble's quant_debug() against a solo quant_debug(): exact equality, key by key."""
    for key in keys:
        if key in ("fmin", "fmax") and case[2] == "custom":
            assert np.isnan(got[key][b]), f"{what}: {key} of member {b} should be NaN under CUSTOM"
            continue
        g, w = got[key][b], want[key]
        assert (g == w) or (g != g and w != w), f"{what}: {key} of member {b}: ensemble {g!r}, solo {w!r}"


_TRAJ = {}


def trajectory(nb, case):
    """The shared reference of a case: initial accelerations, quant_debug() after the constructor, the state after every
    tick of the B = 5 ensemble, quant_debug() after the last tick."""
    if case not in _TRAJ:
        e = make_ens(nb, case)
        acc0 = e.accelerations.numpy()
        dbg0 = e.quant_debug()
        assert e.force_kernel_name() == "ens_grid_step_kernel"
        assert list(dbg0["levels"]) == levels_of(case) == e.levels
        ticks = drive_steps(e)
        dbg5 = e.quant_debug()
        e.close()
        _TRAJ[case] = (acc0, ticks, dbg0, dbg5)
    return _TRAJ[case]


# ---- 1. bit identity with the solo engine, 2. the tables -----------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_step_loop_and_tables_are_bit_identical_to_solo(nb, case):
    acc0, ticks, dbg0, dbg5 = trajectory(nb, case)
    print(f"{IDS[CASES.index(case)]}: fast_path after the constructor {dbg0['fast_path'].tolist()}, after tick {TICKS} "
          f"{dbg5['fast_path'].tolist()}")
    for b in range(B):
        s = make_solo(nb, case, b)
        same_initial(nb, case, b, dbg0, acc0, s.quant_debug())
        s.accelerations = T(acc0[b]).clone()
        for t in range(TICKS):
            if t == 2:
                s.dt = DT2[b]
            s.step()
            same(solo_state(s), [a[b] for a in ticks[t]], f"member {b} tick {t + 1}")
            assert s.force_kernel_name() == "small_step_kernel"
        same_debug(case, dbg5, b, s.quant_debug(), f"after tick {TICKS}")
        s.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_run_is_bit_identical_to_solo_and_to_the_step_loop(nb, case):
    acc0, ticks, _, dbg5 = trajectory(nb, case)
    e = make_ens(nb, case)
    e.run(2)
    same(snapshot(e), ticks[1], "ensemble run(2)")
    e.set_params(dt=DT2)
    e.run(3)
    same(snapshot(e), ticks[4], "ensemble run(2) + run(3)")
    assert e.tick == 5 and e.force_kernel_name() == "ens_grid_step_kernel"
    got = e.quant_debug()
    for key in DEBUG_KEYS + ("levels",):
        assert np.array_equal(got[key], dbg5[key], equal_nan=True), f"quant_debug()[{key!r}] after run(2) + run(3)"
    e.close()
    for b in range(B):
        s = make_solo(nb, case, b, acc0)
        s.run(2)
        same(solo_state(s), [a[b] for a in ticks[1]], f"solo member {b} run(2)")
        s.dt = DT2[b]
        s.run(3)
        same(solo_state(s), [a[b] for a in ticks[4]], f"solo member {b} run(2) + run(3)")
        assert s.force_kernel_name() == "small_step_kernel"
        s.close()


def test_tables_without_the_table_free_path(nb, monkeypatch):
    """NB_NO_GRID_FAST: both engines always read their tables, so the table route is covered whichever the default takes."""
    monkeypatch.setenv("NB_NO_GRID_FAST", "1")
    case = (700, 2, "int8_sim")
    e = make_ens(nb, case)
    acc0, dbg0 = e.accelerations.numpy(), e.quant_debug()
    ticks = drive_steps(e)
    dbg5 = e.quant_debug()
    e.close()
    assert not dbg0["fast_path"].any() and not dbg5["fast_path"].any()
    for b in range(B):
        s = make_solo(nb, case, b)
        same_initial(nb, case, b, dbg0, acc0, s.quant_debug())
        s.accelerations = T(acc0[b]).clone()
        for t in range(TICKS):
            if t == 2:
                s.dt = DT2[b]
            s.step()
            same(solo_state(s), [a[b] for a in ticks[t]], f"member {b} tick {t + 1}")
        assert s.force_kernel_name() == "small_step_kernel"
        same_debug(case, dbg5, b, s.quant_debug(), f"after tick {TICKS}")
        s.close()


# ---- 3. members are independent --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_members_do_not_depend_on_their_neighbours(nb, case):
    acc0, ticks, dbg0, dbg5 = trajectory(nb, case)
    rev = list(reversed(range(B)))
    e = make_ens(nb, case, rev)
    same([e.accelerations.numpy()], [acc0[rev]], "reversed order, initial")
    for t, got in enumerate(drive_steps(e, rev)):
        same(got, [a[rev] for a in ticks[t]], f"reversed order tick {t + 1}")
    got = e.quant_debug()
    for key in DEBUG_KEYS + ("levels",):
        assert np.array_equal(got[key], dbg5[key][rev], equal_nan=True), f"reversed order: quant_debug()[{key!r}]"
    e.close()
    for b in range(B):
        e = make_ens(nb, case, [b])
        assert e.num_members == 1
        same([e.accelerations.numpy()], [acc0[[b]]], f"member {b} alone, initial")
        for t, got in enumerate(drive_steps(e, [b])):
            same(got, [a[[b]] for a in ticks[t]], f"member {b} alone tick {t + 1}")
        e.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_nan_member_leaves_the_others_alone(nb, case):
    acc0, ticks, _, _ = trajectory(nb, case)
    bad = 2
    p = members(case)[0].copy()
    p[bad, 0, 0] = np.nan
    p[bad, min(1, case[0] - 1), 1] = np.inf
    e = make_ens(nb, case, pos=p)
    others = [b for b in range(B) if b != bad]
    same([e.accelerations.numpy()[others]], [acc0[others]], "initial")
    for t, got in enumerate(drive_steps(e)):
        same([g[others] for g in got], [a[others] for a in ticks[t]], f"tick {t + 1}")
    # its own state: NaN propagates silently, as in the reference
    pos, vel, acc = got
    assert np.isnan(acc[bad]).all() and np.isnan(vel[bad]).all() and np.isnan(pos[bad]).all()
    e.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_degenerate_member_equals_its_solo_run(nb, case):
    """All stars of one member at one point: every r^2 is the softening^2, so r2max == eps^2, the log grid is degenerate,
    the forces are zero and (INT8 / INT4) the force snap passes them through."""
    acc0, ticks, _, _ = trajectory(nb, case)
    deg = 1
    p = members(case)[0].copy()
    p[deg] = p[deg, 0]
    e = make_ens(nb, case, pos=p)
    others = [b for b in range(B) if b != deg]
    a0 = e.accelerations.numpy()
    dbg = e.quant_debug()
    assert np.all(a0[deg] == 0), "forces of coincident stars"
    assert dbg["r2max"][deg] == np.float32(SOFT[deg] ** 2), (dbg["r2max"][deg], SOFT[deg] ** 2)
    assert dbg["lmin"][deg] == dbg["lmax"][deg] and not dbg["fast_path"][deg]
    if case[2] != "custom":
        assert dbg["fmin"][deg] == 0 and dbg["fmax"][deg] == 0
    same([a0[others]], [acc0[others]], "initial")
    got = drive_steps(e)
    for t in range(TICKS):
        same([g[others] for g in got[t]], [a[others] for a in ticks[t]], f"tick {t + 1}")
    dbg5 = e.quant_debug()
    e.close()
    s = make_solo(nb, case, deg, pos=p)
    same_initial(nb, case, deg, dbg, a0, s.quant_debug(), pos=p)
    s.accelerations = T(a0[deg]).clone()
    for t in range(TICKS):
        if t == 2:
            s.dt = DT2[deg]
        s.step()
        same(solo_state(s), [a[deg] for a in got[t]], f"degenerate member tick {t + 1}")
    assert s.force_kernel_name() == "small_step_kernel"
    same_debug(case, dbg5, deg, s.quant_debug(), f"degenerate member after tick {TICKS}")
    s.close()


# ---- 4. against the oracle (bars of test_gpu_plan_shapes.check_dense) ----------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_initial_forces_and_grids_match_the_oracle(nb, case):
    from oracle import oracle as O
    n, d, mode = case
    acc0, _, dbg0, _ = trajectory(nb, case)
    p, v, m = members(case)
    tag = IDS[CASES.index(case)]
    for b in range(B):
        L = levels_of(case)[b]
        kw = dict(G=G_[b], softening=SOFT[b], levels=L if mode == "custom" else 0)
        ref = O.accelerations(p[b], m[b], mode, force_quant=False, **kw)
        a = acc0[b].astype(np.float64)
        if mode == "custom":
            err = relerr(a, ref)
            print(f"{tag} member {b} ({L} levels): initial accelerations relerr {err:.3e}")
            assert err < 2e-6, (b, err)
        else:
            fmin, fmax = np.float32(dbg0["fmin"][b]), np.float32(dbg0["fmax"][b])
            r32 = ref.astype(np.float32)
            k = np.rint((r32 - fmin) / (fmax - fmin) * np.float32(L - 1))
            snapped = (k / np.float32(L - 1) * (fmax - fmin) + fmin).astype(np.float64)
            step = float(fmax - fmin) / (L - 1)
            err = float(np.abs(a - snapped).max()) / step
            print(f"{tag} member {b}: initial accelerations within {err:.3f} force-grid steps of the snapped oracle")
            assert err <= 1.01, (b, err)
        rows = min(n, 600)
        _, rdbg = O.accelerations_rows(p[b], m[b], mode, 0, rows, bins=True, **kw)
        print(f"{tag} member {b}: lmin {dbg0['lmin'][b]!r} / oracle {rdbg['lmin']!r}, lmax {dbg0['lmax'][b]!r} / oracle "
              f"{rdbg['lmax']!r}")
        assert np.float32(dbg0["lmin"][b]) == np.float32(rdbg["lmin"]), (b, dbg0["lmin"][b], rdbg["lmin"])
        assert np.float32(dbg0["lmax"][b]) == np.float32(rdbg["lmax"]), (b, dbg0["lmax"][b], rdbg["lmax"])


# ---- 5. energies -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_energies_equal_the_solo_values_and_the_recorded_run_the_plain_one(nb, case):
    _, ticks, _, _ = trajectory(nb, case)
    e = make_ens(nb, case)
    ke0, pe0 = (x.numpy().copy() for x in e.energies())
    e.run(2)
    ke, pe = e.get_kinetic_energy(), e.get_potential_energy()
    kb, pb = (x.numpy().copy() for x in e.energies())
    pos, vel, mass = e.positions, e.velocities, e.masses
    for b in range(B):
        s = nb.GalaxySimulation(pos[b].clone(), vel[b].clone(), mass[b].clone(), precision_mode=nb.PrecisionMode(case[2]),
                                custom_levels=LEVELS[b] if case[2] == "custom" else None, G=G_[b], softening=SOFT[b], dt=DT[b])
        assert ke[b] == s.get_kinetic_energy(), (b, ke[b], s.get_kinetic_energy())
        assert pe[b] == s.get_potential_energy(), (b, pe[b], s.get_potential_energy())
        s.close()
        assert abs(kb[b] - ke[b]) <= 2e-6 * abs(ke[b]) and abs(pb[b] - pe[b]) <= 2e-6 * abs(pe[b]), (b, kb[b], ke[b], pb[b], pe[b])
    same(snapshot(e), ticks[1], "state after the energy calls")
    e.run(2)
    kd, pd = (x.numpy().copy() for x in e.energies())
    e.run(1)
    state5 = snapshot(e)
    e.close()
    r = make_ens(nb, case)
    before = r.launches()
    h = r.run_recorded(5, every=2)
    assert h.ticks == [0, 2, 4] and r.tick == 5 and r.launches() - before == 5
    same(snapshot(r), state5, "run_recorded(5, every=2) vs run(2) + run(2) + run(1)")
    r.close()
    for s, (k, q) in enumerate(((ke0, pe0), (kb, pb), (kd, pd))):
        assert np.array_equal(h.kinetic[s].numpy(), k), f"kinetic of sample {s}"
        assert np.array_equal(h.potential[s].numpy(), q), f"potential of sample {s}"


# ---- 6. one force launch per tick ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["int8_sim", "custom"])
def test_a_tick_is_one_force_launch(nb, mode):
    case = (700, 2, mode)
    e = make_ens(nb, case)
    assert e.launches() == 1            # the constructor's evaluation
    e.step()
    assert e.launches() == 2
    e.run(6)
    # force launches only: the tables and finish launches and the opening kick + drift are not counted
    assert e.launches() == 8 and e.tick == 7
    assert e.force_kernel_name() == "ens_grid_step_kernel"
    e.close()
