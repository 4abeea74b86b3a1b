"""Members of different cast modes in one GalaxyEnsemble (precision_mode as a list): every member bit-identical to the solo
GalaxySimulation of its own mode, through every driver of the tick path, with one force launch per tick.

B = 5 with modes [FLOAT32, BFLOAT16, FLOAT16, FLOAT32, FLOAT16], deliberately not grouped by mode; inputs, G, softening and dt
per member as in test_gpu_ensemble.  Per case the mixed ensemble's step() loop and the five solo runs are computed once and
shared; the tests compare the other drivers with them.  There is no tolerance anywhere: the step body is the uniform
kernel's with the hook read per workgroup.
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_plan_shapes import inputs

pytestmark = pytest.mark.gpu

B = 5
TICKS = 5
SOLO_TICKS = 6                         # run_watched rounds a budget of 5 up to 6
MODES = ["float32", "bfloat16", "float16", "float32", "float16"]
G_ = [0.001, 0.00113, 0.00091, 0.00127, 0.00107]
SOFT = [0.1, 0.113, 0.087, 0.131, 0.071]
DT = [0.01, 0.0123, 0.0071, 0.0157, 0.0093]
DT2 = [0.0137, 0.0091, 0.0113, 0.0077, 0.0129]
UNIFORM_MEMBER = 3

# (N, D): 37 fewer sources than lanes of a target, one partial workgroup; 700 ordinary; 1025 one star past the 1024-source
# LDS tile; 2049 the workgroup size switches 512 -> 256; 257 with 16 / 32 lanes per target instead of 64 (NB_SMALL_LANES,
# read when a handle is created: the ensemble and the solo runs of a case share it)
CASES = [(37, 2), (700, 3), (1025, 2), (2049, 3), (257, 2), (257, 3)]
LANES = {(257, 2): 16, (257, 3): 32}
IDS = [f"n{n}-d{d}" + (f"-lanes{LANES[n, d]}" if (n, d) in LANES else "") for n, d in CASES]


@pytest.fixture(autouse=True)
def lanes_knob(request, monkeypatch):
    case = request.node.callspec.params.get("case") if hasattr(request.node, "callspec") else None
    if case in LANES:
        monkeypatch.setenv("NB_SMALL_LANES", str(LANES[case]))


@pytest.fixture(scope="module")
def nb():
    import nbody_cosmological_simulation_amd as pkg
    assert pkg._native.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return pkg


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def members(case):
    n, d = case
    ms = [inputs(n, d, 2000 + 17 * b, False, uniform=(b == UNIFORM_MEMBER)) for b in range(B)]
    return tuple(np.stack([m[k] for m in ms]) for k in range(3))


def mode_list(nb, order=range(B)):
    return [nb.PrecisionMode(MODES[b]) for b in order]


def make_ens(nb, case, order=range(B), pos=None, modes=None):
    p, v, m = members(case)
    idx = list(order)
    p = p if pos is None else pos
    return nb.GalaxyEnsemble(T(p[idx]), T(v[idx]), T(m[idx]), precision_mode=modes if modes is not None else mode_list(nb, idx),
                             G=[G_[b] for b in idx], softening=[SOFT[b] for b in idx], dt=[DT[b] for b in idx])


def snapshot(e):
    return e.positions.numpy(), e.velocities.numpy(), e.accelerations.numpy()


def same(got, want, what):
    for name, g, w in zip(("positions", "velocities", "accelerations"), got, want):
        assert g.dtype == w.dtype == np.float32 and np.array_equal(g, w, equal_nan=True), f"{what}: {name} differ"


_TRAJ, _SOLO = {}, {}


def trajectory(nb, case):
    """Initial accelerations and the state after each of TICKS step() calls of the mixed ensemble."""
    if case not in _TRAJ:
        e = make_ens(nb, case)
        assert e.force_kernel_name() == "ens_step_mixed_kernel"
        acc0 = e.accelerations.numpy()
        ticks = []
        for _ in range(TICKS):
            e.step()
            ticks.append(snapshot(e))
        e.close()
        _TRAJ[case] = (acc0, ticks)
    return _TRAJ[case]


def make_solo(nb, case, b, acc0, mode=None):
    p, v, m = members(case)
    s = nb.GalaxySimulation(T(p[b]), T(v[b]), T(m[b]), precision_mode=nb.PrecisionMode(mode or MODES[b]), G=G_[b],
                            softening=SOFT[b], dt=DT[b])
    # the constructor's evaluation takes the tiled path and may differ in the last bit: start from the ensemble's
    s.accelerations = T(acc0[b]).clone()
    return s


def solo(nb, case):
    """solo(...)[b][t]: (pos, vel, acc) of member b's GalaxySimulation, in the member's own mode, after t step() calls."""
    if case not in _SOLO:
        acc0 = trajectory(nb, case)[0]
        out = []
        for b in range(B):
            s = make_solo(nb, case, b, acc0)
            states = [(s.positions.numpy(), s.velocities.numpy(), s.accelerations.numpy())]
            for _ in range(SOLO_TICKS):
                s.step()
                assert s.force_kernel_name() == "small_step_kernel"
                states.append((s.positions.numpy(), s.velocities.numpy(), s.accelerations.numpy()))
            s.close()
            out.append(states)
        _SOLO[case] = out
    return _SOLO[case]


def solo_at(nb, case, ticks, order=range(B)):
    """(pos, vel, acc) stacked over the members of `order`, member b after ticks[b] solo steps."""
    ref = solo(nb, case)
    return [np.stack([ref[b][int(t)][k] for b, t in zip(order, ticks)]) for k in range(3)]


# ---- 1. bit identity with the solo engine, driver by driver ---------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_step_loop_is_bit_identical_to_solo(nb, case):
    acc0, ticks = trajectory(nb, case)
    for t in range(TICKS):
        same(ticks[t], solo_at(nb, case, [t + 1] * B), f"tick {t + 1}")
    # the hooks are in force: a cast-mode member does not follow the FLOAT32 run of the same inputs
    for b in (1, 2):
        s = make_solo(nb, case, b, acc0, mode="float32")
        s.step()
        assert not np.array_equal(s.accelerations.numpy(), ticks[0][2][b]), f"member {b} ran without its hook"
        s.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_run_equals_the_step_loop(nb, case):
    _, ticks = trajectory(nb, case)
    e = make_ens(nb, case)
    before = e.launches()
    e.run(TICKS)
    same(snapshot(e), ticks[TICKS - 1], "run(5)")
    assert e.tick == TICKS and e.launches() - before == TICKS
    assert e.force_kernel_name() == "ens_step_mixed_kernel"
    e.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_recorded_and_per_member_runs_are_bit_identical_to_solo(nb, case):
    _, ticks = trajectory(nb, case)
    e = make_ens(nb, case)
    h = e.run_recorded(TICKS, 1)
    same(snapshot(e), ticks[TICKS - 1], "run_recorded(5, 1)")
    assert h.kinetic.shape == (TICKS + 1, B) and bool(torch.isfinite(h.total).all())
    e.close()
    budgets = [5, 3, 0, 4, 1]                            # the instantiation with stops
    e = make_ens(nb, case)
    before = e.launches()
    e.run_members(budgets)
    same(snapshot(e), solo_at(nb, case, budgets), "run_members([5, 3, 0, 4, 1])")
    assert e.member_ticks == budgets and e.launches() - before == 5
    assert e.force_kernel_name() == "ens_step_mixed_kernel"
    e.step()                                             # and on from there, as the solo runs go on
    same(snapshot(e), solo_at(nb, case, [t + 1 for t in budgets]), "run_members, then step()")
    e.close()


@pytest.mark.parametrize("case", CASES[:2] + CASES[4:5], ids=IDS[:2] + IDS[4:5])
def test_watched_runs_leave_every_member_at_a_solo_state(nb, case):
    e = make_ens(nb, case)
    r = e.run_watched(TICKS, check_interval=2)          # budgets round up to 6
    assert (r.stable_ticks <= SOLO_TICKS).all() and (r.stable_ticks[~r.exploded] == SOLO_TICKS).all()
    same(snapshot(e), solo_at(nb, case, r.stable_ticks), "run_watched")
    e.close()
    e = make_ens(nb, case)
    budgets = np.array([5, 4, 5, 2, 5])
    r = e.run_crash_watched(budgets)
    assert ((r.ticks_taken == budgets) | r.crashed).all() and (r.ticks_taken <= budgets).all()
    same(snapshot(e), solo_at(nb, case, r.ticks_taken), "run_crash_watched")
    e.close()


def test_set_params_reaches_every_member(nb):
    case = CASES[1]
    acc0, ticks = trajectory(nb, case)
    e = make_ens(nb, case)
    e.run(2)
    e.set_params(dt=DT2, G=[g * 1.01 for g in G_])
    e.step()
    got = snapshot(e)
    e.close()
    for b in range(B):
        s = make_solo(nb, case, b, acc0)
        s.run(2)
        s.dt, s.G = DT2[b], G_[b] * 1.01
        s.step()
        same([g[b] for g in got], (s.positions.numpy(), s.velocities.numpy(), s.accelerations.numpy()), f"member {b}")
        s.close()


# ---- 2. members are independent -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_permuting_the_members_changes_no_bits(nb, case):
    acc0, ticks = trajectory(nb, case)
    for order in ([4, 3, 2, 1, 0], [2, 0, 4, 1, 3]):     # modes travel with their members
        e = make_ens(nb, case, order)
        assert [m.value for m in e.precision_modes] == [MODES[b] for b in order]
        same([e.accelerations.numpy()], [acc0[order]], f"order {order}, initial")
        for t in range(TICKS):
            e.step()
            same(snapshot(e), [a[order] for a in ticks[t]], f"order {order} tick {t + 1}")
        e.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_nan_member_leaves_the_others_alone(nb, case):
    acc0, ticks = trajectory(nb, case)
    bad = 2
    p = members(case)[0].copy()
    p[bad] = np.nan                                      # the whole member
    e = make_ens(nb, case, pos=p)
    others = [b for b in range(B) if b != bad]
    same([e.accelerations.numpy()[others]], [acc0[others]], "initial")
    for t in range(TICKS):
        e.step()
        got = snapshot(e)
        same([g[others] for g in got], [a[others] for a in ticks[t]], f"tick {t + 1}")
    assert all(np.isnan(g[bad]).all() for g in got)
    e.close()


# ---- 3. energies: the FLOAT32 probe is right for every cast mode ----------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_energies_equal_the_solo_values_in_the_members_own_mode(nb, case):
    e = make_ens(nb, case)
    e.run(2)
    ke, pe, tot = e.get_kinetic_energy(), e.get_potential_energy(), e.get_total_energy()
    pos, vel, mass = e.positions, e.velocities, e.masses
    for b in range(B):
        s = nb.GalaxySimulation(pos[b].clone(), vel[b].clone(), mass[b].clone(), precision_mode=nb.PrecisionMode(MODES[b]),
                                G=G_[b], softening=SOFT[b], dt=DT[b])
        assert ke[b] == s.get_kinetic_energy(), (b, ke[b], s.get_kinetic_energy())
        assert pe[b] == s.get_potential_energy(), (b, pe[b], s.get_potential_energy())
        assert tot[b] == ke[b] + pe[b]
        s.close()
    same(snapshot(e), trajectory(nb, case)[1][1], "state after the energy calls")
    # the batched read-outs see the state alone: a FLOAT32 ensemble holding the same state gives the same values
    u = nb.GalaxyEnsemble(pos, vel, mass, precision_mode=nb.PrecisionMode.FLOAT32, G=G_, softening=SOFT, dt=DT)
    for got, want in zip(e.energies(), u.energies()):
        assert torch.equal(got, want)
    me, mu = e.metrics(num_bins=8), u.metrics(num_bins=8)
    for got, want in zip(me, mu):
        assert np.array_equal(got, want, equal_nan=True)
    assert e.get_state(1)["precision_mode"] == "bfloat16" and e.get_state(3)["precision_mode"] == "float32"
    u.close()
    e.close()


# ---- 4. one launch per tick; the uniform list -----------------------------------------------------------------------------
def test_a_tick_is_one_launch_of_the_mixed_kernel(nb):
    e = make_ens(nb, CASES[1])
    assert e.precision_mode == mode_list(nb) and e.precision_modes == mode_list(nb)
    assert e.force_kernel_name() == "ens_step_mixed_kernel" and e.launches() == 1
    for t in range(3):
        e.step()
        assert e.launches() == 2 + t
    e.run(4)
    assert e.launches() == 8 and e.force_kernel_name() == "ens_step_mixed_kernel"
    e.close()


@pytest.mark.parametrize("mode", ["float32", "bfloat16", "float16"])
def test_an_all_equal_list_is_the_scalar_mode(nb, mode):
    case = CASES[1]
    m = nb.PrecisionMode(mode)
    a, b = make_ens(nb, case, modes=[m] * B), make_ens(nb, case, modes=m)
    assert a.precision_mode == [m] * B and a.precision_modes == b.precision_modes == [m] * B and b.precision_mode == m
    for e in (a, b):
        e.run(3)
        assert e.force_kernel_name() == "ens_step_kernel"
    same(snapshot(a), snapshot(b), mode)
    a.close()
    b.close()


def test_an_all_float64_list_is_the_float64_ensemble(nb):
    ms = [inputs(37, 2, 70 + b, True) for b in range(3)]
    p, v, m = (T(np.stack([x[k] for x in ms])) for k in range(3))
    a = nb.GalaxyEnsemble(p, v, m, precision_mode=[nb.PrecisionMode.FLOAT64] * 3)
    b = nb.GalaxyEnsemble(p, v, m, precision_mode=nb.PrecisionMode.FLOAT64)
    a.run(2)
    b.run(2)
    assert a.force_kernel_name() == "ens_step_kernel" and a.positions.dtype == torch.float64
    assert torch.equal(a.positions, b.positions) and torch.equal(a.velocities, b.velocities)
    a.close()
    b.close()


def test_the_native_constructor_names_a_bad_member(nb):
    import ctypes as C
    from nbody_cosmological_simulation_amd import _native as N
    from nbody_cosmological_simulation_amd.quantization import mode_code
    f32, f64, int8 = (mode_code(nb.PrecisionMode(m)) for m in ("float32", "float64", "int8_sim"))
    ones = (C.c_double * 3)(1.0, 1.0, 1.0)
    for modes, cfg_mode, text in (([f32, f32, f64], f32, "modes[2]"), ([f32, int8, f32], f32, "modes[1]"),
                                  ([f32, f32, f32], f64, "NB_FLOAT32")):
        h = C.c_void_p()
        cfg = N.NbEnsConfig(members=3, n=8, dim=2, mode=cfg_mode, device=0, flags=0)
        rc = N.lib().nb_ens_create_mixed(C.byref(h), C.byref(cfg), (C.c_int32 * 3)(*modes), ones, ones, ones)
        assert rc != 0 and not h.value and text in N.last_error(), N.last_error()
