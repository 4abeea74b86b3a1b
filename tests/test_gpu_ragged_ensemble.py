"""RaggedEnsemble on the GPU: members of different sizes in one launch per tick, every member bit-identical to the solo
GalaxySimulation of its own size and mode through every driver of the tick path.  There is no tolerance anywhere but the
divergence's mean, which takes the rule of test_gpu_ensemble_divergence.

Size sets, deliberately not sorted.  fp32: 2 stars (below one target's lanes), 8 / 9 (one workgroup of targets at 64 lanes
and one star past it), 37, 64 (exactly one stride of sources), 700, 1025 (one star past the 1024-source LDS tile), 2049 (a
solo run switches from 512 to 256 threads there; the ragged launch does not).  fp64: 2049 and 3073 sit behind both solo
switches of the workgroup size, 4096 is the fp64 limit.  [257, 5, 300] runs with 16 and with 32 lanes per target
(NB_SMALL_LANES, read when a handle is created: the ensemble and the solo runs of a case share it).  Every member has its own
G, softening and dt.  Per case the ragged ensemble's step() loop and the solo runs are computed once and shared.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_plan_shapes import inputs

pytestmark = pytest.mark.gpu

TICKS = 5
SOLO_TICKS = 6                         # run_watched rounds a budget of 5 up to 6
SIZES32 = [700, 37, 2049, 2, 1025, 64, 8, 9]
MODES32 = ["float32", "bfloat16", "float16", "float32", "float16", "bfloat16", "float32", "float32"]
SIZES64 = [3073, 37, 2049, 1025, 2, 4096]
SIZES_L = [257, 5, 300]
G_ = [0.001, 0.00113, 0.00091, 0.00127, 0.00107, 0.00097, 0.00119, 0.00103]
SOFT = [0.1, 0.113, 0.087, 0.131, 0.071, 0.093, 0.121, 0.109]
DT = [0.01, 0.0123, 0.0071, 0.0157, 0.0093, 0.0111, 0.0083, 0.0139]
BUDGETS = [5, 0, 3, 1, 5, 2, 4, 5]
BAD = 2                                # the member that holds the NaN: 2049 stars (300 in the lanes cases)

# name -> (sizes, D, modes: one per member, or a string for the uniform handle of that mode, NB_SMALL_LANES or None)
CASES = {
    "mixed-d2": (SIZES32, 2, MODES32, None),
    "mixed-d3": (SIZES32, 3, MODES32, None),
    "f32-d3": (SIZES32, 3, "float32", None),
    "f16-d2": (SIZES32, 2, "float16", None),
    "f64-d2": (SIZES64, 2, "float64", None),
    "f64-d3": (SIZES64, 3, "float64", None),
    "mixed-d2-lanes16": (SIZES_L, 2, ["float32", "float16", "bfloat16"], 16),
    "f64-d3-lanes32": (SIZES_L, 3, "float64", 32),
}
NAMES = list(CASES)


@pytest.fixture(autouse=True)
def lanes_knob(request, monkeypatch):
    case = request.node.callspec.params.get("case") if hasattr(request.node, "callspec") else None
    if case in CASES and CASES[case][3]:
        monkeypatch.setenv("NB_SMALL_LANES", str(CASES[case][3]))


@pytest.fixture(scope="module")
def nb():
    import nbody_cosmological_simulation_amd as pkg
    assert pkg._native.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return pkg


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def member_modes(case):
    sizes, _, modes, _ = CASES[case]
    return list(modes) if isinstance(modes, list) else [modes] * len(sizes)


_MEMBERS = {}


def members(case):
    """Per member (pos, vel, mass) as numpy arrays; member 3 (where there is one) has uniform masses."""
    if case not in _MEMBERS:
        sizes, d, modes, _ = CASES[case]
        _MEMBERS[case] = [inputs(n, d, 3000 + 17 * b, modes == "float64", uniform=(b == 3)) for b, n in enumerate(sizes)]
    return _MEMBERS[case]


def make_ens(nb, case, order=None, pos=None):
    sizes, d, modes, _ = CASES[case]
    idx = list(range(len(sizes))) if order is None else list(order)
    ms = members(case)
    p = [ms[b][0] for b in idx] if pos is None else [pos[b] for b in idx]
    mode = [nb.PrecisionMode(modes[b]) for b in idx] if isinstance(modes, list) else nb.PrecisionMode(modes)
    e = nb.RaggedEnsemble([T(x) for x in p], [T(ms[b][1]) for b in idx], [T(ms[b][2]) for b in idx], precision_mode=mode,
                          G=[G_[b] for b in idx], softening=[SOFT[b] for b in idx], dt=[DT[b] for b in idx])
    assert e.num_stars == [sizes[b] for b in idx] and e.num_members == len(idx)
    return e


def snapshot(e):
    return tuple([t.numpy() for t in getattr(e, name)] for name in ("positions", "velocities", "accelerations"))


def same(got, want, what, only=None):
    """Two snapshots (or lists of per-member arrays per kind), member by member, bit for bit."""
    for name, g, w in zip(("positions", "velocities", "accelerations"), got, want):
        assert len(g) == len(w), (what, name)
        for b, (x, y) in enumerate(zip(g, w)):
            if only is not None and b not in only:
                continue
            assert x.dtype == y.dtype and x.shape == y.shape, (what, name, b, x.dtype, y.dtype, x.shape, y.shape)
            assert np.array_equal(x, y, equal_nan=True), f"{what}: {name} of member {b} differ"


def pick(snap, order):
    return tuple([kind[b] for b in order] for kind in snap)


_TRAJ, _SOLO = {}, {}


def trajectory(nb, case):
    """Initial accelerations and the state after each of TICKS step() calls of the ragged ensemble."""
    if case not in _TRAJ:
        e = make_ens(nb, case)
        assert e.force_kernel_name() == "ens_step_ragged_kernel"
        acc0 = [t.numpy() for t in e.accelerations]
        ticks = []
        for _ in range(TICKS):
            e.step()
            ticks.append(snapshot(e))
        e.close()
        _TRAJ[case] = (acc0, ticks)
    return _TRAJ[case]


def make_solo(nb, case, b, acc0, mode=None):
    p, v, m = members(case)[b]
    s = nb.GalaxySimulation(T(p), T(v), T(m), precision_mode=nb.PrecisionMode(mode or member_modes(case)[b]), G=G_[b],
                            softening=SOFT[b], dt=DT[b])
    # the constructor's evaluation takes the tiled path and may differ in the last bit: start from the ensemble's
    s.accelerations = T(acc0[b]).clone()
    return s


def solo(nb, case):
    """solo(...)[b][t]: (pos, vel, acc) of member b's GalaxySimulation, in the member's own mode, after t step() calls."""
    if case not in _SOLO:
        acc0 = trajectory(nb, case)[0]
        out = []
        for b in range(len(CASES[case][0])):
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


def solo_at(nb, case, ticks, order=None):
    """A snapshot made of the solo runs: member b after ticks[b] solo steps."""
    ref = solo(nb, case)
    order = range(len(ref)) if order is None else order
    return tuple([ref[b][int(t)][k] for b, t in zip(order, ticks)] for k in range(3))


# ---- 1. bit identity with the solo engine, driver by driver ---------------------------------------------------------------
@pytest.mark.parametrize("case", NAMES)
def test_step_loop_is_bit_identical_to_solo(nb, case):
    acc0, ticks = trajectory(nb, case)
    B = len(acc0)
    for t in range(TICKS):
        same(ticks[t], solo_at(nb, case, [t + 1] * B), f"tick {t + 1}")
    # the hooks are in force: a cast-mode member does not follow the FLOAT32 run of the same inputs
    for b, mode in enumerate(member_modes(case)):
        if mode in ("bfloat16", "float16") and CASES[case][0][b] >= 37:
            s = make_solo(nb, case, b, acc0, mode="float32")
            s.step()
            assert not np.array_equal(s.accelerations.numpy(), ticks[0][2][b]), f"member {b} ran without its hook"
            s.close()


@pytest.mark.parametrize("case", NAMES)
def test_run_equals_the_step_loop_and_is_one_launch_per_tick(nb, case):
    _, ticks = trajectory(nb, case)
    e = make_ens(nb, case)
    assert e.launches() == 1 and e.force_kernel_name() == "ens_step_ragged_kernel"
    e.run(TICKS)
    same(snapshot(e), ticks[TICKS - 1], "run(5)")
    assert e.tick == TICKS and e.launches() == 1 + TICKS
    for t in range(3):
        e.step()
        assert e.launches() == 2 + TICKS + t
    assert e.force_kernel_name() == "ens_step_ragged_kernel"
    e.close()


@pytest.mark.parametrize("case", NAMES)
def test_recorded_and_per_member_runs_are_bit_identical_to_solo(nb, case):
    _, ticks = trajectory(nb, case)
    B = len(CASES[case][0])
    e = make_ens(nb, case)
    h = e.run_recorded(TICKS, 1)
    same(snapshot(e), ticks[TICKS - 1], "run_recorded(5, 1)")
    assert h.kinetic.shape == (TICKS + 1, B) and bool(torch.isfinite(h.total).all())
    e.close()
    budgets = BUDGETS[:B]                                # the instantiations with stops
    e = make_ens(nb, case)
    before = e.launches()
    e.run_members(budgets)
    same(snapshot(e), solo_at(nb, case, budgets), f"run_members({budgets})")
    assert e.member_ticks == budgets and e.launches() - before == max(budgets)
    assert e.force_kernel_name() == "ens_step_ragged_kernel"
    e.step()                                             # and on from there, as the solo runs go on
    same(snapshot(e), solo_at(nb, case, [t + 1 for t in budgets]), "run_members, then step()")
    e.close()


@pytest.mark.parametrize("case", ["mixed-d2", "f64-d3", "mixed-d2-lanes16"])
def test_watched_runs_leave_every_member_at_a_solo_state(nb, case):
    e = make_ens(nb, case)
    r = e.run_watched(TICKS, check_interval=2)          # budgets round up to 6
    assert (r.stable_ticks <= SOLO_TICKS).all() and (r.stable_ticks[~r.exploded] == SOLO_TICKS).all()
    same(snapshot(e), solo_at(nb, case, r.stable_ticks), "run_watched")
    e.close()


# ---- 2. energies: a member's are those of an ensemble that holds it alone ---------------------------------------------------
@pytest.mark.parametrize("case", NAMES)
def test_energies_equal_a_one_member_ensemble_of_the_same_system(nb, case):
    _, ticks = trajectory(nb, case)
    e = make_ens(nb, case)
    h = e.run_recorded(TICKS, 1)
    ke, pe = e.energies()
    assert torch.equal(ke, h.kinetic[-1]) and torch.equal(pe, h.potential[-1])
    # the list getters are the batched values
    assert e.get_kinetic_energy() == ke.tolist() and e.get_potential_energy() == pe.tolist()
    assert e.get_total_energy() == [k + p for k, p in zip(ke.tolist(), pe.tolist())]
    same(snapshot(e), ticks[TICKS - 1], "state after the energy calls")
    e.close()
    for b, (p, v, m) in enumerate(members(case)):
        u = nb.GalaxyEnsemble(T(p)[None], T(v)[None], T(m)[None], precision_mode=nb.PrecisionMode(member_modes(case)[b]),
                              G=[G_[b]], softening=[SOFT[b]], dt=[DT[b]])
        hu = u.run_recorded(TICKS, 1)
        assert torch.equal(hu.kinetic[:, 0], h.kinetic[:, b]), (b, hu.kinetic[:, 0], h.kinetic[:, b])
        assert torch.equal(hu.potential[:, 0], h.potential[:, b]), (b, hu.potential[:, 0], h.potential[:, b])
        uk, up = u.energies()
        assert float(uk[0]) == float(ke[b]) and float(up[0]) == float(pe[b])
        # ... and so is the trajectory: one workgroup size serves every size
        for name, k in (("positions", 0), ("velocities", 1), ("accelerations", 2)):
            assert np.array_equal(getattr(u, name)[0].numpy(), ticks[TICKS - 1][k][b]), (name, b)
        u.close()


# ---- 3. members are independent ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NAMES)
def test_permuting_the_members_changes_no_bits(nb, case):
    acc0, ticks = trajectory(nb, case)
    B = len(acc0)
    shuffled = [(5 * b + 3) % B for b in range(B)] if B == 8 else [(b + 2) % B for b in range(B)]
    for order in (list(range(B))[::-1], shuffled):       # the work list's order follows the permutation
        assert sorted(order) == list(range(B))
        e = make_ens(nb, case, order)
        same(([t.numpy() for t in e.accelerations],), ([acc0[b] for b in order],), f"order {order}, initial")
        for t in range(TICKS):
            e.step()
            same(snapshot(e), pick(ticks[t], order), f"order {order} tick {t + 1}")
        e.close()


@pytest.mark.parametrize("case", NAMES)
def test_a_nan_member_leaves_the_others_alone(nb, case):
    acc0, ticks = trajectory(nb, case)
    B = len(acc0)
    p = [m[0].copy() for m in members(case)]
    p[BAD][:] = np.nan                                   # the whole member
    e = make_ens(nb, case, pos=p)
    others = [b for b in range(B) if b != BAD]
    same(([t.numpy() for t in e.accelerations],), (acc0,), "initial", only=others)
    for t in range(TICKS):
        e.step()
        got = snapshot(e)
        same(got, ticks[t], f"tick {t + 1}", only=others)
    assert all(np.isnan(kind[BAD]).all() for kind in got)
    e.close()


# ---- 4. the padding is nobody's ---------------------------------------------------------------------------------------------
def raw(e, name):
    """The handle's whole padded array through nb_ens_get_state."""
    from nbody_cosmological_simulation_amd import _native as N
    out = torch.empty(e._shape(name), dtype=e._dtype)
    args = [None, None, None, None]
    args[{"positions": 0, "velocities": 1, "accelerations": 2, "masses": 3}[name]] = C.c_void_p(out.data_ptr())
    N.check(N.lib().nb_ens_get_state(e._handle, *args, 0))
    return out


def drive(e, B):
    """Every driver of the tick path and every read-out, in a fixed order."""
    e.step()
    e.run(2)
    e.run_members(BUDGETS[:B])
    e.run_recorded(2, 1)
    e.run_watched(2, check_interval=1)
    e.run_diverged(2, 1, baseline=list(range(B)))
    e.divergence(list(range(B)))
    return e.energies() + (torch.tensor(e.get_kinetic_energy()), torch.tensor(e.get_potential_energy()))


@pytest.mark.parametrize("case", NAMES)
def test_no_kernel_touches_the_padding(nb, case):
    from nbody_cosmological_simulation_amd import _native as N
    from nbody_cosmological_simulation_amd.quantization import _TORCH_TO_NB
    sizes = CASES[case][0]
    B = len(sizes)
    a, b = make_ens(nb, case), make_ens(nb, case)
    for e in (a, b):
        drive(e, B)
    same(snapshot(a), snapshot(b), "the drivers are deterministic")
    full = {name: raw(a, name) for name in ("positions", "velocities", "accelerations", "masses")}
    pad = torch.zeros(B, max(sizes), dtype=torch.bool)
    for m, n in enumerate(sizes):
        pad[m, n:] = True
    assert int(pad.sum()) == B * max(sizes) - sum(sizes) > 0
    for name in ("positions", "velocities", "masses"):
        assert bool(torch.isnan(full[name][pad]).all()), f"{name}: a padding row was written"
        assert not bool(torch.isnan(full[name][~pad]).any()), name
    assert bool((full["accelerations"][pad] == 0).all()), "accelerations: a padding row was written"
    # finite junk in every padding row of `a`: nobody reads it
    g = torch.Generator().manual_seed(3)
    for name in full:
        junk = (torch.rand(full[name].shape, generator=g, dtype=torch.float64) * 7 + 0.25).to(full[name].dtype)
        full[name][pad] = junk[pad]
    N.check(N.lib().nb_ens_set_state(a._handle, C.c_void_p(full["positions"].data_ptr()), C.c_void_p(full["velocities"].data_ptr()),
                                     C.c_void_p(full["masses"].data_ptr()), _TORCH_TO_NB[a._dtype], 0))
    N.check(N.lib().nb_ens_set_accelerations(a._handle, C.c_void_p(full["accelerations"].data_ptr()), _TORCH_TO_NB[a._dtype], 0))
    same(snapshot(a), snapshot(b), "the upload kept the members' rows")
    ea, eb = drive(a, B), drive(b, B)
    same(snapshot(a), snapshot(b), "junk in the padding changed a member")
    for x, y in zip(ea, eb):
        assert torch.equal(x, y), "junk in the padding changed an energy"
    for name in full:
        after = raw(a, name)
        assert torch.equal(after[pad], full[name][pad]), f"{name}: a padding row was written"
    a.close()
    b.close()


# ---- 5. equal sizes: the uniform ensemble -----------------------------------------------------------------------------------
@pytest.mark.parametrize("modes", ["float32", ["float32", "bfloat16", "float16", "float32"]], ids=["uniform", "mixed"])
def test_equal_sizes_are_the_galaxy_ensemble(nb, modes):
    ms = [inputs(700, 3, 4100 + b, False) for b in range(4)]
    mode = [nb.PrecisionMode(m) for m in modes] if isinstance(modes, list) else nb.PrecisionMode(modes)
    kw = dict(precision_mode=mode, G=G_[:4], softening=SOFT[:4], dt=DT[:4])
    r = nb.RaggedEnsemble([T(m[0]) for m in ms], [T(m[1]) for m in ms], [T(m[2]) for m in ms], **kw)
    g = nb.GalaxyEnsemble(*(T(np.stack([m[k] for m in ms])) for k in range(3)), **kw)
    assert r.num_stars == [700] * 4 and g.force_kernel_name() in ("ens_step_kernel", "ens_step_mixed_kernel")
    assert torch.equal(torch.stack(r.accelerations), g.accelerations)
    for e in (r, g):
        e.run(3)
        e.step()
    hr, hg = r.run_recorded(2, 1), g.run_recorded(2, 1)
    for name in ("positions", "velocities", "accelerations", "masses"):
        assert torch.equal(torch.stack(getattr(r, name)), getattr(g, name)), name
    assert torch.equal(hr.kinetic, hg.kinetic) and torch.equal(hr.potential, hg.potential)
    assert r.get_state(2)["positions"].shape == (700, 3) and r.get_state(2)["tick"] == 6
    r.close()
    g.close()


# ---- 6. divergence ------------------------------------------------------------------------------------------------------------
DSIZES = [700, 700, 37, 37, 1025, 1025]
DBASE = [0, 0, 2, 2, 4, 4]


def pairs(nb, f64, d=3):
    """Pairs of equal size and parameters; the second of a pair is the first with positions[0, 0] one ulp up."""
    ms = []
    for b, n in enumerate(DSIZES):
        p, v, m = inputs(n, d, 5000 + DBASE[b], f64)
        if b != DBASE[b]:
            p = p.copy()
            p[0, 0] = np.nextafter(p[0, 0], p.dtype.type(np.inf))
        ms.append((p, v, m))
    mode = nb.PrecisionMode.FLOAT64 if f64 else [nb.PrecisionMode(m) for m in ("float32", "float32", "float16", "float16",
                                                                               "bfloat16", "bfloat16")]
    return nb.RaggedEnsemble([T(m[0]) for m in ms], [T(m[1]) for m in ms], [T(m[2]) for m in ms], precision_mode=mode,
                             G=[G_[b] for b in DBASE], softening=[SOFT[b] for b in DBASE], dt=[DT[b] * 4 for b in DBASE])


def check_divergence(got, e, what):
    """got: (max_position, mean_position, max_velocity) rows of B values, against torch on the downloaded members."""
    pos, vel = e.positions, e.velocities
    fp32 = pos[0].dtype == torch.float32
    for b, base in enumerate(DBASE):
        dp, dv = (pos[b] - pos[base]).abs(), (vel[b] - vel[base]).abs()
        mean64 = float(dp.numpy().astype(np.float64).mean())
        g_mp, g_mean, g_mv = (float(t[b]) for t in got)
        print(f"{what} member {b} vs {base}: max_pos {g_mp:.9g} mean {g_mean:.17g} (numpy {mean64:.17g}) max_vel {g_mv:.9g}")
        assert g_mp == float(dp.max().double()), (what, b, g_mp, float(dp.max()))
        assert g_mv == float(dv.max().double()), (what, b, g_mv, float(dv.max()))
        if mean64 == 0.0:
            assert g_mean == 0.0, (what, b, g_mean)
        else:
            assert abs(g_mean - mean64) <= 1e-12 * mean64, (what, b, g_mean, mean64)
            if fp32:
                assert abs(g_mean - float(dp.mean().double())) <= 2e-6 * mean64, (what, b, g_mean, float(dp.mean()))


@pytest.mark.parametrize("f64", [False, True], ids=["mixed", "float64"])
def test_divergence_sample_by_sample(nb, f64):
    e, ref = pairs(nb, f64), pairs(nb, f64)
    check_divergence(e.divergence(DBASE), e, "divergence at entry")
    h = e.run_diverged(TICKS, 1, DBASE)
    assert h.max_position.shape == (TICKS + 1, 6) and h.ticks == list(range(TICKS + 1)) and h.energy is not None
    grew = False
    for s in range(TICKS + 1):
        check_divergence((h.max_position[s], h.mean_position[s], h.max_velocity[s]), ref, f"sample {s}")
        grew = grew or float(h.max_position[s][1]) > 0
        if s < TICKS:
            ref.step()
    assert grew, "the perturbed member never left its twin"
    assert all(float(h.max_position[s][b]) == 0.0 for s in range(TICKS + 1) for b in (0, 2, 4))
    same(snapshot(e), snapshot(ref), "run_diverged leaves run()'s trajectory")
    hr = ref.energies()
    assert torch.equal(h.energy.kinetic[-1], hr[0]) and torch.equal(h.energy.potential[-1], hr[1])
    check_divergence(e.divergence(DBASE), e, "divergence after the run")
    e.close()
    ref.close()


def test_the_native_refusals(nb):
    from nbody_cosmological_simulation_amd import _native as N
    lib = N.lib()
    e = pairs(nb, False, d=2)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    for base in ((0, 0, 0, 2, 4, 4), (1, 0, 3, 2, 5, 2)):
        rc = lib.nb_ens_divergence(e._handle, i32(*base), None, None, None, 0)
        assert rc == -1 and "stars" in N.last_error() and "member" in N.last_error(), (base, rc, N.last_error())
    got = C.c_int32(-1)
    rc = lib.nb_ens_run_diverged(e._handle, 2, 1, i32(0, 0, 2, 2, 4, 0), 0, None, None, None, None, None, 3, 0, C.byref(got))
    assert rc == -1 and got.value == 0 and "member 5 has 1025 stars and member 0 has 700" in N.last_error(), N.last_error()
    assert lib.nb_ens_divergence(e._handle, i32(*DBASE), None, None, None, 0) == 0
    out = (C.c_double * 48)()
    refused = {
        "nb_ens_metrics": lambda: lib.nb_ens_metrics(e._handle, 8, None, 90.0, None, None, None, None),
        "nb_ens_crash_measures": lambda: lib.nb_ens_crash_measures(e._handle, None, 0, None, None),
        "nb_ens_run_crash_watched": lambda: lib.nb_ens_run_crash_watched(e._handle, i32(1, 1, 1, 1, 1, 1), None, None, 0, 0, None,
                                                                         None, None, None, None),
        "nb_ens_quant_info": lambda: lib.nb_ens_quant_info(e._handle, out),
        "nb_ens_quant_bin_sums": lambda: lib.nb_ens_quant_bin_sums(e._handle, None, None, None),
    }
    for name, call in refused.items():
        rc = call()
        assert rc == -5 and name in N.last_error() and "follow-up" in N.last_error(), (name, rc, N.last_error())
    assert e.tick == 0 and e.launches() == 1             # nothing ran
    with pytest.raises(ValueError, match="stars against"):
        e.divergence(0)
    with pytest.raises(NotImplementedError):
        e.metrics()
    e.close()
