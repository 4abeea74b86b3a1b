"""FineGridEnsemble on the GPU: CUSTOM members of up to 4096 grid levels in one force launch per tick.

The setup is test_gpu_quantized_ensemble's: B = 5 members, the clustered-core-plus-halo inputs of test_gpu_plan_shapes with
one seed per member, per-member G / softening / dt, dt changed after the second tick.  LEVELS gives member 0 a table-free
grid inside a wide launch (16), member 1 one level past the single-block tables (257), member 2 a table padded to 512
(300), member 3 a chunk boundary of the tables build (1024) and member 4 the limit (4096).

What is asserted follows the contract in ensemble.py.  Member 0 is bit-identical to its solo one-launch run.  A member above
256 levels has its solo run's tables and the reference's bins, exactly; its sums are deterministic and independent of its
neighbours, exactly; against the solo engine (whose tiled path sums in another order) and the oracle its forces and
trajectories are held to the suite's bars: 2e-6 on the initial accelerations, and max(2e-6, 2 x the solo run's own distance
from the same OracleSim) on positions and velocities after five ticks -- the factor 2 because a single bin flip is a
one-off jump that either run may take.
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_plan_shapes import inputs, relerr
from test_gpu_ensemble import B, TICKS, G_, SOFT, DT, DT2, UNIFORM_MEMBER, T, same, solo_state, snapshot, drive_steps
from test_gpu_bins import checksums

pytestmark = pytest.mark.gpu

LEVELS = [16, 257, 300, 1024, 4096]
FINE = [b for b in range(B) if LEVELS[b] > 256]
ORACLE_LOOP_MAX = 1025                  # OracleSim loops stay at or below this N
ROWS = 600                              # rows of the oracle's bin matrix above it

# (N, D): 37 fewer pairs than bins, one partial workgroup; 1025 one star past the 1024-source LDS tile; 2049 the workgroup
# switches 512 -> 256; 3072 the limit (FIRST_ONLY: the constructor's evaluation alone)
CASES = [(37, 2), (37, 3), (1025, 2), (2049, 3), (3072, 2)]
FIRST_ONLY = {(3072, 2)}
# 16 / 32 lanes per target instead of the default 64 (NB_SMALL_LANES, read when a handle is created)
LANES = {(257, 2): 16, (257, 3): 32}
CASES += list(LANES)
IDS = [f"n{n}-d{d}" + (f"-lanes{LANES[n, d]}" if (n, d) in LANES else "") for n, d in CASES]
STEPPED = [c for c in CASES if c not in FIRST_ONLY]
STEPPED_IDS = [IDS[CASES.index(c)] for c in STEPPED]
EDGE_CASES = [(37, 3), (257, 2), (1025, 2)]
EDGE_IDS = [IDS[CASES.index(c)] for c in EDGE_CASES]
TABLE_KEYS = ("lmin", "lmax", "r2max", "fast_path")


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


@functools.lru_cache(maxsize=None)
def members(case):
    """Initial (B, N, D) positions, velocities and (B, N) masses of a case (numpy float32)."""
    n, d = case
    ms = [inputs(n, d, 1000 + 17 * b, False, uniform=(b == UNIFORM_MEMBER)) for b in range(B)]
    return tuple(np.stack([m[k] for m in ms]) for k in range(3))


def make_ens(nb, case, order=range(B), pos=None, soft=SOFT, dt=DT, cls=None, levels=LEVELS):
    p, v, m = members(case)
    idx = list(order)
    p = p if pos is None else pos
    kw = dict(G=[G_[b] for b in idx], softening=[soft[b] for b in idx], dt=[dt[b] for b in idx])
    if cls is not None:
        return cls(T(p[idx]), T(v[idx]), T(m[idx]), precision_mode=nb.PrecisionMode.CUSTOM,
                   custom_levels=[levels[b] for b in idx], **kw)
    return nb.FineGridEnsemble(T(p[idx]), T(v[idx]), T(m[idx]), custom_levels=[levels[b] for b in idx], **kw)


def make_solo(nb, case, b, pos=None, soft=SOFT):
    p, v, m = members(case)
    p = p if pos is None else pos
    return nb.GalaxySimulation(T(p[b]), T(v[b]), T(m[b]), precision_mode=nb.PrecisionMode.CUSTOM, custom_levels=LEVELS[b],
                               G=G_[b], softening=soft[b], dt=DT[b])


_TRAJ = {}


def trajectory(nb, case):
    """The shared reference of a case, computed once and never modified: initial accelerations, quant_debug() after the
    constructor, the state after every tick of the B = 5 ensemble driven with step() (None for a FIRST_ONLY case),
    quant_debug() after the last tick.  No read-out is called on the way."""
    if case not in _TRAJ:
        e = make_ens(nb, case)
        acc0 = e.accelerations.numpy()
        dbg0 = e.quant_debug()
        assert e.force_kernel_name() == "ens_grid_step_wide_kernel"
        assert list(dbg0["levels"]) == LEVELS == e.levels
        ticks = dbg5 = None
        if case not in FIRST_ONLY:
            before = e.launches()
            ticks = drive_steps(e)
            assert e.launches() - before == TICKS and e.force_kernel_name() == "ens_grid_step_wide_kernel"
            dbg5 = e.quant_debug()
        e.close()
        _TRAJ[case] = (acc0, ticks, dbg0, dbg5)
    return _TRAJ[case]


def oracle_sums(case, b, pos, soft=SOFT):
    """(rows, s1, s2): the check-sums of the first `rows` rows of the oracle's bin matrix of member b at positions pos."""
    from oracle import oracle as O
    n = case[0]
    m = members(case)[2]
    kw = dict(G=G_[b], softening=soft[b], levels=LEVELS[b])
    if n <= ORACLE_LOOP_MAX:
        k = O.accelerations(pos, m[b], "custom", debug=True, **kw)[1]["d2bins"]
    else:
        k = O.accelerations_rows(pos, m[b], "custom", 0, ROWS, bins=True, **kw)[1]["d2bins"]
    return (k.shape[0],) + checksums(k)


def check_bins(nb, case, got, pos, what, soft=SOFT, who=range(B)):
    """quant_bin_sums() of an ensemble at positions pos (B, N, D): exact against the oracle and the solo tiled read-out."""
    n = case[0]
    assert got["sum_k"].shape == got["sum_kw"].shape == (B, n) and got["sum_k"].dtype == np.int64
    assert list(got["levels"]) == LEVELS
    for b in who:
        rows, s1, s2 = oracle_sums(case, b, pos[b], soft)
        assert np.array_equal(got["sum_k"][b, :rows], s1), f"{what}: sum_k of member {b} ({LEVELS[b]} levels) vs the oracle"
        assert np.array_equal(got["sum_kw"][b, :rows], s2), f"{what}: sum_kw of member {b} ({LEVELS[b]} levels) vs the oracle"
        s = make_solo(nb, case, b, soft=soft)
        s.positions = T(pos[b]).clone()
        solo = s.quant_bin_sums("tiled")
        s.close()
        assert np.array_equal(got["sum_k"][b], solo["sum_k"]), f"{what}: sum_k of member {b} vs the solo tiled read-out"
        assert np.array_equal(got["sum_kw"][b], solo["sum_kw"]), f"{what}: sum_kw of member {b} vs the solo tiled read-out"
        assert got["pairs_table_free"][b] + got["pairs_table"][b] == n * n, (what, b)      # every pair once, no padding
        if LEVELS[b] > 256:
            assert got["pairs_table_free"][b] == 0, f"{what}: member {b} took the table-free route"


# ---- 1. which kernel runs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_member_above_256_levels_selects_the_wide_kernel(nb, case):
    trajectory(nb, case)                # asserts the name after the constructor and after the ticks


@pytest.mark.parametrize("case", [(257, 2), (1025, 2)], ids=["n257-d2-lanes16", "n1025-d2"])
def test_up_to_256_levels_it_is_quantized_ensembles_launch(nb, case):
    lv = [16, 64, 256, 2, 3]
    f = make_ens(nb, case, range(3), levels=lv)
    q = make_ens(nb, case, range(3), levels=lv, cls=nb.QuantizedEnsemble)
    assert f.force_kernel_name() == q.force_kernel_name() == "ens_grid_step_kernel"
    same(snapshot(f), snapshot(q), "after the constructors")
    for t, (a, b_) in enumerate(zip(drive_steps(f, range(3)), drive_steps(q, range(3)))):
        same(a, b_, f"tick {t + 1}")
    assert f.force_kernel_name() == "ens_grid_step_kernel" and f.launches() == q.launches() == 1 + TICKS
    fd, qd = f.quant_debug(), q.quant_debug()
    for key in TABLE_KEYS:
        assert np.array_equal(fd[key], qd[key], equal_nan=True), key
    fb, qb = f.quant_bin_sums(), q.quant_bin_sums()
    for key in ("sum_k", "sum_kw", "pairs_table_free", "pairs_table"):
        assert np.array_equal(fb[key], qb[key]), key
    pos5, m = f.positions.numpy(), members(case)[2]
    f.close()
    q.close()
    # the narrow read-out against the oracle's bin matrix at the positions after the ticks
    from oracle import oracle as O
    for b in range(3):
        k = O.accelerations(pos5[b], m[b], "custom", debug=True, G=G_[b], softening=SOFT[b], levels=lv[b])[1]["d2bins"]
        s1, s2 = checksums(k)
        assert np.array_equal(qb["sum_k"][b], s1) and np.array_equal(qb["sum_kw"][b], s2), f"member {b} ({lv[b]} levels)"
        assert qb["pairs_table_free"][b] + qb["pairs_table"][b] == case[0] ** 2


@pytest.mark.parametrize("mode,levels", [("int8_sim", 256), ("int4_sim", 16)])
def test_the_read_out_serves_the_other_grid_modes(nb, mode, levels):
    """quant_bin_sums() on an INT8 / INT4 QuantizedEnsemble: the oracle's bins, and state and force bounds untouched."""
    from oracle import oracle as O
    case = (257, 3)
    p, v, m = members(case)
    e = nb.QuantizedEnsemble(T(p), T(v), T(m), precision_mode=nb.PrecisionMode(mode), G=G_, softening=SOFT, dt=DT)
    e.run(2)
    before, dbg, launches = snapshot(e), e.quant_debug(), e.launches()
    got = e.quant_bin_sums()
    same(snapshot(e), before, "after the read-out")
    after = e.quant_debug()
    for key in TABLE_KEYS + ("fmin", "fmax"):
        assert np.array_equal(after[key], dbg[key], equal_nan=True), key
    assert e.launches() == launches and e.tick == 2 and list(got["levels"]) == [levels] * B
    for b in range(B):
        k = O.accelerations(before[0][b], m[b], mode, debug=True, G=G_[b], softening=SOFT[b])[1]["d2bins"]
        s1, s2 = checksums(k)
        assert np.array_equal(got["sum_k"][b], s1) and np.array_equal(got["sum_kw"][b], s2), f"member {b}"
    e.run(1)
    r = nb.QuantizedEnsemble(T(p), T(v), T(m), precision_mode=nb.PrecisionMode(mode), G=G_, softening=SOFT, dt=DT)
    r.run(3)
    same(snapshot(e), snapshot(r), "run(2) + read-out + run(1) vs run(3)")
    e.close()
    r.close()


# ---- 2. the member of up to 256 levels inside a wide launch ------------------------------------------------------------------
@pytest.mark.parametrize("case", STEPPED, ids=STEPPED_IDS)
def test_the_16_level_member_is_bit_identical_to_its_solo_one_launch_run(nb, case):
    acc0, ticks, dbg0, dbg5 = trajectory(nb, case)
    b = 0
    s = make_solo(nb, case, b)
    solo0 = s.quant_debug()
    for key in TABLE_KEYS:
        assert dbg0[key][b] == solo0[key], f"after the constructor: {key}: ensemble {dbg0[key][b]!r}, solo {solo0[key]!r}"
    # the solo constructor evaluates on the tiled path, whose sums may differ in the last bit: start from the ensemble's
    s.accelerations = T(acc0[b]).clone()
    for t in range(TICKS):
        if t == 2:
            s.dt = DT2[b]
        s.step()
        same(solo_state(s), [a[b] for a in ticks[t]], f"member {b} tick {t + 1}")
        assert s.force_kernel_name() == "small_step_kernel"
    solo5 = s.quant_debug()
    for key in TABLE_KEYS:
        assert dbg5[key][b] == solo5[key], f"after tick {TICKS}: {key}: ensemble {dbg5[key][b]!r}, solo {solo5[key]!r}"
    s.close()


# ---- 3. tables, 5. forces ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tables_are_the_solo_runs_and_initial_forces_meet_the_bar(nb, case):
    from oracle import oracle as O
    n, d = case
    acc0, _, dbg0, _ = trajectory(nb, case)
    p, v, m = members(case)
    tag = IDS[CASES.index(case)]
    for b in range(B):
        L = LEVELS[b]
        kw = dict(G=G_[b], softening=SOFT[b], levels=L)
        ref = O.accelerations(p[b], m[b], "custom", force_quant=False, **kw)
        err = relerr(acc0[b].astype(np.float64), ref)
        s = make_solo(nb, case, b)
        solo_dbg, solo_acc = s.quant_debug(), s.accelerations.numpy()
        s.close()
        amax = np.float32(np.abs(acc0[b]).max())
        ulps = float(np.abs(acc0[b].astype(np.float64) - solo_acc.astype(np.float64)).max() / np.spacing(amax))
        print(f"{tag} member {b} ({L} levels): initial accelerations relerr {err:.3e} vs the oracle; {ulps:.2f} fp32 ulps of "
              f"max |a| from the solo constructor's")
        assert err < 2e-6, (b, err)
        if L <= 256:
            continue
        for key in ("lmin", "lmax", "r2max"):
            assert dbg0[key][b] == solo_dbg[key], f"{key} of member {b}: ensemble {dbg0[key][b]!r}, solo {solo_dbg[key]!r}"
        assert not dbg0["fast_path"][b] and not solo_dbg["fast_path"], (b, dbg0["fast_path"][b], solo_dbg["fast_path"])
        _, rdbg = O.accelerations_rows(p[b], m[b], "custom", 0, min(n, ROWS), bins=False, **kw)
        assert np.float32(dbg0["lmin"][b]) == np.float32(rdbg["lmin"]), (b, dbg0["lmin"][b], rdbg["lmin"])
        assert np.float32(dbg0["lmax"][b]) == np.float32(rdbg["lmax"]), (b, dbg0["lmax"][b], rdbg["lmax"])


@pytest.mark.parametrize("case", STEPPED, ids=STEPPED_IDS)
def test_tables_after_the_ticks_are_the_solo_runs(nb, case):
    """A solo handle set to the member's positions after tick 5 builds, in its constructor, the tables the member holds."""
    _, ticks, _, dbg5 = trajectory(nb, case)
    pos5 = ticks[TICKS - 1][0]
    for b in FINE:
        s = make_solo(nb, case, b, pos=pos5)
        solo = s.quant_debug()
        s.close()
        for key in ("lmin", "lmax", "r2max"):
            assert dbg5[key][b] == solo[key], f"{key} of member {b}: ensemble {dbg5[key][b]!r}, solo {solo[key]!r}"
        assert not dbg5["fast_path"][b]


# ---- 4. bins -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bins_are_the_references_and_the_read_out_is_an_observer(nb, case):
    acc0, ticks, dbg0, dbg5 = trajectory(nb, case)
    p = members(case)[0]
    e = make_ens(nb, case)
    before = e.launches()
    got = e.quant_bin_sums()
    assert e.launches() == before and e.tick == 0
    same(snapshot(e), (p, members(case)[1], acc0), "after the read-out behind the constructor")
    dbg = e.quant_debug()
    for key in TABLE_KEYS:
        assert np.array_equal(dbg[key], dbg0[key], equal_nan=True), f"quant_debug()[{key!r}] after the read-out"
    check_bins(nb, case, got, p, "after the constructor")
    if case in FIRST_ONLY:
        e.close()
        return
    for t in range(TICKS):
        if t == 2:
            e.set_params(dt=DT2)
        e.step()
        mid = e.quant_bin_sums()
        same(snapshot(e), ticks[t], f"tick {t + 1} with a read-out after every tick")
    assert e.launches() - before == TICKS and e.tick == TICKS
    dbg = e.quant_debug()
    for key in TABLE_KEYS:
        assert np.array_equal(dbg[key], dbg5[key], equal_nan=True), f"quant_debug()[{key!r}] after tick {TICKS} and read-outs"
    e.close()
    check_bins(nb, case, mid, ticks[TICKS - 1][0], f"after tick {TICKS}")


# ---- 6. trajectories -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in STEPPED if c[0] <= ORACLE_LOOP_MAX],
                         ids=[IDS[CASES.index(c)] for c in STEPPED if c[0] <= ORACLE_LOOP_MAX])
def test_trajectories_stay_as_close_to_the_oracle_as_the_solo_run(nb, case):
    from oracle import oracle as O
    _, ticks, _, _ = trajectory(nb, case)
    p, v, m = members(case)
    tag = IDS[CASES.index(case)]
    for b in range(B):
        ref = O.OracleSim(p[b], v[b], m[b], "custom", G=G_[b], softening=SOFT[b], dt=DT[b], levels=LEVELS[b])
        s = make_solo(nb, case, b)
        for t in range(TICKS):
            if t == 2:
                ref.dt = DT2[b]
                s.dt = DT2[b]
            ref.step()
            s.step()
        solo = solo_state(s)
        s.close()
        for k, name in enumerate(("positions", "velocities")):
            want = (ref.positions, ref.velocities)[k]
            d_ens, d_solo = relerr(ticks[TICKS - 1][k][b], want), relerr(solo[k], want)
            bar = max(2e-6, 2 * d_solo)
            print(f"{tag} member {b} ({LEVELS[b]} levels) {name} after {TICKS} ticks: ensemble {d_ens:.3e}, solo {d_solo:.3e} "
                  f"from the oracle (bar {bar:.3e})")
            assert d_ens <= bar, (b, name, d_ens, d_solo)


# ---- 7. self-consistency, all exact ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STEPPED, ids=STEPPED_IDS)
def test_members_do_not_depend_on_their_neighbours(nb, case):
    acc0, ticks, dbg0, dbg5 = trajectory(nb, case)
    rev = list(reversed(range(B)))
    e = make_ens(nb, case, rev)
    same([e.accelerations.numpy()], [acc0[rev]], "reversed order, initial")
    for t, got in enumerate(drive_steps(e, rev)):
        same(got, [a[rev] for a in ticks[t]], f"reversed order tick {t + 1}")
    got = e.quant_debug()
    for key in TABLE_KEYS + ("levels",):
        assert np.array_equal(got[key], dbg5[key][rev], equal_nan=True), f"reversed order: quant_debug()[{key!r}]"
    e.close()
    for b in range(B):
        e = make_ens(nb, case, [b])
        assert e.num_members == 1
        assert e.force_kernel_name() == ("ens_grid_step_wide_kernel" if LEVELS[b] > 256 else "ens_grid_step_kernel")
        same([e.accelerations.numpy()], [acc0[[b]]], f"member {b} alone, initial")
        for t, got in enumerate(drive_steps(e, [b])):
            same(got, [a[[b]] for a in ticks[t]], f"member {b} alone tick {t + 1}")
        e.close()


@pytest.mark.parametrize("case", STEPPED, ids=STEPPED_IDS)
def test_every_driver_gives_the_step_loops_bits(nb, case):
    _, ticks, _, dbg5 = trajectory(nb, case)
    e = make_ens(nb, case)
    before = e.launches()
    e.run(2)
    same(snapshot(e), ticks[1], "run(2)")
    e.set_params(dt=DT2)
    e.run(3)
    same(snapshot(e), ticks[4], "run(2) + run(3)")
    assert e.tick == 5 and e.launches() - before == 5 and e.force_kernel_name() == "ens_grid_step_wide_kernel"
    got = e.quant_debug()
    for key in TABLE_KEYS:
        assert np.array_equal(got[key], dbg5[key], equal_nan=True), f"quant_debug()[{key!r}] after run(2) + run(3)"
    e.close()
    # one dt throughout: run(5), five step() calls, run_recorded(5, every=2) and run_members with equal budgets
    runs = {}
    for how in ("run", "steps", "recorded", "members"):
        e = make_ens(nb, case)
        before = e.launches()
        if how == "run":
            e.run(TICKS)
        elif how == "steps":
            for _ in range(TICKS):
                e.step()
        elif how == "recorded":
            h = e.run_recorded(TICKS, every=2)
            assert h.ticks == [0, 2, 4]
        else:
            e.run_members([TICKS] * B)
        assert e.tick == TICKS and e.launches() - before == TICKS, how
        runs[how] = snapshot(e)
        e.close()
    for how in ("steps", "recorded", "members"):
        same(runs[how], runs["run"], f"{how} vs run({TICKS})")


@pytest.mark.parametrize("case", STEPPED, ids=STEPPED_IDS)
def test_a_stopped_member_equals_the_member_run_alone(nb, case):
    budgets = [0, 1, 3, 5, 5]
    e = make_ens(nb, case)
    before = e.launches()
    e.run_members(budgets)
    assert e.member_ticks == budgets and e.tick == max(budgets) and e.launches() - before == max(budgets)
    got = snapshot(e)
    dbg = e.quant_debug()
    e.close()
    for b in range(B):
        a = make_ens(nb, case, [b])
        if budgets[b]:
            a.run(budgets[b])
        same(snapshot(a), [g[[b]] for g in got], f"member {b} after {budgets[b]} ticks")
        alone = a.quant_debug()
        a.close()
        for key in TABLE_KEYS:
            assert np.array_equal(alone[key], dbg[key][[b]], equal_nan=True), f"member {b}: quant_debug()[{key!r}]"


# ---- 8. edges, each on the member of 1024 levels ---------------------------------------------------------------------------
EDGE = 3
assert LEVELS[EDGE] == 1024
OTHERS = [b for b in range(B) if b != EDGE]


def others_keep_their_bits(e, acc0, ticks):
    same([e.accelerations.numpy()[OTHERS]], [acc0[OTHERS]], "initial")
    got = drive_steps(e)
    for t in range(TICKS):
        same([g[OTHERS] for g in got[t]], [a[OTHERS] for a in ticks[t]], f"tick {t + 1}")
    return got


@pytest.mark.parametrize("case", EDGE_CASES, ids=EDGE_IDS)
def test_a_degenerate_fine_member(nb, case):
    """All stars at one point: every r^2 is the softening^2, so r2max == eps^2, the log grid is degenerate and the forces
    are zero."""
    acc0, ticks, _, _ = trajectory(nb, case)
    p = members(case)[0].copy()
    p[EDGE] = p[EDGE, 0]
    e = make_ens(nb, case, pos=p)
    a0, dbg = e.accelerations.numpy(), e.quant_debug()
    assert np.all(a0[EDGE] == 0), "forces of coincident stars"
    assert dbg["r2max"][EDGE] == np.float32(SOFT[EDGE] ** 2), (dbg["r2max"][EDGE], SOFT[EDGE] ** 2)
    assert dbg["lmin"][EDGE] == dbg["lmax"][EDGE] and not dbg["fast_path"][EDGE]
    s = make_solo(nb, case, EDGE, pos=p)
    solo = s.quant_debug()
    s.close()
    for key in TABLE_KEYS:
        assert dbg[key][EDGE] == solo[key], key
    got = others_keep_their_bits(e, acc0, ticks)
    e.close()
    # the velocities differ, so the stars part after the first drift: from there on it is an ordinary member, alone or not
    a = make_ens(nb, case, [EDGE], pos=p)
    for t, alone in enumerate(drive_steps(a, [EDGE])):
        same(alone, [g[[EDGE]] for g in got[t]], f"degenerate member alone, tick {t + 1}")
    a.close()


@pytest.mark.parametrize("case", EDGE_CASES, ids=EDGE_IDS)
def test_a_nan_fine_member_leaves_the_others_alone(nb, case):
    acc0, ticks, _, _ = trajectory(nb, case)
    p = members(case)[0].copy()
    p[EDGE, 0, 0] = np.nan
    p[EDGE, min(1, case[0] - 1), 1] = np.inf
    e = make_ens(nb, case, pos=p)
    got = others_keep_their_bits(e, acc0, ticks)
    pos, vel, acc = got[TICKS - 1]
    # its own state: NaN propagates silently, as in the reference
    assert np.isnan(acc[EDGE]).all() and np.isnan(vel[EDGE]).all() and np.isnan(pos[EDGE]).all()
    e.close()


@pytest.mark.parametrize("case", EDGE_CASES, ids=EDGE_IDS)
def test_a_fine_member_with_softening_below_the_grid_floor(nb, case):
    """softening^2 = 0.0025 < 0.01: the grid starts at the floor, the diagonal and every close pair sit in bin 0."""
    from oracle import oracle as O
    acc0, ticks, _, _ = trajectory(nb, case)
    p, v, m = members(case)
    soft = list(SOFT)
    soft[EDGE] = 0.05
    e = make_ens(nb, case, soft=soft)
    a0, dbg, bins = e.accelerations.numpy(), e.quant_debug(), e.quant_bin_sums()
    assert np.float32(dbg["lmin"][EDGE]) == np.float32(np.log(np.float64(np.float32(0.01)))), dbg["lmin"][EDGE]
    s = make_solo(nb, case, EDGE, soft=soft)
    solo = s.quant_debug()
    s.close()
    for key in TABLE_KEYS:
        assert dbg[key][EDGE] == solo[key], key
    ref = O.accelerations(p[EDGE], m[EDGE], "custom", force_quant=False, G=G_[EDGE], softening=soft[EDGE], levels=LEVELS[EDGE])
    err = relerr(a0[EDGE].astype(np.float64), ref)
    print(f"{IDS[CASES.index(case)]}: softening 0.05 on the 1024-level member: initial accelerations relerr {err:.3e}")
    assert err < 2e-6, err
    check_bins(nb, case, bins, p, "softening below the floor", soft=soft, who=[EDGE])
    others_keep_their_bits(e, acc0, ticks)
    e.close()
