"""RaggedQuantizedEnsemble on the GPU: grid-mode members of different sizes in one force launch per tick, every member
bit-identical to the solo GalaxySimulation of its own size, mode and level count -- state, accelerations, quant_debug() and
the bins of quant_bin_sums() -- through every driver of the tick path.  Every comparison is ==; there is no tolerance.

Sizes, deliberately not sorted: 700; 37; 2049 (a solo run takes 256 threads per workgroup there, the ragged launch 512: the
member that checks that a wave holds the same pairs at either size); 2 (the smallest); 1025 (one star past the 1024-source
LDS tile); 64; 8 / 9 (one 512-thread workgroup of targets at 64 lanes and one star past it).  CUSTOM levels per member
[256, 16, 64, 2, 3, 255, 17, 128].  Every member has its own G, softening and dt (softening^2 on both sides of the grid's
floor of 0.01).  [257, 5, 300] runs with 16 and 32 lanes per target (NB_SMALL_LANES), and two cases run with the table-free
pair path switched off (NB_NO_GRID_FAST); both knobs are read when a handle is created, so the ensemble and the solo runs
of a case share them.  Per case the ragged ensemble's step() loop and the solo runs are computed once and shared.

A solo constructor evaluates on the tiled path, whose sums may differ from the one-launch step's in the last bit: every solo
run starts from the ensemble's initial accelerations, and quant_debug() after the constructor is compared on the entries
that do not depend on the path (lmin, lmax, r2max, fast_path); from the first tick on, on all six.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_plan_shapes import inputs

pytestmark = pytest.mark.gpu

TICKS = 5
SOLO_TICKS = 6                         # run_watched rounds a budget of 5 up to 6
SIZES = [700, 37, 2049, 2, 1025, 64, 8, 9]
LEVELS = [256, 16, 64, 2, 3, 255, 17, 128]
SIZES_L = [257, 5, 300]
LEVELS_L = [256, 2, 17]
FIXED = {"int8_sim": 256, "int4_sim": 16}
G_ = [0.001, 0.00113, 0.00091, 0.00127, 0.00107, 0.00097, 0.00119, 0.00103]
SOFT = [0.1, 0.113, 0.087, 0.131, 0.071, 0.093, 0.121, 0.109]
DT = [0.01, 0.0123, 0.0071, 0.0157, 0.0093, 0.0111, 0.0083, 0.0139]
BUDGETS = [5, 0, 3, 1, 5, 2, 4, 5]
BAD = 2                                # the member that holds the NaN: 2049 stars
DEG = 4                                # the member with all stars at one point: 1025 stars
DEBUG_KEYS = ("lmin", "lmax", "r2max", "fmin", "fmax", "fast_path")
PATH_FREE_KEYS = ("lmin", "lmax", "r2max", "fast_path")
KERNEL = "ens_grid_step_ragged_kernel"

# name -> (sizes, D, mode, NB_SMALL_LANES or None, NB_NO_GRID_FAST)
CASES = {
    "int8-d2": (SIZES, 2, "int8_sim", None, False),
    "int8-d3": (SIZES, 3, "int8_sim", None, False),
    "int4-d2": (SIZES, 2, "int4_sim", None, False),
    "int4-d3": (SIZES, 3, "int4_sim", None, False),
    "custom-d2": (SIZES, 2, "custom", None, False),
    "custom-d3": (SIZES, 3, "custom", None, False),
    "int8-d3-nofast": (SIZES, 3, "int8_sim", None, True),
    "custom-d2-nofast": (SIZES, 2, "custom", None, True),
    "int4-d2-lanes16": (SIZES_L, 2, "int4_sim", 16, False),
    "custom-d3-lanes16": (SIZES_L, 3, "custom", 16, False),
    "int8-d3-lanes32": (SIZES_L, 3, "int8_sim", 32, False),
    "custom-d2-lanes32": (SIZES_L, 2, "custom", 32, False),
}
NAMES = list(CASES)
MAIN = NAMES[:6]


@pytest.fixture(autouse=True)
def knobs(request, monkeypatch):
    case = request.node.callspec.params.get("case") if hasattr(request.node, "callspec") else None
    if case in CASES and CASES[case][3]:
        monkeypatch.setenv("NB_SMALL_LANES", str(CASES[case][3]))
    if case in CASES and CASES[case][4]:
        monkeypatch.setenv("NB_NO_GRID_FAST", "1")


@pytest.fixture(scope="module")
def nb():
    import nbody_cosmological_simulation_amd as pkg
    assert pkg._native.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return pkg


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def levels_of(case):
    sizes, _, mode, _, _ = CASES[case]
    if mode != "custom":
        return [FIXED[mode]] * len(sizes)
    return LEVELS if sizes is SIZES else LEVELS_L


_MEMBERS = {}


def members(case):
    """Per member (pos, vel, mass) as numpy float32 arrays; member 3 (where there is one) has uniform masses."""
    sizes, d = CASES[case][0], CASES[case][1]
    key = (tuple(sizes), d)
    if key not in _MEMBERS:
        _MEMBERS[key] = [inputs(n, d, 7000 + 17 * b, False, uniform=(b == 3)) for b, n in enumerate(sizes)]
    return _MEMBERS[key]


def make_ens(nb, case, order=None, pos=None):
    sizes, d, mode, _, _ = CASES[case]
    idx = list(range(len(sizes))) if order is None else list(order)
    ms = members(case)
    p = [ms[b][0] for b in idx] if pos is None else [pos[b] for b in idx]
    lv = [levels_of(case)[b] for b in idx] if mode == "custom" else None
    e = nb.RaggedQuantizedEnsemble([T(x) for x in p], [T(ms[b][1]) for b in idx], [T(ms[b][2]) for b in idx],
                                   precision_mode=nb.PrecisionMode(mode), custom_levels=lv, G=[G_[b] for b in idx],
                                   softening=[SOFT[b] for b in idx], dt=[DT[b] for b in idx])
    assert e.num_stars == [sizes[b] for b in idx] and e.num_members == len(idx)
    assert e.levels == [levels_of(case)[b] for b in idx]
    return e


def make_solo(nb, case, b, acc0, pos=None):
    p, v, m = members(case)[b]
    mode = CASES[case][2]
    s = nb.GalaxySimulation(T(p if pos is None else pos), T(v), T(m), precision_mode=nb.PrecisionMode(mode),
                            custom_levels=levels_of(case)[b] if mode == "custom" else None, G=G_[b], softening=SOFT[b],
                            dt=DT[b])
    dbg = s.quant_debug()
    # the constructor's evaluation takes the tiled path and may differ in the last bit: start from the ensemble's
    s.accelerations = T(acc0).clone()
    return s, dbg


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


def same_debug(case, got, b, want, what, keys=DEBUG_KEYS):
    """Member b of the ensemble's quant_debug() against a solo quant_debug() (or a member of another ensemble's, given as a
    dict of scalars): exact equality, key by key."""
    for key in keys:
        if key in ("fmin", "fmax") and CASES[case][2] == "custom":
            assert np.isnan(got[key][b]), f"{what}: {key} of member {b} should be NaN under CUSTOM"
            continue
        g, w = got[key][b], want[key]
        assert (g == w) or (g != g and w != w), f"{what}: {key} of member {b}: ensemble {g!r}, solo {w!r}"


def debug_of(dbg, b):
    return {key: dbg[key][b] for key in DEBUG_KEYS}


def same_bins(got, b, want, what):
    """Member b of the ensemble's quant_bin_sums() against a solo quant_bin_sums(): both check-sums per star, both counters."""
    for key in ("sum_k", "sum_kw"):
        assert got[key][b].dtype == np.int64 and got[key][b].shape == want[key].shape, (what, key, b, got[key][b].shape)
        assert np.array_equal(got[key][b], want[key]), f"{what}: {key} of member {b} differ"
    for key in ("pairs_table_free", "pairs_table"):
        assert int(got[key][b]) == int(want[key]), f"{what}: {key} of member {b}: ensemble {got[key][b]}, solo {want[key]}"
    assert int(got["levels"][b]) == int(want["levels"]), (what, b)


_TRAJ, _SOLO = {}, {}


def trajectory(nb, case):
    """The ragged ensemble driven with step(): initial accelerations, quant_debug() and quant_bin_sums() after the
    constructor, then per tick (snapshot, quant_debug()), and quant_bin_sums() after the last tick."""
    if case not in _TRAJ:
        e = make_ens(nb, case)
        assert e.force_kernel_name() == KERNEL and e.launches() == 1
        acc0 = [t.numpy() for t in e.accelerations]
        dbg0, bins0 = e.quant_debug(), e.quant_bin_sums()
        assert list(dbg0["levels"]) == levels_of(case)
        ticks = []
        for t in range(TICKS):
            e.step()
            assert e.launches() == 2 + t
            ticks.append((snapshot(e), e.quant_debug()))
        before = snapshot(e)
        bins5 = e.quant_bin_sums()
        same(snapshot(e), before, "the bin read-out is an observer")
        assert e.launches() == 1 + TICKS and e.tick == TICKS
        e.close()
        _TRAJ[case] = (acc0, dbg0, bins0, ticks, bins5)
    return _TRAJ[case]


def solo(nb, case):
    """solo(...)[b]: (states, debugs, bins) of member b's GalaxySimulation -- states[t] = (pos, vel, acc) and debugs[t] =
    quant_debug() after t step() calls (debugs[0]: after the constructor), bins = {0, TICKS: quant_bin_sums("small")}."""
    if case not in _SOLO:
        acc0 = trajectory(nb, case)[0]
        out = []
        for b in range(len(CASES[case][0])):
            s, dbg = make_solo(nb, case, b, acc0[b])
            states = [(s.positions.numpy(), s.velocities.numpy(), s.accelerations.numpy())]
            debugs, bins = [dbg], {0: s.quant_bin_sums("small")}
            for t in range(SOLO_TICKS):
                s.step()
                assert s.force_kernel_name() == "small_step_kernel"
                states.append((s.positions.numpy(), s.velocities.numpy(), s.accelerations.numpy()))
                debugs.append(s.quant_debug())
                if t + 1 == TICKS:
                    bins[TICKS] = s.quant_bin_sums("small")
                    assert bins[TICKS]["path"] == "small"
            s.close()
            out.append((states, debugs, bins))
        _SOLO[case] = out
    return _SOLO[case]


def solo_at(nb, case, ticks, order=None):
    """A snapshot made of the solo runs: member b after ticks[b] solo steps."""
    ref = solo(nb, case)
    order = range(len(ref)) if order is None else order
    return tuple([ref[b][0][int(t)][k] for b, t in zip(order, ticks)] for k in range(3))


# ---- 1. the step loop: state, accelerations and tables after every tick -----------------------------------------------------
@pytest.mark.parametrize("case", NAMES)
def test_step_loop_and_tables_are_bit_identical_to_solo(nb, case):
    acc0, dbg0, _, ticks, _ = trajectory(nb, case)
    ref = solo(nb, case)
    B = len(acc0)
    print(f"{case}: fast_path after the constructor {dbg0['fast_path'].tolist()}, after tick {TICKS} "
          f"{ticks[-1][1]['fast_path'].tolist()}")
    if CASES[case][4]:
        assert not dbg0["fast_path"].any() and not ticks[-1][1]["fast_path"].any()
    for b in range(B):
        same_debug(case, dbg0, b, ref[b][1][0], "after the constructor", keys=PATH_FREE_KEYS)
    for t in range(TICKS):
        same(ticks[t][0], solo_at(nb, case, [t + 1] * B), f"tick {t + 1}")
        for b in range(B):
            same_debug(case, ticks[t][1], b, ref[b][1][t + 1], f"tick {t + 1}")
    # the grid is in force: the largest members do not follow the FLOAT32 run of the same inputs
    b = int(np.argmax(CASES[case][0]))
    p, v, m = members(case)[b]
    s = nb.GalaxySimulation(T(p), T(v), T(m), precision_mode=nb.PrecisionMode.FLOAT32, G=G_[b], softening=SOFT[b], dt=DT[b])
    s.accelerations = T(acc0[b]).clone()
    s.step()
    assert not np.array_equal(s.accelerations.numpy(), ticks[0][0][2][b]), f"member {b} ran without its grid"
    s.close()


# ---- 2. run() ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NAMES)
def test_run_equals_the_step_loop_and_is_one_launch_per_tick(nb, case):
    _, _, _, ticks, _ = trajectory(nb, case)
    e = make_ens(nb, case)
    assert e.launches() == 1 and e.force_kernel_name() == KERNEL
    e.run(TICKS)
    same(snapshot(e), ticks[TICKS - 1][0], "run(5)")
    got = e.quant_debug()
    for key in DEBUG_KEYS + ("levels",):
        assert np.array_equal(got[key], ticks[TICKS - 1][1][key], equal_nan=True), f"quant_debug()[{key!r}] after run(5)"
    assert e.tick == TICKS and e.launches() == 1 + TICKS
    for t in range(3):
        e.step()
        assert e.launches() == 2 + TICKS + t
    assert e.force_kernel_name() == KERNEL
    e.close()
    e = make_ens(nb, case)
    h = e.run_recorded(TICKS, 1)
    same(snapshot(e), ticks[TICKS - 1][0], "run_recorded(5, 1)")
    assert h.kinetic.shape == (TICKS + 1, len(CASES[case][0])) and e.launches() == 1 + TICKS
    ke, pe = e.energies()
    assert torch.equal(ke, h.kinetic[-1]) and torch.equal(pe, h.potential[-1])
    assert e.get_kinetic_energy() == ke.tolist() and e.get_potential_energy() == pe.tolist()
    assert e.get_state(1)["positions"].shape == (CASES[case][0][1], CASES[case][1]) and e.get_state(1)["tick"] == TICKS
    e.close()


# ---- 3. the bins ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NAMES)
def test_bin_sums_equal_the_solo_read_out(nb, case):
    _, dbg0, bins0, ticks, bins5 = trajectory(nb, case)
    ref = solo(nb, case)
    sizes = CASES[case][0]
    for b, n in enumerate(sizes):
        assert bins0["sum_k"][b].shape == (n,) and bins5["sum_kw"][b].shape == (n,)
        same_bins(bins0, b, ref[b][2][0], "after the constructor")
        same_bins(bins5, b, ref[b][2][TICKS], f"after tick {TICKS}")
        # every pair was counted once: n * n of them, whichever route binned them
        assert int(bins5["pairs_table_free"][b]) + int(bins5["pairs_table"][b]) == n * n, (b, n)
    if CASES[case][4]:
        assert not bins5["pairs_table_free"].any()


# ---- 4. members stop at their own tick -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MAIN + ["int4-d2-lanes16"])
def test_stopped_members_keep_their_state_and_their_tables(nb, case):
    acc0, dbg0, _, _, _ = trajectory(nb, case)
    ref = solo(nb, case)
    B = len(acc0)
    budgets = BUDGETS[:B]
    e = make_ens(nb, case)
    before = e.launches()
    e.run_members(budgets)
    same(snapshot(e), solo_at(nb, case, budgets), f"run_members({budgets})")
    assert e.member_ticks == budgets and e.launches() - before == max(budgets) and e.force_kernel_name() == KERNEL
    got = e.quant_debug()
    for b, t in enumerate(budgets):
        # a stopped member: the tables and force bounds of its last evaluation (a budget of 0: the constructor's)
        same_debug(case, got, b, ref[b][1][t] if t else debug_of(dbg0, b), f"run_members, member {b} after {t} ticks")
    e.step()                                             # and on from there, as the solo runs go on
    same(snapshot(e), solo_at(nb, case, [t + 1 for t in budgets]), "run_members, then step()")
    got = e.quant_debug()
    for b, t in enumerate(budgets):
        same_debug(case, got, b, ref[b][1][t + 1], f"run_members, then step(): member {b}")
    e.close()
    e = make_ens(nb, case)
    r = e.run_watched(TICKS, check_interval=2)          # budgets round up to 6
    assert (r.stable_ticks <= SOLO_TICKS).all() and (r.stable_ticks[~r.exploded] == SOLO_TICKS).all()
    same(snapshot(e), solo_at(nb, case, r.stable_ticks), "run_watched")
    got = e.quant_debug()
    for b, t in enumerate(r.stable_ticks):
        same_debug(case, got, b, ref[b][1][int(t)] if t else debug_of(dbg0, b), f"run_watched, member {b} after {t} ticks")
    e.close()


# ---- 5. / 6. members are independent ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MAIN + ["custom-d3-lanes16"])
def test_permuting_the_members_changes_no_bits(nb, case):
    acc0, dbg0, _, ticks, bins5 = trajectory(nb, case)
    B = len(acc0)
    shuffled = [(5 * b + 3) % B for b in range(B)] if B == 8 else [(b + 2) % B for b in range(B)]
    for order in (list(range(B))[::-1], shuffled):       # the work list's order follows the permutation
        assert sorted(order) == list(range(B))
        e = make_ens(nb, case, order)
        same(([t.numpy() for t in e.accelerations],), ([acc0[b] for b in order],), f"order {order}, initial")
        for t in range(TICKS):
            e.step()
            same(snapshot(e), pick(ticks[t][0], order), f"order {order} tick {t + 1}")
        got, bins = e.quant_debug(), e.quant_bin_sums()
        for key in DEBUG_KEYS + ("levels",):
            assert np.array_equal(got[key], ticks[-1][1][key][order], equal_nan=True), f"order {order}: quant_debug()[{key!r}]"
        for k, b in enumerate(order):
            assert np.array_equal(bins["sum_k"][k], bins5["sum_k"][b]) and np.array_equal(bins["sum_kw"][k], bins5["sum_kw"][b])
        e.close()


@pytest.mark.parametrize("case", MAIN)
def test_a_nan_member_leaves_the_others_alone(nb, case):
    acc0, _, _, ticks, _ = trajectory(nb, case)
    B = len(acc0)
    p = [m[0].copy() for m in members(case)]
    p[BAD][:] = np.nan                                   # the whole member
    e = make_ens(nb, case, pos=p)
    others = [b for b in range(B) if b != BAD]
    same(([t.numpy() for t in e.accelerations],), (acc0,), "initial", only=others)
    for t in range(TICKS):
        e.step()
        got = snapshot(e)
        same(got, ticks[t][0], f"tick {t + 1}", only=others)
        dbg = e.quant_debug()
        for key in DEBUG_KEYS:
            assert np.array_equal(dbg[key][others], ticks[t][1][key][others], equal_nan=True), (t, key)
    assert all(np.isnan(kind[BAD]).all() for kind in got)
    e.close()


# ---- 7. the padding is nobody's ------------------------------------------------------------------------------------------------
def raw(e, name):
    """The handle's whole padded array through nb_ens_get_state."""
    from nbody_cosmological_simulation_amd import _native as N
    out = torch.empty(e._shape(name), dtype=e._dtype)
    args = [None, None, None, None]
    args[{"positions": 0, "velocities": 1, "accelerations": 2, "masses": 3}[name]] = C.c_void_p(out.data_ptr())
    N.check(N.lib().nb_ens_get_state(e._handle, *args, 0))
    return out


@pytest.mark.parametrize("case", ["int8-d2", "int4-d3", "custom-d3", "custom-d2-lanes32"])
def test_no_kernel_touches_the_padding(nb, case):
    sizes = CASES[case][0]
    B = len(sizes)
    pad = torch.zeros(B, max(sizes), dtype=torch.bool)
    for m, n in enumerate(sizes):
        pad[m, n:] = True
    assert int(pad.sum()) == B * max(sizes) - sum(sizes) > 0
    e = make_ens(nb, case)

    def check(what):
        for name in ("positions", "velocities", "masses"):
            full = raw(e, name)
            assert bool(torch.isnan(full[pad]).all()), f"{what}: a padding row of {name} was written"
            assert not bool(torch.isnan(full[~pad]).any()), f"{what}: a padding row of {name} was read"
        assert bool((raw(e, "accelerations")[pad] == 0).all()), f"{what}: a padding row of the accelerations was written"

    check("constructor")
    e.step()
    check("step")
    e.run(3)                                             # two NB_KICK_CLOSE_OPEN launches: both position buffers
    check("run")
    e.run_members(BUDGETS[:B])
    check("run_members")
    e.quant_bin_sums()
    check("quant_bin_sums")
    e.run_diverged(2, 1, baseline=list(range(B)))
    check("run_diverged")
    dbg = e.quant_debug()
    assert np.isfinite(dbg["r2max"]).all() and np.isfinite(dbg["lmax"]).all(), "a padding row reached a member's maximum"
    e.close()


# ---- 8. equal sizes: the QuantizedEnsemble -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["int8_sim", "int4_sim", "custom"])
def test_equal_sizes_are_the_quantized_ensemble(nb, mode):
    ms = [inputs(700, 3, 8100 + b, False) for b in range(4)]
    kw = dict(precision_mode=nb.PrecisionMode(mode), custom_levels=[256, 2, 17, 64] if mode == "custom" else None, G=G_[:4],
              softening=SOFT[:4], dt=DT[:4])
    r = nb.RaggedQuantizedEnsemble([T(m[0]) for m in ms], [T(m[1]) for m in ms], [T(m[2]) for m in ms], **kw)
    q = nb.QuantizedEnsemble(*(T(np.stack([m[k] for m in ms])) for k in range(3)), **kw)
    assert r.num_stars == [700] * 4 and q.force_kernel_name() == "ens_grid_step_kernel" and r.force_kernel_name() == KERNEL
    assert torch.equal(torch.stack(r.accelerations), q.accelerations)
    for e in (r, q):
        e.run(3)
        e.step()
    hr, hq = r.run_recorded(2, 1), q.run_recorded(2, 1)
    for name in ("positions", "velocities", "accelerations", "masses"):
        assert torch.equal(torch.stack(getattr(r, name)), getattr(q, name)), name
    assert torch.equal(hr.kinetic, hq.kinetic) and torch.equal(hr.potential, hq.potential)
    dr, dq = r.quant_debug(), q.quant_debug()
    for key in DEBUG_KEYS + ("levels",):
        assert np.array_equal(dr[key], dq[key], equal_nan=True), key
    br, bq = r.quant_bin_sums(), q.quant_bin_sums()
    assert np.array_equal(np.stack(br["sum_k"]), bq["sum_k"]) and np.array_equal(np.stack(br["sum_kw"]), bq["sum_kw"])
    assert np.array_equal(br["pairs_table_free"], bq["pairs_table_free"]) and np.array_equal(br["pairs_table"], bq["pairs_table"])
    assert r.launches() == q.launches() == 7
    r.close()
    q.close()


# ---- 9. divergence ---------------------------------------------------------------------------------------------------------------
DSIZES = [700, 700, 37, 37, 1025, 1025]
DBASE = [0, 0, 2, 2, 4, 4]


def pairs(nb, mode, d=3):
    """Pairs of equal size, parameters and levels; the second of a pair is the first with positions[0, 0] one ulp up."""
    ms = []
    for b, n in enumerate(DSIZES):
        p, v, m = inputs(n, d, 9000 + DBASE[b], False)
        if b != DBASE[b]:
            p = p.copy()
            p[0, 0] = np.nextafter(p[0, 0], p.dtype.type(np.inf))
        ms.append((p, v, m))
    return nb.RaggedQuantizedEnsemble([T(m[0]) for m in ms], [T(m[1]) for m in ms], [T(m[2]) for m in ms],
                                      precision_mode=nb.PrecisionMode(mode),
                                      custom_levels=[256, 256, 16, 16, 3, 3] if mode == "custom" else None,
                                      G=[G_[b] for b in DBASE], softening=[SOFT[b] for b in DBASE], dt=[DT[b] * 4 for b in DBASE])


def check_divergence(got, e, what):
    """got: (max_position, max_velocity) rows of B values, against torch on the downloaded members."""
    pos, vel = e.positions, e.velocities
    for b, base in enumerate(DBASE):
        dp, dv = (pos[b] - pos[base]).abs(), (vel[b] - vel[base]).abs()
        g_mp, g_mv = (float(t[b]) for t in got)
        print(f"{what} member {b} vs {base}: max_pos {g_mp:.9g} max_vel {g_mv:.9g}")
        assert g_mp == float(dp.max().double()), (what, b, g_mp, float(dp.max()))
        assert g_mv == float(dv.max().double()), (what, b, g_mv, float(dv.max()))


@pytest.mark.parametrize("mode", ["int8_sim", "int4_sim", "custom"])
def test_divergence_sample_by_sample(nb, mode):
    e, ref = pairs(nb, mode), pairs(nb, mode)
    d = e.divergence(DBASE)
    check_divergence((d.max_position, d.max_velocity), e, "divergence at entry")
    h = e.run_diverged(TICKS, 1, DBASE)
    assert h.max_position.shape == (TICKS + 1, 6) and h.ticks == list(range(TICKS + 1)) and h.energy is not None
    for s in range(TICKS + 1):
        check_divergence((h.max_position[s], h.max_velocity[s]), ref, f"sample {s}")
        if s < TICKS:
            ref.step()
    assert all(float(h.max_position[s][b]) == 0.0 for s in range(TICKS + 1) for b in (0, 2, 4))
    same(snapshot(e), snapshot(ref), "run_diverged leaves run()'s trajectory")
    hr = ref.energies()
    assert torch.equal(h.energy.kinetic[-1], hr[0]) and torch.equal(h.energy.potential[-1], hr[1])
    assert e.launches() == 1 + TICKS
    with pytest.raises(ValueError, match="stars against"):
        e.divergence(0)
    e.close()
    ref.close()


# ---- 10. a degenerate member -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MAIN)
def test_a_degenerate_member_equals_its_solo_run(nb, case):
    """All stars of one member at one point: every r^2 is the softening^2, so r2max == eps^2, the log grid is degenerate,
    the forces are zero and (INT8 / INT4) the force snap passes them through."""
    acc0, _, _, ticks, _ = trajectory(nb, case)
    B = len(acc0)
    p = [m[0].copy() for m in members(case)]
    p[DEG][:] = p[DEG][0]
    e = make_ens(nb, case, pos=p)
    others = [b for b in range(B) if b != DEG]
    a0 = [t.numpy() for t in e.accelerations]
    dbg = e.quant_debug()
    assert np.all(a0[DEG] == 0), "forces of coincident stars"
    assert dbg["r2max"][DEG] == np.float32(SOFT[DEG] ** 2), (dbg["r2max"][DEG], SOFT[DEG] ** 2)
    assert dbg["lmin"][DEG] == dbg["lmax"][DEG] and not dbg["fast_path"][DEG]
    if CASES[case][2] != "custom":
        assert dbg["fmin"][DEG] == 0 and dbg["fmax"][DEG] == 0
    same((a0,), (acc0,), "initial", only=others)
    s, sdbg = make_solo(nb, case, DEG, a0[DEG], pos=p[DEG])
    same_debug(case, dbg, DEG, sdbg, "degenerate member after the constructor", keys=PATH_FREE_KEYS)
    for t in range(TICKS):
        e.step()
        s.step()
        got = snapshot(e)
        same(got, ticks[t][0], f"tick {t + 1}", only=others)
        want = (s.positions.numpy(), s.velocities.numpy(), s.accelerations.numpy())
        for name, g, w in zip(("positions", "velocities", "accelerations"), got, want):
            assert np.array_equal(g[DEG], w, equal_nan=True), f"degenerate member tick {t + 1}: {name} differ"
        same_debug(case, e.quant_debug(), DEG, s.quant_debug(), f"degenerate member tick {t + 1}")
    assert s.force_kernel_name() == "small_step_kernel"
    # the bins: a degenerate grid has none -- the solo read-out refuses, the ensemble's reports zeros for that member (as
    # QuantizedEnsemble's does) and the other members' bins are those of their solo runs at these positions
    from nbody_cosmological_simulation_amd._native import NativeError
    with pytest.raises(NativeError, match="degenerate grid"):
        s.quant_bin_sums("small")
    bins = e.quant_bin_sums()
    assert not bins["sum_k"][DEG].any() and not bins["sum_kw"][DEG].any() and bins["sum_k"][DEG].shape == (CASES[case][0][DEG],)
    ref = solo(nb, case)
    for b in others:
        same_bins(bins, b, ref[b][2][TICKS], f"beside a degenerate member, after tick {TICKS}")
    s.close()
    e.close()


# ---- the refusals that need a handle -------------------------------------------------------------------------------------------
def test_the_native_refusals_and_the_read_outs(nb):
    from nbody_cosmological_simulation_amd import _native as N
    lib = N.lib()
    e = pairs(nb, "int8_sim", d=2)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    rc = lib.nb_ens_divergence(e._handle, i32(0, 0, 0, 2, 4, 4), None, None, None, 0)
    assert rc == -1 and "stars" in N.last_error(), (rc, N.last_error())
    refused = {
        "nb_ens_metrics": lambda: lib.nb_ens_metrics(e._handle, 8, None, 90.0, None, None, None, None),
        "nb_ens_crash_measures": lambda: lib.nb_ens_crash_measures(e._handle, None, 0, None, None),
        "nb_ens_run_crash_watched": lambda: lib.nb_ens_run_crash_watched(e._handle, i32(1, 1, 1, 1, 1, 1), None, None, 0, 0, None,
                                                                         None, None, None, None),
    }
    for name, call in refused.items():
        rc = call()
        assert rc == -5 and name in N.last_error() and "follow-up" in N.last_error(), (name, rc, N.last_error())
    out = (C.c_double * 48)()
    assert lib.nb_ens_quant_info(e._handle, out) == 0            # served on a ragged GRID handle
    assert lib.nb_ens_quant_bin_sums(e._handle, None, None, None) == 0
    assert e.tick == 0 and e.launches() == 1                     # nothing ran
    for call in (e.metrics, e.crash_measures, lambda: e.run_crash_watched(3)):
        with pytest.raises(NotImplementedError):
            call()
    e.close()
