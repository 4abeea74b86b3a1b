"""Read-outs between steps leave the trajectory bit-identical.

A handle carries hidden state from one native call to the next: the speculative next positions (`spec_open`, `pos_alt`,
`sym.packed`), the tracked max-r2 search's seed, the grid tables and the force-quantisation bounds, `last_kernel`, and on
the Python side the tensor cache and the energy memo.  Every read-only entry point queues kernels on the same stream and
reuses some of those buffers, and the reference's scripts read energies, metrics and state every tick or every few ticks.
So for every path a step can take (table below: one-launch small step, pair-symmetric and one-sided tiles, fused and
large grid tables, tracked search, speculation of both kinds) run A advances through

    step(), step(), run(3), step(), run(2), step()

untouched while run B, built from the same seeded state, calls observers after every segment.  After every segment the
DEVICE state (nb_get_state, never the cached properties) of the two must be equal bit for bit, integer views so that NaN
patterns would count; after every observer the cached properties that exist must equal the device state.

Both runs must report the same force_kernel_name() and step_path_name().  One exception, written down here: an observer
that rewrites a buffer the speculative next positions live in (the pair-symmetric potential repacks `sym.packed`; spin_up
evaluates the forces) voids the speculation, which is the documented invalidation, not a changed trajectory.  B's next
call then opens with its own kick + drift launch instead of `spec_read` and its first force launch carries no "|4"
(opening kick on read).  For exactly those observers (DROPS_SPECULATION) the paths are compared after that is normalised
away; for every other observer the strings must be identical.  (In the "all observers" cases spin_up comes last and voids
the speculation after every segment, so what an earlier observer does to it shows in the per-observer cases only: a
scratch build without the `spec_open = false` of energy_eval's symmetric-potential branch turns float32-n3200-d2-pe, -te
and -collect_metrics red, and their float64-n5200-d2 and float32-n4200-d3 twins, while the "all" cases stay green.)

The "all observers" cases also pin the read-outs themselves mid-run: the oracle at the bars of
test_small_system_single_launch_step_vs_oracle, the production bin read-out and lmax against the oracle's bin matrix of
the current positions (the tracked search has then run twice on one set of positions), and a fresh handle built from
the downloaded state (the load_snapshot route), which must return bit-equal energies and continue bit for bit.
"""
import re
from collections import namedtuple

import numpy as np
import pytest
import torch

import plan_shapes as P

pytestmark = pytest.mark.gpu

GRID = ("int8_sim", "int4_sim", "custom")
SEGMENTS = (("step", 1), ("step", 1), ("run", 3), ("step", 1), ("run", 2), ("step", 1))
TICKS = sum(k for _, k in SEGMENTS)


@pytest.fixture(scope="module")
def nb():
    import nbody_cosmological_simulation_amd as pkg
    assert pkg._native.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return pkg


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- the paths and the smallest sizes that reach them (thresholds of nb_plan.cpp / nb_step.cpp: one-launch step up to
# 3072 with fp32 state / 4096 with fp64 state; symmetric tiling from 1024 (fp32 family) / 5120 (fp64), 2-D; tracked
# max-r2 search above 3072).  steps: what step() / run() run on; tiled: what _compute_accelerations / "tiled" run on,
# "sym<R>" or "onesided" (None: not pinned for that row).
Row = namedtuple("Row", "mode levels n d steps tiled")


def _rows():
    rows = [Row("float64", None, 300, 2, "small", "sym1"), Row("float64", None, 3000, 2, "small", "onesided"),
            Row("float64", None, 5200, 2, "sym", "sym4"), Row("float64", None, 700, 3, "small", None)]
    for mode in ("float32", "bfloat16", "float16") + GRID:
        rows += [Row(mode, None, 300, 2, "small", "onesided"), Row(mode, None, 1500, 2, "small", "sym2"),
                 Row(mode, None, 3200, 2, "sym", "sym2")]
    rows += [Row("custom", 1000, 1500, 2, "sym", "sym2")]        # large tables: no small step
    rows += [Row("float32", None, 700, 3, "small", None), Row("int8_sim", None, 700, 3, "small", None),
             Row("float32", None, 4200, 3, "sym", "sym2"), Row("int8_sim", None, 4200, 3, "sym", "sym2")]
    return rows


ROWS = _rows()


def row_id(r):
    return f"{r.mode}{r.levels or ''}-n{r.n}-d{r.d}"


def is_grid(row):
    return row.mode in GRID


def small_applies(row):
    return row.steps == "small"


def kernel_prefix(row, which):
    """force_kernel_name() of the steps ("steps") or of a tiled evaluation ("tiled")."""
    T_ = "double" if row.mode == "float64" else "float"
    if which == "steps" and row.steps == "small":
        return "small_step_kernel"
    what = "sym" if which == "steps" else row.tiled
    if what is None:
        return "force_"
    if what.startswith("sym"):
        return f"force_sym_kernel<{T_}"
    return "force_f64_kernel" if row.mode == "float64" else "force_f32_kernel"


def initial_state(row, unequal):
    rng = np.random.default_rng(1000 * row.n + row.d)
    dt = np.float64 if row.mode == "float64" else np.float32
    pos = (rng.standard_normal((row.n, row.d)) * 4).astype(np.float32).astype(dt)
    vel = (rng.standard_normal((row.n, row.d)) * 0.05).astype(np.float32).astype(dt)
    mass = ((0.5 + rng.random(row.n)).astype(np.float32) if unequal else np.ones(row.n, np.float32)).astype(dt)
    return pos, vel, mass


def make(nb, row, state, **kw):
    pos, vel, mass = state
    return nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=nb.PrecisionMode(row.mode), softening=0.1, dt=0.01,
                               custom_levels=row.levels, **kw)


# ---- bit-level comparison ---------------------------------------------------------------------------------------------
_INT = {8: torch.int64, 4: torch.int32, 2: torch.int16}


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(_INT[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def device_state(sim):
    return {name: sim._download(name) for name in ("positions", "velocities", "accelerations")}


def check_cache(sim, what):
    """Every cached property equals the device state, and no observer marked one as edited."""
    for name, (t, version, dirty) in list(sim._cache.items()):
        assert not dirty and t._version == version, (what, name)
        assert same_bits(t, sim._download(name)), f"after {what}: the cached {name} is not what the device holds"


def norm_path(path):
    """step_path_name() with the speculation taken out: the opening site, and the "|4" of the launch that read it."""
    parts = []
    for part in path.split(" "):
        key, _, sites = part.partition("=")
        toks = []
        for tok in sites.split("+"):
            tok = tok.replace("|4", "")
            if key == "open" and re.fullmatch(r"spec_read|kick_drift|pack:1", tok):
                tok = "OPEN"
            if tok not in toks:
                toks.append(tok)
        parts.append(key + "=" + "+".join(toks))
    return " ".join(parts)


# ---- observers ----------------------------------------------------------------------------------------------------------
class Ctx:
    def __init__(self, nb, row, sim, tmp_path, pe_sym=True):
        self.nb, self.row, self.sim, self.tmp_path, self.pe_sym = nb, row, sim, tmp_path, pe_sym
        self.calls = 0


def _pe_kernel_is_pinned(cx):
    """The potential ran on the kernel the row's plan selects (nb_step.cpp energy_eval)."""
    sym = cx.pe_sym and cx.row.tiled in ("sym2", "sym4")
    name = cx.sim.pe_kernel_name()
    assert name.startswith("potential_sym_kernel<" if sym else "potential_kernel<"), (name, cx.row)
    if sym:
        assert name.split(",")[2] == cx.row.tiled[3:], (name, cx.row)


def obs_state_reads(cx):
    s = cx.sim
    for name in ("positions", "velocities", "accelerations", "masses"):
        assert same_bits(getattr(s, name), s._download(name)), name
    st = s.get_state()
    assert same_bits(st["positions"], s._download("positions")) and same_bits(st["velocities"], s._download("velocities"))
    assert st["tick"] == s.tick


def obs_ke(cx):
    assert np.isfinite(cx.sim.get_kinetic_energy())


def obs_pe(cx):
    assert np.isfinite(cx.sim.get_potential_energy())
    _pe_kernel_is_pinned(cx)


def obs_te(cx):
    assert np.isfinite(cx.sim.get_total_energy())
    _pe_kernel_is_pinned(cx)


def obs_collect_metrics(cx):
    from nbody_cosmological_simulation_amd import metrics
    m = metrics.SimulationMetrics()
    metrics.collect_metrics(cx.sim, cx.sim.tick, m)
    assert m.ticks == [cx.sim.tick] and len(m.rotation_curves) == 1 and np.isfinite(m.total_energy[0])


def obs_native_metrics(cx):
    from nbody_cosmological_simulation_amd import metrics
    m = metrics.native_metrics(None, None, None, simulation=cx.sim)
    assert sum(m["count"]) >= cx.row.n - 1 and 0.0 <= m["bound_fraction"] <= 1.0      # (the farthest star is in no bin)


def obs_snapshot(cx):
    from nbody_cosmological_simulation_amd import checkpoint
    cx.calls += 1
    h = checkpoint.save_snapshot(cx.sim, str(cx.tmp_path / f"snap{cx.calls}.npz"))
    assert h == checkpoint.state_hash(cx.sim)


def obs_names_sync(cx):
    s = cx.sim
    s.synchronize()
    assert s.force_kernel_name().startswith(kernel_prefix(cx.row, "steps"))
    assert s.pe_kernel_name() and s.step_path_name().startswith("open=")


def obs_kernel_time(cx):
    ms, launches = cx.sim.kernel_time()
    assert launches >= 1 and ms > 0.0


def obs_spin_up(cx):
    cx.sim.spin_up(2)
    assert cx.sim.force_kernel_name().startswith(kernel_prefix(cx.row, "tiled")), (cx.sim.force_kernel_name(), cx.row)


def same_debug(a, b):
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            if not np.array_equal(x, y):
                return False
        elif x is None or y is None:
            if x is not y:
                return False
        elif not (x == y or (x != x and y != y)):
            return False
    return True


def obs_quant_debug(cx):
    d = cx.sim.quant_debug()
    assert d["lmax"] > d["lmin"]
    if cx.row.n <= 1500:
        full = cx.sim.quant_debug(bins=True)
        assert full["d2bins"].shape == (cx.row.n, cx.row.n) and same_debug(d, dict(full, d2bins=None, fbins=None))
        assert np.array_equal(full["d2bins"][0:3], cx.sim.quant_bins_rows(0, 3))


def obs_bins_rows(cx):
    k = cx.sim.quant_bins_rows(0, 3)
    assert k.shape == (3, cx.row.n) and (k >= -1).all()


def _bin_sums(cx, which, path, shape=None):
    """One bin read-out, quant_debug() before and after it must agree; path None: documented as unsupported."""
    from nbody_cosmological_simulation_amd import _native
    before = cx.sim.quant_debug()
    if path is None:
        with pytest.raises(_native.NativeError, match="small-system step does not apply"):
            cx.sim.quant_bin_sums(which)
    else:
        bs = cx.sim.quant_bin_sums(which)
        assert bs["path"] == path and (shape is None or bs["shape"] == shape), (which, bs["path"], bs["shape"], cx.row)
        assert bs["pairs_table_free"] + bs["pairs_table"] >= cx.row.n * (cx.row.n - 1) // 2
    after = cx.sim.quant_debug()
    assert same_debug(before, after), (which, before, after)


def _tiled_path(row):
    if row.tiled is None:
        return "onesided", None            # (700, 3): below the symmetric tiling in every family
    return ("sym", int(row.tiled[3:])) if row.tiled.startswith("sym") else ("onesided", None)


def obs_bin_sums_last(cx):
    # (the last evaluation: the steps', unless an observer in between evaluated the forces on the tiled path)
    if small_applies(cx.row) and cx.sim.force_kernel_name() == "small_step_kernel":
        _bin_sums(cx, "last", "small")
    else:
        _bin_sums(cx, "last", *_tiled_path(cx.row))


def obs_bin_sums_tiled(cx):
    _bin_sums(cx, "tiled", *_tiled_path(cx.row))


def obs_bin_sums_small(cx):
    _bin_sums(cx, "small", "small" if small_applies(cx.row) else None)


OBSERVERS = {
    "state_reads": obs_state_reads, "ke": obs_ke, "pe": obs_pe, "te": obs_te, "pe_nosym": obs_pe, "te_nosym": obs_te,
    "collect_metrics": obs_collect_metrics, "native_metrics": obs_native_metrics, "snapshot": obs_snapshot,
    "names_sync": obs_names_sync, "kernel_time": obs_kernel_time, "spin_up": obs_spin_up,
}
GRID_OBSERVERS = {
    "quant_debug": obs_quant_debug, "bins_rows": obs_bins_rows, "bin_sums_last": obs_bin_sums_last,
    "bin_sums_tiled": obs_bin_sums_tiled, "bin_sums_small": obs_bin_sums_small,
}
# "all of them, in this order" (the energies' memo: the total comes first so that it is the native call with both parts)
ALL_ORDER = ("state_reads", "te", "ke", "pe", "collect_metrics", "native_metrics", "snapshot", "names_sync", "spin_up")
ALL_GRID_ORDER = ("quant_debug", "bins_rows", "bin_sums_last", "bin_sums_tiled", "bin_sums_small", "bin_sums_last")
# observers that rewrite a buffer the speculative next positions live in (module docstring)
DROPS_SPECULATION = {"pe", "te", "collect_metrics", "spin_up", "all"}


# ---- run A, computed once per (row, masses, profile) and left unchanged ------------------------------------------------
_RUN_A = {}


def advance(sim, seg):
    kind, k = seg
    if kind == "step":
        assert k == 1
        sim.step()
    else:
        sim.run(k)


def run_a(nb, row, unequal, profile=False):
    key = (row, unequal, profile)
    if key not in _RUN_A:
        sim = make(nb, row, initial_state(row, unequal), profile=profile)
        out = []
        for i, seg in enumerate(SEGMENTS):
            advance(sim, seg)
            rec = device_state(sim)
            rec["kernel"], rec["path"] = sim.force_kernel_name(), sim.step_path_name()
            assert rec["kernel"].startswith(kernel_prefix(row, "steps")), (rec["kernel"], row)
            if i == 1 and not is_grid(row):
                # the second step() of a Python loop starts from the first one's speculative positions (kind 1: small
                # step, kind 2: reduce_sym): the hidden state the observers must not disturb is really there
                assert rec["path"].startswith("open=spec_read"), rec["path"]
            out.append(rec)
        sim.close()
        _RUN_A[key] = out
    return _RUN_A[key]


def check_plan(row):
    """The table's plan columns against the planner itself (device-free), so that a retune shows up here."""
    from nbody_cosmological_simulation_amd import _native as N
    p = P.plan(row.n, row.d, is_f64=row.mode == "float64", mode=N.MODE_CODES[row.mode], work=False)
    if row.tiled is None:
        return
    if row.tiled == "onesided":
        assert not p["enabled"], (row, p)
    else:
        assert p["enabled"] and p["r"] == int(row.tiled[3:]), (row, p)


def run_b(nb, monkeypatch, tmp_path, row, unequal, names, label, profile=False):
    """Run B with the observers `names` after every segment, against run A.  Returns (sim, ctx)."""
    check_plan(row)
    ref = run_a(nb, row, unequal, profile)
    pe_sym = not any(n.endswith("_nosym") for n in names)
    if not pe_sym:
        monkeypatch.setenv("NB_NO_PE_SYM", "1")          # (knobs are read when the handle is created)
    sim = make(nb, row, initial_state(row, unequal), profile=profile)
    if not pe_sym:
        monkeypatch.delenv("NB_NO_PE_SYM")
    cx = Ctx(nb, row, sim, tmp_path, pe_sym)
    table = dict(OBSERVERS, **GRID_OBSERVERS)
    for i, seg in enumerate(SEGMENTS):
        advance(sim, seg)
        got = device_state(sim)
        for name in ("positions", "velocities", "accelerations"):
            assert same_bits(got[name], ref[i][name]), f"{label}: {name} differ after segment {i} {seg}"
        assert sim.force_kernel_name() == ref[i]["kernel"], (label, i)
        path = sim.step_path_name()
        if label in DROPS_SPECULATION:
            assert norm_path(path) == norm_path(ref[i]["path"]), (label, i, path, ref[i]["path"])
        else:
            assert path == ref[i]["path"], (label, i, path, ref[i]["path"])
        for name in names:
            table[name](cx)
            check_cache(sim, name)
        after = device_state(sim)
        for name in ("positions", "velocities", "accelerations"):
            assert same_bits(after[name], got[name]), f"{label}: the observers changed the device's {name} (segment {i})"
    return sim, cx


def _cases():
    out = []
    for row in ROWS:
        for name in list(OBSERVERS) + (list(GRID_OBSERVERS) if is_grid(row) else []):
            out.append(pytest.param(row, name, id=f"{row_id(row)}-{name}"))
    return out


@pytest.mark.parametrize("row,name", _cases())
def test_one_observer_between_segments_leaves_the_trajectory_alone(nb, monkeypatch, tmp_path, row, name):
    """Each observer alone, after every segment, on every path (unequal masses: the general-mass kernels)."""
    sim, _ = run_b(nb, monkeypatch, tmp_path, row, True, [name], name, profile=name == "kernel_time")
    sim.close()


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def checksums(k):
    k64 = np.asarray(k, np.int64)
    w = (np.arange(k64.shape[1], dtype=np.int64) % 65521) + 1
    return k64.sum(axis=1), (k64 * w[None, :]).sum(axis=1)


@pytest.mark.parametrize("masses", ["unequal", "equal"])
@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_all_observers_between_segments_and_the_read_outs_mid_run(nb, monkeypatch, tmp_path, row, masses):
    """All observers in one order after every segment, equal masses (uniform kernels, uniform potential) and unequal;
    then the read-outs themselves: oracle anchor, production bins of the current positions, fresh-handle restart."""
    from oracle import oracle as O
    unequal = masses == "unequal"
    names = list(ALL_ORDER) + (list(ALL_GRID_ORDER) if is_grid(row) else [])
    sim, cx = run_b(nb, monkeypatch, tmp_path, row, unequal, names, "all")
    pos0, vel0, mass = initial_state(row, unequal)

    # ---- oracle anchor: the bars of test_small_system_single_launch_step_vs_oracle for the mode
    ref = O.OracleSim(pos0, vel0, mass, row.mode, levels=row.levels or 0)
    ref.run(TICKS)
    p = sim._download("positions").numpy().astype(np.float64)
    v = sim._download("velocities").numpy().astype(np.float64)
    if row.mode == "float64":
        assert relerr(p, ref.positions) < 1e-13 and relerr(v, ref.velocities) < 1e-12
        assert abs(sim.get_total_energy() - ref.get_total_energy()) <= 1e-12 * abs(ref.get_total_energy())
    elif is_grid(row):
        err = np.abs(v - ref.velocities.astype(np.float64)).max(axis=1) / max(np.abs(ref.velocities).max(), 1e-30)
        print(f"{row_id(row)} {masses}: velocity error vs oracle q99 {np.quantile(err, 0.99):.3e} max {err.max():.3e}")
        assert np.quantile(err, 0.99) < (2e-6 if row.mode == "custom" else 2e-3)
        assert err.max() < (1e-3 if row.mode == "custom" else 5e-2)
    else:
        assert relerr(p, ref.positions) < 2e-6 and relerr(v, ref.velocities) < 2e-5

    # ---- grid modes: the production pair loop's bins and the grid's upper end, of the CURRENT positions
    if is_grid(row):
        cur = sim._download("positions").numpy()
        _, rdbg = O.accelerations(cur, mass, row.mode, levels=row.levels or 0, debug=True)
        want1, want2 = checksums(rdbg["d2bins"])
        bs = sim.quant_bin_sums("last")
        bad = np.nonzero((bs["sum_k"] != want1) | (bs["sum_kw"] != want2))[0]
        assert bad.size == 0, f"{bad.size} particles with a wrong bin checksum on path {bs['path']}, first {bad[:5]}"
        assert np.float32(sim.quant_debug()["lmax"]) == np.float32(rdbg["lmax"])
        check_cache(sim, "final bin read-out")

    # ---- a fresh handle from the downloaded state, the stored accelerations restored: same energies, same continuation
    state = {n: sim._download(n) for n in ("positions", "velocities", "masses", "accelerations")}
    fresh = nb.GalaxySimulation(state["positions"].clone(), state["velocities"].clone(), state["masses"].clone(),
                                precision_mode=nb.PrecisionMode(row.mode), softening=0.1, dt=0.01, custom_levels=row.levels)
    fresh.accelerations = state["accelerations"].clone()
    for get in ("get_kinetic_energy", "get_potential_energy", "get_total_energy"):
        a, b = getattr(sim, get)(), getattr(fresh, get)()
        assert np.float64(a).view(np.int64) == np.float64(b).view(np.int64), (get, a, b)
    sim.run(2)
    fresh.run(2)
    a, b = device_state(sim), device_state(fresh)
    for name in a:
        assert same_bits(a[name], b[name]), f"restart: {name} differ two ticks after the fresh handle took over"
    assert sim.force_kernel_name() == fresh.force_kernel_name()
    sim.close()
    fresh.close()


# ---- ensembles ------------------------------------------------------------------------------------------------------------
ENS_SEGMENTS = (("step", 1), ("run", 3), ("step", 1), ("run", 2))
ENS_G, ENS_SOFTENING, ENS_DT = [0.001, 0.002, 0.0015], [0.1, 0.05, 0.2], [0.01, 0.005, 0.02]


def make_ensemble(nb, mode, n, d):
    from nbody_cosmological_simulation_amd import ensemble
    rng = np.random.default_rng(7 * n + d)
    dt = np.float64 if mode == "float64" else np.float32
    pos = (rng.standard_normal((3, n, d)) * 3).astype(dt)
    vel = (rng.standard_normal((3, n, d)) * 0.05).astype(dt)
    mass = (0.5 + rng.random((3, n))).astype(dt)
    kw = dict(precision_mode=nb.PrecisionMode(mode), G=ENS_G, softening=ENS_SOFTENING, dt=ENS_DT)
    if mode in GRID:
        levels = [64, 32, 200] if mode == "custom" else None
        return ensemble.QuantizedEnsemble(T(pos), T(vel), T(mass), custom_levels=levels, **kw)
    return ensemble.GalaxyEnsemble(T(pos), T(vel), T(mass), **kw)


def observe_ensemble(ens, prev_positions, quantized):
    ke, pe = ens.energies()
    assert ke.shape == (3,) and torch.isfinite(ke).all() and torch.isfinite(pe).all()
    k, p, t = ens.get_kinetic_energy(), ens.get_potential_energy(), ens.get_total_energy()
    assert len(k) == len(p) == len(t) == 3 and np.isfinite(t).all()
    m = ens.metrics()
    assert (m.num_stars_per_bin.sum(axis=1) >= ens.num_stars - 1).all()      # (the farthest star is in no bin)
    still = ens.crash_measures()
    moved = ens.crash_measures(prev_positions)
    assert not still.has_nan.any() and (still.max_displacement == 0).all() and (moved.max_displacement > 0).all()
    for b in range(3):
        st = ens.get_state(b)
        assert same_bits(st["positions"], ens._download("positions")[b]) and st["tick"] == ens.member_ticks[b]
    assert ens.member_ticks == [ens.tick] * 3
    assert ens.launches() > 0 and ens.force_kernel_name() != "none"
    if quantized:
        q = ens.quant_debug()
        assert (q["lmax"] > q["lmin"]).all()
    ens.synchronize()


@pytest.mark.parametrize("n,d", [(96, 2), (96, 3), (700, 2), (700, 3)])
@pytest.mark.parametrize("mode", ["float64", "float32", "int8_sim", "custom"])
def test_ensemble_observers_between_segments_leave_every_member_alone(nb, mode, n, d):
    """GalaxyEnsemble / QuantizedEnsemble, three members with their own G, softening and dt: the observed ensemble's
    device state equals the unobserved one's bit for bit after every segment, member by member."""
    a, b = make_ensemble(nb, mode, n, d), make_ensemble(nb, mode, n, d)
    for i, seg in enumerate(ENS_SEGMENTS):
        prev = b._download("positions")
        advance(a, seg)
        advance(b, seg)
        for name in ("positions", "velocities", "accelerations"):
            x, y = a._download(name), b._download(name)
            for m in range(3):
                assert same_bits(x[m], y[m]), f"{name} of member {m} differ after segment {i} {seg}"
        assert a.tick == b.tick and a.launches() == b.launches() and a.force_kernel_name() == b.force_kernel_name()
        observe_ensemble(b, prev, mode in GRID)
        for name in ("positions", "velocities", "accelerations"):
            assert same_bits(b._download(name), a._download(name)), f"the observers changed the ensemble's {name}"
    a.close()
    b.close()
