"""Many small systems stepped together: `GalaxyEnsemble`.

The reference's sweeps (falsification_tests.py:284-356 over softening lengths and time steps,
reproducibility.py:362 over seeds, stability_test.py over precision modes, sensitivity_test.py and
jitter_test.py over one parameter) are Python loops of independent `GalaxySimulation`s with a few hundred to
a few thousand stars.  One such system is a single latency-bound kernel launch per tick that leaves most of
the chip idle.  A `GalaxyEnsemble` holds B of them -- same N, D, precision mode and state dtype; own
positions, velocities, masses, G, softening and dt -- and advances all of them one tick per launch
(include/nbody_amd.h nb_ens_*, csrc/nb_ensemble.hip).  No arithmetic crosses members, and every member's
state is bit-identical to the `GalaxySimulation` that takes the same steps.

Unlike `GalaxySimulation`, the array attributes are SNAPSHOTS: `positions`, `velocities`, `masses` and
`accelerations` return fresh (B, ...) tensors at every read, and in-place edits of them are not tracked.
Writes go through `set_state`, `set_accelerations` and `set_params`.

Energy curves -- what the sweeps above record -- stay on the device: `energies()` evaluates every member's kinetic
and potential energy in one batched pass (two launches, csrc/nb_ens_energy.hip) and `run_recorded(num_ticks, every)`
runs the ticks and samples the energies between them without a host round trip, returning an `EnergyHistory`.  Their
values agree with `get_kinetic_energy()` / `get_potential_energy()` (which stay solo-equal bit for bit, one member
at a time) to 1e-12 relative under FLOAT64 and 2e-6 under the other modes; `run_recorded` leaves the trajectory
bit-identical to `run`.

`GalaxyEnsemble` runs the FLOAT64 / FLOAT32 / BFLOAT16 / FLOAT16 modes; state already in its settled dtype (fp64
tensors under FLOAT64, fp32 under the others); N up to the one-launch step's limit (4096 fp64, 3072 fp32) --
above it a single system already fills the chip; B up to 1024; one device.

The grid modes -- what the reference's stability_test.py (INT8, INT4) and falsification_tests.py:44-104 (the number of
grid levels itself) and :284-356 (softening and time step under a 16-level grid) sweep -- are `QuantizedEnsemble`'s:
INT8_SIM, INT4_SIM and CUSTOM with `custom_levels` per member (2 .. 256), fp32 state, N up to 3072.  Every member has
its own quantisation tables, built on the device from its own exact max r^2, softening, G and level count, so they are
the tables of its solo run and the member stays bit-identical to `GalaxySimulation(custom_levels=levels[b])`.  A tick
is two launches over all members (max r^2 + tables, pair sweep) and under INT8 / INT4 a third (force snap + kicks);
`quant_debug()` reads every member's grid bounds back, and `quant_bin_sums()` the bin every pair was given: the solo
`quant_bin_sums` check-sums per member and star, read out of the production pair loop (its BINS instantiation) on the
members' current positions.  It is an observer -- the read-out's forces go to a scratch buffer, the tables are rebuilt from
the same positions -- so positions, velocities, accelerations, `tick`, `launches()` and every later tick stay bit-identical.
It inherits everything else from `GalaxyEnsemble`.

Finer grids -- the convergence sweep of falsification_tests.py:44-104 steps one galaxy under CUSTOM grids of 4, 8, ...
levels -- are `FineGridEnsemble`'s: a `QuantizedEnsemble` in CUSTOM mode whose `custom_levels` go up to
MAX_FINE_LEVELS = 4096, the capacity of the threshold tables (C-ABI nb_ens_create_grid_wide).  While no member exceeds
256 levels it launches exactly what `QuantizedEnsemble` launches ("ens_grid_step_kernel").  Otherwise a tick is still one
force launch, "ens_grid_step_wide_kernel" -- the same pair loop with the tables in LDS sized for the widest member -- behind
the max r^2 launch and one more tables launch that builds the multi-chunk tables of the members above 256 levels.  Contract:
  * a member with <= 256 levels is bit-identical to `GalaxySimulation(custom_levels=L)` on the one-launch path, whatever its
    neighbours' level counts (QuantizedEnsemble's contract);
  * a member with 257 .. 4096 levels has the tables of its solo run (`lmin`, `lmax`, `r2max` of `quant_debug()` equal the
    solo's exactly, `fast_path` is False); every pair gets the bin the reference gives it (`quant_bin_sums()` equals the
    check-sums of the reference formula's bin matrix and the solo `quant_bin_sums("tiled")` at the same positions, exactly) and the
    table entry the solo run uses, so its accelerations are the same fp32 products summed in the one-launch body's order:
    deterministic, independent of the other members, their order and number; `run(T)`, T calls of `step()`,
    `run_recorded(T, every)` and `run_members` with equal budgets give the same bits, and a stopped or halted member
    equals the same member run alone for as many ticks, bit for bit;
  * against the solo run -- which above 256 levels takes the tiled path and sums in another order -- accelerations and
    trajectories of such a member agree at the suite's bars (2e-6 relative), not bit for bit.

Galaxy diagnostics -- the rotation curve the sweeps record beside the energies, and `collect_metrics`' radius, bound
fraction and dispersion -- are batched too: `metrics(num_bins, max_radius, percentile)` evaluates all four diagnostics of
metrics.py for every member from the device-resident state in ONE launch (one workgroup per member,
csrc/nb_ens_metrics.hip: both rankings are sorted in LDS, the edges are built on the device from the member's own
maximum radius or its given `max_radius[b]`, G is the member's own) and returns an `EnsembleMetrics`.  Contract: every
per-star decision (bin membership, bound flag, order statistic) and every returned number equals what
`metrics.native_metrics` gives for that member alone wherever the value does not depend on the order of a float64 sum
-- bit for bit; where it can (the centre of mass, enclosed masses, bin means and dispersion of arbitrary masses) bin means
and dispersion agree to 2e-6 relative, `galaxy_radius`, counts and edges exactly and the bound fraction to 3 / N.  Members
never influence each other; the trajectory, the tick and `launches()` are untouched.  Not part of it: metric samples
inside `run_recorded`, float16 / bfloat16-typed evaluation (the state is fp32 or fp64), more than 255 bins, mixed dtypes.

Per-member tick counts -- what the time-step sweeps (falsification_tests.py:321-356 and jitter_test.py:193-250 give every
dt its own tick count so that the simulated time is equal) and the stability sweep (stability_test.py:33-61,94-105 stops a
system at the first check that finds it "exploded") need -- are `run_members(num_ticks, every)` and
`run_watched(max_ticks, check_interval)`, each ONE native call with no host round trip between ticks.  The members' stop
ticks live in a device array that every kernel of the tick path reads: a member that has taken its ticks is left alone by
every later launch.  Contract: member b takes exactly `num_ticks[b]` ticks, and its positions, velocities and
accelerations are then bit-identical to the `GalaxySimulation` that took as many steps (a budget of 0: not touched);
later calls of any kind go on from there as the solo run would; `launches()` and `tick` grow by the largest budget,
`member_ticks[b]` by the member's own ticks.  Samples follow `run_recorded`'s rule, and a stopped member keeps being
sampled at its frozen state.  `run_watched` applies the reference's three explosion criteria (`explosion_reason` is their
definition) on the device at every check after the first sample, to every member that is still running; a member that trips
one is halted at that tick, its state that of its solo run of `stable_ticks[b]` steps, and tick and reason are read back
once, in a `StabilityReport`.  The decision uses the batched energies of `run_recorded` (at the bars above, not the solo
engine's bits), exactly as `explosion_reason` applied to the returned history gives it.  With equal budgets `run_members`
is `run_recorded`, launch for launch and bit for bit.  `QuantizedEnsemble` inherits all of it: a stopped member's tables,
force bounds and `quant_debug()` stay those of its last evaluation, which is its solo run's last.

Crash points -- the reference's crash_point_test.py:142-466 sweeps velocity multipliers, time steps, grid levels and
softening lengths, steps every system tick by tick and asks detect_crash (:46-139) after each tick whether it has "crashed":
eight whole-array reductions and six criteria, two of them about the motion since the tick before -- are
`run_crash_watched(max_ticks)`, ONE native call: every tick is sampled, and behind its energy launches one more launch
(csrc/nb_ens_crash.hip, one workgroup per member) measures every running member against its positions of the tick before
and applies the criteria on the device, in the reference's order, halting the member at that tick.  `crash_kind` is the
definition of the decision and `crash_value` / `crash_severity` give the reference's report fields; the result is a
`CrashPointReport`.  `crash_measures(prev_positions)` is the same kernel on the resident state alone and returns the
`CrashMeasures`.  Contract of the measures: in the state dtype, a star's squared norm is (c0*c0 + c1*c1) + c2*c2 with
separate multiplies and adds (torch's order for a last dimension of 2 or 3); `max_displacement`, `max_speed` and
`max_radius` are the correctly rounded roots of the largest squared norm of pos - prev, vel and pos; `max_abs_velocity` is
the largest |component|; the NaN / Inf flags cover positions and velocities; the maxima of a member that has either flag
are not defined (the reference returns before it computes them).  The decision uses the batched energies of `run_recorded`
(E of the tick's sample against the sample before), exactly as `crash_kind` applied to the returned history and measures
gives it.  A halted member's state is that of its solo run of `ticks_taken[b]` steps, bit for bit, `stable_ticks[b]` is the
reference's 0-based index of the tick whose check fired, and later calls go on from there; `tick`, `member_ticks` and
`launches()` move as under `run_members`, and a halted QuantizedEnsemble member keeps the tables of its last evaluation.

Members of different cast modes -- the reference's comparison runs put FLOAT32 beside FLOAT16 (reality_glitch_tests.py:
148-256, whose universe C rounds r^2 through half() exactly as PrecisionMode.FLOAT16 does; simulation.py:199-250
run_comparison) -- share one ensemble: `precision_mode` may be a list of B modes drawn from FLOAT32, BFLOAT16 and FLOAT16
(`check_mode_list`), `precision_modes` always holds the B modes in force, and a tick is still ONE force launch
("ens_step_mixed_kernel": the member's hook is read per workgroup, the step body is the uniform kernel's).  Contract: member
b is bit-identical to the `GalaxySimulation` of mode `precision_modes[b]`, no tolerance; every other method works unchanged.
A list whose entries are all equal is the scalar mode (FLOAT64 included).  FLOAT64 cannot be mixed in (different storage
type), nor the grid modes (per-member tables: `QuantizedEnsemble`).

Divergence between members -- what those comparison loops and omega_point_test.py:665-766 (_test_point) read back after
every tick as (a.positions - b.positions).abs().max().item() -- is measured on the device: `divergence(baseline)` compares
every member b with member `baseline[b]` (an int: one member for all) in one launch (csrc/nb_ens_diverge.hip, one workgroup
per member) and returns a `Divergence`; `run_diverged(num_ticks, every, baseline, energies)` runs the ticks and samples the
divergence (and, asked for, the energies of run_recorded) between them with no host round trip, returning a
`DivergenceHistory`.  Sampling rule: sample 0 is the state at entry, sample s the state after tick s * every of the call; a
sampled tick is issued closed, so the trajectory is bit-identical to run(num_ticks).  Contract of the values: differences
are formed in the state dtype, one subtraction each; `max_position` / `max_velocity` equal torch's
(a - b).abs().max() widened to double -- NaN rule: NaN if any element is NaN (inf - inf included), +inf an ordinary value;
`mean_position` is a fixed-order fp64 sum over n * D divided in double (deterministic; NaN if any term is; within
n * D * 2^-53 relative of any other fp64 order).  `entropy_bits` and `divergence_rate` are the reference's derived
quantities in numpy float64.

Members of different sizes -- the reference's density sweeps (omega_point_test.py:595-766 scans 100 .. 2000 stars, two
simulations per point with the divergence read back every tick; density_limit_test.py:206-246 runs 100 .. 4000) -- are
`RaggedEnsemble`'s, for the cast modes: `positions` / `velocities` / `masses` are sequences of per-member (N_b, D) / (N_b,)
tensors (`check_ragged_arguments`), `precision_mode` one mode or a list as above, and a tick is still ONE force launch
("ens_step_ragged_kernel", csrc/nb_ens_ragged.hip: a 1-D grid over a work list of {member, target block}, largest members
first).  Storage is padded to the largest member -- the constructor pads with NaN, and no kernel reads or writes a padding
row.  Contract: member b is bit-identical to the `GalaxySimulation` of its own size and mode, no tolerance (a target's sum
does not depend on the workgroup size, so the one size of the launch serves every N); `energies()`, the samples of
`run_recorded` and the get_*_energy() lists of member b equal those of a one-member `GalaxyEnsemble` of the same system bit
for bit; step, run, run_recorded, run_members, run_watched, divergence and run_diverged are inherited, the last two with
baselines of the member's own size (ValueError otherwise).  `num_stars` is the list of sizes; the array attributes return
lists of per-member tensors and `set_state` / `set_accelerations` take them.  `metrics`, `run_crash_watched` and
`crash_measures` raise NotImplementedError: ragged metrics and the ragged crash watch are follow-ups.

The grid half of those sweeps -- the scan's "int8" / "int4" points and the density test's "broken" runs are 256- and
16-level grids on r^2 -- is `RaggedQuantizedEnsemble`'s: a `RaggedEnsemble` under INT8_SIM, INT4_SIM or CUSTOM with
`custom_levels` per member (2 .. 256; `check_ragged_grid_arguments`), fp32 state, N_b up to 3072 (C-ABI
nb_ens_create_ragged_grid).  A tick is QuantizedEnsemble's launches whatever the sizes: max r^2 + tables over all members
(a workgroup beyond its member's size returns at once, and the last of the member's OWN workgroups builds its tables), ONE
force launch over the work list ("ens_grid_step_ragged_kernel") and under INT8 / INT4 the force snap + kicks.  Contract:
member b is bit-identical to `GalaxySimulation(..., precision_mode, custom_levels=levels[b])` of its own size, no
tolerance -- positions, velocities and accelerations after every tick, the `quant_debug()` values (length-B arrays, as
QuantizedEnsemble's) and the bins of `quant_bin_sums()` (`sum_k` / `sum_kw`: lists of per-member (N_b,) arrays) -- because
a wave holds the same pairs at the ragged launch's 512 threads as at the 256 a solo run takes for N in 2049 .. 3072
(DESIGN.md 4.9); no kernel reads or writes a padding row; a stopped member keeps the tables and force bounds of its last
evaluation.  Everything RaggedEnsemble inherits works, and its three refusals stand; a member above 256 levels is refused
(ValueError: the ragged wide grid is a follow-up, `FineGridEnsemble` serves members of one size).

Not covered: more than 4096 levels (a solo `GalaxySimulation` serves them through its generic kernel), INT8 / INT4 beside
CUSTOM members, FLOAT64 or grid-mode members beside cast-mode members, stopping members on a divergence
threshold, a crash check interval other than 1, crash thresholds
other than the reference's constants,
compacting the launch grid as members finish (a finished member costs its workgroups one load each), mixed dtypes and the
fp32 -> fp64 promotion timeline, subclass overrides, checkpoints, multi-GPU.
"""
import ctypes as C
import numbers
from collections.abc import Sequence
from typing import Callable, NamedTuple

import torch

from . import _native as N
from . import runtime
from .quantization import PrecisionMode, mode_code, _TORCH_TO_NB

MAX_MEMBERS = 1024
MAX_STARS = {torch.float64: 4096, torch.float32: 3072}     # the solo one-launch step's limits (csrc/nb_step.cpp)
MAX_BINS = 255                        # rotation-curve bins of metrics() (csrc/nb_ens_metrics.hip: the edges live in LDS)
MAX_HISTORY_BYTES = 256 << 20         # an EnergyHistory's kinetic + potential samples (16 bytes per member and sample)
DIVERGENCE_SAMPLE_BYTES = 24          # a DivergenceHistory's three values per member and sample, under the same limit
_MODES = (PrecisionMode.FLOAT64, PrecisionMode.FLOAT32, PrecisionMode.BFLOAT16, PrecisionMode.FLOAT16)
_GRID_MODES = (PrecisionMode.INT8_SIM, PrecisionMode.INT4_SIM, PrecisionMode.CUSTOM)
MIN_LEVELS, MAX_LEVELS = 2, 256       # MAX_LEVELS: above it the solo engine leaves the one-launch step (csrc/nb_step.cpp)
MAX_FINE_LEVELS = 4096                # FineGridEnsemble: the threshold tables' capacity (csrc/nb_internal.h NB_MAX_LUT)
DEFAULT_CUSTOM_LEVELS = 64            # the reference's default (quantization.py:67)
# why run_watched halted a member (include/nbody_amd.h NB_ENS_REASON_*; `explosion_reason`)
REASON_NONE, REASON_NONFINITE, REASON_ENERGY, REASON_UNBOUND = 0, 1, 2, 3
# why run_crash_watched halted a member, in the reference's order of precedence (include/nbody_amd.h NB_ENS_CRASH_*;
# `crash_kind`), and the reference's crash_type strings (crash_point_test.py:61-137)
CRASH_NONE, CRASH_NAN, CRASH_INF, CRASH_TELEPORT, CRASH_VELOCITY, CRASH_ENERGY, CRASH_RADIUS = range(7)
CRASH_TYPES = ("", "NaN_EXPLOSION", "INFINITY_OVERFLOW", "TELEPORTATION", "VELOCITY_OVERFLOW", "ENERGY_SINGULARITY",
               "GALAXY_EXPLOSION")


def state_dtype(precision_mode) -> torch.dtype:
    """The settled state dtype of a mode: what positions, velocities, masses and accelerations all have."""
    return torch.float64 if precision_mode == PrecisionMode.FLOAT64 else torch.float32


def _typed(name, v, kind=numbers.Integral, what="an int"):
    """`v` if it is a `kind` (numbers.Integral or numbers.Real) and no bool, else TypeError "`name` must be `what`, got
    <type>"."""
    if isinstance(v, bool) or not isinstance(v, kind):
        raise TypeError(f"{name} must be {what}, got {type(v).__name__}")
    return v


def _scalar_or_list(value, noun, kind, what, check=None, loose=False):
    """An argument that is one value for all members or one per member -> a Python scalar or a list.  Tensors and numpy
    arrays / scalars go through tolist(), lists, tuples and other Sequences (range and the like) become lists.  Every
    entry must pass `_typed(noun, entry, kind, what)`; `check(entry)` follows each entry's type test.  loose (the
    constructors' G / softening / dt, as they have always been read): only tensors, lists and tuples count as sequences and
    float() alone judges their entries."""
    if isinstance(value, torch.Tensor) or not loose and type(value).__module__ == "numpy" and hasattr(value, "tolist"):
        value = value.tolist()
    elif isinstance(value, (list, tuple)) or not loose and isinstance(value, Sequence) and not isinstance(value, (str, bytes)):
        value = list(value)
    for v in (value if not loose else []) if isinstance(value, list) else [value]:
        _typed(noun, v, kind, what)
        if check is not None:
            check(v)
    return value


def _param_list(name, value, members):
    """A float, or a sequence of `members` floats -> list of floats (members None: any length)."""
    value = _scalar_or_list(value, name, numbers.Real, "a float or a sequence of floats", loose=True)
    if isinstance(value, list):
        out = [float(v) for v in value]
        if members is not None and len(out) != members:
            raise ValueError(f"{name} has {len(out)} entries for {members} members")
        return out
    return None if members is None else [float(value)] * members


def check_arguments(positions, velocities, masses, precision_mode=PrecisionMode.FLOAT64, G=0.001, softening=0.1, dt=0.01):
    """Validate constructor arguments without touching a device.  Returns (positions, velocities, masses, G, softening,
    dt) with the tensors shaped (B, N, D) / (B, N) and the parameters as length-B lists; raises ValueError / TypeError."""
    if not isinstance(precision_mode, PrecisionMode):
        raise TypeError(f"precision_mode must be a PrecisionMode, got {type(precision_mode).__name__}")
    if precision_mode not in _MODES:
        raise ValueError(f"GalaxyEnsemble runs the FLOAT64, FLOAT32, BFLOAT16 and FLOAT16 modes; {precision_mode.name} needs "
                         "per-member quantisation tables (use GalaxySimulation)")
    return _check_state(positions, velocities, masses, precision_mode, G, softening, dt)


def check_mode_list(modes, members=None) -> list:
    """Validate a per-member list of precision modes without touching a device: `members` entries (None: any length),
    all equal (any cast mode or FLOAT64: the uniform ensemble of that mode) or drawn from FLOAT32, BFLOAT16 and FLOAT16.
    Returns the list; raises TypeError / ValueError naming the reason."""
    if isinstance(modes, (str, bytes)) or not isinstance(modes, Sequence):
        raise TypeError(f"precision modes must be a sequence of PrecisionMode, got {type(modes).__name__}")
    modes = list(modes)
    for m in modes:
        if not isinstance(m, PrecisionMode):
            raise TypeError(f"precision modes must be PrecisionMode values, got {type(m).__name__}")
    if not modes:
        raise ValueError("precision modes: an empty list")
    if members is not None and len(modes) != int(members):
        raise ValueError(f"precision_mode has {len(modes)} entries for {int(members)} members")
    for b, m in enumerate(modes):
        if m in _GRID_MODES:
            raise ValueError(f"precision_mode[{b}] = {m.name}: a grid mode needs per-member quantisation tables, which the "
                             "cast-mode members of a GalaxyEnsemble do not have (use QuantizedEnsemble)")
    if len(set(modes)) > 1:
        for b, m in enumerate(modes):
            if m == PrecisionMode.FLOAT64:
                raise ValueError(f"precision_mode[{b}] = FLOAT64 beside other modes: FLOAT64 members have a different storage "
                                 "type (fp64 state) from FLOAT32 / BFLOAT16 / FLOAT16 members (fp32) and cannot share an "
                                 "ensemble with them")
    return modes


def _mode_or_list(precision_mode):
    """One precision mode or a list of them, as the cast-mode constructors take it -> (modes, storage): the checked list
    (`check_mode_list`; its length is the caller's to check) and the mode the state is stored and checked under -- the
    list's one mode, else FLOAT32 -- or (None, precision_mode) for anything that is no list: the caller judges it."""
    if not isinstance(precision_mode, (list, tuple)):
        return None, precision_mode
    modes = check_mode_list(precision_mode)
    return modes, modes[0] if len(set(modes)) == 1 else PrecisionMode.FLOAT32


def _check_tensor(name, t, member=None, shape=None, dtype=None, mode=None):
    """The per-tensor tests of every state check, in this order: `t` is a tensor, has `shape` (None: not tested) and
    `dtype` (None: not tested; mode: the settled dtype of that precision mode, and the refusal says so).  member: `t` is
    entry `member` of the list `name`, and the refusals name it."""
    label = name if member is None else f"{name}[{member}]"
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{label} must be a torch.Tensor" + ("" if member is None else f", got {type(t).__name__}"))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{label} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if dtype is not None and t.dtype != dtype:
        if mode is None:
            raise TypeError(f"{label} must be {dtype}, got {t.dtype}")
        raise TypeError(f"{label} must be {dtype} under {mode.name} (got {t.dtype}): an ensemble holds settled state only; "
                        "mixed dtypes and the promotion timeline are GalaxySimulation's")


def _check_state(positions, velocities, masses, precision_mode, G, softening, dt, more_lists=()):
    """check_arguments behind the mode check; more_lists: lengths of further per-member lists a lone galaxy is broadcast over."""
    for name, t in (("positions", positions), ("velocities", velocities), ("masses", masses)):
        _check_tensor(name, t)
    if positions.dim() == 2 and masses.dim() == 1:
        # one galaxy under a parameter sweep: as many members as the longest parameter list
        lens = [len(p) for p in (_param_list("G", G, None), _param_list("softening", softening, None),
                                 _param_list("dt", dt, None)) if p is not None] + list(more_lists)
        members = max(lens) if lens else 1
        if velocities.dim() != 2:
            raise ValueError(f"velocities must be (N, D) like positions, got {tuple(velocities.shape)}")
        positions, velocities, masses = (t.unsqueeze(0).expand(members, *t.shape) for t in (positions, velocities, masses))
    if positions.dim() != 3 or masses.dim() != 2:
        raise ValueError(f"positions must be (B, N, D) with (B, N) masses, or (N, D) with (N,) masses; got "
                         f"{tuple(positions.shape)} and {tuple(masses.shape)}")
    B, n, d = (int(v) for v in positions.shape)
    if d not in (2, 3):
        raise ValueError(f"D must be 2 or 3, got {d}")
    if tuple(velocities.shape) != (B, n, d) or tuple(masses.shape) != (B, n):
        raise ValueError(f"positions {tuple(positions.shape)}, velocities {tuple(velocities.shape)} and masses "
                         f"{tuple(masses.shape)} disagree on (B, N, D)")
    if not 1 <= B <= MAX_MEMBERS:
        raise ValueError(f"B must be in [1, {MAX_MEMBERS}], got {B}")
    want = state_dtype(precision_mode)
    for name, t in (("positions", positions), ("velocities", velocities), ("masses", masses)):
        _check_tensor(name, t, dtype=want, mode=precision_mode)
    if not 1 <= n <= MAX_STARS[want]:
        raise ValueError(f"N must be in [1, {MAX_STARS[want]}] for {want} state, got {n}: above it a single system fills the "
                         "chip (use GalaxySimulation)")
    return (positions, velocities, masses, _param_list("G", G, B), _param_list("softening", softening, B),
            _param_list("dt", dt, B))


def check_ragged_arguments(positions, velocities, masses, precision_mode=PrecisionMode.FLOAT64, G=0.001, softening=0.1,
                           dt=0.01):
    """Validate RaggedEnsemble's constructor arguments without touching a device.  `positions` / `velocities`: sequences of
    B tensors (N_b, D); `masses`: a sequence of B tensors (N_b,); `precision_mode`: one cast mode or a list of B modes as
    GalaxyEnsemble takes it.  Returns (positions, velocities, masses, sizes, modes, G, softening, dt): the three as lists,
    the B star counts, the checked mode list (None for one mode) and the parameters as length-B lists; raises TypeError /
    ValueError naming the member."""
    modes, storage = _mode_or_list(precision_mode)
    if modes is None and not isinstance(precision_mode, PrecisionMode):
        raise TypeError(f"precision_mode must be a PrecisionMode or a list of them, got {type(precision_mode).__name__}")
    if modes is None and precision_mode not in _MODES:
        raise ValueError(f"RaggedEnsemble runs the FLOAT64, FLOAT32, BFLOAT16 and FLOAT16 modes; {precision_mode.name} needs "
                         "per-member quantisation tables (the ragged grid modes are a follow-up; members of one size: "
                         "QuantizedEnsemble)")
    positions, velocities, masses, sizes, G, softening, dt = _check_ragged_state(positions, velocities, masses, storage, G,
                                                                                 softening, dt, modes)
    return positions, velocities, masses, sizes, modes, G, softening, dt


def _check_ragged_state(positions, velocities, masses, storage, G, softening, dt, modes=None, more_lists=()):
    """check_ragged_arguments / check_ragged_grid_arguments behind their own mode rules: the three lists, every member's
    tensors under the storage mode `storage`, the sizes and the parameters as length-B lists.  modes: a mode list, whose
    length is checked once B is known; more_lists: (name, length) of further per-member lists, checked the same way."""
    lists = []
    for name, seq in (("positions", positions), ("velocities", velocities), ("masses", masses)):
        if isinstance(seq, torch.Tensor) or isinstance(seq, (str, bytes)) or not isinstance(seq, Sequence):
            raise TypeError(f"{name} must be a sequence of per-member tensors, got {type(seq).__name__} (members of one size: "
                            "GalaxyEnsemble)")
        lists.append(list(seq))
    positions, velocities, masses = lists
    B = len(positions)
    if len(velocities) != B or len(masses) != B:
        raise ValueError(f"positions has {B} members, velocities {len(velocities)} and masses {len(masses)}: the three lists "
                         "must have one entry per member")
    if not 1 <= B <= MAX_MEMBERS:
        raise ValueError(f"B must be in [1, {MAX_MEMBERS}], got {B}")
    if modes is not None:
        check_mode_list(modes, B)
    for name, length in more_lists:
        if length != B:
            raise ValueError(f"{name} has {length} entries for {B} members")
    want = state_dtype(storage)
    sizes, dim = [], None
    for b in range(B):
        for name, t in (("positions", positions[b]), ("velocities", velocities[b]), ("masses", masses[b])):
            _check_tensor(name, t, b)
        if positions[b].dim() != 2 or masses[b].dim() != 1:
            raise ValueError(f"member {b}: positions must be (N, D) with (N,) masses, got {tuple(positions[b].shape)} and "
                             f"{tuple(masses[b].shape)}")
        n, d = (int(v) for v in positions[b].shape)
        if d not in (2, 3):
            raise ValueError(f"member {b}: D must be 2 or 3, got {d}")
        if dim is not None and d != dim:
            raise ValueError(f"member {b} has D = {d} and member 0 has D = {dim}: the members of an ensemble share D")
        dim = d
        if n < 1:
            raise ValueError(f"member {b} is empty: every member needs at least one star")
        if tuple(velocities[b].shape) != (n, d) or tuple(masses[b].shape) != (n,):
            raise ValueError(f"member {b}: positions {tuple(positions[b].shape)}, velocities {tuple(velocities[b].shape)} and "
                             f"masses {tuple(masses[b].shape)} disagree on (N, D)")
        for name, t in (("positions", positions[b]), ("velocities", velocities[b]), ("masses", masses[b])):
            _check_tensor(name, t, b, dtype=want, mode=storage)
        if n > MAX_STARS[want]:
            raise ValueError(f"member {b} has N = {n}, above the limit of {MAX_STARS[want]} for {want} state: a single system "
                             "of that size fills the chip (use GalaxySimulation)")
        sizes.append(n)
    return (positions, velocities, masses, sizes, _param_list("G", G, B), _param_list("softening", softening, B),
            _param_list("dt", dt, B))


def _level_list(value):
    """custom_levels as given -> None, an int, or a list of ints (entries type-checked, not yet range- or length-checked)."""
    if value is None:
        return None
    value = _scalar_or_list(value, "custom_levels", numbers.Integral, "an int or a sequence of ints")
    return [int(v) for v in value] if isinstance(value, list) else int(value)


def _grid_arguments(positions, velocities, masses, precision_mode, levels, cap, tail, G, softening, dt):
    """check_grid_arguments / check_fine_grid_arguments behind their own mode rules: `levels` (from _level_list) in
    [MIN_LEVELS, cap] -- tail(v) ends the refusal of a v outside --, the state, and the levels as a length-B list."""
    for v in (levels if isinstance(levels, list) else [levels] if levels is not None else []):
        if not MIN_LEVELS <= v <= cap:
            raise ValueError(f"custom_levels must be in [{MIN_LEVELS}, {cap}], got {v}{tail(v)}")
    positions, velocities, masses, G, softening, dt = _check_state(
        positions, velocities, masses, precision_mode, G, softening, dt, [len(levels)] if isinstance(levels, list) else [])
    B = int(positions.shape[0])
    if precision_mode == PrecisionMode.INT8_SIM:
        levels = [256] * B
    elif precision_mode == PrecisionMode.INT4_SIM:
        levels = [16] * B
    elif levels is None:
        levels = [DEFAULT_CUSTOM_LEVELS] * B
    elif not isinstance(levels, list):
        levels = [levels] * B
    elif len(levels) != B:
        raise ValueError(f"custom_levels has {len(levels)} entries for {B} members")
    return positions, velocities, masses, levels, G, softening, dt


def check_grid_arguments(positions, velocities, masses, precision_mode=PrecisionMode.INT8_SIM, custom_levels=None, G=0.001,
                         softening=0.1, dt=0.01):
    """Validate QuantizedEnsemble's constructor arguments without touching a device.  Returns (positions, velocities,
    masses, levels, G, softening, dt) with the tensors shaped (B, N, D) / (B, N) and levels and the parameters as length-B
    lists; raises ValueError / TypeError."""
    if not isinstance(precision_mode, PrecisionMode):
        raise TypeError(f"precision_mode must be a PrecisionMode, got {type(precision_mode).__name__}")
    if precision_mode not in _GRID_MODES:
        raise ValueError(f"QuantizedEnsemble runs the INT8_SIM, INT4_SIM and CUSTOM modes; {precision_mode.name} is "
                         "GalaxyEnsemble's")
    levels = _level_list(custom_levels)
    if precision_mode != PrecisionMode.CUSTOM and levels is not None:
        fixed = 256 if precision_mode == PrecisionMode.INT8_SIM else 16
        raise ValueError(f"custom_levels belongs to the CUSTOM mode: {precision_mode.name} has {fixed} levels (pass None)")
    tail = (f": above {MAX_LEVELS} a solo run leaves the one-launch step, so a member would have no bit-identical "
            "counterpart")
    return _grid_arguments(positions, velocities, masses, precision_mode, levels, MAX_LEVELS, lambda v: tail, G, softening, dt)


def check_fine_grid_arguments(positions, velocities, masses, custom_levels=None, G=0.001, softening=0.1, dt=0.01):
    """Validate FineGridEnsemble's constructor arguments without touching a device: check_grid_arguments under CUSTOM with
    the level range [2, MAX_FINE_LEVELS].  Returns (positions, velocities, masses, levels, G, softening, dt) as there; raises
    ValueError / TypeError."""
    def tail(v):
        return (": a solo GalaxySimulation(custom_levels=...) serves such grids through its generic kernel"
                if v > MAX_FINE_LEVELS else "")
    return _grid_arguments(positions, velocities, masses, PrecisionMode.CUSTOM, _level_list(custom_levels), MAX_FINE_LEVELS,
                           tail, G, softening, dt)


def check_ragged_grid_arguments(positions, velocities, masses, precision_mode=PrecisionMode.INT8_SIM, custom_levels=None,
                                G=0.001, softening=0.1, dt=0.01):
    """Validate RaggedQuantizedEnsemble's constructor arguments without touching a device: the lists of
    check_ragged_arguments (fp32 state) under the mode and level rules of check_grid_arguments.  Returns (positions,
    velocities, masses, sizes, levels, G, softening, dt): the three as lists, the B star counts, and the levels and the
    parameters as length-B lists; raises TypeError / ValueError naming the member."""
    if not isinstance(precision_mode, PrecisionMode):
        raise TypeError(f"precision_mode must be a PrecisionMode, got {type(precision_mode).__name__}")
    if precision_mode not in _GRID_MODES:
        raise ValueError(f"RaggedQuantizedEnsemble runs the INT8_SIM, INT4_SIM and CUSTOM modes; {precision_mode.name} is "
                         "RaggedEnsemble's")
    levels = _level_list(custom_levels)
    if precision_mode != PrecisionMode.CUSTOM and levels is not None:
        fixed = 256 if precision_mode == PrecisionMode.INT8_SIM else 16
        raise ValueError(f"custom_levels belongs to the CUSTOM mode: {precision_mode.name} has {fixed} levels (pass None)")
    for v in (levels if isinstance(levels, list) else [levels] if levels is not None else []):
        if not MIN_LEVELS <= v <= MAX_LEVELS:
            tail = (f": above {MAX_LEVELS} levels with members of different sizes is a follow-up (members of one size: "
                    "FineGridEnsemble)") if v > MAX_LEVELS else ""
            raise ValueError(f"custom_levels must be in [{MIN_LEVELS}, {MAX_LEVELS}], got {v}{tail}")
    positions, velocities, masses, sizes, G, softening, dt = _check_ragged_state(
        positions, velocities, masses, precision_mode, G, softening, dt,
        more_lists=[("custom_levels", len(levels))] if isinstance(levels, list) else ())
    B = len(sizes)
    if precision_mode == PrecisionMode.INT8_SIM:
        levels = [256] * B
    elif precision_mode == PrecisionMode.INT4_SIM:
        levels = [16] * B
    elif levels is None:
        levels = [DEFAULT_CUSTOM_LEVELS] * B
    elif not isinstance(levels, list):
        levels = [levels] * B
    return positions, velocities, masses, sizes, levels, G, softening, dt


def check_record_arguments(num_ticks, every, members) -> list:
    """Validate run_recorded's arguments without touching a device.  Returns the tick offsets of the samples relative to
    the tick at entry, [0, every, 2 * every, ...] up to num_ticks; raises TypeError / ValueError."""
    for name, v in (("num_ticks", num_ticks), ("every", every), ("members", members)):
        _typed(name, v)
    num_ticks, every, members = int(num_ticks), int(every), int(members)
    if num_ticks < 0:
        raise ValueError(f"num_ticks must be >= 0, got {num_ticks}")
    if every < 1:
        raise ValueError(f"every must be >= 1, got {every}")
    if members < 1:
        raise ValueError(f"members must be >= 1, got {members}")
    samples = 1 + num_ticks // every
    if samples * members * 16 > MAX_HISTORY_BYTES:
        raise ValueError(f"{samples} samples of {members} members are {samples * members * 16} bytes of history, above the "
                         f"limit of {MAX_HISTORY_BYTES}: raise `every` (or record the run in shorter stretches)")
    return list(range(0, num_ticks + 1, every))


def check_member_ticks_arguments(num_ticks, every, members):
    """Validate run_members' arguments without touching a device.  `num_ticks`: an int (every member's budget) or a
    sequence, tensor or numpy array of `members` ints, each >= 0; `every`: None (no samples) or an int >= 1.  Returns
    (budgets, offsets): the length-`members` list of budgets and the tick offsets of the samples relative to the tick at
    entry, [0, every, 2 * every, ...] up to the largest budget (None without samples); raises TypeError / ValueError."""
    members = int(_typed("members", members))
    if members < 1:
        raise ValueError(f"members must be >= 1, got {members}")
    if every is not None:
        _typed("every", every, what="None or an int")
    num_ticks = _scalar_or_list(num_ticks, "num_ticks", numbers.Integral, "an int or a sequence of ints")
    if isinstance(num_ticks, list) and len(num_ticks) != members:
        raise ValueError(f"num_ticks has {len(num_ticks)} entries for {members} members")
    budgets = [int(v) for v in num_ticks] if isinstance(num_ticks, list) else [int(num_ticks)] * members
    for v in budgets:
        if v < 0:
            raise ValueError(f"num_ticks must be >= 0, got {v}")
        if v >= 2 ** 31:
            raise ValueError(f"num_ticks must fit an int32, got {v}")
    if every is None:
        return budgets, None
    return budgets, check_record_arguments(max(budgets), int(every), members)


def check_divergence_arguments(num_ticks, every, baseline, members):
    """Validate run_diverged's arguments without touching a device (divergence(): num_ticks = 0, every = 1).  `baseline`:
    an int (one member for all) or a sequence, tensor or numpy array of `members` ints, each in [0, members).  Returns
    (baselines, offsets): the length-`members` list and the tick offsets of the samples relative to the tick at entry;
    raises TypeError / ValueError."""
    offsets = check_record_arguments(num_ticks, every, members)
    members = int(members)
    baseline = _scalar_or_list(baseline, "baseline", numbers.Integral, "an int or a sequence of ints")
    if isinstance(baseline, list) and len(baseline) != members:
        raise ValueError(f"baseline has {len(baseline)} entries for {members} members")
    baselines = [int(v) for v in baseline] if isinstance(baseline, list) else [int(baseline)] * members
    for v in baselines:
        if not 0 <= v < members:
            raise ValueError(f"baseline must name a member, 0 .. {members - 1}, got {v}")
    if len(offsets) * members * DIVERGENCE_SAMPLE_BYTES > MAX_HISTORY_BYTES:
        raise ValueError(f"{len(offsets)} samples of {members} members are {len(offsets) * members * DIVERGENCE_SAMPLE_BYTES} "
                         f"bytes of divergence history, above the limit of {MAX_HISTORY_BYTES}: raise `every` (or record the "
                         "run in shorter stretches)")
    return baselines, offsets


def entropy_bits(max_position_diff):
    """The reference's "bits of uncertainty" of a largest position difference (reality_glitch_tests.py:245-247), elementwise
    in numpy float64: log2(x / 1e-10 + 1) where x > 1e-10, else 0.0 (a NaN compares false: 0.0)."""
    import numpy as np
    x = np.asarray(max_position_diff, np.float64)
    out = np.zeros(x.shape, np.float64)
    hit = x > 1e-10
    out[hit] = np.log2(x[hit] / 1e-10 + 1)
    return out if out.ndim else float(out)


def divergence_rate(series):
    """The reference's Lyapunov-style rate (reality_glitch_tests.py:250-253) of a series of largest position differences as
    the reference accumulates it, one value per step(), along axis 0: entry i is
    log(max(series[i-1], 1e-15) / series[i-10]) / 10 if i > 10 and series[i-10] > 1e-15, else 0.0 -- the window is the ten
    entries before the current one.  numpy float64, with Python's max() as the reference calls it."""
    import numpy as np
    x = np.asarray(series, np.float64)
    if x.ndim < 1:
        raise ValueError("divergence_rate needs a series (one value per step)")
    out = np.zeros(x.shape, np.float64)
    if x.shape[0] <= 11:
        return out
    cols_in, cols_out = x.reshape(x.shape[0], -1), out.reshape(x.shape[0], -1)       # (views: out is filled through cols_out)
    for i in range(11, x.shape[0]):
        for c in range(cols_in.shape[1]):
            first, last = cols_in[i - 10, c], cols_in[i - 1, c]
            if first > 1e-15:
                with np.errstate(all="ignore"):
                    cols_out[i, c] = np.log(max(last, 1e-15) / first) / 10
    return out


def explosion_reason(initial_energy, energy, finite) -> int:
    """The reference's detect_explosion (stability_test.py:34-61) with the criterion that fired: the definition of what
    run_watched decides on the device for one member at one check.  `finite`: all of the member's positions and
    velocities are finite.  The comparisons are the reference's own, in its order, so a NaN energy trips nothing."""
    initial_energy, energy = float(initial_energy), float(energy)
    if not finite:
        return REASON_NONFINITE
    if abs(initial_energy) > 1e-10 and abs(energy - initial_energy) / abs(initial_energy) > 10.0:
        return REASON_ENERGY
    if initial_energy < 0 and energy > abs(initial_energy):
        return REASON_UNBOUND
    return REASON_NONE


def crash_kind(has_nan, has_inf, max_displacement, max_abs_velocity, max_speed, max_radius, energy, prev_energy, dt) -> int:
    """The reference's detect_crash (crash_point_test.py:46-139) with the criterion that fired: the definition of what
    run_crash_watched decides on the device for one member at one check, from the member's measures (`CrashMeasures`),
    its total energy at this check and at the one before, and its dt as given.  The comparisons are the reference's own,
    in its order and in Python floats, so a NaN energy ratio trips nothing and a zero `prev_energy` of either sign skips
    the energy test."""
    max_displacement, max_abs_velocity, max_speed, max_radius = (
        float(max_displacement), float(max_abs_velocity), float(max_speed), float(max_radius))
    energy, prev_energy, dt = float(energy), float(prev_energy), float(dt)
    if has_nan:
        return CRASH_NAN
    if has_inf:
        return CRASH_INF
    if max_displacement > max_abs_velocity * dt * 10 and max_displacement > 1.0:
        return CRASH_TELEPORT
    if max_speed > 100.0:
        return CRASH_VELOCITY
    if prev_energy != 0:
        energy_ratio = abs(energy / prev_energy)
        if energy_ratio > 100 or energy_ratio < 0.01:
            return CRASH_ENERGY
    if max_radius > 1000:
        return CRASH_RADIUS
    return CRASH_NONE


def crash_value(kind, max_displacement, max_speed, max_radius, energy) -> float:
    """The reference's CrashReport.value as detect_crash sets it for the criterion `kind` (NaN for CRASH_NONE)."""
    kind = int(kind)
    if kind in (CRASH_NAN, CRASH_INF):
        return 0.0
    if kind == CRASH_NONE:
        return float("nan")
    return float({CRASH_TELEPORT: max_displacement, CRASH_VELOCITY: max_speed, CRASH_ENERGY: energy,
                  CRASH_RADIUS: max_radius}[kind])


def crash_severity(kind, max_displacement, max_speed, max_radius, energy, prev_energy) -> float:
    """The reference's CrashReport.severity for the criterion `kind` (0 for CRASH_NONE)."""
    import numpy as np
    kind = int(kind)
    if kind == CRASH_NONE:
        return 0.0
    if kind in (CRASH_NAN, CRASH_INF):
        return 1.0
    if kind == CRASH_ENERGY:
        ratio = abs(float(energy) / float(prev_energy))
        if ratio == 0 or ratio == float("inf"):         # |log10| is inf
            return 1.0
        return min(1.0, float(abs(np.log10(ratio))) / 5)      # numpy's log10, as the reference takes it
    value = crash_value(kind, max_displacement, max_speed, max_radius, energy)
    return min(1.0, value / {CRASH_TELEPORT: 100, CRASH_VELOCITY: 1000, CRASH_RADIUS: 10000}[kind])


def check_metrics_arguments(num_bins, max_radius, percentile, members):
    """Validate metrics()' arguments without touching a device.  Returns (num_bins, max_radius, percentile) with
    max_radius None (every member's own maximum radius) or a list of `members` floats; raises TypeError / ValueError."""
    for name, v in (("num_bins", num_bins), ("members", members)):
        _typed(name, v)
    num_bins, members = int(num_bins), int(members)
    if members < 1:
        raise ValueError(f"members must be >= 1, got {members}")
    if not 0 <= num_bins <= MAX_BINS:
        raise ValueError(f"num_bins must be in [0, {MAX_BINS}], got {num_bins}")
    _typed("percentile", percentile, numbers.Real, "a number")
    if percentile != percentile:
        raise ValueError("percentile is NaN")
    if max_radius is not None:
        def not_negative(v):
            if v < 0:
                raise ValueError(f"max_radius must be >= 0, got {v}")
        max_radius = _scalar_or_list(max_radius, "max_radius", numbers.Real, "None, a number or a sequence of numbers",
                                     check=not_negative)
        if not isinstance(max_radius, list):
            max_radius = [max_radius] * members
        elif len(max_radius) != members:
            raise ValueError(f"max_radius has {len(max_radius)} entries for {members} members")
        max_radius = [float(v) for v in max_radius]
    return num_bins, max_radius, float(percentile)


class EnsembleMetrics(NamedTuple):
    """What metrics() returns, numpy arrays with the member first: `edges` (B, num_bins + 1) float32 and the bin centres
    `radii` (B, num_bins) float32; `velocities` (B, num_bins) float64, the mean tangential speed per bin (NaN where
    `num_stars_per_bin`, int64, is 0); and (B,) float64 `max_radius` (the end of the edges), `galaxy_radius` (the
    percentile radius), `bound_fraction` and `velocity_dispersion`."""
    edges: "np.ndarray"
    radii: "np.ndarray"
    velocities: "np.ndarray"
    num_stars_per_bin: "np.ndarray"
    max_radius: "np.ndarray"
    galaxy_radius: "np.ndarray"
    bound_fraction: "np.ndarray"
    velocity_dispersion: "np.ndarray"

    def rotation_curve(self, b: int) -> dict:
        """Member b's curve as the reference's compute_rotation_curve dict (metrics.py:74-78)."""
        b = int(b)
        if not 0 <= b < self.edges.shape[0]:
            raise IndexError(f"member {b} of {self.edges.shape[0]}")
        return {"radii": self.radii[b], "velocities": self.velocities[b],
                "num_stars_per_bin": [int(c) for c in self.num_stars_per_bin[b]]}


class EnergyHistory(NamedTuple):
    """What run_recorded returns: `ticks[s]` is the absolute tick of sample s; `kinetic` and `potential` are float64
    tensors of shape (samples, members)."""
    ticks: list
    kinetic: torch.Tensor
    potential: torch.Tensor

    @property
    def total(self) -> torch.Tensor:
        return self.kinetic + self.potential


class Divergence(NamedTuple):
    """What divergence() returns, (B,) float64 tensors: member b against its baseline member -- the largest and the mean
    |position difference| and the largest |velocity difference| over the N * D elements (module docstring: contract)."""
    max_position: torch.Tensor
    mean_position: torch.Tensor
    max_velocity: torch.Tensor


class DivergenceHistory(NamedTuple):
    """What run_diverged returns: `ticks[s]` is the absolute tick of sample s; `baseline` the B baseline members;
    `max_position`, `mean_position` and `max_velocity` are float64 tensors of shape (samples, members); `energy` is the
    EnergyHistory of the same samples, or None."""
    ticks: list
    baseline: list
    max_position: torch.Tensor
    mean_position: torch.Tensor
    max_velocity: torch.Tensor
    energy: "EnergyHistory"

    def entropy_bits(self):
        """`entropy_bits` of every sample's max_position: a (samples, members) numpy array."""
        return entropy_bits(self.max_position.cpu().numpy())

    def divergence_rate(self):
        """`divergence_rate` per member: the reference's series holds one value per step(), so the rule is applied to
        samples 1.. and the entry sample reports 0.  A (samples, members) numpy array."""
        import numpy as np
        x = self.max_position.cpu().numpy()
        out = np.zeros(x.shape, np.float64)
        out[1:] = divergence_rate(x[1:])
        return out

    def peak(self):
        """The running maximum of max_position over the samples (omega_point_test.py _test_point's max_divergence, which
        Python's max() keeps: a NaN sample never replaces the maximum so far): a (samples, members) numpy array."""
        import numpy as np
        x = self.max_position.cpu().numpy()
        out = np.empty(x.shape, np.float64)
        best = np.zeros(x.shape[1:], np.float64)
        for s in range(x.shape[0]):
            best = np.where(x[s] > best, x[s], best)          # max(best, x): x wins only where it compares greater
            out[s] = best
        return out

    def butterfly(self, threshold: float = 0.1):
        """Per member: the peak went above `threshold` (_test_point's "butterfly"): a (members,) bool numpy array."""
        return self.peak()[-1] > threshold


class StabilityReport(NamedTuple):
    """What run_watched returns, (B,) numpy arrays: `stable_ticks` int64, the ticks the member took in the call before it
    stopped (its budget, or the check that halted it); `exploded` bool; `reason` int64, REASON_NONE / REASON_NONFINITE /
    REASON_ENERGY / REASON_UNBOUND; `initial_energy` and `final_energy` float64, sample 0 and the member's last sample
    of `history`, the call's EnergyHistory (one sample per check)."""
    stable_ticks: "np.ndarray"
    exploded: "np.ndarray"
    reason: "np.ndarray"
    initial_energy: "np.ndarray"
    final_energy: "np.ndarray"
    history: EnergyHistory


class CrashMeasures(NamedTuple):
    """What crash_measures returns, (B,) numpy arrays: `has_nan`, `has_inf` bool (positions and velocities); the four
    measures of detect_crash, float64 widened exactly from the state dtype: `max_displacement`, `max_abs_velocity`,
    `max_speed`, `max_radius` (not defined for a member with either flag)."""
    has_nan: "np.ndarray"
    has_inf: "np.ndarray"
    max_displacement: "np.ndarray"
    max_abs_velocity: "np.ndarray"
    max_speed: "np.ndarray"
    max_radius: "np.ndarray"


class CrashPointReport(NamedTuple):
    """What run_crash_watched returns, (B,) numpy arrays: `ticks_taken` int64, the ticks the member took in the call;
    `stable_ticks` int64, the reference's results[...]["stable_ticks"] (the budget without a crash, else the 0-based index
    of the tick whose check fired, ticks_taken - 1); `crashed` bool; `kind` int64, CRASH_NONE .. CRASH_RADIUS; `crash_type`,
    a list of the reference's strings ("" for none); `value` and `severity` float64, the reference's report fields (NaN and
    0 for none); `measures`, the CrashMeasures of every member's last check (zeros for a member never checked); `history`,
    the call's EnergyHistory (one sample per tick)."""
    ticks_taken: "np.ndarray"
    stable_ticks: "np.ndarray"
    crashed: "np.ndarray"
    kind: "np.ndarray"
    crash_type: list
    value: "np.ndarray"
    severity: "np.ndarray"
    measures: CrashMeasures
    history: EnergyHistory


def _crash_measures(flags, meas) -> CrashMeasures:
    """The native flags (B,) int32 and measures (B, 4) float64 as a CrashMeasures."""
    return CrashMeasures((flags & 1) != 0, (flags & 2) != 0, meas[:, 0].copy(), meas[:, 1].copy(), meas[:, 2].copy(),
                         meas[:, 3].copy())


def _doubles(values):
    return (C.c_double * len(values))(*values)


class GalaxyEnsemble:
    """B independent N-body systems advanced one tick per kernel launch (see the module docstring)."""

    def __init__(self, positions, velocities, masses, precision_mode=PrecisionMode.FLOAT64,
                 G=0.001, softening=0.1, dt=0.01, device=None):
        self._handle = C.c_void_p()
        modes, storage = _mode_or_list(precision_mode)
        if modes is not None:
            # one mode per member: the state is checked under the storage mode, a lone galaxy is broadcast over the list
            positions, velocities, masses, self.G, self.softening, self.dt = _check_state(
                positions, velocities, masses, storage, G, softening, dt, [len(modes)])
            check_mode_list(modes, int(positions.shape[0]))
        else:
            positions, velocities, masses, self.G, self.softening, self.dt = check_arguments(
                positions, velocities, masses, precision_mode, G, softening, dt)
        self._construct(positions, velocities, masses, precision_mode, device, modes)

    def _construct(self, positions, velocities, masses, precision_mode, device, modes=None):
        """Everything behind the argument checks: the native handle, the upload and the initial accelerations.  modes: the
        checked per-member list, if the caller gave one."""
        self.device = torch.device(device) if device is not None else positions.device
        self.precision_mode = precision_mode
        self.num_members, self.num_stars, self._dim = (int(v) for v in positions.shape)
        self.precision_modes = list(modes) if modes is not None else [precision_mode] * self.num_members
        self._mixed = len(set(self.precision_modes)) > 1
        precision_mode = PrecisionMode.FLOAT32 if self._mixed else self.precision_modes[0]     # what the handle is created with
        self._dtype = state_dtype(precision_mode)
        self.tick = 0
        if self.device.type == "cuda":
            dev = self.device.index if self.device.index is not None else torch.cuda.current_device()
        else:
            dev = runtime.default_hip_device()
        cfg = N.NbEnsConfig(members=self.num_members, n=self.num_stars, dim=self._dim, mode=mode_code(precision_mode),
                            device=int(dev), flags=0)
        self._create(cfg, (_doubles(self.G), _doubles([s ** 2 for s in self.softening]), _doubles(self.dt)))
        self.set_state(positions=positions, velocities=velocities, masses=masses)
        N.check(N.lib().nb_ens_compute_accelerations(self._handle))

    # ------------------------------------------------------------------ native plumbing
    def _create(self, cfg, params):
        """The native handle of this kind of ensemble; params: the members' G, softening^2 and dt as C arrays."""
        if self._mixed:
            codes = (C.c_int32 * self.num_members)(*[mode_code(m) for m in self.precision_modes])
            N.check(N.lib().nb_ens_create_mixed(C.byref(self._handle), C.byref(cfg), codes, *params))
        else:       # (an all-equal list too: exactly the scalar mode's handle)
            N.check(N.lib().nb_ens_create(C.byref(self._handle), C.byref(cfg), *params))

    def close(self):
        """Release the native handle (device buffers, stream) now instead of at garbage collection."""
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            try:
                N.lib().nb_ens_destroy(h)
            except Exception:
                pass
            h.value = None

    def __del__(self):
        self.close()

    def _shape(self, name):
        return (self.num_members, self.num_stars) if name == "masses" else (self.num_members, self.num_stars, self._dim)

    def _pointer(self, name, t):
        """(contiguous tensor kept alive by the caller, pointer, on_device) of an upload; shape and dtype checked."""
        _check_tensor(name, t, shape=self._shape(name), dtype=self._dtype)
        t = t.detach().contiguous()
        on_device = t.device.type == "cuda"
        if on_device:
            torch.cuda.current_stream(t.device).synchronize()
        return t, C.c_void_p(t.data_ptr()), on_device

    def _download(self, name):
        out = torch.empty(self._shape(name), dtype=self._dtype, device=self.device)
        args = [None, None, None, None]
        args[{"positions": 0, "velocities": 1, "accelerations": 2, "masses": 3}[name]] = C.c_void_p(out.data_ptr())
        N.check(N.lib().nb_ens_get_state(self._handle, args[0], args[1], args[2], args[3], int(out.device.type == "cuda")))
        return out

    positions = property(lambda s: s._download("positions"))
    velocities = property(lambda s: s._download("velocities"))
    masses = property(lambda s: s._download("masses"))
    accelerations = property(lambda s: s._download("accelerations"))

    # ------------------------------------------------------------------ writes
    def set_state(self, positions=None, velocities=None, masses=None):
        """Replace whole (B, N, D) / (B, N) arrays of the state; the accelerations are NOT recomputed (as assigning
        `sim.positions` on a GalaxySimulation leaves them)."""
        given = [(n, t) for n, t in (("positions", positions), ("velocities", velocities), ("masses", masses)) if t is not None]
        if not given:
            return
        held = [self._pointer(n, t) for n, t in given]
        for on_device in sorted({h[2] for h in held}):
            ptr = {n: h[1] for (n, _), h in zip(given, held) if h[2] == on_device}
            N.check(N.lib().nb_ens_set_state(self._handle, ptr.get("positions"), ptr.get("velocities"), ptr.get("masses"),
                                             _TORCH_TO_NB[self._dtype], int(on_device)))

    def set_accelerations(self, accelerations):
        """Replace the stored (B, N, D) accelerations (what the next tick's opening kick uses)."""
        t, ptr, on_device = self._pointer("accelerations", accelerations)
        N.check(N.lib().nb_ens_set_accelerations(self._handle, ptr, _TORCH_TO_NB[self._dtype], int(on_device)))

    def set_params(self, G=None, softening=None, dt=None):
        """New G / softening / dt (each a float for all members or a length-B sequence); read by the next launch."""
        B = self.num_members
        new = {k: _param_list(k, v, B) for k, v in (("G", G), ("softening", softening), ("dt", dt)) if v is not None}
        if not new:
            return
        self.G, self.softening, self.dt = new.get("G", self.G), new.get("softening", self.softening), new.get("dt", self.dt)
        N.check(N.lib().nb_ens_set_params(self._handle, _doubles(self.G) if "G" in new else None,
                                          _doubles([s ** 2 for s in self.softening]) if "softening" in new else None,
                                          _doubles(self.dt) if "dt" in new else None))

    # ------------------------------------------------------------------ hot path
    def step(self):
        """One kick-drift-kick leapfrog tick of every member (reference simulation.py:120-143)."""
        N.check(N.lib().nb_ens_step(self._handle, 1))
        self._advance(1)

    def run(self, num_ticks: int, callback: Callable = None, callback_interval: int = 100):
        """`num_ticks` ticks; `callback(self, self.tick)` every `callback_interval` (the contract of
        GalaxySimulation.run).  Stretches between callbacks are one native call: one launch per tick."""
        done = 0
        while done < num_ticks:
            nxt = min(num_ticks, (done // callback_interval + 1) * callback_interval) if callback else num_ticks
            N.check(N.lib().nb_ens_step(self._handle, nxt - done))
            self._advance(nxt - done)
            done = nxt
            if callback and done % callback_interval == 0:
                callback(self, self.tick)

    def run_recorded(self, num_ticks: int, every: int = 1) -> EnergyHistory:
        """`num_ticks` ticks like run(), recording every member's kinetic and potential energy on the device: at entry and
        after every `every`-th tick of this call.  One native call; nothing is copied to the host in between.  The
        trajectory is bit-identical to run(num_ticks)."""
        offsets = check_record_arguments(num_ticks, every, self.num_members)
        return self._recorded_call("nb_ens_run_recorded", (int(num_ticks), int(every)), offsets, advance=int(num_ticks))

    def _recorded_call(self, entry, head, offsets, tail=(), advance=None, own=None, energies=True):
        """One recorded native run: `entry`(handle, *head, kinetic, potential, capacity, on_device, &samples, *tail) with
        room for one sample per offset (`offsets` None or empty, or energies False: no energy buffers), the sample count
        checked, the clocks advanced by `advance` / `own` (_advance; None: the caller does it).  Returns the EnergyHistory at
        the absolute ticks, or None without energy samples."""
        S, B = len(offsets or ()), self.num_members
        ke = pe = None
        if S and energies:
            ke = torch.empty((S, B), dtype=torch.float64, device=self.device)
            pe = torch.empty((S, B), dtype=torch.float64, device=self.device)
        got = C.c_int32()
        N.check(getattr(N.lib(), entry)(
            self._handle, *head, C.c_void_p(ke.data_ptr()) if ke is not None else None,
            C.c_void_p(pe.data_ptr()) if pe is not None else None, S, int(self.device.type == "cuda"), C.byref(got), *tail))
        if got.value != S:
            raise RuntimeError(f"{entry} wrote {got.value} samples, expected {S}")
        history = EnergyHistory([self.tick + o for o in offsets], ke, pe) if ke is not None else None
        if advance is not None:
            self._advance(advance, own=own)
        return history

    def _advance(self, ticks, own=None):
        """The clocks after a call: `tick` by `ticks`, every member's by the same or by its `own`."""
        mine = self.__dict__.get("_member_ticks")          # absent until the first uneven call
        if own is not None or mine is not None:
            mine = mine if mine is not None else [self.tick] * self.num_members
            own = [ticks] * self.num_members if own is None else own
            self._member_ticks = [m + int(o) for m, o in zip(mine, own)]
        self.tick += ticks

    @property
    def member_ticks(self) -> list:
        """Ticks every member has taken since construction; all equal `tick` until the first uneven call."""
        mine = self.__dict__.get("_member_ticks")
        return list(mine) if mine is not None else [self.tick] * self.num_members

    def _run_members(self, budgets, every, offsets, watch):
        """The native call behind run_members / run_watched: (EnergyHistory or None, stop ticks, reasons)."""
        import numpy as np
        B = self.num_members
        stop, reason = np.zeros(B, np.int32), np.zeros(B, np.int32)
        pi32 = C.POINTER(C.c_int32)
        history = self._recorded_call("nb_ens_run_members", ((C.c_int32 * B)(*budgets), int(every or 0), int(bool(watch))),
                                      offsets, (stop.ctypes.data_as(pi32), reason.ctypes.data_as(pi32)),
                                      advance=max(budgets), own=stop)
        return history, stop.astype(np.int64), reason.astype(np.int64)

    def run_members(self, num_ticks, every=None):
        """Member b takes `num_ticks[b]` ticks (an int: every member as many) in one native call and is then left alone,
        bit-identical to its solo run of as many steps.  `every`: None, or record the energies like run_recorded -- at
        entry and after every `every`-th tick up to the largest budget, a stopped member at its frozen state -- and
        return the EnergyHistory.  `tick` advances by the largest budget, `member_ticks` by each member's own."""
        budgets, offsets = check_member_ticks_arguments(num_ticks, every, self.num_members)
        return self._run_members(budgets, every, offsets, watch=False)[0]

    def run_watched(self, max_ticks, check_interval: int = 50) -> StabilityReport:
        """The reference's stability loop (stability_test.py:94-105) for every member at once: batches of
        `check_interval` ticks, ceil(max_ticks[b] / check_interval) of them for member b (`max_ticks`: an int or one
        per member), and after every batch the explosion test of `explosion_reason` on the device.  A member that trips
        it is halted there; nothing is read back before the end of the call."""
        import numpy as np
        check_interval = int(_typed("check_interval", check_interval))
        if check_interval < 1:
            raise ValueError(f"check_interval must be >= 1, got {check_interval}")
        budgets, _ = check_member_ticks_arguments(max_ticks, None, self.num_members)
        budgets, offsets = check_member_ticks_arguments([-(-v // check_interval) * check_interval for v in budgets],
                                                        check_interval, self.num_members)
        history, stop, reason = self._run_members(budgets, check_interval, offsets, watch=True)
        total = history.total.cpu().numpy()
        last = total[stop // check_interval, np.arange(self.num_members)]
        return StabilityReport(stop, reason != REASON_NONE, reason, total[0].copy(), last, history)

    def run_crash_watched(self, max_ticks) -> CrashPointReport:
        """The reference's crash-point loop (crash_point_test.py:186-215) for every member at once: up to `max_ticks[b]`
        ticks (`max_ticks`: an int or one per member), and after every tick detect_crash's test (`crash_kind`) on the
        device, against the member's positions and energy of the tick before.  A member that trips it is halted there;
        nothing is read back before the end of the call."""
        import numpy as np
        budgets, offsets = check_member_ticks_arguments(max_ticks, 1, self.num_members)
        B = self.num_members
        stop, kind, flags = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
        meas = np.zeros((B, 4), np.float64)
        pi32 = C.POINTER(C.c_int32)
        history = self._recorded_call("nb_ens_run_crash_watched", ((C.c_int32 * B)(*budgets),), offsets,
                                      (stop.ctypes.data_as(pi32), kind.ctypes.data_as(pi32), flags.ctypes.data_as(pi32),
                                       meas.ctypes.data_as(C.POINTER(C.c_double))))
        return self._crash_report(budgets, stop, kind, flags, meas, history)

    def _crash_report(self, budgets, stop, kind, flags, meas, history) -> CrashPointReport:
        """The clocks and the report behind run_crash_watched's native call: value and severity are the reference's,
        from the measures of the member's last check and the history's samples at and before its last tick."""
        import numpy as np
        B = self.num_members
        stop, kind = np.asarray(stop).astype(np.int64), np.asarray(kind).astype(np.int64)
        self._advance(max(budgets), own=stop)
        measures = _crash_measures(np.asarray(flags), np.asarray(meas))
        total = history.total.cpu().numpy()
        crashed = kind != CRASH_NONE
        value, severity = np.full(B, np.nan), np.zeros(B)
        for b in np.nonzero(crashed)[0]:
            args = (int(kind[b]), measures.max_displacement[b], measures.max_speed[b], measures.max_radius[b],
                    total[stop[b], b])
            value[b] = crash_value(*args)
            severity[b] = crash_severity(*args, total[stop[b] - 1, b])
        return CrashPointReport(stop, np.where(crashed, stop - 1, np.asarray(budgets, np.int64)), crashed, kind,
                                [CRASH_TYPES[k] for k in kind], value, severity, measures, history)

    # ------------------------------------------------------------------ reads
    def crash_measures(self, prev_positions=None) -> CrashMeasures:
        """detect_crash's measures (crash_point_test.py:60-127) of every member from the resident state: one launch, one
        copy-out.  `prev_positions`: None (displacement 0) or a (B, N, D) tensor of the state dtype on either device."""
        import numpy as np
        held, ptr, on_device = (None, None, False) if prev_positions is None else self._pointer("prev_positions", prev_positions)
        B = self.num_members
        flags, meas = np.zeros(B, np.int32), np.zeros((B, 4), np.float64)
        N.check(N.lib().nb_ens_crash_measures(self._handle, ptr, int(on_device), flags.ctypes.data_as(C.POINTER(C.c_int32)),
                                              meas.ctypes.data_as(C.POINTER(C.c_double))))
        del held
        return _crash_measures(flags, meas)

    def divergence(self, baseline=0) -> Divergence:
        """How far every member is from its baseline member (`baseline`: an int, one member for all, or one per member)
        on the resident state: one launch, one copy-out (module docstring: contract)."""
        baselines, _ = check_divergence_arguments(0, 1, baseline, self.num_members)
        B = self.num_members
        out = [torch.empty(B, dtype=torch.float64, device=self.device) for _ in range(3)]
        N.check(N.lib().nb_ens_divergence(self._handle, (C.c_int32 * B)(*baselines), *[C.c_void_p(t.data_ptr()) for t in out],
                                          int(self.device.type == "cuda")))
        return Divergence(*out)

    def run_diverged(self, num_ticks: int, every: int = 1, baseline=0, energies: bool = True) -> DivergenceHistory:
        """`num_ticks` ticks like run(), recording every member's divergence from its baseline member on the device: at
        entry and after every `every`-th tick of this call; `energies`: also the EnergyHistory of run_recorded at the same
        samples (False: no energy launch is issued, `energy` is None).  One native call; nothing is copied to the host in
        between.  The trajectory is bit-identical to run(num_ticks)."""
        baselines, offsets = check_divergence_arguments(num_ticks, every, baseline, self.num_members)
        S, B = len(offsets), self.num_members
        dv = [torch.empty((S, B), dtype=torch.float64, device=self.device) for _ in range(3)]
        ticks = [self.tick + o for o in offsets]
        head = (int(num_ticks), int(every), (C.c_int32 * B)(*baselines), int(bool(energies)),
                *[C.c_void_p(t.data_ptr()) for t in dv])
        energy = self._recorded_call("nb_ens_run_diverged", head, offsets, advance=int(num_ticks), energies=bool(energies))
        return DivergenceHistory(ticks, baselines, dv[0], dv[1], dv[2], energy)

    def energies(self):
        """(kinetic, potential): float64 tensors of shape (B,) on `self.device`, all members evaluated in one batched
        pass.  Equal to get_kinetic_energy() / get_potential_energy() to the project's bars, not bit for bit."""
        ke = torch.empty(self.num_members, dtype=torch.float64, device=self.device)
        pe = torch.empty(self.num_members, dtype=torch.float64, device=self.device)
        N.check(N.lib().nb_ens_energies(self._handle, C.c_void_p(ke.data_ptr()), C.c_void_p(pe.data_ptr()),
                                        int(self.device.type == "cuda")))
        return ke, pe

    def metrics(self, num_bins: int = 20, max_radius=None, percentile: float = 90) -> EnsembleMetrics:
        """Rotation curve, percentile radius, bound fraction and velocity dispersion of every member (reference
        metrics.py:25-156) from the resident state: one launch, one copy-out.  `max_radius`: None (each member's own
        maximum radius), a number, or one per member."""
        import numpy as np
        num_bins, max_radius, percentile = check_metrics_arguments(num_bins, max_radius, percentile, self.num_members)
        B = self.num_members
        mean = np.empty((B, num_bins), np.float64)
        count = np.empty((B, num_bins), np.int64)
        edges = np.empty((B, num_bins + 1), np.float32)
        sc = np.empty((B, 5), np.float64)
        N.check(N.lib().nb_ens_metrics(self._handle, num_bins, _doubles(max_radius) if max_radius is not None else None,
                                       percentile, mean.ctypes.data_as(C.POINTER(C.c_double)),
                                       count.ctypes.data_as(C.POINTER(C.c_int64)),
                                       edges.ctypes.data_as(C.POINTER(C.c_float)), sc.ctypes.data_as(C.POINTER(C.c_double))))
        if num_bins == 0:                 # linspace(0, R, 1) is [0] (the library writes no edges without bins)
            edges[:] = 0
        radii = ((edges[:, :-1] + edges[:, 1:]) / np.float32(2)).astype(np.float32)
        return EnsembleMetrics(edges, radii, mean, count, sc[:, 4].copy(), sc[:, 1].copy(), sc[:, 2].copy(), sc[:, 3].copy())

    def _energy(self, kinetic, potential):
        B = self.num_members
        ke, pe = (C.c_double * B)(), (C.c_double * B)()
        N.check(N.lib().nb_ens_energy(self._handle, ke if kinetic else None, pe if potential else None))
        return list(ke), list(pe)

    def get_kinetic_energy(self) -> list:
        """Per member, sum(0.5 * m * v^2) (reference simulation.py:170-174)."""
        return self._energy(True, False)[0]

    def get_potential_energy(self) -> list:
        """Per member, -G * sum_{i<j} m_i m_j / sqrt(r_ij^2 + eps^2) (reference simulation.py:176-192)."""
        return self._energy(False, True)[1]

    def get_total_energy(self) -> list:
        ke, pe = self._energy(True, True)
        return [k + p for k, p in zip(ke, pe)]

    def get_state(self, b: int) -> dict:
        """Member b's state as the reference's get_state() dict (simulation.py:160-168)."""
        b = int(b)
        if not 0 <= b < self.num_members:
            raise IndexError(f"member {b} of {self.num_members}")
        return {
            "positions": self.positions[b].clone(),
            "velocities": self.velocities[b].clone(),
            "masses": self.masses[b].clone(),
            "tick": self.member_ticks[b],
            "precision_mode": self.precision_modes[b].value,
        }

    def _info(self):
        members, launches, name = C.c_int32(), C.c_int64(), C.c_char_p()
        N.check(N.lib().nb_ens_info(self._handle, C.byref(members), C.byref(launches), C.byref(name)))
        return members.value, launches.value, (name.value or b"none").decode()

    def launches(self) -> int:
        """Batched force launches since construction: one for the constructor's evaluation, one per tick.  The
        elementwise opening kick + drift launch of every step() / run() stretch is not counted."""
        return self._info()[1]

    def force_kernel_name(self) -> str:
        return self._info()[2]

    def synchronize(self):
        N.check(N.lib().nb_ens_synchronize(self._handle))


class QuantizedEnsemble(GalaxyEnsemble):
    """A GalaxyEnsemble under INT8_SIM, INT4_SIM or CUSTOM: every member with its own quantisation tables and, under
    CUSTOM, its own number of grid levels (`custom_levels`: None = 64, an int, or one per member; 2 .. 256).  `levels` holds
    the B level counts in force; they are fixed for the life of the object (see the module docstring)."""

    def __init__(self, positions, velocities, masses, precision_mode=PrecisionMode.INT8_SIM, custom_levels=None,
                 G=0.001, softening=0.1, dt=0.01, device=None):
        self._handle = C.c_void_p()
        positions, velocities, masses, self.levels, self.G, self.softening, self.dt = check_grid_arguments(
            positions, velocities, masses, precision_mode, custom_levels, G, softening, dt)
        self._construct(positions, velocities, masses, precision_mode, device)

    def _create(self, cfg, params):
        levels = (C.c_int32 * len(self.levels))(*self.levels) if self.precision_mode == PrecisionMode.CUSTOM else None
        N.check(N.lib().nb_ens_create_grid(C.byref(self._handle), C.byref(cfg), levels, *params))

    def quant_debug(self) -> dict:
        """Grid internals of every member's last force evaluation, as GalaxySimulation.quant_debug() gives them for a solo
        run: length-B numpy arrays `lmin`, `lmax` (log grid on r^2), `r2max`, `fmin`, `fmax` (linear force grid; NaN under
        CUSTOM, which does not quantise forces), `fast_path` (bool: the table-free pair path was enabled) and `levels`."""
        import numpy as np
        B = self.num_members
        info = (C.c_double * (8 * B))()
        N.check(N.lib().nb_ens_quant_info(self._handle, info))
        a = np.asarray(info, np.float64).reshape(B, 8)
        return dict(lmin=a[:, 0].copy(), lmax=a[:, 1].copy(), fmin=a[:, 2].copy(), fmax=a[:, 3].copy(), r2max=a[:, 4].copy(),
                    fast_path=a[:, 5] != 0, levels=np.asarray(self.levels, np.int64))

    def quant_bin_sums(self) -> dict:
        """The bin every pair was given, read out of the production pair loop on the members' current positions, as
        GalaxySimulation.quant_bin_sums() gives it for a solo run: `sum_k` and `sum_kw`, (B, N) int64 numpy arrays -- per
        star p the check-sums sum_q k(p, q) and sum_q k(p, q) ((q mod 65521) + 1) over all q -- `pairs_table_free` and
        `pairs_table`, (B,) int64 (pair evaluations binned by the table-free estimate alone / through a threshold table),
        and `levels`.  An observer: state, accelerations, `tick` and `launches()` stay as they are (module docstring)."""
        import numpy as np
        B, n = self.num_members, self.num_stars
        s1, s2, pairs = np.zeros((B, n), np.int64), np.zeros((B, n), np.int64), np.zeros((B, 2), np.int64)
        N.check(N.lib().nb_ens_quant_bin_sums(self._handle, C.c_void_p(s1.ctypes.data), C.c_void_p(s2.ctypes.data),
                                              C.c_void_p(pairs.ctypes.data)))
        return dict(sum_k=s1, sum_kw=s2, pairs_table_free=pairs[:, 0].copy(), pairs_table=pairs[:, 1].copy(),
                    levels=np.asarray(self.levels, np.int64))


class FineGridEnsemble(QuantizedEnsemble):
    """A QuantizedEnsemble in CUSTOM mode whose members take up to MAX_FINE_LEVELS = 4096 grid levels (`custom_levels`: None
    = 64, an int, or one per member).  A member of up to 256 levels keeps QuantizedEnsemble's bit identity with its solo run;
    a finer one has its solo run's tables and bins and a deterministic sum of its own (see the module docstring)."""

    def __init__(self, positions, velocities, masses, custom_levels=None, G=0.001, softening=0.1, dt=0.01, device=None):
        self._handle = C.c_void_p()
        positions, velocities, masses, self.levels, self.G, self.softening, self.dt = check_fine_grid_arguments(
            positions, velocities, masses, custom_levels, G, softening, dt)
        self._construct(positions, velocities, masses, PrecisionMode.CUSTOM, device)

    def _create(self, cfg, params):
        levels = (C.c_int32 * len(self.levels))(*self.levels)
        N.check(N.lib().nb_ens_create_grid_wide(C.byref(self._handle), C.byref(cfg), levels, *params))


class RaggedEnsemble(GalaxyEnsemble):
    """A GalaxyEnsemble whose members have their own star counts (see the module docstring): `positions` / `velocities` are
    sequences of (N_b, D) tensors, `masses` of (N_b,) tensors; `num_stars` is the list of sizes; the array attributes and
    set_state / set_accelerations speak lists of per-member tensors.  Everything else is GalaxyEnsemble's."""

    def __init__(self, positions, velocities, masses, precision_mode=PrecisionMode.FLOAT64, G=0.001, softening=0.1, dt=0.01,
                 device=None):
        self._handle = C.c_void_p()
        positions, velocities, masses, sizes, modes, self.G, self.softening, self.dt = check_ragged_arguments(
            positions, velocities, masses, precision_mode, G, softening, dt)
        self._sizes, self._capacity = list(sizes), max(sizes)
        self.num_members, self._dim = len(sizes), int(positions[0].shape[1])
        self._dtype = positions[0].dtype
        padded = [self._padded(name, t) for name, t in (("positions", positions), ("velocities", velocities), ("masses", masses))]
        self._construct(*padded, precision_mode, device, modes)       # (num_stars: the capacity, for the handle's shape)
        self.num_stars = list(sizes)

    def _create(self, cfg, params):
        B = self.num_members
        codes = (C.c_int32 * B)(*[mode_code(m) for m in self.precision_modes]) if self._mixed else None
        N.check(N.lib().nb_ens_create_ragged(C.byref(self._handle), C.byref(cfg), (C.c_int32 * B)(*self._sizes), codes, *params))

    def _shape(self, name):
        return (self.num_members, self._capacity) if name == "masses" else (self.num_members, self._capacity, self._dim)

    def _padded(self, name, members):
        """A list of per-member tensors -> the whole (B, Nmax, ...) block the handle holds, the rows behind a member's own
        filled with NaN: no kernel touches them, and one that did would poison a result.  A tensor of the block's shape
        is taken as it is."""
        if members is None or isinstance(members, torch.Tensor) and tuple(members.shape) == self._shape(name):
            return members
        if isinstance(members, torch.Tensor) or not isinstance(members, Sequence):
            raise TypeError(f"{name} must be a sequence of {self.num_members} per-member tensors, or the whole padded "
                            f"{self._shape(name)} block")
        members = list(members)
        if len(members) != self.num_members:
            raise ValueError(f"{name} has {len(members)} entries for {self.num_members} members")
        for b, t in enumerate(members):
            _check_tensor(name, t, b, shape=(self._sizes[b],) + self._shape(name)[2:], dtype=self._dtype)
        out = torch.full(self._shape(name), float("nan"), dtype=self._dtype, device=members[0].device)
        for b, t in enumerate(members):
            out[b, :self._sizes[b]] = t.detach().to(out.device)
        return out

    def _members_of(self, name):
        full = self._download(name)
        return [full[b, :n].clone() for b, n in enumerate(self._sizes)]

    positions = property(lambda s: s._members_of("positions"))
    velocities = property(lambda s: s._members_of("velocities"))
    masses = property(lambda s: s._members_of("masses"))
    accelerations = property(lambda s: s._members_of("accelerations"))

    def set_state(self, positions=None, velocities=None, masses=None):
        """Replace the state: each argument None or a list of per-member (N_b, D) / (N_b,) tensors (re-padded with NaN); the
        accelerations are NOT recomputed."""
        super().set_state(self._padded("positions", positions), self._padded("velocities", velocities),
                          self._padded("masses", masses))

    def set_accelerations(self, accelerations):
        """Replace the stored accelerations: a list of per-member (N_b, D) tensors."""
        super().set_accelerations(self._padded("accelerations", accelerations))

    def _same_size_baselines(self, baseline):
        baselines, _ = check_divergence_arguments(0, 1, baseline, self.num_members)
        for b, base in enumerate(baselines):
            if self._sizes[base] != self._sizes[b]:
                raise ValueError(f"baseline of member {b} is member {base}: {self._sizes[b]} stars against {self._sizes[base]}; "
                                 "a member is compared with a member of its own size")

    def divergence(self, baseline=0) -> Divergence:
        self._same_size_baselines(baseline)
        return super().divergence(baseline)

    def run_diverged(self, num_ticks: int, every: int = 1, baseline=0, energies: bool = True) -> DivergenceHistory:
        self._same_size_baselines(baseline)
        return super().run_diverged(num_ticks, every, baseline, energies)

    divergence.__doc__ = GalaxyEnsemble.divergence.__doc__
    run_diverged.__doc__ = GalaxyEnsemble.run_diverged.__doc__

    def metrics(self, *args, **kwargs):
        """Not implemented for members of different sizes: its kernel is one workgroup per member of one shape."""
        raise NotImplementedError("RaggedEnsemble.metrics: ragged metrics are a follow-up (members of one size: GalaxyEnsemble)")

    def run_crash_watched(self, *args, **kwargs):
        """Not implemented for members of different sizes."""
        raise NotImplementedError("RaggedEnsemble.run_crash_watched: the ragged crash watch is a follow-up (members of one "
                                  "size: GalaxyEnsemble)")

    def crash_measures(self, *args, **kwargs):
        """Not implemented for members of different sizes."""
        raise NotImplementedError("RaggedEnsemble.crash_measures: the ragged crash watch is a follow-up (members of one size: "
                                  "GalaxyEnsemble)")


class RaggedQuantizedEnsemble(RaggedEnsemble):
    """A RaggedEnsemble under INT8_SIM, INT4_SIM or CUSTOM: members of their own star counts, every member with its own
    quantisation tables and, under CUSTOM, its own number of grid levels (`custom_levels`: None = 64, an int, or one per
    member; 2 .. 256).  `levels` holds the B level counts in force.  Everything else is RaggedEnsemble's, refusals
    included (see the module docstring)."""

    def __init__(self, positions, velocities, masses, precision_mode=PrecisionMode.INT8_SIM, custom_levels=None,
                 G=0.001, softening=0.1, dt=0.01, device=None):
        self._handle = C.c_void_p()
        positions, velocities, masses, sizes, self.levels, self.G, self.softening, self.dt = check_ragged_grid_arguments(
            positions, velocities, masses, precision_mode, custom_levels, G, softening, dt)
        self._sizes, self._capacity = list(sizes), max(sizes)
        self.num_members, self._dim = len(sizes), int(positions[0].shape[1])
        self._dtype = positions[0].dtype
        padded = [self._padded(name, t) for name, t in (("positions", positions), ("velocities", velocities), ("masses", masses))]
        self._construct(*padded, precision_mode, device)              # (num_stars: the capacity, for the handle's shape)
        self.num_stars = list(sizes)

    def _create(self, cfg, params):
        B = self.num_members
        levels = (C.c_int32 * B)(*self.levels) if self.precision_mode == PrecisionMode.CUSTOM else None
        N.check(N.lib().nb_ens_create_ragged_grid(C.byref(self._handle), C.byref(cfg), (C.c_int32 * B)(*self._sizes), levels,
                                                  *params))

    quant_debug = QuantizedEnsemble.quant_debug

    def quant_bin_sums(self) -> dict:
        """QuantizedEnsemble.quant_bin_sums() for members of different sizes: `sum_k` and `sum_kw` are lists of per-member
        (N_b,) int64 numpy arrays, `pairs_table_free`, `pairs_table` and `levels` (B,) int64 arrays.  An observer."""
        import numpy as np
        B, cap = self.num_members, self._capacity
        s1, s2, pairs = np.zeros((B, cap), np.int64), np.zeros((B, cap), np.int64), np.zeros((B, 2), np.int64)
        N.check(N.lib().nb_ens_quant_bin_sums(self._handle, C.c_void_p(s1.ctypes.data), C.c_void_p(s2.ctypes.data),
                                              C.c_void_p(pairs.ctypes.data)))
        return dict(sum_k=[s1[b, :n].copy() for b, n in enumerate(self._sizes)],
                    sum_kw=[s2[b, :n].copy() for b, n in enumerate(self._sizes)],
                    pairs_table_free=pairs[:, 0].copy(), pairs_table=pairs[:, 1].copy(),
                    levels=np.asarray(self.levels, np.int64))
