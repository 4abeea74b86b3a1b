/*
 * nbody_amd.h -- C-ABI of the MI355X-native direct-summation N-body engine.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference
 * (nuclearbombmods/nbody-cosmological-simulation) has no FFI layer of its own: its operator
 * boundary is the Python class `GalaxySimulation` (simulation.py:12) plus the module-level
 * precision hooks of quantization.py.  Every entry point below names the reference
 * interface it replaces; the Python binding a maintainer would add is a ctypes stub
 * (INTEGRATION.md, and nbody_cosmological_simulation_amd/_native.py in this repo).
 *
 * Conventions
 *   - plain C types only; every function returns 0 (NB_OK) or a negative nb_status and
 *     leaves a thread-local message retrievable with nb_last_error();
 *   - the caller owns every buffer it passes in (host or device, flagged per call); the
 *     library owns the per-handle device state;
 *   - a handle is bound to one HIP device and one stream; distinct handles may be used
 *     concurrently from different threads, one handle must not be;
 *   - NaN/Inf propagate exactly as IEEE arithmetic dictates; nothing traps;
 *   - there is NO CPU fallback: without a HIP device nb_create() fails with NB_ERR_NO_DEVICE.
 */
#ifndef NBODY_AMD_H
#define NBODY_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NB_ABI_VERSION 3

typedef enum nb_status {
    NB_OK = 0,
    NB_ERR_INVALID = -1,       /* bad argument / shape / dtype                     */
    NB_ERR_NO_DEVICE = -2,     /* no HIP device, or device ordinal out of range    */
    NB_ERR_HIP = -3,           /* a HIP runtime call failed (message has details)  */
    NB_ERR_OOM = -4,           /* device allocation failed                         */
    NB_ERR_UNSUPPORTED = -5,   /* combination not implemented yet (message says)   */
    NB_ERR_COMM = -6           /* RCCL failure                                     */
} nb_status;

/* element types of caller buffers and of the Python-visible state tensors */
typedef enum nb_dtype { NB_F16 = 0, NB_BF16 = 1, NB_F32 = 2, NB_F64 = 3 } nb_dtype;

/* quantization.py:10-18 `PrecisionMode` (same order as the enum's declaration) */
typedef enum nb_mode {
    NB_FLOAT64 = 0, NB_FLOAT32 = 1, NB_BFLOAT16 = 2, NB_FLOAT16 = 3,
    NB_INT8_SIM = 4, NB_INT4_SIM = 5, NB_CUSTOM = 6
} nb_mode;

typedef struct nb_sim nb_sim;   /* opaque handle == one GalaxySimulation instance */

/* constructor arguments of GalaxySimulation.__init__ (simulation.py:31-40) */
typedef struct nb_config {
    int32_t n;             /* num_stars                                                     */
    int32_t dim;           /* 2 or 3 (positions are (n, dim) row-major)                     */
    int32_t mode;          /* nb_mode                                                       */
    int32_t levels;        /* CUSTOM grid levels (>= 2; above 4096 on the generic per-pair path); 0 -> 64 (quantization.py:66) */
    double  G;             /* gravitational constant                                        */
    double  softening_sq;  /* softening**2 evaluated in Python double (simulation.py:59)    */
    double  dt;            /* time step                                                     */
    int32_t device;        /* HIP device ordinal                                            */
    int32_t rank;          /* shard index of this process (0 for a single GPU)              */
    int32_t nranks;        /* number of shards = GPUs  (1 for a single GPU)                 */
    int32_t flags;         /* NB_FLAG_*                                                     */
} nb_config;

#define NB_FLAG_PROFILE       1   /* bracket every force launch with HIP events (nb_kernel_time) */
#define NB_FLAG_CUSTOM_FORCEQ 2   /* CUSTOM mode also quantises forces (never set by the stock class) */
#define NB_FLAG_NO_COMM       4   /* nranks > 1 without RCCL: nb_compute_accelerations leaves this rank's
                                     PARTIAL sums (no all-reduce, no force quantisation) for the caller
                                     to reduce; nb_step is refused.  Used by single-GPU shard tests.   */

#define NB_FLAG_F64_STORAGE   16   /* at least one of positions / velocities / masses will be uploaded as fp64 although the
                                     first upload may be fp32: keep the state in fp64 storage from the start (torch
                                     promotes such a simulation to fp64 through the mass product / the first kick) */

#define NB_FLAG_SHARD_TIMING   8   /* timing experiments on ONE GPU: compute only shard `rank` of `nranks`
                                     but run the collectives on a 1-rank communicator.  Results are
                                     partial sums -- never use for physics.                            */

/* ---- lifetime ------------------------------------------------------------------------ */

/* GalaxySimulation.__init__ (simulation.py:31-72) minus the state upload and first force. */
int nb_create(nb_sim **out, const nb_config *cfg);
int nb_destroy(nb_sim *s);

/* Handles keep their stream and (up to 64 MiB) device allocation in a bounded process-level cache when they are
 * destroyed, for the next handle on the same device: the reference's scripts build many short simulations
 * (simulation.py:199-250 run_comparison builds one per mode; main.py:140-176 one per requested mode), and hipFree / hipStreamDestroy wait for the whole device.  nb_cache_trim releases
 * everything the cache holds (bytes of device memory returned through released_bytes, may be NULL). */
int nb_cache_trim(int64_t *released_bytes);

/* attribute writes `sim.G = ..`, `sim.dt = ..`, `sim.softening_sq = ..` between steps
 * (crash_point_test.py, falsification_tests.py read/write them; simulation.py reads them
 * at every use :86,:101,:132-141). */
int nb_set_params(nb_sim *s, double G, double softening_sq, double dt);

/* ---- state --------------------------------------------------------------------------- */

/* simulation.py:63-65 (clone -> device).  pos/vel: n*dim elements, mass: n elements, all of
 * `dtype`; `on_device` != 0 means the pointers are device pointers on the handle's device.
 * Any of pos/vel/mass may be NULL to leave that array untouched (re-upload after an
 * in-place edit such as omega_point_test.py:738). */
int nb_set_state(nb_sim *s, const void *pos, const void *vel, const void *mass,
                 int dtype, int on_device);

/* Writes the Python-visible tensors: each non-NULL destination receives the array in its
 * CURRENT logical dtype (query with nb_state_dtypes).  Synchronises the handle's stream. */
int nb_get_state(nb_sim *s, void *pos, void *vel, void *acc, void *mass, int on_device);

/* dtypes[4] = {positions, velocities, masses, accelerations} as the reference would report
 * them at this moment (SURVEY.md section 8a "Facts": fp32 state is promoted to fp64 by the
 * first step() in FLOAT64 mode, accelerations are fp64 from __init__ on). */
int nb_state_dtypes(nb_sim *s, int32_t dtypes[4]);

/* Replace the stored accelerations (subclasses overriding _compute_accelerations,
 * sensitivity_test.py:61-76: the override's tensor becomes self.accelerations). */
int nb_set_accelerations(nb_sim *s, const void *acc, int dtype, int on_device);

/* ---- the hot path -------------------------------------------------------------------- */

/* GalaxySimulation._compute_accelerations (simulation.py:74-118) on the current positions,
 * including quantize_distance_squared (quantization.py:21-71) and, for INT8/INT4,
 * quantize_force (quantization.py:130-157).  With nranks > 1 the partial sums over this
 * rank's source block are all-reduced (RCCL) before force quantisation. */
int nb_compute_accelerations(nb_sim *s);

/* GalaxySimulation.step (simulation.py:120-143), `nsteps` times, entirely on the device. */
int nb_step(nb_sim *s, int32_t nsteps);

/* The two halves of step() around an externally supplied force (override path):
 * nb_kick_drift: v += a*(dt/2); x += v*dt   (simulation.py:132,135)
 * nb_kick:       v += a*(dt/2)              (simulation.py:141)                          */
int nb_kick_drift(nb_sim *s);
int nb_kick(nb_sim *s);

/* get_kinetic_energy / get_potential_energy (simulation.py:170-192); either may be NULL. */
int nb_energy(nb_sim *s, double *kinetic, double *potential);

/* ---- ensembles: many small systems per launch ------------------------------------------------ */

/* The reference's sweeps (falsification_tests.py:284-356 over softening lengths and time steps,
 * reproducibility.py:362 over seeds, stability_test.py over modes) are Python loops of independent
 * GalaxySimulations of a few hundred to a few thousand stars.  An nb_ens holds `members` such systems of the
 * same n, dim, precision mode and state dtype, each with its own state, G, softening and dt, and advances all
 * of them one tick per kernel launch.  No arithmetic crosses members; a member's state is bit-identical to
 * the nb_sim that takes the same steps on the one-launch small-system path.
 * Limits: nb_ens_create takes the modes NB_FLOAT64 .. NB_FLOAT16 (the grid modes need per-member tables:
 * NB_ERR_UNSUPPORTED there), nb_ens_create_grid takes NB_INT8_SIM, NB_INT4_SIM and NB_CUSTOM with up to 256
 * levels per member, and nb_ens_create_grid_wide takes NB_CUSTOM with up to 4096 levels per member (above
 * 256 levels a member is no longer bit-identical to its nb_sim, see there); state of the settled dtype only (NB_F64 under NB_FLOAT64, NB_F32 otherwise); n at most
 * the one-launch step's limit (4096 fp64, 3072 fp32); 1 <= members <= 1024; one device, no communicator.
 * Arrays are whole (members, n, dim) / (members, n) row-major blocks, host or device as flagged.
 * Grid modes: an evaluation is two launches over all members (max r^2 + tables, the pair sweep) and under
 * INT8 / INT4 a third (force snap + kicks); every member has its own tables (49 KB of device memory each),
 * built from its own exact max r^2, softening, G and level count, so they are the tables of its solo run.
 * A handle of nb_ens_create_grid_wide with a member above 256 levels adds one tables launch per evaluation
 * for those members and keeps its pair sweep's tables (up to 2 * 4097 floats) in LDS sized per launch. */
typedef struct nb_ens nb_ens;
typedef struct nb_ens_config {
    int32_t members;       /* B                                                              */
    int32_t n;             /* stars per member                                               */
    int32_t dim;           /* 2 or 3                                                         */
    int32_t mode;          /* nb_mode: NB_FLOAT64 .. NB_FLOAT16, or a grid mode (nb_ens_create_grid) */
    int32_t device;        /* HIP device ordinal                                             */
    int32_t flags;         /* 0                                                              */
} nb_ens_config;

/* G / softening_sq / dt: `members` doubles each (softening**2 evaluated by the caller, as in nb_config) */
int nb_ens_create(nb_ens **out, const nb_ens_config *cfg, const double *G, const double *softening_sq,
                  const double *dt);
/* The same for the grid modes: cfg->mode is NB_INT8_SIM, NB_INT4_SIM or NB_CUSTOM (any other:
 * NB_ERR_UNSUPPORTED, as is n above the fp32 limit).  levels: under NB_CUSTOM `members` level counts, each in
 * [2, 256] (else NB_ERR_INVALID), or NULL for 64 everywhere; under the other two modes it must be NULL (256 /
 * 16 levels).  Levels are fixed for the life of the handle.  The handle is an ordinary nb_ens: every nb_ens_*
 * entry works on it, and a member is bit-identical to the nb_sim of the same mode and levels. */
int nb_ens_create_grid(nb_ens **out, const nb_ens_config *cfg, const int32_t *levels, const double *G,
                       const double *softening_sq, const double *dt);
/* NB_CUSTOM with up to 4096 levels per member (the threshold tables' capacity): cfg->mode must be NB_CUSTOM (any
 * other: NB_ERR_UNSUPPORTED, as is n above the fp32 limit); levels: `members` level counts, each in [2, 4096]
 * (else NB_ERR_INVALID with the member's index and the range), or NULL for 64 everywhere.  Arguments are refused
 * before a device is looked for.  While no member exceeds 256 levels the handle is nb_ens_create_grid's, launch
 * for launch ("ens_grid_step_kernel").  Otherwise a tick is still ONE force launch, "ens_grid_step_wide_kernel":
 * a member of up to 256 levels stays bit-identical to its nb_sim whatever its neighbours' level counts; a
 * member of 257 .. 4096 levels has the tables of its nb_sim (lmin, lmax, r2max equal, fast_ok = 0), gives every
 * pair the bin and the table entry the nb_sim gives it, and sums the products in the one-launch step's order --
 * deterministic and independent of the other members, but not the order of the nb_sim's tiled path, so
 * accelerations agree with the nb_sim's to rounding, not bit for bit. */
int nb_ens_create_grid_wide(nb_ens **out, const nb_ens_config *cfg, const int32_t *levels, const double *G,
                            const double *softening_sq, const double *dt);
/* Members of different cast modes in one handle: cfg->mode must be NB_FLOAT32 (the storage mode of every cast mode)
 * and modes holds `members` entries, each NB_FLOAT32, NB_BFLOAT16 or NB_FLOAT16 (anything else: NB_ERR_UNSUPPORTED
 * with the member's index -- NB_FLOAT64 is stored differently, the grid modes need per-member tables).  One force
 * launch per tick serves all members ("ens_step_mixed_kernel"), and member b is bit-identical to the nb_sim of mode
 * modes[b].  The handle is an ordinary nb_ens: every nb_ens_* entry works on it; the energies do not pass through the
 * hook, so nb_ens_energy gives each member the value of its solo run in its own mode. */
int nb_ens_create_mixed(nb_ens **out, const nb_ens_config *cfg, const int32_t *modes, const double *G,
                        const double *softening_sq, const double *dt);
/* Members of different SIZES in one handle (the reference's density sweeps: omega_point_test.py:595-766 scans 100 ..
 * 2000 stars, density_limit_test.py:206-246 100 .. 4000).  cfg->n is the CAPACITY, the largest member; sizes holds
 * `members` star counts, each in [1, cfg->n] (else NB_ERR_INVALID naming the member).  cfg->mode is NB_FLOAT64 ..
 * NB_FLOAT16 (a grid mode: NB_ERR_UNSUPPORTED); modes is NULL for that mode everywhere, else as in nb_ens_create_mixed
 * (cfg->mode NB_FLOAT32).  Limits as nb_ens_create's, with the capacity for n.  Arguments are refused before a device
 * is looked for.
 * Layout: padded, not packed -- the arrays are whole (members, cfg->n, dim) / (members, cfg->n) blocks as on every
 * handle; member b owns the first sizes[b] rows of its block and NO kernel reads or writes the rows behind them.
 * nb_ens_set_state / nb_ens_get_state / nb_ens_set_accelerations move whole blocks, padding included.
 * A tick is ONE force launch ("ens_step_ragged_kernel") over a work list of sum_b ceil(sizes[b] / (512 / lanes))
 * workgroups, largest members first (nb_ens_ragged_plan), and member b is bit-identical to the nb_sim of its own size
 * and mode.  The handle is an ordinary nb_ens: step, run_recorded, run_members (with the explosion watch), energies,
 * divergence and run_diverged work on it with every member's own size; nb_ens_energy returns nb_ens_energies' values
 * (those of a handle of the member's size alone, bit for bit).  nb_ens_divergence / nb_ens_run_diverged refuse a
 * baseline of another size than the member's (NB_ERR_INVALID naming both).  NB_ERR_UNSUPPORTED, as follow-ups:
 * nb_ens_metrics (ragged metrics), nb_ens_crash_measures and nb_ens_run_crash_watched (ragged crash watch),
 * nb_ens_quant_info and nb_ens_quant_bin_sums (ragged grid modes: a handle of nb_ens_create_ragged_grid has them). */
int nb_ens_create_ragged(nb_ens **out, const nb_ens_config *cfg, const int32_t *sizes, const int32_t *modes,
                         const double *G, const double *softening_sq, const double *dt);
/* The grid modes for members of different sizes (the grid half of the same density sweeps: omega_point_test.py's
 * "int8" / "int4" points and density_limit_test.py's "broken" runs are 256- and 16-level grids on r^2).  sizes and
 * the padded layout as nb_ens_create_ragged; cfg->mode and levels as nb_ens_create_grid: NB_INT8_SIM, NB_INT4_SIM
 * (levels must be NULL) or NB_CUSTOM with `members` level counts in [2, 256] or NULL for 64 everywhere (any other
 * mode: NB_ERR_UNSUPPORTED; a count outside: NB_ERR_INVALID -- grids above 256 levels for members of different sizes
 * are a follow-up, nb_ens_create_grid_wide serves members of one size).  Refusals in the order of every creator: null,
 * shape, mode, levels, sizes, the fp32 limit on cfg->n, the device.
 * An evaluation is nb_ens_create_grid's launches, whatever the sizes: max r^2 + tables (a workgroup beyond its
 * member's size returns at once; the last of the member's OWN workgroups builds its tables), ONE force launch over
 * the work list ("ens_grid_step_ragged_kernel", 512 threads per workgroup for every member) and under INT8 / INT4 the
 * force snap + kicks.  Member b is bit-identical to the nb_sim of its own size, mode and levels -- state,
 * accelerations, nb_ens_quant_info and nb_ens_quant_bin_sums (rows of cfg->n entries of which member b's first
 * sizes[b] are written) -- and no kernel reads or writes a padding row.  Everything else is as on a handle of
 * nb_ens_create_ragged, the three NB_ERR_UNSUPPORTED follow-ups included. */
int nb_ens_create_ragged_grid(nb_ens **out, const nb_ens_config *cfg, const int32_t *sizes, const int32_t *levels,
                              const double *G, const double *softening_sq, const double *dt);
/* The work list of a ragged handle's force launch, without a device: `members` sizes (each >= 1), lanes 16 / 32 /
 * 64 lanes per target (a workgroup of 512 threads holds 512 / lanes targets).  *items = the number of work items;
 * work: NULL to ask for the count alone, else room for `capacity` items of {member, blk} (2 int32 each; capacity
 * below *items: NB_ERR_INVALID).  Members by size descending, ties by index; blk ascending within a member. */
int nb_ens_ragged_plan(const int32_t *sizes, int32_t members, int32_t lanes, int32_t *work, int64_t capacity,
                       int64_t *items);
int nb_ens_destroy(nb_ens *e);
/* any array may be NULL to keep its values; the device copy is updated on the handle's stream */
int nb_ens_set_params(nb_ens *e, const double *G, const double *softening_sq, const double *dt);
/* as nb_set_state / nb_get_state / nb_set_accelerations, for all members at once */
int nb_ens_set_state(nb_ens *e, const void *pos, const void *vel, const void *mass, int dtype, int on_device);
int nb_ens_get_state(nb_ens *e, void *pos, void *vel, void *acc, void *mass, int on_device);
int nb_ens_set_accelerations(nb_ens *e, const void *acc, int dtype, int on_device);
/* every member's forces on its current positions: one launch */
int nb_ens_compute_accelerations(nb_ens *e);
/* `nsteps` leapfrog ticks of every member: one elementwise launch (opening kick + drift), then one force
 * launch per tick that closes the tick and opens the next */
int nb_ens_step(nb_ens *e, int32_t nsteps);
/* kinetic / potential: `members` doubles each, either may be NULL; the values nb_energy gives for the
 * member's state on an nb_sim, bit for bit (off the hot path: evaluated member by member) */
int nb_ens_energy(nb_ens *e, double *kinetic, double *potential);
/* The same energies for all members in ONE batched evaluation (two kernel launches on the handle's stream, one
 * copy per output, one wait): kinetic / potential are `members` doubles each, host or device memory as
 * `on_device` says; either may be NULL.  Needs positions and masses, and velocities when kinetic is asked for.
 * The values agree with nb_ens_energy to the project's bars (1e-12 relative under NB_FLOAT64, 2e-6 otherwise),
 * not bit for bit: every unordered pair is evaluated once per 256-star tile pair and summed in fp64 in a fixed
 * order, so they are deterministic and independent of the other members.  A member whose softening_sq is zero
 * in the state dtype has potential NaN, as upstream (0 / 0 on the masked diagonal, simulation.py:189). */
int nb_ens_energies(nb_ens *e, double *kinetic, double *potential, int on_device);
/* nb_ens_step(nsteps) that also records the energies on the device: sample 0 is the state at entry, sample s
 * the state after tick s * every of this call, 1 + nsteps / every samples in all (written to *samples if not
 * NULL).  kinetic / potential: `capacity` * members doubles each, sample-major (index s * members + b), host or
 * device as `on_device` says; either may be NULL.  Preconditions of nb_ens_step, and every >= 1, nsteps >= 0,
 * capacity >= 1 + nsteps / every (else NB_ERR_INVALID).  A sampled tick is issued as a one-tick nb_ens_step
 * issues it (the force launch closes the tick, the energy launches follow, a separate kick + drift launch opens
 * the next tick), so the trajectory is bit-identical to nb_ens_step(nsteps); force_launches grows by nsteps.
 * Nothing waits on the stream between the first launch and the copy-out of the history at the end. */
int nb_ens_run_recorded(nb_ens *e, int32_t nsteps, int32_t every, double *kinetic, double *potential,
                        int64_t capacity, int on_device, int32_t *samples);
/* Every member with a tick budget of its own, and optionally the reference's explosion watch
 * (stability_test.py:34-61,94-105), in one call with no host round trip between ticks.  nsteps: `members`
 * budgets, each >= 0.  Member b takes exactly nsteps[b] leapfrog ticks and is then left alone by every later
 * launch of the call, its positions, velocities and accelerations bit-identical to nb_ens_step(nsteps[b]) of it
 * alone (a budget of 0: not touched); max(nsteps) force launches are issued over all members (force_launches
 * grows by that), a stopped member's workgroups return after reading their member's stop tick.
 * every = 0: no samples (kinetic, potential, capacity and samples are not used; *samples = 0).  every >= 1: the
 * history of nb_ens_run_recorded(max(nsteps), every), layout and sampling rule as there (capacity >=
 * 1 + max(nsteps) / every); a stopped member keeps being sampled at its frozen state.
 * watch = 1 (needs every >= 1): at every sampled tick after the first, behind the energy launches, each member
 * that is still running is tested on the device, in this order: a non-finite position or velocity
 * (NB_ENS_REASON_NONFINITE); fabs(E0) > 1e-10 && fabs(E - E0) / fabs(E0) > 10.0 (NB_ENS_REASON_ENERGY);
 * E0 < 0 && E > fabs(E0) (NB_ENS_REASON_UNBOUND), with E0 / E = kinetic + potential of sample 0 / this sample in
 * double.  A member that trips one is halted at that tick (a sampled tick is issued closed, so its state is
 * that of nb_ens_step(tick)).  A NaN energy by itself trips nothing, as in the reference.
 * stop_tick / reason: host arrays of `members` entries, either may be NULL, copied once at the end of the call:
 * the tick of this call at which the member stopped (its budget, or the tick that halted it) and why (0 unless
 * halted).  With equal budgets and watch = 0 the launches, the trajectory and the history are those of
 * nb_ens_run_recorded, bit for bit.  Preconditions of nb_ens_step; NB_ERR_INVALID for a negative budget, every < 0,
 * watch without samples, or too small a capacity. */
#define NB_ENS_REASON_NONE      0
#define NB_ENS_REASON_NONFINITE 1
#define NB_ENS_REASON_ENERGY    2
#define NB_ENS_REASON_UNBOUND   3
int nb_ens_run_members(nb_ens *e, const int32_t *nsteps, int32_t every, int32_t watch, double *kinetic,
                       double *potential, int64_t capacity, int on_device, int32_t *samples, int32_t *stop_tick,
                       int32_t *reason);
/* The reference's crash-point detector (crash_point_test.py:46-139) for every member, on the device.  Per member,
 * in the state dtype: max_displacement, max_speed and max_radius are the correctly rounded square roots of the
 * largest squared norm over stars of pos - prev_pos, vel and pos, a squared norm being (c0*c0 + c1*c1) + c2*c2 with
 * separate multiplies and adds (c2 under dim 3 only); max_abs_velocity is the largest |component| of vel; the NaN
 * and Inf flags cover positions and velocities.  The kinds, in the reference's order of precedence: a NaN; an Inf;
 * max_displacement > max_abs_velocity * dt * 10 && max_displacement > 1.0; max_speed > 100.0; E_prev != 0 &&
 * (fabs(E / E_prev) > 100 || < 0.01); max_radius > 1000 -- all in double, dt the member's as given. */
#define NB_ENS_CRASH_NONE     0
#define NB_ENS_CRASH_NAN      1
#define NB_ENS_CRASH_INF      2
#define NB_ENS_CRASH_TELEPORT 3
#define NB_ENS_CRASH_VELOCITY 4
#define NB_ENS_CRASH_ENERGY   5
#define NB_ENS_CRASH_RADIUS   6
/* The measures of the resident state in ONE launch.  flags: members int32 (bit 0 NaN, bit 1 Inf); measures:
 * members * 4 doubles {max_displacement, max_abs_velocity, max_speed, max_radius}; host arrays, either may be NULL.
 * prev_pos: NULL (displacement 0) or a (members, n, dim) block of the state dtype, host or device as flagged.
 * The maxima of a member with a NaN or an Inf are not defined.  Needs positions and velocities.  Changes neither the
 * state nor force_launches. */
int nb_ens_crash_measures(nb_ens *e, const void *prev_pos, int on_device, int32_t *flags, double *measures);
/* The loop of crash_point_test.py:186-215 for every member: nb_ens_run_members(nsteps, every = 1) with the
 * detector in the explosion watch's place.  Budgets, history (1 + max(nsteps) samples), capacity, stop_tick,
 * preconditions and error codes as there.  After every tick, behind the energy launches, each member that is still
 * running is measured against its positions of the tick before (at entry: the resident ones) and tested with
 * E = kinetic + potential of the tick's sample and E_prev of the sample before; a member that trips a criterion is
 * halted at that tick, its state that of nb_ens_step(tick).  A member with a budget of 0 is never checked, and none
 * is checked after its last tick's check.  kind: NB_ENS_CRASH_* per member; flags / measures: as
 * nb_ens_crash_measures, each member's LAST check (0 for a member never checked); host arrays, any may be NULL,
 * copied once at the end of the call.  force_launches grows by max(nsteps). */
int nb_ens_run_crash_watched(nb_ens *e, const int32_t *nsteps, double *kinetic, double *potential,
                             int64_t capacity, int on_device, int32_t *samples, int32_t *stop_tick,
                             int32_t *kind, int32_t *flags, double *measures);
/* How far members have drifted apart (the reference's comparison loops: reality_glitch_tests.py:148-256,
 * omega_point_test.py:665-766), measured on the device in ONE launch, one workgroup per member: member b against
 * member baseline[b] (`members` entries, each in [0, members), else NB_ERR_INVALID naming the member; b itself is
 * allowed).  Over the n * dim elements, differences formed in the state dtype with one subtraction each:
 * max_pos[b] = max |pos_b - pos_base| and max_vel[b] = max |vel_b - vel_base| with torch's max() semantics (NaN if
 * any element is NaN, inf - inf included; +inf is an ordinary value), widened to double; mean_pos[b] = the fp64 sum
 * of |pos_b - pos_base| in a fixed order (deterministic; NaN if any term is) divided by n * dim.  Outputs: `members`
 * doubles each, host or device as `on_device` says; any may be NULL.  One launch, one copy-out, one wait.  Needs
 * positions and velocities.  Changes neither the state nor force_launches. */
int nb_ens_divergence(nb_ens *e, const int32_t *baseline, double *max_pos, double *mean_pos, double *max_vel,
                      int on_device);
/* nb_ens_step(nsteps) that records the divergence of nb_ens_divergence on the device, and with with_energies != 0
 * the energies of nb_ens_run_recorded beside it (with_energies == 0: no energy launch is issued, kinetic and
 * potential are not used).  Sampling rule, layout (index s * members + b), capacity and *samples as
 * nb_ens_run_recorded: sample 0 is the state at entry, sample s the state after tick s * every.  A sampled tick is
 * issued closed -- force launch, the energy launches if asked, the divergence launch, a separate kick + drift -- so
 * the trajectory is bit-identical to nb_ens_step(nsteps); force_launches grows by nsteps; every member takes nsteps
 * ticks.  Nothing waits on the stream before the one copy-out.  NB_ERR_INVALID for every < 1, nsteps < 0, a
 * baseline that is no member or too small a capacity, before anything is launched. */
int nb_ens_run_diverged(nb_ens *e, int32_t nsteps, int32_t every, const int32_t *baseline, int32_t with_energies,
                        double *max_pos, double *mean_pos, double *max_vel, double *kinetic, double *potential,
                        int64_t capacity, int on_device, int32_t *samples);
/* The diagnostics of nb_metrics (rotation curve, r_percentile, bound fraction, dispersion) for every member, from
 * the resident state, in ONE kernel launch (one workgroup per member; no host round trip before the copy-out).
 * num_bins in [0, 255].  max_radius: `members` doubles, each >= 0 or NaN, the end of that member's bin edges; or
 * NULL: each member's own largest radius, found on the device.  The edges are torch.linspace(0, max_radius[b],
 * num_bins + 1) in float32, built on the device.  Outputs are host arrays, any may be NULL: curve_mean /
 * curve_count members * num_bins (member-major; an empty bin has mean NaN), edges members * (num_bins + 1),
 * scalars members * 5 = per member {max r, r_kth, bound fraction, dispersion, max_radius used}, the layout of
 * nb_metrics' scalars[5]; G is the member's own.  Per-star arithmetic is nb_metrics' in the state dtype, so bin
 * membership, bound flags and the order statistic are a solo evaluation's; the fp64 sums behind the centre of
 * mass, enclosed masses, bin means and dispersion are added in a fixed order of their own (deterministic,
 * independent of the other members; equal to nb_metrics wherever the value does not depend on that order, else
 * to 2e-6 relative).  Needs positions, velocities and masses.  Changes neither the state nor force_launches.
 * NB_ERR_INVALID for num_bins outside [0, 255], a negative max_radius entry or a NaN percentile. */
int nb_ens_metrics(nb_ens *e, int32_t num_bins, const double *max_radius, double percentile, double *curve_mean,
                   int64_t *curve_count, float *edges, double *scalars);
/* members; batched force launches issued since creation (nb_ens_compute_accelerations and one per tick;
 * the opening kick + drift launch of an nb_ens_step is not counted); name of the last force kernel
 * ("ens_step_kernel", "ens_step_mixed_kernel" on a handle of nb_ens_create_mixed, "ens_step_ragged_kernel" on a
 * handle of nb_ens_create_ragged, "ens_grid_step_ragged_kernel" on one of nb_ens_create_ragged_grid, or "ens_grid_step_kernel" on a
 * grid-mode handle -- "ens_grid_step_wide_kernel" when a member exceeds 256 levels -- whose table and finish launches
 * are not counted either; "none" before the first).  Any output may be NULL. */
int nb_ens_info(nb_ens *e, int32_t *members, int64_t *force_launches, const char **kernel_name);
/* Grid-mode handles: out[8 b .. 8 b + 7] = member b's {lmin, lmax, fmin, fmax, r2max, fast_ok, fast_maxdev,
 * fast_maxrel} of the LAST evaluation, the layout of nb_quant_debug's info (fmin / fmax NaN under NB_CUSTOM,
 * which does not quantise forces).  NB_ERR_UNSUPPORTED on a handle of nb_ens_create. */
int nb_ens_quant_info(nb_ens *e, double *out /* members * 8 */);
/* Grid-mode handles: nb_quant_bin_sums for every member, read out of the production pair sweep (its BINS
 * instantiation) on the members' CURRENT positions: sum_k / sum_kw are (members, n) -- per star p the check-sums
 * s1 = sum_q k(p, q) and s2 = sum_q k(p, q) ((q mod 65521) + 1) of the bin every pair was given -- and
 * pairs[2 b], pairs[2 b + 1] member b's pair evaluations binned table-free / through a threshold table.  Any
 * output may be NULL.  An observer: the forces of the read-out go to a scratch buffer, the tables are rebuilt
 * from the same positions (the same values); state, accelerations and force_launches are untouched.  A member on
 * a degenerate grid (values pass through, no bins) reports zeros.  NB_ERR_UNSUPPORTED on a handle of nb_ens_create
 * or nb_ens_create_mixed. */
int nb_ens_quant_bin_sums(nb_ens *e, int64_t *sum_k, int64_t *sum_kw, int64_t *pairs /* members * 2 */);
int nb_ens_synchronize(nb_ens *e);

/* ---- precision-hook introspection ---------------------------------------------------- */

/* Grid-mode internals of the LAST force evaluation: info[0..3] = lmin, lmax (log-grid of
 * quantization.py:109-113), fmin, fmax (linear force grid, quantization.py:78-79);
 * info[4] = max r^2 over all pairs; info[5] = 1 when the table-free pair path was enabled for that evaluation,
 * info[6] = measured deviation of its bin estimate at the bin edges (in bins), info[7] = measured relative
 * deviation of its force factors from the exact table entries (enabled only when <= 1e-6).  If d2bins != NULL (host, n*n int16, row i / column j)
 * the distance-bin index of every pair is recomputed on the device with the same tables the
 * force kernel used; fbins (host, n*dim int16) likewise for the force bins of INT8/INT4.
 * -1 marks "degenerate grid: value passed through" (quantization.py:115-116 / :81-82). */
int nb_quant_debug(nb_sim *s, double info[8], int16_t *d2bins, int16_t *fbins);
/* The same distance-bin indices for target rows [i0, i1) only (host, (i1-i0)*n int16): sizes where n*n is out of reach. */
int nb_quant_bins_rows(nb_sim *s, int32_t i0, int32_t i1, int16_t *d2bins);
/* Quant-bin assignments (the index round(normalized * (levels - 1)) of quantization.py:119-121) read out of the
 * PRODUCTION pair loop itself.  The two calls above walk the exact threshold tables in a kernel of their own; this one
 * runs the evaluation once more on the current positions with the very kernel templates the force path launches,
 * instantiated with an integer read-out at the point where each pair's bin is decided (table-free estimate, wave
 * ballot, threshold fallback, uniform / general-mass kernels, packed and scalar sweeps, the one-launch small-system
 * kernel), and returns per particle p (host arrays of n int64):
 *     sum_k[p]  = sum over all q of k(p, q)
 *     sum_kw[p] = sum over all q of k(p, q) * ((q mod 65521) + 1)
 * (q = p included: the reference's N x N bin matrix holds k = 0 on the diagonal).  Integer sums: exact, independent
 * of the summation order, comparable bit for bit with the same sums over a row of the reference's bin matrix.
 * which: 0 = the path the last evaluation / step took (nb_force_kernel_name), 1 = the tiled evaluation path of
 * nb_compute_accelerations, 2 = the one-launch small-system step kernel.
 * info (may be NULL): [0] path taken (1 pair-symmetric tiles, 2 one-sided tiles, 3 small-system kernel), [1] targets
 * per lane (path 1) / lanes per target (path 3), [2] 1 if the uniform-mass packed kernel did the work, [3] 1 if the
 * tables enabled the table-free pair path, [4] pair evaluations binned by the table-free estimate alone, [5] pair
 * evaluations binned through a threshold table, [6] grid levels.  Degenerate grids (values pass through, no bins),
 * the generic per-pair path and handles with a communicator return NB_ERR_UNSUPPORTED.  A read-only call: the pair
 * sums of the extra evaluation go to a scratch buffer and no force quantisation follows, so positions, velocities,
 * accelerations (values and dtype), the force bins and bounds nb_quant_debug reports and nb_force_kernel_name are what
 * the last evaluation left, and the steps that follow are bit-identical to those of a handle that was never read.  The
 * grid tables are rebuilt from the same positions (same values). */
int nb_quant_bin_sums(nb_sim *s, int32_t which, int64_t *sum_k, int64_t *sum_kw, double info[8]);

/* ---- tensor-level hooks (quantization.py module functions used by override subclasses) -- */

/* quantize_distance_squared(dist_sq, mode, custom_levels, min_dist_sq) quantization.py:21.
 * in/out: `count` elements of `dtype` (NB_F32 or NB_F64); *out_dtype receives the result
 * dtype (FLOAT64 -> f64, FLOAT32/BF16/F16 -> f32, grid modes -> input dtype). */
int nb_quantize_distance_squared(int device, const void *in, void *out, int64_t count, int dtype,
                                 int mode, int levels, double min_dist_sq, int on_device,
                                 int32_t *out_dtype);
/* quantize_force(force, mode, custom_levels) quantization.py:130 */
int nb_quantize_force(int device, const void *in, void *out, int64_t count, int dtype,
                      int mode, int levels, int on_device, int32_t *out_dtype);
/* _grid_quantize(tensor, levels) quantization.py:74 */
int nb_grid_quantize(int device, const void *in, void *out, int64_t count, int dtype,
                     int levels, int on_device);
/* _grid_quantize_safe(tensor, levels, min_val) quantization.py:91 */
int nb_grid_quantize_safe(int device, const void *in, void *out, int64_t count, int dtype,
                          int levels, double min_val, int on_device);

/* Stream of the calling thread for the handle-less entry points on `device` (the four hooks above and
 * nb_metrics_tensors): they queue their kernels there and, for device-resident buffers, return without waiting --
 * ordered with the caller's own device work like any other stream operation.  enable = 0 restores the default
 * (NULL stream, blocking).  Thread-local; no device allocation per call (a per-device scratch is cached). */
int nb_set_hook_stream(int device, void *hip_stream, int enable);

/* ---- diagnostics --------------------------------------------------------------------- */

/* metrics.py:25-156 on the handle's CURRENT state, on the device (stable radix sort + fixed-order scan for the
 * order statistic and the enclosed masses):
 *   compute_rotation_curve  -> curve_mean[num_bins] (NaN for empty bins), curve_count[num_bins]
 *   compute_galaxy_radius   -> scalars[1] = sorted(r)[min(int(n * percentile / 100), n - 1)]
 *   compute_bound_fraction  -> scalars[2]        compute_velocity_dispersion -> scalars[3]
 *   scalars[0] = radii.max(), scalars[4] = the max_radius the bin edges were built from.
 * edges: host, num_bins + 1 float32 (what torch.linspace(0, max_radius, num_bins + 1) returns), or NULL to have
 * them built here from max_radius (< 0: radii.max()).  radius_only != 0: only scalars[0] (first phase of a caller
 * that builds the edges itself).  Any output pointer may be NULL. */
int nb_metrics(nb_sim *s, int32_t num_bins, const float *edges, double max_radius, double percentile,
               int32_t radius_only, double *curve_mean, int64_t *curve_count, double scalars[5]);
/* The same on caller tensors (n x dim positions / velocities, n masses; NB_F32 or NB_F64; host or device). */
int nb_metrics_tensors(int device, const void *pos, const void *vel, const void *mass, int32_t n, int32_t dim,
                       int dtype, int on_device, double G, int32_t num_bins, const float *edges, double max_radius,
                       double percentile, int32_t radius_only, double *curve_mean, int64_t *curve_count,
                       double scalars[5]);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) --------------------------------- */

/* Partition: every rank holds the full O(N) state.  The pair work is split by
 * TARGET super-rows of the pair-symmetric kernel (snake-dealt, equal pair counts) -- or, on the one-sided
 * kernels, by contiguous SOURCE blocks [rank*N/P, (rank+1)*N/P) -- each rank produces partial accelerations
 * for all particles, and one all-reduce (sum) of the (n, dim) force vectors per step -- RCCL, or the direct path
 * declared below -- completes them
 * (issued in 1..4 prefix slices that overlap the remaining pair work when a step is long enough).
 *
 * ONE communicator per process, shared by every handle of the process:
 *   rank 0 obtains an id (ncclGetUniqueId) and ships the bytes to the other ranks by any means
 *   (torch.distributed store / gloo broadcast); every rank then calls nb_comm_init on its first handle
 *   (collective).  Later handles attach with nb_comm_init(h, NULL, 0) -- no communication.
 *   nb_destroy() never touches the communicator; nb_comm_shutdown() destroys it and is collective:
 *   every rank calls it once, after its last step and before the transport that carried the id goes away. */
int nb_comm_unique_id(void *id_out, int32_t *id_bytes /* in: capacity, out: size */);
int nb_comm_init(nb_sim *s, const void *id /* NULL: attach the existing process communicator */, int32_t id_bytes);
int nb_comm_ready(void);      /* ranks of the process communicator, 0 when there is none */
/* What the process communicator is (for the caller's records): info = {ranks, rank, device, 1 if direct-only (no RCCL),
 * ncclCommCount() of the RCCL communicator (-1: none), state of the direct all-reduce (0 none, 1 attached, 2 enabled),
 * its rank count, communicator generation (handles attached to an older generation fail with NB_ERR_COMM)}. */
int nb_comm_info(int32_t info[8]);
int nb_comm_quiesce(void);    /* first half of a shutdown: wait for this process's device work (then: a barrier of the
                               * host transport, so that no rank frees buffers a peer still reads; then nb_comm_shutdown) */
int nb_comm_shutdown(void);

/* Direct xGMI all-reduce of small force vectors (csrc/nb_p2p.hip).  The per-step collective at
 * the benchmark size is 1 MiB between 8 GPUs -- pure latency -- so, next to the RCCL communicator, the ranks of ONE
 * node can attach a two-hop all-reduce that loads directly from the peers' memory over xGMI (one kernel, rank-ordered
 * sums: bit-identical on all ranks).  Setup, driven by the host language over its own transport:
 *   every rank: nb_comm_p2p_export (allocates the shared region; returns its HIP IPC handle)
 *   all-gather the handles in rank order; every rank: nb_comm_p2p_import(handles, nranks)
 *   barrier; every rank: nb_comm_p2p_selftest (collective; bounded waits); combine the verdicts (logical AND);
 *   every rank: nb_comm_p2p_enable(verdict).
 * A handle may also attach WITHOUT any RCCL communicator: when no process communicator exists yet, the direct path is
 * enabled between exactly the handle's ranks and nb_comm_init gets a NULL id, the process communicator becomes
 * "direct only" -- every sum (forces, potential energy) takes the direct path, vectors above capacity_bytes are an
 * error.  (Several ranks may then share one GPU, which RCCL refuses: how the multi-rank step is tested on one GPU.)
 * Once enabled, nb_step / nb_compute_accelerations use it for force vectors of at most capacity_bytes (fp32: even
 * element counts), and RCCL for everything else; NB_NO_P2P=1 (read at nb_create) keeps a handle on RCCL.  A peer that
 * does not arrive within 300 s raises an error at the next nb_synchronize.  nb_comm_shutdown releases the region. */
int nb_comm_p2p_export(int32_t device, int32_t rank, int32_t nranks, int64_t capacity_bytes, void *handle_out,
                       int32_t *handle_bytes /* in: capacity (>= 64), out: size */);
int nb_comm_p2p_import(const void *handles /* nranks handles, rank order */, int32_t nranks);
int nb_comm_p2p_selftest(int32_t rounds, double timeout_s);
int nb_comm_p2p_enable(int32_t on);
int nb_comm_p2p_state(void);  /* 0 none, 1 attached, 2 enabled */
/* measurement (collective): average microseconds of `iters` back-to-back all-reduces of this handle's force-vector
 * size on zeroed scratch -- which = 0: RCCL, 1: the direct path -- so a multi-GPU bench can state what its collective
 * costs on the node it ran on.  s = NULL: a 1 MiB vector of doubles on the process communicator / the attached direct
 * path (what the host language compares before it enables the direct path) */
int nb_comm_allreduce_time(nb_sim *s, int32_t which, int32_t iters, double *us_per_call);
/* tests: the direct all-reduce kernel between `nranks` VIRTUAL ranks inside this process (a one-GPU box can then run
 * the 8-rank geometry): concurrent = 0 runs the ranks' kernels one after the other with pre-satisfied flags, twice;
 * concurrent = 1 uses one stream per rank and the real barriers (as many hardware queues as ranks: up to 4),
 * concurrent = 2 runs all ranks in one dispatch (co-resident by construction, any rank count); both report the time
 * per all-reduce.  concurrent = 3: like 1, but the last rank never launches its all-reduce (a dead peer): the others
 * must leave their barriers after timeout_s, raise their status word and drain -- the call returns NB_OK with
 * *bad >= 1e6.  *bad = elements that differ from the closed form (+1e6 per rank whose barrier timed out). */
int nb_comm_p2p_virtual_test(int32_t device, int32_t nranks, int64_t count, int32_t dtype, int32_t concurrent,
                             int32_t iters, double timeout_s, int32_t *bad, double *us_per_call);
/* tests: all-reduce `count` host elements (NB_F32 / NB_F64) in place through the direct path (collective) */
int nb_comm_p2p_allreduce(void *host_inout, int64_t count, int32_t dtype, double timeout_s);

/* The work plan of the pair-symmetric kernels for one rank, computed WITHOUT a device (pure host code; what
 * nb_set_state uploads).  For tests of the partition: the union over ranks must cover every tile pair once.
 * info[0..11] = enabled, targets per lane R, tile size, padded tiles, padded particles, work items, row slots,
 * column-slab entries, source tiles per item, pipeline chunks, column-slab MiB, row-slab MiB; info[12] = step pieces
 * of the row-split work items (0: classic items), info[13] = targets per thread of the one-sided fp64 kernel,
 * info[14] / info[15] = source chunks of the one-sided kernels (force, potential energy, generic) and sources per chunk
 * for this rank's j-range.
 * work: items x 8 int32 {tile_i, jt_begin, jt_end, slot, slot_stride, col_ord, s_begin, s_count};
 * row_slot0 / row_nslots / col_upto: one int32 per padded tile; chunk_work / chunk_tile: chunks + 1 offsets
 * (work-item ranges / tile boundaries; chunk_tile is the same on every rank).  Any output may be NULL.
 * multi != 0: a communicator will sum the partial forces (enables pipeline chunks); cus: compute units (256). */
int nb_plan_debug(const nb_config *cfg, int32_t is_f64, int32_t multi, int32_t cus, int32_t info[16], int32_t *work,
                  int64_t work_capacity, int32_t *row_slot0, int32_t *row_nslots, int32_t *col_upto,
                  int32_t *chunk_work, int32_t *chunk_tile);

/* ---- measurement --------------------------------------------------------------------- */

/* With NB_FLAG_PROFILE: HIP-event time of the force kernel launches since the last call
 * (events recorded on the handle's own stream).  total_ms / launches = average duration. */
int nb_kernel_time(nb_sim *s, double *total_ms, int32_t *launches);
/* Name of the force kernel the last nb_compute_accelerations / nb_step launched (for matching
 * rocprofv3 rows by prefix): "force_sym_kernel<double", "force_sym_kernel<float", "force_f64_kernel",
 * "force_f32_kernel" or "none". */
const char *nb_force_kernel_name(nb_sim *s);
/* The potential-energy kernel variant the last nb_energy(..., potential) launched, with its template arguments, e.g.
 * "potential_sym_kernel<double,2,4,f32t=0,uniform=0,mass=f32,rowsplit>" or "potential_kernel<double,3,pa_f32=1,hp=f16>";
 * "none" before the first potential-energy evaluation. */
const char *nb_pe_kernel_name(nb_sim *s);
/* Where the leapfrog kicks of the last nb_step / nb_kick_drift / nb_kick ran, noted on the host where the launches are
 * issued (no device work): up to three space-separated parts, each a '+'-joined list of "<site>[:<kick mode>]",
 *   open=   opening kick + drift of the call's first step: "spec_read" (the previous call's speculative positions,
 *           kick applied on read), "pack:1", "kick_drift", "kick_a32" (fp32-typed accelerations on fp64 storage)
 *   mid=    interior steps: closing kick + next opening kick + drift in one launch (mode 2: "reduce_sym:2", "reduce:2",
 *           "small:2", "fq_finish:2,packed,red_mm", "p2p:2,x64", "sums64:2", "pack:2" for a deferred closing kick), or
 *           the separate launches of a step that cannot fuse them
 *   close=  closing kick of the last step: mode 1, or 3 when the launch also leaves the next step's positions
 *           ("reduce_sym:3", "small:3"); "|4" marks a launch that applied its step's opening kick on read; "axpy"
 * e.g. "open=spec_read close=reduce_sym:3|4", "open=kick_drift mid=small:2 close=small:3".  "none" before the first.
 * The pointer is owned by the handle and valid until the next call on it. */
const char *nb_step_path_name(nb_sim *s);
/* Block until all work queued on the handle's stream has finished. */
int nb_synchronize(nb_sim *s);

/* ---- misc ---------------------------------------------------------------------------- */
int nb_device_count(int32_t *count);
int nb_abi_version(void);
const char *nb_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_AMD_H */
