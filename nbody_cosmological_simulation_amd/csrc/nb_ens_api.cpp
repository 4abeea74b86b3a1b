// nb_ens_api.cpp -- nb_ens handles (include/nbody_amd.h): B independent systems, each with its own G / softening / dt,
// advanced together -- ONE force launch per tick where a loop of solo handles issues B.  Host orchestration only, as in
// nb_api.cpp / nb_step.cpp.
//
// Layout.  Contiguous (B, N, D) positions (two buffers: they ping-pong as in the solo step), velocities, accelerations and
// (B, N) masses in the storage type (fp64 under FLOAT64, else fp32), and a device array of one EnsScalars record per
// member, cast on the host exactly as the solo launch casts them.  Beside these, by the kind of handle: the members' hooks
// (a mode list: every member its own cast mode); one GridTables and one level count per member and, under INT8 / INT4, the
// force launch's per-workgroup {min, max} partials and a (B, 2) array of force bounds (the grid modes); the members' sizes
// and the work list of the step (members of different sizes: cfg.n is then the capacity, member b owns the first sizes[b]
// rows of its slice and no kernel touches the rest).  Everything an observer or a sampled run needs is created on first
// use.  Every device buffer is a DevBuf the handle owns, and what the step kernels read is listed once, in the handle's
// EnsStepArgs (nb_internal.h).
//
// Creation.  The six nb_ens_create* entries are their own argument checks in front of ONE create(): the shared
// refusals in their order (null, shape, the entry's mode rule, the lists, the n limit, the device), every allocation and
// upload, one wait, one failure exit.
//
// The launch train.  launch_force is one force evaluation: it picks the step launcher from what the record holds (tables:
// a grid step behind the tables launches, with the finish launch under INT8 / INT4, which snaps the forces and carries
// the kicks IN PLACE -- with sizes as well: the same three launches in their ragged forms; sizes: the ragged step over the
// work list; hooks: the mixed step; else the uniform step) and notes
// the kernel's name.  run_train is nb_ens_step's train of launches: one kick + drift, then one force launch per tick.  The
// members' stop ticks, where a run has them, are a device array that every kernel of the tick path reads (nb_device.h)
// and a watch kernel lowers on the device (nb_ens_watch.hip, nb_ens_crash.hip); without one the instantiations without
// stops are launched, and `sizes` selects the instantiations for members of different sizes in the same way.
//
// The sampled run.  nb_ens_run_recorded, nb_ens_run_members, nb_ens_run_crash_watched and nb_ens_run_diverged are
// argument checks in front of run_sampled: the same train with samples (energies, nb_ens_energy.hip; the divergence
// between members, nb_ens_diverge.hip) into histories on the device, copied out once at the end, and one wait.
//
// Observers.  nb_ens_energy must equal a solo handle's energies bit for bit, whichever kernel variant the solo engine
// picks for this shape and these masses: each member's slice is handed (device to device) to one solo handle of the same
// shape kept for that purpose, and nb_energy runs there (a ragged handle returns the batched values: the probe would have
// the capacity's shape).  nb_ens_energies, nb_ens_divergence, nb_ens_crash_measures and nb_ens_metrics are one sampler's
// kernels alone on the resident state; nb_ens_quant_bin_sums runs the grid evaluation once more with the BINS
// instantiation of the pair sweep, forces into a scratch buffer.  The entries whose kernels are one workgroup per member
// of one shape refuse a ragged handle, and the grid modes' read-outs one that is no grid handle (refuse_ragged).
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <initializer_list>

#include "nb_state.h"

using namespace nbhost;

namespace {

// A device buffer the handle owns: grows, never shrinks, freed with the handle.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    // Room for `want` bytes.  The old block goes before the new one comes: no launch reads the old block -- a buffer of a
    // fixed size is reserved once, and every call that fills one that grows (a history, the diagnostics' results) copies it
    // out and waits before it returns.
    hipError_t reserve(size_t want)
    {
        if (want <= bytes) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        const hipError_t he = hipMalloc(&p, want);
        if (he == hipSuccess) bytes = want;
        else p = nullptr;
        return he;
    }
    template <typename T>
    T *as() const { return (T *)p; }
};

// `cap` samples of a few values per member, on the device: plane k holds value k of every sample, index s * members + b
struct History {
    DevBuf buf;
    int64_t cap = 0;
    double *plane(int k, int members) const { return buf.as<double>() + (size_t)k * cap * members; }
};

}  // namespace

struct nb_ens {
    nb_ens_config cfg{};
    hipStream_t stream = nullptr;
    EnsStepArgs step{};                       // what the step launchers read: filled once by create(); pos_in / pos_out swap
    std::vector<double> G, eps2, dt;          // per member, as given
    std::vector<char> prm_host;               // what the device array holds (or is about to)
    bool have_pos = false, have_vel = false, have_mass = false, have_acc = false;
    int64_t force_launches = 0;               // batched force launches since creation (kick + drift launches not counted)
    const char *last_kernel = "none";
    nb_sim *probe = nullptr;                  // solo handle of the members' shape: energies (created on first use)
    // grid modes only (nb_ens_create_grid, nb_ens_create_grid_wide)
    bool grid = false, fq = false;            // HOOK_GRID; INT8 / INT4: forces snapped (and kicks applied) by the finish launch
    int allow_fast = 1;                       // the table-free pair path may be used (NB_NO_GRID_FAST unset), as nb_sim reads it
    int grid_blocks = 0;                      // workgroups per member of the grid step: min / max partials per member (members
                                              // of different sizes: the capacity's, at the ragged launch's workgroup size)
    std::vector<int32_t> levels;              // per member
    // what is uploaded / read back around a run (free to rewrite: every call that uploads one waits before it returns)
    std::vector<int32_t> stops_host;          // members stop ticks, then members halt reasons
    std::vector<double> crash_host;           // members * 4 measures, then members flags
    std::vector<int32_t> base_host;           // the members' baselines
    std::vector<int32_t> sizes_host;          // members of different sizes (nb_ens_create_ragged): every member's size
    struct {
        DevBuf prm;                           // one EnsScalars of the storage type per member
        DevBuf pos, pos_alt, vel, acc, mass;
        DevBuf hooks;                         // a mode list: the hook of every member
        DevBuf tabs, levels;                  // grid modes: one GridTables (max r2, arrival counter, the evaluation's tables)
                                              // and one level count per member
        DevBuf fpart, fbounds;                // INT8 / INT4: members * grid_blocks * 2 partials; members * {fmin, fmax}
        DevBuf work, sizes;                   // members of different sizes: the work list of the step, built once; the sizes
        // created on first use
        DevBuf epart;                         // batched energies: members * tile pairs * {pe, ke} slots
        DevBuf mscratch;                      // batched diagnostics: vt, |v| and bin of every star of every member
        DevBuf mout, mradius, medges;         // ... members * (5 + 2 bins) results; members given max_radius; the edges
        DevBuf bin_acc, bin_out;              // nb_ens_quant_bin_sums: the read-out's forces; members * (2 n + 2) words
        DevBuf stops;                         // members stop ticks, then members halt reasons
        DevBuf prev_pos, dt, crash_out;       // crash-point detector: the positions of the previous tick; the members' dt as
                                              // given; members * 4 measures, then members flags
        DevBuf base;                          // divergence between members: the members' baselines
    } dev;
    History ehist;                            // batched energies: kinetic, potential
    History dhist;                            // divergence: max |d position|, mean |d position|, max |d velocity|
};

namespace {

// what run_train launches behind the energy launches of a sampled tick
enum WatchMode { WATCH_NONE, WATCH_EXPLOSION, WATCH_CRASH };
// what a sample of run_train holds (a bit set; 0: the run takes no samples)
enum SampleBits { SAMPLE_ENERGIES = 1, SAMPLE_DIVERGENCE = 2 };

inline size_t el(const nb_ens *e) { return e->step.is_f64 ? 8 : 4; }
inline size_t cnt_nd(const nb_ens *e) { return (size_t)e->cfg.members * e->cfg.n * e->cfg.dim; }
inline size_t cnt_n(const nb_ens *e) { return (size_t)e->cfg.members * e->cfg.n; }

// one EnsScalars<T> per member with the casts of nb_launch_small_step / launch_s: (T)G, (T)eps2, (T)(dt / 2), (T)dt
template <typename T>
void fill_params(nb_ens *e)
{
    e->prm_host.resize(e->G.size() * sizeof(EnsScalars<T>));
    for (size_t b = 0; b < e->G.size(); ++b) {
        const EnsScalars<T> p = {(T)e->G[b], (T)e->eps2[b], (T)(e->dt[b] / 2), (T)e->dt[b]};
        memcpy(e->prm_host.data() + b * sizeof p, &p, sizeof p);
    }
}

void fill_params(nb_ens *e)
{
    if (e->step.is_f64) fill_params<double>(e);
    else fill_params<float>(e);
}

int upload_params(nb_ens *e)
{
    fill_params(e);
    // on the handle's stream, behind the launches that still read the old values; the wait keeps prm_host free to rewrite
    HIPCHK(hipMemcpyAsync(e->dev.prm.p, e->prm_host.data(), e->prm_host.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return NB_OK;
}

// the tables of one evaluation of a grid-mode ensemble: max r2 of every member and its single-block tables in one launch;
// members above NB_LUT_MIN levels get theirs from a second one (neither is counted by force_launches)
int launch_tables(nb_ens *e, const int *stop, int t)
{
    const EnsStepArgs &a = e->step;
    GridTables *tabs = e->dev.tabs.as<GridTables>();
    const int *levels = e->dev.levels.as<int>();
    HIPCHK(nb_launch_ens_r2max_tables((const float *)a.pos_in, a.members, a.n, a.dim, a.prm, tabs, levels, 0.01f, e->allow_fast,
                                      stop, t, e->stream, a.sizes));
    if (a.max_levels > NB_LUT_MIN)
        HIPCHK(nb_launch_ens_tables_wide(a.members, a.max_levels, a.prm, tabs, levels, 0.01f, e->allow_fast, stop, t, e->stream));
    return NB_OK;
}

// a NB_KICK_CLOSE_OPEN evaluation left the drifted positions in pos_out (else in place: INT8 / INT4)
inline void advance_positions(nb_ens *e)
{
    if (!e->fq) std::swap(e->step.pos_in, e->step.pos_out);
}

// One force evaluation: the step launcher of this kind of handle and its kernel's name.  A grid-mode one is step_small's
// sequence (nb_step.cpp) batched: the tables, the grid step, and under INT8 / INT4 the finish launch (stop / t:
// nb_internal.h).
int launch_force(nb_ens *e, int do_kick, const int *stop = nullptr, int t = 0)
{
    const EnsStepArgs &a = e->step;
    const char *name;
    if (e->grid) {
        if (int rc = launch_tables(e, stop, t)) return rc;
        if (a.max_levels > NB_LUT_MIN) {        // (CUSTOM only: no force bounds, no finish launch)
            HIPCHK(nb_launch_ens_grid_step_wide(a, do_kick, stop, t, e->stream));
            name = "ens_grid_step_wide_kernel";
        } else if (a.sizes) {                   // members of different sizes: the same three launches, each with `sizes`
            HIPCHK(nb_launch_ens_grid_step_ragged(a, e->fq ? NB_KICK_NONE : do_kick, stop, t, e->stream));
            if (e->fq)
                HIPCHK(nb_launch_ens_force_quant_finish((float *)a.acc, a.members, a.n * a.dim, e->levels[0], a.part,
                                                        e->grid_blocks, e->dev.fbounds.as<double>(), (float *)a.vel,
                                                        (float *)a.pos_in, a.prm, do_kick, stop, t, e->stream, a.sizes, a.dim,
                                                        NB_ENS_RAGGED_BLOCK / a.lanes));
            name = "ens_grid_step_ragged_kernel";
        } else {
            HIPCHK(nb_launch_ens_grid_step(a, e->fq ? NB_KICK_NONE : do_kick, stop, t, e->stream));
            if (e->fq)      // levels[0]: under INT8 / INT4 every member has the mode's 256 / 16 levels
                HIPCHK(nb_launch_ens_force_quant_finish((float *)a.acc, a.members, a.n * a.dim, e->levels[0], a.part,
                                                        e->grid_blocks, e->dev.fbounds.as<double>(), (float *)a.vel,
                                                        (float *)a.pos_in, a.prm, do_kick, stop, t, e->stream));
            name = "ens_grid_step_kernel";
        }
    } else if (a.sizes) {
        HIPCHK(nb_launch_ens_step_ragged(a, do_kick, stop, t, e->stream));
        name = "ens_step_ragged_kernel";
    } else if (a.hooks) {
        HIPCHK(nb_launch_ens_step_mixed(a, do_kick, stop, t, e->stream));
        name = "ens_step_mixed_kernel";
    } else {
        HIPCHK(nb_launch_ens_step(a, do_kick, stop, t, e->stream));
        name = "ens_step_kernel";
    }
    e->force_launches++;
    e->last_kernel = name;
    return NB_OK;
}

int copy_in(nb_ens *e, void *dst, const void *src, size_t count, int on_device)
{
    HIPCHK(hipMemcpyAsync(dst, src, count * el(e), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream));
    return NB_OK;
}

int copy_out(nb_ens *e, void *dst, const void *src, size_t count, int on_device)
{
    HIPCHK(hipMemcpyAsync(dst, src, count * el(e), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e->stream));
    return NB_OK;
}

// the probe, then the buffers (the handle's DevBufs), then the stream
void release(nb_ens *e)
{
    if (e->probe) (void)nb_destroy(e->probe);
    const hipStream_t stream = e->stream;
    delete e;
    if (stream) (void)hipStreamDestroy(stream);
}

// room for `samples` samples of `planes` values per member in `h` (`what` names the history in the error)
int history_room(nb_ens *e, History &h, int64_t samples, int planes, const char *what)
{
    if (samples <= h.cap) return NB_OK;
    h.cap = 0;
    const hipError_t he = h.buf.reserve((size_t)samples * e->cfg.members * planes * sizeof(double));
    if (he != hipSuccess)
        return fail(he == hipErrorOutOfMemory ? NB_ERR_OOM : NB_ERR_HIP, "%s history of %lld samples: %s", what,
                    (long long)samples, hipGetErrorString(he));
    h.cap = samples;
    return NB_OK;
}

// the first `samples` samples (may be 0) of the planes of `h` to the caller's arrays (any may be null); does not wait
int history_out(nb_ens *e, const History &h, int64_t samples, std::initializer_list<double *> out, int on_device)
{
    const size_t bytes = (size_t)samples * e->cfg.members * sizeof(double);
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    int k = 0;
    for (double *dst : out) {
        if (dst && bytes) HIPCHK(hipMemcpyAsync(dst, h.plane(k, e->cfg.members), bytes, kind, e->stream));
        ++k;
    }
    return NB_OK;
}

// room for `samples` samples of the batched energies
int energy_buffers(nb_ens *e, int64_t samples)
{
    HIPCHK(e->dev.epart.reserve((size_t)e->cfg.members * nb_ens_energy_pairs(e->cfg.n) * 2 * sizeof(double)));
    return history_room(e, e->ehist, samples, 2, "energy");
}

// room for `samples` samples of the divergence and for the baselines
int divergence_buffers(nb_ens *e, int64_t samples)
{
    HIPCHK(e->dev.base.reserve((size_t)e->cfg.members * sizeof(int)));
    return history_room(e, e->dhist, samples, 3, "divergence");
}

// baseline[0 .. members) name members; then on their way to the device (base_host is free to rewrite: every call that
// uploads it waits before it returns)
int upload_baselines(nb_ens *e, const int32_t *baseline)
{
    const int B = e->cfg.members;
    if (!baseline) return fail(NB_ERR_INVALID, "null baseline");
    for (int b = 0; b < B; ++b)
        if (baseline[b] < 0 || baseline[b] >= B)
            return fail(NB_ERR_INVALID, "baseline[%d] = %d is no member: must be in [0, %d)", b, baseline[b], B);
    for (int b = 0; e->step.sizes && b < B; ++b)
        if (e->sizes_host[baseline[b]] != e->sizes_host[b])
            return fail(NB_ERR_INVALID, "baseline[%d] = %d: member %d has %d stars and member %d has %d; a member is compared "
                                        "with a member of its own size", b, baseline[b], b, e->sizes_host[b], baseline[b],
                        e->sizes_host[baseline[b]]);
    e->base_host.assign(baseline, baseline + B);
    static_assert(sizeof(int32_t) == sizeof(int), "the kernel reads ints");
    HIPCHK(hipMemcpyAsync(e->dev.base.p, e->base_host.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, e->stream));
    return NB_OK;
}

// sample `s` of the divergence history: the resident state, one launch behind whatever the stream holds
int launch_divergence(nb_ens *e, int64_t s)
{
    const EnsStepArgs &a = e->step;
    HIPCHK(nb_launch_ens_divergence(a.pos_in, a.vel, a.members, a.n, a.dim, a.is_f64, e->dev.base.as<int>(), s,
                                    e->dhist.plane(0, a.members), e->dhist.plane(1, a.members), e->dhist.plane(2, a.members),
                                    e->stream, a.sizes));
    return NB_OK;
}

// the crash-point detector's buffers (fixed sizes: created once)
int crash_buffers(nb_ens *e)
{
    const size_t B = (size_t)e->cfg.members;
    HIPCHK(e->dev.prev_pos.reserve(cnt_nd(e) * el(e)));
    HIPCHK(e->dev.dt.reserve(B * sizeof(double)));
    HIPCHK(e->dev.crash_out.reserve(B * (4 * sizeof(double) + sizeof(int32_t))));
    return NB_OK;
}

inline int *crash_flags(nb_ens *e) { return (int *)(e->dev.crash_out.as<double>() + 4 * (size_t)e->cfg.members); }

// flags and measures to the host copy (the caller waits, then hands them on with crash_results)
int crash_out_async(nb_ens *e)
{
    const size_t B = (size_t)e->cfg.members;
    e->crash_host.resize(4 * B + (B + 1) / 2);          // the int32 flags ride behind the doubles
    HIPCHK(hipMemcpyAsync(e->crash_host.data(), e->dev.crash_out.p, B * (4 * sizeof(double) + sizeof(int32_t)),
                          hipMemcpyDeviceToHost, e->stream));
    return NB_OK;
}

void crash_results(const nb_ens *e, int32_t *flags, double *measures)
{
    const size_t B = (size_t)e->cfg.members;
    if (measures) memcpy(measures, e->crash_host.data(), 4 * B * sizeof(double));
    if (flags) memcpy(flags, e->crash_host.data() + 4 * B, B * sizeof(int32_t));
}

// sample `s` of the history: the resident state's energies, two launches behind whatever the stream holds
int launch_energy(nb_ens *e, int64_t s, bool with_kinetic)
{
    const EnsStepArgs &a = e->step;
    HIPCHK(nb_launch_ens_energy(a.pos_in, with_kinetic ? a.vel : nullptr, a.mass, a.members, a.n, a.dim, a.is_f64, a.prm,
                                e->dev.epart.as<double>(), e->ehist.plane(0, a.members), e->ehist.plane(1, a.members), s,
                                e->stream, a.sizes));
    return NB_OK;
}

// every member's energies from the resident state in one batched pass (nb_ens_energy.hip): two launches, one copy-out, one
// wait (nb_ens_energies; nb_ens_energy on a ragged handle)
int batched_energies(nb_ens *e, double *kinetic, double *potential, int on_device)
{
    if (int rc = energy_buffers(e, 1)) return rc;
    if (int rc = launch_energy(e, 0, kinetic != nullptr)) return rc;
    if (int rc = history_out(e, e->ehist, 1, {kinetic, potential}, on_device)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return NB_OK;
}

// The launch train of nb_ens_step and of every sampled run: `nmax` ticks (simulation.py:120-143).  One
// elementwise launch opens the first tick (kick + drift), then one force launch per tick closes it and opens the next
// (NB_KICK_CLOSE_OPEN: the drifted positions go to the second buffer); the last one only closes.  every >= 1: sample 0 is
// taken at entry, and a sampled tick is issued as a one-tick nb_ens_step issues it -- the force launch only closes the tick
// (velocities and positions are then what a reader sees), the two energy launches follow, then the watch of `watch`
// (none, the explosion watch, or the crash-point detector, which needs every = 1 and crash_buffers), and a separate
// kick + drift launch opens the next tick.  what: the SampleBits of a sample (0 with every = 0) -- the energy launches
// are issued with SAMPLE_ENERGIES, and SAMPLE_DIVERGENCE adds the divergence launch (divergence_buffers, upload_baselines)
// behind the watch, in front of the kick + drift.  stop: null, or the members' stop ticks on the device;
// every launch of the tick path gets it with the number of ticks closed so far.  Nothing waits on the stream.
int run_train(nb_ens *e, int32_t nmax, int32_t every, int *stop, WatchMode watch, unsigned what)
{
    const EnsStepArgs &a = e->step;          // (pos_in is read at every use: advance_positions swaps it)
    const int B = a.members;
    auto open_tick = [&](int t) {
        return nb_launch_ens_kick_drift(a.pos_in, a.vel, a.acc, B, a.n, a.dim, a.is_f64, a.prm, stop, t, e->stream, a.sizes);
    };
    if (what & SAMPLE_ENERGIES)
        if (int rc = launch_energy(e, 0, true)) return rc;
    if (what & SAMPLE_DIVERGENCE)
        if (int rc = launch_divergence(e, 0)) return rc;
    if (nmax >= 1) HIPCHK(open_tick(0));
    for (int t = 1; t <= nmax; ++t) {
        const bool last = (t == nmax), sampled = (what && t % every == 0);
        if (sampled || last) {
            if (int rc = launch_force(e, NB_KICK_CLOSE, stop, t - 1)) return rc;
            if (sampled && (what & SAMPLE_ENERGIES)) {
                if (int rc = launch_energy(e, t / every, true)) return rc;
                if (watch == WATCH_EXPLOSION)
                    HIPCHK(nb_launch_ens_watch(a.pos_in, a.vel, B, a.n, a.dim, a.is_f64, e->ehist.plane(0, B), e->ehist.plane(1, B),
                                               t / every, t, stop, stop + B, e->stream, a.sizes));
                else if (watch == WATCH_CRASH)
                    HIPCHK(nb_launch_ens_crash(a.pos_in, e->dev.prev_pos.p, a.vel, B, a.n, a.dim, a.is_f64, e->dev.dt.as<double>(),
                                               e->ehist.plane(0, B), e->ehist.plane(1, B), t / every, t, stop, stop + B,
                                               crash_flags(e), e->dev.crash_out.as<double>(), e->stream));
            }
            if (sampled && (what & SAMPLE_DIVERGENCE))
                if (int rc = launch_divergence(e, t / every)) return rc;
            if (!last) HIPCHK(open_tick(t));
        } else {
            if (int rc = launch_force(e, NB_KICK_CLOSE_OPEN, stop, t - 1)) return rc;
            advance_positions(e);                        // the launch wrote the drifted positions to the second buffer
        }
    }
    return NB_OK;
}

// what every stepping entry asks of the handle
int check_steppable(const nb_ens *e)
{
    if (!e) return fail(NB_ERR_INVALID, "null handle");
    if (!e->have_pos || !e->have_vel || !e->have_mass) return fail(NB_ERR_INVALID, "state incomplete");
    if (!e->have_acc) return fail(NB_ERR_INVALID, "no accelerations yet: call nb_ens_compute_accelerations first");
    return NB_OK;
}

// nsteps[0 .. members) are tick budgets: all >= 0, *nmax the largest
int check_budgets(const nb_ens *e, const int32_t *nsteps, int32_t *nmax)
{
    if (!nsteps) return fail(NB_ERR_INVALID, "null nsteps");
    *nmax = 0;
    for (int b = 0; b < e->cfg.members; ++b) {
        if (nsteps[b] < 0) return fail(NB_ERR_INVALID, "nsteps[%d] must be >= 0 (got %d)", b, nsteps[b]);
        *nmax = std::max(*nmax, nsteps[b]);
    }
    return NB_OK;
}

// what a sampled run is asked for: `nmax` ticks of run_train sampled every `every` (0: never) under `watch`, a sample
// holding `what` (SampleBits; with every >= 1)
struct SampledRun {
    int32_t nmax = 0, every = 0;
    WatchMode watch = WATCH_NONE;
    unsigned what = 0;
    const int32_t *budgets = nullptr;         // the members' stop ticks, or null: NO stop array is passed (kernels without stops)
    const int32_t *baseline = nullptr;        // SAMPLE_DIVERGENCE: the members' baselines (checked here: upload_baselines)
    double *kinetic = nullptr, *potential = nullptr;                      // out, `capacity` samples each; any may be null
    double *max_pos = nullptr, *mean_pos = nullptr, *max_vel = nullptr;
    int64_t capacity = 0;
    int on_device = 0;                        // where the five arrays above live
    int32_t *samples = nullptr;               // out: the samples taken; set last
    int32_t *stop_tick = nullptr, *why = nullptr;                         // out with budgets: stop ticks, halt reasons
    int32_t *flags = nullptr;                 // out under WATCH_CRASH: the detector's flags and measures
    double *measures = nullptr;
};

// The sampled run behind nb_ens_run_recorded / _members / _crash_watched / _diverged, arguments checked.  The budgets are
// uploaded beside halt reasons of 0 and read back into stop_tick / why.  The baselines are checked behind the capacity and
// in front of every launch: nothing is launched for a bad one.  WATCH_CRASH primes the detector in front of the launches
// (dt; zeroed flags and measures, which a member that is never checked -- budget 0 -- reports; the previous positions)
// and reads flags / measures back.  One wait, behind the copies of the histories.
int run_sampled(nb_ens *e, const SampledRun &r)
{
    const size_t B = (size_t)e->cfg.members;
    const int64_t S = r.every ? 1 + (int64_t)(r.nmax / r.every) : 0;
    if (r.capacity < S && r.watch == WATCH_CRASH)
        return fail(NB_ERR_INVALID, "capacity of %lld samples is below the %lld of %d ticks sampled every tick",
                    (long long)r.capacity, (long long)S, r.nmax);
    if (r.capacity < S)
        return fail(NB_ERR_INVALID, "capacity of %lld samples is below the %lld of %d ticks sampled every %d",
                    (long long)r.capacity, (long long)S, r.nmax, r.every);
    DeviceGuard guard(e->cfg.device);
    if (r.what & SAMPLE_DIVERGENCE) {
        if (int rc = divergence_buffers(e, S)) return rc;
        if (int rc = upload_baselines(e, r.baseline)) return rc;
    }
    if (r.what & SAMPLE_ENERGIES)
        if (int rc = energy_buffers(e, S)) return rc;
    if (r.watch == WATCH_CRASH)
        if (int rc = crash_buffers(e)) return rc;
    const size_t stop_bytes = 2 * B * sizeof(int32_t);
    int32_t *stops = nullptr;
    if (r.budgets) {
        HIPCHK(e->dev.stops.reserve(stop_bytes));
        stops = e->dev.stops.as<int32_t>();
        // stops_host is free to rewrite: every call that uploads it waits before it returns (e->dt: nb_ens_set_params waits too)
        static_assert(NB_ENS_REASON_NONE == 0 && NB_ENS_CRASH_NONE == 0, "one initial value serves both watches");
        e->stops_host.assign(2 * B, 0);
        std::copy(r.budgets, r.budgets + B, e->stops_host.begin());
        HIPCHK(hipMemcpyAsync(stops, e->stops_host.data(), stop_bytes, hipMemcpyHostToDevice, e->stream));
    }
    if (r.watch == WATCH_CRASH) {
        HIPCHK(hipMemcpyAsync(e->dev.dt.p, e->dt.data(), B * sizeof(double), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemsetAsync(e->dev.crash_out.p, 0, B * (4 * sizeof(double) + sizeof(int32_t)), e->stream));
        HIPCHK(hipMemcpyAsync(e->dev.prev_pos.p, e->step.pos_in, cnt_nd(e) * el(e), hipMemcpyDeviceToDevice, e->stream));
    }
    if (int rc = run_train(e, r.nmax, r.every, stops, r.watch, r.what)) return rc;
    if (r.budgets) HIPCHK(hipMemcpyAsync(e->stops_host.data(), stops, stop_bytes, hipMemcpyDeviceToHost, e->stream));
    if (r.watch == WATCH_CRASH)
        if (int rc = crash_out_async(e)) return rc;
    if (r.what & SAMPLE_DIVERGENCE)
        if (int rc = history_out(e, e->dhist, S, {r.max_pos, r.mean_pos, r.max_vel}, r.on_device)) return rc;
    if (r.what & SAMPLE_ENERGIES)
        if (int rc = history_out(e, e->ehist, S, {r.kinetic, r.potential}, r.on_device)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));      // the one wait of the call (with S = 0 too)
    if (r.budgets && r.stop_tick) std::copy(e->stops_host.begin(), e->stops_host.begin() + B, r.stop_tick);
    if (r.budgets && r.why) std::copy(e->stops_host.begin() + B, e->stops_host.end(), r.why);
    if (r.watch == WATCH_CRASH) crash_results(e, r.flags, r.measures);
    if (r.samples) *r.samples = (int32_t)S;
    return NB_OK;
}

// the entries a handle of nb_ens_create_ragged refuses: their kernels are one workgroup per member of the handle's n, or
// the grid modes' (which serve a handle of nb_ens_create_ragged_grid)
int refuse_ragged(const nb_ens *e, const char *entry, const char *follow_up)
{
    if (e->step.sizes)
        return fail(NB_ERR_UNSUPPORTED, "%s is not implemented for members of different sizes (nb_ens_create_ragged): %s is a "
                                        "follow-up", entry, follow_up);
    return NB_OK;
}

// what every constructor asks of the shape
int check_shape(const nb_ens_config *cfg)
{
    if (cfg->members < 1 || cfg->members > NB_ENS_MAX_MEMBERS)
        return fail(NB_ERR_INVALID, "members must be in [1, %d] (got %d)", NB_ENS_MAX_MEMBERS, cfg->members);
    if (cfg->n < 1) return fail(NB_ERR_INVALID, "n must be >= 1 (got %d)", cfg->n);
    if (cfg->dim != 2 && cfg->dim != 3) return fail(NB_ERR_INVALID, "dim must be 2 or 3 (got %d)", cfg->dim);
    return NB_OK;
}

// what a creator asks create() for
struct CreateSpec {
    nb_ens **out;
    const nb_ens_config *cfg;
    const double *G, *softening_sq, *dt;      // per member
    // a grid-mode handle (level_cap != 0): levels is null (the mode's 256 / 16 levels; 64 under CUSTOM) or `members` level
    // counts in [2, level_cap]; above_cap ends the refusal of a count outside
    const int32_t *levels = nullptr;
    int level_cap = 0;
    const char *above_cap = nullptr;
    const int32_t *modes = nullptr;           // null, or the cast mode of every member (cfg->mode: NB_FLOAT32)
    const int32_t *sizes = nullptr;           // null, or the size of every member, each in [1, cfg->n]
};

// The one creation path.  Refusals in the order every creator has them: null, shape, the creator's own rule for cfg->mode
// (mode_rule(): NB_OK or its fail()), the lists, the n limit, the device.  Then every allocation and upload of the handle,
// one wait and one failure exit.
template <typename ModeRule>
int create(const CreateSpec &s, ModeRule mode_rule)
{
    if (!s.out || !s.cfg || !s.G || !s.softening_sq || !s.dt) return fail(NB_ERR_INVALID, "null argument");
    *s.out = nullptr;
    const nb_ens_config *cfg = s.cfg;
    if (int rc = check_shape(cfg)) return rc;
    if (int rc = mode_rule()) return rc;
    const int B = cfg->members;
    std::vector<int32_t> lv;
    if (s.level_cap) {
        lv.assign(B, cfg->mode == NB_INT8_SIM ? 256 : cfg->mode == NB_INT4_SIM ? 16 : 64);
        if (s.levels) lv.assign(s.levels, s.levels + B);
        for (int b = 0; b < B; ++b)
            if (lv[b] < 2 || lv[b] > s.level_cap)
                return fail(NB_ERR_INVALID, "levels[%d] = %d is outside [2, %d]: %s", b, lv[b], s.level_cap, s.above_cap);
    }
    for (int b = 0; s.modes && b < B; ++b)
        if (s.modes[b] != NB_FLOAT32 && s.modes[b] != NB_BFLOAT16 && s.modes[b] != NB_FLOAT16)
            return fail(NB_ERR_UNSUPPORTED, "modes[%d] = %d: members of one ensemble mix the FLOAT32, BFLOAT16 and FLOAT16 modes "
                                            "only (FLOAT64 is stored differently, the grid modes need per-member tables)", b,
                        s.modes[b]);
    for (int b = 0; s.sizes && b < B; ++b)
        if (s.sizes[b] < 1 || s.sizes[b] > cfg->n)
            return fail(NB_ERR_INVALID, "sizes[%d] = %d is outside [1, %d]: member %d must fit the capacity cfg->n", b, s.sizes[b],
                        cfg->n, b);
    const bool f64 = cfg->mode == NB_FLOAT64;
    if (cfg->n > small_max_n(f64))
        return fail(NB_ERR_UNSUPPORTED, "n = %d is above the one-launch step's limit of %d for this mode: a single system of "
                                        "that size fills the chip, step it with nb_sim", cfg->n, small_max_n(f64));
    int ndev = 0;
    hipError_t err = hipGetDeviceCount(&ndev);
    if (err != hipSuccess || ndev == 0)
        return fail(NB_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU fallback",
                    err == hipSuccess ? "0 devices" : hipGetErrorString(err));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(NB_ERR_NO_DEVICE, "device %d out of range [0,%d)", cfg->device, ndev);
    DeviceGuard guard(cfg->device);
    nb_ens *e = new nb_ens();
    EnsStepArgs &a = e->step;
    e->cfg = *cfg;
    a.members = B; a.n = cfg->n; a.dim = cfg->dim; a.is_f64 = f64;
    a.hook = s.modes ? HOOK_AT_RUN_TIME : mode_hook(cfg->mode);
    const NbKnobs knobs = nb_read_knobs();
    a.lanes = knobs.small_lanes ? knobs.small_lanes : nb_small_lanes(cfg->n);     // as step_small picks them
    e->G.assign(s.G, s.G + B);
    e->eps2.assign(s.softening_sq, s.softening_sq + B);
    e->dt.assign(s.dt, s.dt + B);
    fill_params(e);
    // what the uploads below read until the wait: prm_host, e->levels and e->sizes_host, and these two
    std::vector<int> hooks;
    std::vector<EnsWork> work;
    static_assert(sizeof(int32_t) == sizeof(int), "the kernels read ints");
    hipError_t he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    auto room = [&](DevBuf &buf, size_t bytes) {
        if (he == hipSuccess) he = buf.reserve(bytes);
    };
    auto zeroed = [&](DevBuf &buf, size_t bytes) {
        room(buf, bytes);
        if (he == hipSuccess) he = hipMemsetAsync(buf.p, 0, bytes, e->stream);
    };
    auto uploaded = [&](DevBuf &buf, const void *src, size_t bytes) {
        room(buf, bytes);
        if (he == hipSuccess) he = hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, e->stream);
    };
    const size_t nd_bytes = cnt_nd(e) * el(e);
    uploaded(e->dev.prm, e->prm_host.data(), e->prm_host.size());
    room(e->dev.pos, nd_bytes);
    room(e->dev.pos_alt, nd_bytes);
    room(e->dev.vel, nd_bytes);
    zeroed(e->dev.acc, nd_bytes);
    room(e->dev.mass, cnt_n(e) * el(e));
    if (s.level_cap) {
        e->grid = true;
        e->fq = cfg->mode != NB_CUSTOM;
        e->allow_fast = knobs.no_grid_fast ? 0 : 1;
        // (a ragged handle: the one workgroup size of its launch, not the capacity's solo choice)
        e->grid_blocks = s.sizes ? nb_ens_ragged_blocks(cfg->n, a.lanes) : nb_small_blocks(cfg->n, a.lanes);
        e->levels = lv;
        a.max_levels = *std::max_element(lv.begin(), lv.end());
        // zeroed once: every evaluation puts a member's maximum and arrival counter back (grid_tables_body)
        zeroed(e->dev.tabs, (size_t)B * sizeof(GridTables));
        uploaded(e->dev.levels, e->levels.data(), (size_t)B * sizeof(int));
        if (e->fq) {      // CUSTOM does not quantise forces: no partials, no bounds
            zeroed(e->dev.fpart, (size_t)B * e->grid_blocks * 2 * sizeof(double));
            zeroed(e->dev.fbounds, (size_t)B * 2 * sizeof(double));
        }
    }
    if (s.modes) {
        hooks.resize(B);
        for (int b = 0; b < B; ++b) hooks[b] = mode_hook(s.modes[b]);
        uploaded(e->dev.hooks, hooks.data(), (size_t)B * sizeof(int));
    }
    if (s.sizes) {
        e->sizes_host.assign(s.sizes, s.sizes + B);
        a.items = (int)nb_plan_ragged(s.sizes, B, a.lanes, &work);
        uploaded(e->dev.work, work.data(), work.size() * sizeof(EnsWork));
        // sizes last: a handle that holds them is complete
        uploaded(e->dev.sizes, e->sizes_host.data(), (size_t)B * sizeof(int));
    }
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);       // (the uploads have consumed their host copies)
    if (he != hipSuccess) {
        release(e);
        return fail(he == hipErrorOutOfMemory ? NB_ERR_OOM : NB_ERR_HIP, "ensemble allocation failed: %s", hipGetErrorString(he));
    }
    a.pos_in = e->dev.pos.p; a.pos_out = e->dev.pos_alt.p; a.vel = e->dev.vel.p; a.acc = e->dev.acc.p; a.mass = e->dev.mass.p;
    a.prm = e->dev.prm.p;
    a.hooks = e->dev.hooks.as<int>();
    a.sizes = e->dev.sizes.as<int>(); a.work = e->dev.work.as<EnsWork>();
    a.tabs = e->dev.tabs.as<GridTables>(); a.part = e->dev.fpart.as<double>();
    *s.out = e;
    return NB_OK;
}

}  // namespace

extern "C" {

int nb_ens_create(nb_ens **out, const nb_ens_config *cfg, const double *G, const double *softening_sq, const double *dt)
{
    const CreateSpec s{out, cfg, G, softening_sq, dt};
    return create(s, [&] {
        if (cfg->mode < NB_FLOAT64 || cfg->mode > NB_FLOAT16)
            return fail(NB_ERR_UNSUPPORTED, "ensembles run the FLOAT64, FLOAT32, BFLOAT16 and FLOAT16 modes (got mode %d): the "
                                            "grid modes need per-member tables", cfg->mode);
        return (int)NB_OK;
    });
}

int nb_ens_create_grid(nb_ens **out, const nb_ens_config *cfg, const int32_t *levels, const double *G, const double *softening_sq,
                       const double *dt)
{
    CreateSpec s{out, cfg, G, softening_sq, dt};
    s.levels = levels; s.level_cap = NB_LUT_MIN; s.above_cap = "above it a solo run leaves the one-launch step";
    return create(s, [&] {
        if (cfg->mode != NB_INT8_SIM && cfg->mode != NB_INT4_SIM && cfg->mode != NB_CUSTOM)
            return fail(NB_ERR_UNSUPPORTED, "nb_ens_create_grid runs the INT8_SIM, INT4_SIM and CUSTOM modes (got mode %d): the "
                                            "other modes are nb_ens_create's", cfg->mode);
        if (cfg->mode != NB_CUSTOM && levels)
            return fail(NB_ERR_INVALID, "levels must be NULL under INT8_SIM / INT4_SIM (256 / 16 levels)");
        return (int)NB_OK;
    });
}

int nb_ens_create_grid_wide(nb_ens **out, const nb_ens_config *cfg, const int32_t *levels, const double *G,
                            const double *softening_sq, const double *dt)
{
    CreateSpec s{out, cfg, G, softening_sq, dt};
    s.levels = levels; s.level_cap = NB_MAX_LUT; s.above_cap = "finer grids are the solo engine's generic kernel's";
    return create(s, [&] {
        if (cfg->mode != NB_CUSTOM)
            return fail(NB_ERR_UNSUPPORTED, "nb_ens_create_grid_wide runs the CUSTOM mode (got mode %d): INT8_SIM / INT4_SIM are "
                                            "nb_ens_create_grid's, the other modes nb_ens_create's", cfg->mode);
        return (int)NB_OK;
    });
}

int nb_ens_create_mixed(nb_ens **out, const nb_ens_config *cfg, const int32_t *modes, const double *G,
                        const double *softening_sq, const double *dt)
{
    if (!modes) return fail(NB_ERR_INVALID, "null argument");
    CreateSpec s{out, cfg, G, softening_sq, dt};
    s.modes = modes;
    return create(s, [&] {
        if (cfg->mode != NB_FLOAT32)
            return fail(NB_ERR_UNSUPPORTED, "nb_ens_create_mixed: cfg->mode must be NB_FLOAT32, the storage mode of every cast "
                                            "mode (got mode %d)", cfg->mode);
        return (int)NB_OK;
    });
}

int nb_ens_create_ragged(nb_ens **out, const nb_ens_config *cfg, const int32_t *sizes, const int32_t *modes, const double *G,
                         const double *softening_sq, const double *dt)
{
    if (!sizes) return fail(NB_ERR_INVALID, "null argument");
    CreateSpec s{out, cfg, G, softening_sq, dt};
    s.modes = modes; s.sizes = sizes;
    return create(s, [&] {
        if (cfg->mode < NB_FLOAT64 || cfg->mode > NB_FLOAT16)
            return fail(NB_ERR_UNSUPPORTED, "nb_ens_create_ragged runs the FLOAT64, FLOAT32, BFLOAT16 and FLOAT16 modes (got mode "
                                            "%d): the ragged grid modes are a follow-up", cfg->mode);
        if (modes && cfg->mode != NB_FLOAT32)
            return fail(NB_ERR_UNSUPPORTED, "nb_ens_create_ragged: with a mode list cfg->mode must be NB_FLOAT32, the storage mode "
                                            "of every cast mode (got mode %d)", cfg->mode);
        return (int)NB_OK;
    });
}

int nb_ens_create_ragged_grid(nb_ens **out, const nb_ens_config *cfg, const int32_t *sizes, const int32_t *levels, const double *G,
                              const double *softening_sq, const double *dt)
{
    if (!sizes) return fail(NB_ERR_INVALID, "null argument");
    CreateSpec s{out, cfg, G, softening_sq, dt};
    s.levels = levels; s.level_cap = NB_LUT_MIN; s.sizes = sizes;
    s.above_cap = "the ragged wide grid is a follow-up (members of one size: nb_ens_create_grid_wide)";
    return create(s, [&] {
        if (cfg->mode != NB_INT8_SIM && cfg->mode != NB_INT4_SIM && cfg->mode != NB_CUSTOM)
            return fail(NB_ERR_UNSUPPORTED, "nb_ens_create_ragged_grid runs the INT8_SIM, INT4_SIM and CUSTOM modes (got mode "
                                            "%d): the other modes are nb_ens_create_ragged's", cfg->mode);
        if (cfg->mode != NB_CUSTOM && levels)
            return fail(NB_ERR_INVALID, "levels must be NULL under INT8_SIM / INT4_SIM (256 / 16 levels)");
        return (int)NB_OK;
    });
}

int nb_ens_ragged_plan(const int32_t *sizes, int32_t members, int32_t lanes, int32_t *work, int64_t capacity, int64_t *items)
{
    if (!sizes || !items) return fail(NB_ERR_INVALID, "null argument");
    *items = 0;
    if (members < 1 || members > NB_ENS_MAX_MEMBERS)
        return fail(NB_ERR_INVALID, "members must be in [1, %d] (got %d)", NB_ENS_MAX_MEMBERS, members);
    if (lanes != 16 && lanes != 32 && lanes != 64) return fail(NB_ERR_INVALID, "lanes must be 16, 32 or 64 (got %d)", lanes);
    for (int b = 0; b < members; ++b)
        if (sizes[b] < 1) return fail(NB_ERR_INVALID, "sizes[%d] = %d: member %d must have at least one star", b, sizes[b], b);
    std::vector<EnsWork> list;
    *items = nb_plan_ragged(sizes, members, lanes, work ? &list : nullptr);
    if (!work) return NB_OK;
    if (capacity < *items)
        return fail(NB_ERR_INVALID, "capacity of %lld work items is below the %lld of this list", (long long)capacity,
                    (long long)*items);
    for (size_t w = 0; w < list.size(); ++w) { work[2 * w] = list[w].member; work[2 * w + 1] = list[w].blk; }
    return NB_OK;
}

int nb_ens_destroy(nb_ens *e)
{
    if (!e) return NB_OK;
    DeviceGuard guard(e->cfg.device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    release(e);
    return NB_OK;
}

int nb_ens_set_params(nb_ens *e, const double *G, const double *softening_sq, const double *dt)
{
    if (!e) return fail(NB_ERR_INVALID, "null handle");
    DeviceGuard guard(e->cfg.device);
    const int B = e->cfg.members;
    if (G) e->G.assign(G, G + B);
    if (softening_sq) e->eps2.assign(softening_sq, softening_sq + B);
    if (dt) e->dt.assign(dt, dt + B);
    return upload_params(e);
}

int nb_ens_set_state(nb_ens *e, const void *pos, const void *vel, const void *mass, int dtype, int on_device)
{
    if (!e) return fail(NB_ERR_INVALID, "null handle");
    const EnsStepArgs &a = e->step;
    if (dtype != (a.is_f64 ? NB_F64 : NB_F32))
        return fail(NB_ERR_UNSUPPORTED, "ensemble state is %s under this mode (got dtype %d): mixed dtypes and the promotion "
                                        "timeline are nb_sim's", a.is_f64 ? "fp64" : "fp32", dtype);
    DeviceGuard guard(e->cfg.device);
    if (pos) { if (int rc = copy_in(e, a.pos_in, pos, cnt_nd(e), on_device)) return rc; e->have_pos = true; }
    // a ragged handle: the second buffer too -- no kernel writes the rows behind a member's own, so after a swap they would
    // hold whatever the allocation held instead of the caller's padding
    if (pos && a.sizes) if (int rc = copy_in(e, a.pos_out, pos, cnt_nd(e), on_device)) return rc;
    if (vel) { if (int rc = copy_in(e, a.vel, vel, cnt_nd(e), on_device)) return rc; e->have_vel = true; }
    if (mass) { if (int rc = copy_in(e, e->dev.mass.p, mass, cnt_n(e), on_device)) return rc; e->have_mass = true; }
    HIPCHK(hipStreamSynchronize(e->stream));      // the copies have consumed the caller's buffers
    return NB_OK;
}

int nb_ens_get_state(nb_ens *e, void *pos, void *vel, void *acc, void *mass, int on_device)
{
    if (!e) return fail(NB_ERR_INVALID, "null handle");
    const EnsStepArgs &a = e->step;
    DeviceGuard guard(e->cfg.device);
    if (pos) if (int rc = copy_out(e, pos, a.pos_in, cnt_nd(e), on_device)) return rc;
    if (vel) if (int rc = copy_out(e, vel, a.vel, cnt_nd(e), on_device)) return rc;
    if (acc) if (int rc = copy_out(e, acc, a.acc, cnt_nd(e), on_device)) return rc;
    if (mass) if (int rc = copy_out(e, mass, a.mass, cnt_n(e), on_device)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return NB_OK;
}

int nb_ens_set_accelerations(nb_ens *e, const void *acc, int dtype, int on_device)
{
    if (!e || !acc) return fail(NB_ERR_INVALID, "null argument");
    const bool f64 = e->step.is_f64;
    if (dtype != (f64 ? NB_F64 : NB_F32)) return fail(NB_ERR_UNSUPPORTED, "acceleration dtype %d on %s state", dtype, f64 ? "fp64" : "fp32");
    DeviceGuard guard(e->cfg.device);
    if (int rc = copy_in(e, e->step.acc, acc, cnt_nd(e), on_device)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    e->have_acc = true;
    return NB_OK;
}

int nb_ens_compute_accelerations(nb_ens *e)
{
    if (!e) return fail(NB_ERR_INVALID, "null handle");
    if (!e->have_pos || !e->have_mass) return fail(NB_ERR_INVALID, "positions/masses not set");
    DeviceGuard guard(e->cfg.device);
    if (int rc = launch_force(e, NB_KICK_NONE)) return rc;
    e->have_acc = true;
    return NB_OK;
}

// `nsteps` leapfrog ticks of every member: run_train without samples
int nb_ens_step(nb_ens *e, int32_t nsteps)
{
    if (int rc = check_steppable(e)) return rc;
    if (nsteps < 1) return NB_OK;
    DeviceGuard guard(e->cfg.device);
    return run_train(e, nsteps, 0, nullptr, WATCH_NONE, 0u);
}

int nb_ens_energy(nb_ens *e, double *kinetic, double *potential)
{
    if (!e) return fail(NB_ERR_INVALID, "null handle");
    if (!kinetic && !potential) return NB_OK;
    if (!e->have_mass || (kinetic && !e->have_vel) || (potential && !e->have_pos)) return fail(NB_ERR_INVALID, "state incomplete");
    DeviceGuard guard(e->cfg.device);
    const nb_ens_config &c = e->cfg;
    const EnsStepArgs &a = e->step;
    if (a.sizes) {
        // the probe has the capacity's shape, not the member's: a ragged member's energies are the batched kernels', which
        // give it the values of a handle of its own size (nb_ens_energy.hip)
        if (!e->have_pos) return fail(NB_ERR_INVALID, "state incomplete");
        return batched_energies(e, kinetic, potential, 0);
    }
    if (!e->probe) {
        nb_config pc{};
        pc.n = c.n; pc.dim = c.dim; pc.mode = c.mode; pc.G = e->G[0]; pc.softening_sq = e->eps2[0]; pc.dt = e->dt[0];
        pc.device = c.device; pc.rank = 0; pc.nranks = 1; pc.flags = 0;
        if (int rc = nb_create(&e->probe, &pc)) return rc;
    }
    HIPCHK(hipStreamSynchronize(e->stream));         // the probe reads the members' slices on a stream of its own
    const int dtype = a.is_f64 ? NB_F64 : NB_F32;
    const size_t nd_b = (size_t)c.n * c.dim * el(e), n_b = (size_t)c.n * el(e);
    for (int b = 0; b < c.members; ++b) {
        if (int rc = nb_set_params(e->probe, e->G[b], e->eps2[b], e->dt[b])) return rc;
        if (int rc = nb_set_state(e->probe, (const char *)a.pos_in + b * nd_b, (const char *)a.vel + b * nd_b,
                                  (const char *)a.mass + b * n_b, dtype, 1))
            return rc;
        if (int rc = nb_energy(e->probe, kinetic ? kinetic + b : nullptr, potential ? potential + b : nullptr)) return rc;
    }
    return NB_OK;
}

int nb_ens_energies(nb_ens *e, double *kinetic, double *potential, int on_device)
{
    if (!e) return fail(NB_ERR_INVALID, "null handle");
    if (!kinetic && !potential) return NB_OK;
    if (!e->have_mass || !e->have_pos || (kinetic && !e->have_vel)) return fail(NB_ERR_INVALID, "state incomplete");
    DeviceGuard guard(e->cfg.device);
    return batched_energies(e, kinetic, potential, on_device);
}

// run_sampled with the energies in every sample and no stop array
int nb_ens_run_recorded(nb_ens *e, int32_t nsteps, int32_t every, double *kinetic, double *potential, int64_t capacity,
                        int on_device, int32_t *samples)
{
    if (samples) *samples = 0;
    if (int rc = check_steppable(e)) return rc;
    if (nsteps < 0) return fail(NB_ERR_INVALID, "nsteps must be >= 0 (got %d)", nsteps);
    if (every < 1) return fail(NB_ERR_INVALID, "every must be >= 1 (got %d)", every);
    SampledRun r;
    r.nmax = nsteps; r.every = every; r.what = SAMPLE_ENERGIES;
    r.kinetic = kinetic; r.potential = potential; r.capacity = capacity; r.on_device = on_device; r.samples = samples;
    return run_sampled(e, r);
}

// run_sampled with the members' budgets as their stop ticks (and the watch lowering them)
int nb_ens_run_members(nb_ens *e, const int32_t *nsteps, int32_t every, int32_t watch, double *kinetic, double *potential,
                       int64_t capacity, int on_device, int32_t *samples, int32_t *stop_tick, int32_t *reason)
{
    if (samples) *samples = 0;
    if (int rc = check_steppable(e)) return rc;
    SampledRun r;
    if (int rc = check_budgets(e, nsteps, &r.nmax)) return rc;
    if (every < 0) return fail(NB_ERR_INVALID, "every must be >= 0 (got %d)", every);
    if (watch != 0 && watch != 1) return fail(NB_ERR_INVALID, "watch must be 0 or 1 (got %d)", watch);
    if (watch && every < 1) return fail(NB_ERR_INVALID, "the watch tests sampled ticks: it needs every >= 1");
    r.every = every; r.watch = watch ? WATCH_EXPLOSION : WATCH_NONE; r.what = every ? SAMPLE_ENERGIES : 0u;
    r.budgets = nsteps; r.stop_tick = stop_tick; r.why = reason;
    r.kinetic = kinetic; r.potential = potential; r.capacity = capacity; r.on_device = on_device; r.samples = samples;
    return run_sampled(e, r);
}

// the detector's kernel alone on the resident state: one launch, one copy-out, one wait
int nb_ens_crash_measures(nb_ens *e, const void *prev_pos, int on_device, int32_t *flags, double *measures)
{
    if (!e) return fail(NB_ERR_INVALID, "null handle");
    if (int rc = refuse_ragged(e, "nb_ens_crash_measures", "the ragged crash watch")) return rc;
    if (!e->have_pos || !e->have_vel) return fail(NB_ERR_INVALID, "state incomplete");
    DeviceGuard guard(e->cfg.device);
    const EnsStepArgs &a = e->step;
    if (int rc = crash_buffers(e)) return rc;
    const void *prev = prev_pos;
    if (prev_pos && !on_device) {          // (the wait below: the upload has consumed prev_pos)
        if (int rc = copy_in(e, e->dev.prev_pos.p, prev_pos, cnt_nd(e), 0)) return rc;
        prev = e->dev.prev_pos.p;
    }
    HIPCHK(nb_launch_ens_crash(a.pos_in, const_cast<void *>(prev), a.vel, a.members, a.n, a.dim, a.is_f64, nullptr, nullptr,
                               nullptr, 0, 0, nullptr, nullptr, crash_flags(e), e->dev.crash_out.as<double>(), e->stream));
    if (int rc = crash_out_async(e)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    crash_results(e, flags, measures);
    return NB_OK;
}

// nb_ens_run_members with every tick sampled and the crash-point detector as the watch
int nb_ens_run_crash_watched(nb_ens *e, const int32_t *nsteps, double *kinetic, double *potential, int64_t capacity,
                             int on_device, int32_t *samples, int32_t *stop_tick, int32_t *kind, int32_t *flags, double *measures)
{
    if (samples) *samples = 0;
    if (int rc = check_steppable(e)) return rc;
    if (int rc = refuse_ragged(e, "nb_ens_run_crash_watched", "the ragged crash watch")) return rc;
    SampledRun r;
    if (int rc = check_budgets(e, nsteps, &r.nmax)) return rc;
    r.every = 1; r.watch = WATCH_CRASH; r.what = SAMPLE_ENERGIES;
    r.budgets = nsteps; r.stop_tick = stop_tick; r.why = kind; r.flags = flags; r.measures = measures;
    r.kinetic = kinetic; r.potential = potential; r.capacity = capacity; r.on_device = on_device; r.samples = samples;
    return run_sampled(e, r);
}

// the divergence kernel alone on the resident state: one launch, one copy-out, one wait
int nb_ens_divergence(nb_ens *e, const int32_t *baseline, double *max_pos, double *mean_pos, double *max_vel, int on_device)
{
    if (!e) return fail(NB_ERR_INVALID, "null handle");
    if (!e->have_pos || !e->have_vel) return fail(NB_ERR_INVALID, "state incomplete");
    DeviceGuard guard(e->cfg.device);
    if (int rc = divergence_buffers(e, 1)) return rc;
    if (int rc = upload_baselines(e, baseline)) return rc;
    if (int rc = launch_divergence(e, 0)) return rc;
    if (int rc = history_out(e, e->dhist, 1, {max_pos, mean_pos, max_vel}, on_device)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return NB_OK;
}

// run_sampled with the divergence (and, asked for, the energies) in every sample and no stop array
int nb_ens_run_diverged(nb_ens *e, int32_t nsteps, int32_t every, const int32_t *baseline, int32_t with_energies,
                        double *max_pos, double *mean_pos, double *max_vel, double *kinetic, double *potential, int64_t capacity,
                        int on_device, int32_t *samples)
{
    if (samples) *samples = 0;
    if (int rc = check_steppable(e)) return rc;
    if (nsteps < 0) return fail(NB_ERR_INVALID, "nsteps must be >= 0 (got %d)", nsteps);
    if (every < 1) return fail(NB_ERR_INVALID, "every must be >= 1 (got %d)", every);
    SampledRun r;
    r.nmax = nsteps; r.every = every; r.what = SAMPLE_DIVERGENCE | (with_energies ? SAMPLE_ENERGIES : 0u);
    r.baseline = baseline; r.max_pos = max_pos; r.mean_pos = mean_pos; r.max_vel = max_vel;
    r.kinetic = kinetic; r.potential = potential; r.capacity = capacity; r.on_device = on_device; r.samples = samples;
    return run_sampled(e, r);
}

// the diagnostics of every member from the resident state: one launch, two copies, one wait
int nb_ens_metrics(nb_ens *e, int32_t num_bins, const double *max_radius, double percentile, double *curve_mean,
                   int64_t *curve_count, float *edges, double *scalars)
{
    if (!e) return fail(NB_ERR_INVALID, "null handle");
    if (int rc = refuse_ragged(e, "nb_ens_metrics", "ragged metrics")) return rc;
    if (!e->have_pos || !e->have_vel || !e->have_mass) return fail(NB_ERR_INVALID, "state incomplete");
    if (num_bins < 0 || num_bins > 255) return fail(NB_ERR_INVALID, "num_bins must be in [0, 255] (got %d)", num_bins);
    if (percentile != percentile) return fail(NB_ERR_INVALID, "percentile is NaN");
    const nb_ens_config &c = e->cfg;
    const size_t B = (size_t)c.members, nb = (size_t)num_bins;
    for (size_t b = 0; max_radius && b < B; ++b)
        if (max_radius[b] < 0.0)
            return fail(NB_ERR_INVALID, "max_radius[%d] = %g is negative (pass NULL for every member's own maximum radius)",
                        (int)b, max_radius[b]);
    DeviceGuard guard(c.device);
    const bool f64 = e->step.is_f64;
    HIPCHK(e->dev.mscratch.reserve(nb_ens_metrics_scratch_bytes(c.members, c.n, f64)));
    HIPCHK(e->dev.mradius.reserve(B * sizeof(double)));
    HIPCHK(e->dev.mout.reserve(B * (5 + 2 * nb) * sizeof(double)));
    HIPCHK(e->dev.medges.reserve(B * (nb + 1) * sizeof(float)));
    if (max_radius) HIPCHK(hipMemcpyAsync(e->dev.mradius.p, max_radius, B * sizeof(double), hipMemcpyHostToDevice, e->stream));
    NbEnsMetricsArgs a{};
    a.pos = e->step.pos_in; a.vel = e->step.vel; a.mass = e->step.mass;
    a.members = c.members; a.n = c.n; a.dim = c.dim; a.is_f64 = f64;
    a.prm = e->step.prm;
    a.max_radius = max_radius ? e->dev.mradius.as<double>() : nullptr;
    a.num_bins = num_bins;
    const long long k = (long long)((double)c.n * percentile / 100.0);     // int(len(radii) * percentile / 100), as nb_metrics
    a.kth = (int)std::min<long long>(std::max<long long>(k, 0), c.n - 1);
    a.scratch = e->dev.mscratch.p;
    a.out = e->dev.mout.as<double>();
    a.edges_out = e->dev.medges.as<float>();
    HIPCHK(nb_launch_ens_metrics(a, e->stream));
    const size_t per = 5 + 2 * nb;
    std::vector<double> host(B * per);
    HIPCHK(hipMemcpyAsync(host.data(), a.out, host.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (edges && nb > 0)
        HIPCHK(hipMemcpyAsync(edges, a.edges_out, B * (nb + 1) * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));         // (also: the upload has consumed max_radius)
    for (size_t b = 0; b < B; ++b) {
        const double *h = host.data() + b * per;
        if (scalars) {
            double *o = scalars + b * 5;
            o[0] = h[0];
            o[1] = h[1];
            o[2] = (double)((float)h[2] / (float)c.n);       // bound_mask.float().mean(), as nb_metrics forms it
            o[3] = h[3];
            o[4] = h[4];
        }
        for (size_t q = 0; q < nb; ++q) {
            if (curve_mean) curve_mean[b * nb + q] = h[5 + q];
            if (curve_count) curve_count[b * nb + q] = (int64_t)h[5 + nb + q];
        }
    }
    return NB_OK;
}

int nb_ens_info(nb_ens *e, int32_t *members, int64_t *force_launches, const char **kernel_name)
{
    if (!e) return fail(NB_ERR_INVALID, "null handle");
    if (members) *members = e->cfg.members;
    if (force_launches) *force_launches = e->force_launches;
    if (kernel_name) *kernel_name = e->last_kernel;
    return NB_OK;
}

int nb_ens_quant_info(nb_ens *e, double *out)
{
    if (!e || !out) return fail(NB_ERR_INVALID, "null argument");
    if (!e->grid) {        // (a ragged GRID handle -- nb_ens_create_ragged_grid -- is served; a ragged cast handle says why not)
        if (int rc = refuse_ragged(e, "nb_ens_quant_info", "the ragged grid modes")) return rc;
        return fail(NB_ERR_UNSUPPORTED, "quant info is only defined for the grid modes (nb_ens_create_grid)");
    }
    DeviceGuard guard(e->cfg.device);
    const size_t B = (size_t)e->cfg.members;
    // the scalars behind the tables of every member, not the 48 KB of tables in front of them
    constexpr size_t off = offsetof(GridTables, lmin), width = sizeof(GridTables) - off;
    std::vector<char> tail(B * width);
    std::vector<double> fb(B * 2, __builtin_nan(""));
    HIPCHK(hipMemcpy2DAsync(tail.data(), width, e->dev.tabs.as<char>() + off, sizeof(GridTables), width, B, hipMemcpyDeviceToHost,
                            e->stream));
    if (e->fq) HIPCHK(hipMemcpyAsync(fb.data(), e->dev.fbounds.p, B * 2 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (size_t b = 0; b < B; ++b) {
        GridTables h;                      // only the members from lmin on are filled in and read
        memcpy((char *)&h + off, tail.data() + b * width, width);
        double *o = out + b * 8;
        o[0] = h.lmin; o[1] = h.lmax; o[2] = fb[2 * b]; o[3] = fb[2 * b + 1]; o[4] = h.r2max;
        o[5] = h.fast_ok; o[6] = h.fast_maxdev; o[7] = h.fast_maxrel;
    }
    return NB_OK;
}

// the evaluation once more on the current positions with the BINS instantiation of the pair sweep this handle runs:
// tables (the same values: a function of the positions), then the sweep with the forces into bin_acc and no kick
int nb_ens_quant_bin_sums(nb_ens *e, int64_t *sum_k, int64_t *sum_kw, int64_t *pairs)
{
    if (!e) return fail(NB_ERR_INVALID, "null handle");
    if (!e->grid) {
        if (int rc = refuse_ragged(e, "nb_ens_quant_bin_sums", "the ragged grid modes")) return rc;
        return fail(NB_ERR_UNSUPPORTED, "the quant-bin read-out is only defined for the grid modes (nb_ens_create_grid, "
                                        "nb_ens_create_grid_wide)");
    }
    if (!e->have_pos || !e->have_mass) return fail(NB_ERR_INVALID, "positions/masses not set");
    DeviceGuard guard(e->cfg.device);
    const EnsStepArgs &a = e->step;
    const size_t B = (size_t)a.members, n = (size_t)a.n, per = 2 * n + 2, bytes = B * per * sizeof(unsigned long long);
    HIPCHK(e->dev.bin_acc.reserve(cnt_nd(e) * sizeof(float)));
    HIPCHK(e->dev.bin_out.reserve(bytes));
    unsigned long long *bin_out = e->dev.bin_out.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(bin_out, 0, bytes, e->stream));
    if (int rc = launch_tables(e, nullptr, 0)) return rc;
    if (a.sizes)
        HIPCHK(nb_launch_ens_grid_bins_ragged(a, e->dev.bin_acc.as<float>(), bin_out, e->stream));
    else
        HIPCHK(nb_launch_ens_grid_bins((const float *)a.pos_in, e->dev.bin_acc.as<float>(), (const float *)a.mass, a.members, a.n,
                                       a.dim, a.prm, a.lanes, a.tabs, a.max_levels, bin_out, e->stream));
    std::vector<unsigned long long> host(B * per);
    HIPCHK(hipMemcpyAsync(host.data(), bin_out, bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (size_t b = 0; b < B; ++b) {
        // a ragged member's block is packed for its own size nb; of its rows of the (members, n) outputs only the first nb
        // entries are written
        const unsigned long long *h = host.data() + b * per;
        const size_t nb = a.sizes ? (size_t)e->sizes_host[b] : n;
        for (size_t i = 0; i < nb; ++i) {
            if (sum_k) sum_k[b * n + i] = (int64_t)h[i];
            if (sum_kw) sum_kw[b * n + i] = (int64_t)h[nb + i];
        }
        if (pairs) { pairs[2 * b] = (int64_t)h[2 * nb]; pairs[2 * b + 1] = (int64_t)h[2 * nb + 1]; }
    }
    return NB_OK;
}

int nb_ens_synchronize(nb_ens *e)
{
    if (!e) return fail(NB_ERR_INVALID, "null handle");
    DeviceGuard guard(e->cfg.device);
    HIPCHK(hipStreamSynchronize(e->stream));
    return NB_OK;
}

}  // extern "C"
