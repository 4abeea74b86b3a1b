// nb_ens_api.cpp -- nb_ens handles (include/nbody_amd.h): B independent systems of the same shape, precision mode and
// state dtype, each with its own G / softening / dt, advanced together -- ONE force launch per tick (nb_ensemble.hip) where
// a loop of solo handles issues B.  Host orchestration only, as in nb_api.cpp / nb_step.cpp.
//
// Layout: contiguous (B, N, D) positions (two buffers: they ping-pong as in the solo step), velocities, accelerations and
// (B, N) masses in the storage type (fp64 under FLOAT64, else fp32), and a device array of one EnsScalars record per
// member, cast on the host exactly as the solo launch casts them.  Nothing here is indexed by anything but the member.
//
// Grid modes (nb_ens_create_grid: INT8_SIM / INT4_SIM / CUSTOM, fp32 state) add, beside these: one GridTables and one level
// count per member, and under INT8 / INT4 the force launch's per-workgroup {min, max} partials and a (B, 2) array of force
// bounds.  An evaluation is then step_small's sequence (nb_step.cpp) batched: max r2 + tables, the grid step, and under
// INT8 / INT4 the finish launch that snaps the forces and carries the kicks IN PLACE (no ping-pong of the positions).
// nb_ens_create_grid_wide (CUSTOM, up to NB_MAX_LUT levels per member) is the same handle; once a member exceeds NB_LUT_MIN
// levels, a second tables launch builds those members' multi-chunk tables and the pair sweep is the wide kernel (tables in
// dynamic LDS) -- still one force launch per tick.  nb_ens_quant_bin_sums runs the evaluation once more with the BINS
// instantiation of the pair sweep in use, forces into a scratch buffer: an observer.
//
// Energies are off the hot path and must equal a solo handle's bit for bit, whichever kernel variant the solo engine
// picks for this shape and these masses: each member's slice is handed (device to device) to one solo handle of the same
// shape kept for that purpose, and nb_energy runs there.  nb_ens_energies and nb_ens_run_recorded evaluate all members at
// once instead (nb_ens_energy.hip: two launches on the handle's stream, values at the project's bars rather than the
// solo engine's bits), the latter between the ticks of a run into a history that is copied out once at the end.
//
// nb_ens_step issues ONE launch train (run_train) and returns; nb_ens_run_recorded, nb_ens_run_members and
// nb_ens_run_crash_watched are argument checks in front of run_sampled: the same train with samples, the members' stop
// ticks in a device array that every kernel of the tick path reads (nb_device.h) and a watch kernel lowers on the device
// (nb_ens_watch.hip, nb_ens_crash.hip), and one wait.  The step and run_recorded pass no array: no member ever stops, and
// the kernels launched are the instantiations without stops.  nb_ens_crash_measures is the detector's kernel alone.
//
// nb_ens_create_mixed: fp32 state, every member with its own cast mode (FLOAT32 / BFLOAT16 / FLOAT16) -- the handle keeps
// the members' hooks on the device and launch_force launches ens_step_mixed_kernel, which reads them; everything else is
// the FLOAT32 handle's.  nb_ens_divergence / nb_ens_run_diverged compare every member with another member of the handle on
// the device (nb_ens_diverge.hip): the kernel alone, or as part of run_train's samples.
//
// nb_ens_create_ragged: members of different sizes.  cfg.n is the capacity, member b owns the first sizes[b] rows of its
// slice and no kernel touches the rest; launch_force launches ens_step_ragged_kernel over the work list built at creation
// (nb_plan_ragged), and every other launch of the tick path gets `sizes` (null on every other handle: the instantiations
// without sizes).  The solo probe has the capacity's shape, so nb_ens_energy returns the batched values there; the entries
// whose kernels are one workgroup per member of one shape, and the grid modes', refuse such a handle (refuse_ragged).
#include <algorithm>
#include <cstddef>
#include <cstring>

#include "nb_state.h"

using namespace nbhost;

struct nb_ens {
    nb_ens_config cfg{};
    hipStream_t stream = nullptr;
    bool is_f64 = false;
    int hook = HOOK_NONE, lanes = 64;
    std::vector<double> G, eps2, dt;          // per member, as given
    std::vector<char> prm_host;               // what the device array holds (or is about to)
    void *prm = nullptr;                      // device: one EnsScalars of the storage type per member
    void *pos = nullptr, *pos_alt = nullptr, *vel = nullptr, *acc = nullptr, *mass = nullptr;
    bool have_pos = false, have_vel = false, have_mass = false, have_acc = false;
    int64_t force_launches = 0;               // batched force launches since creation (kick + drift launches not counted)
    const char *last_kernel = "none";
    nb_sim *probe = nullptr;                  // solo handle of the members' shape: energies (created on first use)
    double *epart = nullptr;                  // batched energies: members * tile pairs * {pe, ke} slots (created on first use)
    double *ehist = nullptr;                  // batched energies: ehist_cap samples of kinetic, then as many of potential
    int64_t ehist_cap = 0;
    // batched diagnostics (nb_ens_metrics; created on first use, sized for mbins_cap bins)
    void *mscratch = nullptr;                 // vt, |v| and bin of every star of every member
    double *mout = nullptr, *mradius = nullptr;   // members * (5 + 2 mbins_cap) results; members given max_radius
    float *medges = nullptr;                  // members * (mbins_cap + 1) edges
    int mbins_cap = -1;
    // grid modes only (nb_ens_create_grid)
    bool grid = false, fq = false;            // HOOK_GRID; INT8 / INT4: forces snapped (and kicks applied) by the finish launch
    int allow_fast = 1;                       // the table-free pair path may be used (NB_NO_GRID_FAST unset), as nb_sim reads it
    int grid_blocks = 0;                      // workgroups per member of the grid step: min / max partials per member
    std::vector<int32_t> levels;              // per member
    GridTables *tabs = nullptr;               // device: one per member (max r2, arrival counter, the evaluation's tables)
    int *levels_dev = nullptr;
    double *fpart = nullptr, *fbounds = nullptr;   // INT8 / INT4: members * grid_blocks * 2 partials; members * {fmin, fmax}
    int max_levels = 0;                       // the largest of `levels`: above NB_LUT_MIN the tick runs the wide kernels
    // nb_ens_quant_bin_sums (created on first use): the read-out's forces; members * (2 n + 2) checksum / counter words
    float *bin_acc = nullptr;
    unsigned long long *bin_out = nullptr;
    // nb_ens_run_members (created on first use): members stop ticks, then members halt reasons; what is uploaded / read back
    int32_t *stops = nullptr;
    std::vector<int32_t> stops_host;
    // crash-point detector (created on first use): the positions of the previous tick; the members' dt as given; members * 4
    // measures, then members flags; what is read back of the last
    void *prev_pos = nullptr;
    double *dt_dev = nullptr, *crash_out = nullptr;
    std::vector<double> crash_host;
    // members of different cast modes (nb_ens_create_mixed): the hook of every member, as given and on the device
    bool mixed = false;
    std::vector<int> hooks_host;
    int *hooks = nullptr;
    // divergence between members (created on first use): the members' baselines, as uploaded and on the device; dhist_cap
    // samples of max |d position|, then as many of mean |d position|, then of max |d velocity|
    std::vector<int32_t> base_host;
    int *base_dev = nullptr;
    double *dhist = nullptr;
    int64_t dhist_cap = 0;
    // members of different sizes (nb_ens_create_ragged): cfg.n is the capacity; every member's size, as given and on the
    // device (null on every other handle: the kernels without sizes run); the work list of the step, built once
    std::vector<int32_t> sizes_host;
    int *sizes = nullptr;
    EnsWork *work = nullptr;
    int work_items = 0;
};

namespace {

// what run_train launches behind the energy launches of a sampled tick
enum WatchMode { WATCH_NONE, WATCH_EXPLOSION, WATCH_CRASH };
// what a sample of run_train holds (a bit set; 0: the run takes no samples)
enum SampleBits { SAMPLE_ENERGIES = 1, SAMPLE_DIVERGENCE = 2 };

inline size_t el(const nb_ens *e) { return e->is_f64 ? 8 : 4; }
inline size_t cnt_nd(const nb_ens *e) { return (size_t)e->cfg.members * e->cfg.n * e->cfg.dim; }
inline size_t cnt_n(const nb_ens *e) { return (size_t)e->cfg.members * e->cfg.n; }

// one EnsScalars<T> per member with the casts of nb_launch_small_step / launch_s: (T)G, (T)eps2, (T)(dt / 2), (T)dt
template <typename T>
void fill_params(nb_ens *e)
{
    for (size_t b = 0; b < e->G.size(); ++b) {
        const EnsScalars<T> p = {(T)e->G[b], (T)e->eps2[b], (T)(e->dt[b] / 2), (T)e->dt[b]};
        memcpy(e->prm_host.data() + b * sizeof p, &p, sizeof p);
    }
}

int upload_params(nb_ens *e)
{
    if (e->is_f64) fill_params<double>(e);
    else fill_params<float>(e);
    // on the handle's stream, behind the launches that still read the old values; the wait keeps prm_host free to rewrite
    HIPCHK(hipMemcpyAsync(e->prm, e->prm_host.data(), e->prm_host.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return NB_OK;
}

// the tables of one evaluation of a grid-mode ensemble: max r2 of every member and its single-block tables in one launch;
// members above NB_LUT_MIN levels get theirs from a second one (neither is counted by force_launches)
int launch_tables(nb_ens *e, const int *stop, int t)
{
    const nb_ens_config &c = e->cfg;
    HIPCHK(nb_launch_ens_r2max_tables((const float *)e->pos, c.members, c.n, c.dim, e->prm, e->tabs, e->levels_dev, 0.01f,
                                      e->allow_fast, stop, t, e->stream));
    if (e->max_levels > NB_LUT_MIN)
        HIPCHK(nb_launch_ens_tables_wide(c.members, e->max_levels, e->prm, e->tabs, e->levels_dev, 0.01f, e->allow_fast, stop, t,
                                         e->stream));
    return NB_OK;
}

// one evaluation of a grid-mode ensemble, as step_small issues a solo one (stop / t: nb_internal.h)
int launch_force_grid(nb_ens *e, int do_kick, const int *stop, int t)
{
    const nb_ens_config &c = e->cfg;
    if (int rc = launch_tables(e, stop, t)) return rc;
    if (e->max_levels > NB_LUT_MIN) {        // (CUSTOM only: no force bounds, no finish launch)
        HIPCHK(nb_launch_ens_grid_step_wide((const float *)e->pos, (float *)e->pos_alt, (float *)e->vel, (float *)e->acc,
                                            (const float *)e->mass, c.members, c.n, c.dim, e->prm, do_kick, e->lanes, e->tabs,
                                            e->max_levels, stop, t, e->stream));
        e->force_launches++;
        e->last_kernel = "ens_grid_step_wide_kernel";
        return NB_OK;
    }
    HIPCHK(nb_launch_ens_grid_step((const float *)e->pos, (float *)e->pos_alt, (float *)e->vel, (float *)e->acc,
                                   (const float *)e->mass, c.members, c.n, c.dim, e->prm, e->fq ? NB_KICK_NONE : do_kick, e->lanes,
                                   e->tabs, e->fq ? e->fpart : nullptr, stop, t, e->stream));
    if (e->fq)      // levels[0]: under INT8 / INT4 every member has the mode's 256 / 16 levels
        HIPCHK(nb_launch_ens_force_quant_finish((float *)e->acc, c.members, c.n * c.dim, e->levels[0], e->fpart, e->grid_blocks,
                                                e->fbounds, (float *)e->vel, (float *)e->pos, e->prm, do_kick, stop, t,
                                                e->stream));
    e->force_launches++;
    e->last_kernel = "ens_grid_step_kernel";
    return NB_OK;
}

// a NB_KICK_CLOSE_OPEN evaluation left the drifted positions in pos_alt (else in place: INT8 / INT4)
inline void advance_positions(nb_ens *e)
{
    if (!e->fq) std::swap(e->pos, e->pos_alt);
}

int launch_force(nb_ens *e, int do_kick, const int *stop = nullptr, int t = 0)
{
    const nb_ens_config &c = e->cfg;
    if (e->grid) return launch_force_grid(e, do_kick, stop, t);
    if (e->sizes) {
        HIPCHK(nb_launch_ens_step_ragged(e->pos, e->pos_alt, e->vel, e->acc, e->mass, c.members, c.n, c.dim, e->is_f64,
                                         e->mixed ? HOOK_AT_RUN_TIME : e->hook, e->prm, do_kick, e->lanes, e->sizes, e->work,
                                         e->work_items, e->hooks, stop, t, e->stream));
        e->force_launches++;
        e->last_kernel = "ens_step_ragged_kernel";
        return NB_OK;
    }
    if (e->mixed) {
        HIPCHK(nb_launch_ens_step_mixed((const float *)e->pos, (float *)e->pos_alt, (float *)e->vel, (float *)e->acc,
                                        (const float *)e->mass, c.members, c.n, c.dim, e->prm, do_kick, e->lanes, e->hooks, stop,
                                        t, e->stream));
        e->force_launches++;
        e->last_kernel = "ens_step_mixed_kernel";
        return NB_OK;
    }
    HIPCHK(nb_launch_ens_step(e->pos, e->pos_alt, e->vel, e->acc, e->mass, c.members, c.n, c.dim, e->is_f64, e->hook, e->prm,
                              do_kick, e->lanes, stop, t, e->stream));
    e->force_launches++;
    e->last_kernel = "ens_step_kernel";
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

void release(nb_ens *e)
{
    if (e->probe) (void)nb_destroy(e->probe);
    for (void *p : {e->prm, e->pos, e->pos_alt, e->vel, e->acc, e->mass, (void *)e->epart, (void *)e->ehist, (void *)e->tabs,
                    (void *)e->levels_dev, (void *)e->fpart, (void *)e->fbounds, e->mscratch, (void *)e->mout, (void *)e->mradius,
                    (void *)e->medges, (void *)e->stops, e->prev_pos, (void *)e->dt_dev, (void *)e->crash_out, (void *)e->hooks,
                    (void *)e->base_dev, (void *)e->dhist, (void *)e->bin_acc, (void *)e->bin_out, (void *)e->sizes, (void *)e->work})
        if (p) (void)hipFree(p);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

// room for `samples` samples of the batched energies (buffers grow, never shrink)
int energy_buffers(nb_ens *e, int64_t samples)
{
    const size_t B = (size_t)e->cfg.members;
    if (!e->epart) HIPCHK(hipMalloc((void **)&e->epart, B * nb_ens_energy_pairs(e->cfg.n) * 2 * sizeof(double)));
    if (samples > e->ehist_cap) {
        // no launch reads the old history: every call that fills it copies it out and waits before it returns
        if (e->ehist) { (void)hipFree(e->ehist); e->ehist = nullptr; e->ehist_cap = 0; }
        hipError_t he = hipMalloc((void **)&e->ehist, (size_t)samples * B * 2 * sizeof(double));
        if (he != hipSuccess)
            return fail(he == hipErrorOutOfMemory ? NB_ERR_OOM : NB_ERR_HIP, "energy history of %lld samples: %s",
                        (long long)samples, hipGetErrorString(he));
        e->ehist_cap = samples;
    }
    return NB_OK;
}

// room for `samples` samples of the divergence (buffers grow, never shrink) and for the baselines
int divergence_buffers(nb_ens *e, int64_t samples)
{
    const size_t B = (size_t)e->cfg.members;
    if (!e->base_dev) HIPCHK(hipMalloc((void **)&e->base_dev, B * sizeof(int)));
    if (samples > e->dhist_cap) {
        // no launch reads the old history: every call that fills it copies it out and waits before it returns
        if (e->dhist) { (void)hipFree(e->dhist); e->dhist = nullptr; e->dhist_cap = 0; }
        hipError_t he = hipMalloc((void **)&e->dhist, (size_t)samples * B * 3 * sizeof(double));
        if (he != hipSuccess)
            return fail(he == hipErrorOutOfMemory ? NB_ERR_OOM : NB_ERR_HIP, "divergence history of %lld samples: %s",
                        (long long)samples, hipGetErrorString(he));
        e->dhist_cap = samples;
    }
    return NB_OK;
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
    for (int b = 0; e->sizes && b < B; ++b)
        if (e->sizes_host[baseline[b]] != e->sizes_host[b])
            return fail(NB_ERR_INVALID, "baseline[%d] = %d: member %d has %d stars and member %d has %d; a member is compared "
                                        "with a member of its own size", b, baseline[b], b, e->sizes_host[b], baseline[b],
                        e->sizes_host[baseline[b]]);
    e->base_host.assign(baseline, baseline + B);
    static_assert(sizeof(int32_t) == sizeof(int), "the kernel reads ints");
    HIPCHK(hipMemcpyAsync(e->base_dev, e->base_host.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, e->stream));
    return NB_OK;
}

// sample `s` of the divergence history: the resident state, one launch behind whatever the stream holds
int launch_divergence(nb_ens *e, int64_t s)
{
    const nb_ens_config &c = e->cfg;
    const size_t plane = (size_t)e->dhist_cap * c.members;
    HIPCHK(nb_launch_ens_divergence(e->pos, e->vel, c.members, c.n, c.dim, e->is_f64, e->base_dev, s, e->dhist,
                                    e->dhist + plane, e->dhist + 2 * plane, e->stream, e->sizes));
    return NB_OK;
}

// the first `samples` samples of the divergence history to the caller's arrays (any may be null); does not wait
int divergence_out(nb_ens *e, int64_t samples, double *max_pos, double *mean_pos, double *max_vel, int on_device)
{
    const size_t bytes = (size_t)samples * e->cfg.members * sizeof(double), plane = (size_t)e->dhist_cap * e->cfg.members;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (max_pos && bytes) HIPCHK(hipMemcpyAsync(max_pos, e->dhist, bytes, kind, e->stream));
    if (mean_pos && bytes) HIPCHK(hipMemcpyAsync(mean_pos, e->dhist + plane, bytes, kind, e->stream));
    if (max_vel && bytes) HIPCHK(hipMemcpyAsync(max_vel, e->dhist + 2 * plane, bytes, kind, e->stream));
    return NB_OK;
}

// the crash-point detector's buffers (fixed sizes: created once)
int crash_buffers(nb_ens *e)
{
    const size_t B = (size_t)e->cfg.members;
    if (!e->prev_pos) HIPCHK(hipMalloc(&e->prev_pos, cnt_nd(e) * el(e)));
    if (!e->dt_dev) HIPCHK(hipMalloc((void **)&e->dt_dev, B * sizeof(double)));
    if (!e->crash_out) HIPCHK(hipMalloc((void **)&e->crash_out, B * (4 * sizeof(double) + sizeof(int32_t))));
    return NB_OK;
}

inline int *crash_flags(nb_ens *e) { return (int *)(e->crash_out + 4 * (size_t)e->cfg.members); }

// flags and measures to the host copy (the caller waits, then hands them on with crash_results)
int crash_out_async(nb_ens *e)
{
    const size_t B = (size_t)e->cfg.members;
    e->crash_host.resize(4 * B + (B + 1) / 2);          // the int32 flags ride behind the doubles
    HIPCHK(hipMemcpyAsync(e->crash_host.data(), e->crash_out, B * (4 * sizeof(double) + sizeof(int32_t)), hipMemcpyDeviceToHost,
                          e->stream));
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
    const nb_ens_config &c = e->cfg;
    HIPCHK(nb_launch_ens_energy(e->pos, with_kinetic ? e->vel : nullptr, e->mass, c.members, c.n, c.dim, e->is_f64, e->prm,
                                e->epart, e->ehist, e->ehist + e->ehist_cap * c.members, s, e->stream, e->sizes));
    return NB_OK;
}

// the first `samples` samples (may be 0) to the caller's arrays (either may be null), then the one wait of the call
int history_out(nb_ens *e, int64_t samples, double *kinetic, double *potential, int on_device)
{
    const size_t bytes = (size_t)samples * e->cfg.members * sizeof(double);
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (kinetic && bytes) HIPCHK(hipMemcpyAsync(kinetic, e->ehist, bytes, kind, e->stream));
    if (potential && bytes) HIPCHK(hipMemcpyAsync(potential, e->ehist + e->ehist_cap * e->cfg.members, bytes, kind, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return NB_OK;
}

// The launch train of nb_ens_step / nb_ens_run_recorded / nb_ens_run_members: `nmax` ticks (simulation.py:120-143).  One
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
    const nb_ens_config &c = e->cfg;
    auto open_tick = [&](int t) {
        return nb_launch_ens_kick_drift(e->pos, e->vel, e->acc, c.members, c.n, c.dim, e->is_f64, e->prm, stop, t, e->stream,
                                        e->sizes);
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
                    HIPCHK(nb_launch_ens_watch(e->pos, e->vel, c.members, c.n, c.dim, e->is_f64, e->ehist,
                                               e->ehist + e->ehist_cap * c.members, t / every, t, stop, stop + c.members,
                                               e->stream, e->sizes));
                else if (watch == WATCH_CRASH)
                    HIPCHK(nb_launch_ens_crash(e->pos, e->prev_pos, e->vel, c.members, c.n, c.dim, e->is_f64, e->dt_dev, e->ehist,
                                               e->ehist + e->ehist_cap * c.members, t / every, t, stop, stop + c.members,
                                               crash_flags(e), e->crash_out, e->stream));
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

// The recorded run behind nb_ens_run_recorded / _members / _crash_watched, arguments checked: `nmax` ticks of run_train
// sampled every `every` (0: never) under `watch`.  budgets: the members' stop ticks, uploaded beside halt reasons of 0 and
// read back into stop_tick / why -- or null: NO stop array is passed and the kernels without stops run.  WATCH_CRASH primes
// the detector in front of the launches (dt; zeroed flags and measures, which a member that is never checked -- budget 0
// -- reports; the previous positions) and reads flags / measures back.  history_out is the one wait; *samples is set last.
int run_sampled(nb_ens *e, const int32_t *budgets, int32_t nmax, int32_t every, WatchMode watch, double *kinetic,
                double *potential, int64_t capacity, int on_device, int32_t *samples, int32_t *stop_tick, int32_t *why,
                int32_t *flags, double *measures)
{
    const size_t B = (size_t)e->cfg.members;
    const int64_t S = every ? 1 + (int64_t)(nmax / every) : 0;
    if (capacity < S && watch == WATCH_CRASH)
        return fail(NB_ERR_INVALID, "capacity of %lld samples is below the %lld of %d ticks sampled every tick",
                    (long long)capacity, (long long)S, nmax);
    if (capacity < S)
        return fail(NB_ERR_INVALID, "capacity of %lld samples is below the %lld of %d ticks sampled every %d",
                    (long long)capacity, (long long)S, nmax, every);
    DeviceGuard guard(e->cfg.device);
    if (S)
        if (int rc = energy_buffers(e, S)) return rc;
    if (watch == WATCH_CRASH)
        if (int rc = crash_buffers(e)) return rc;
    const size_t stop_bytes = 2 * B * sizeof(int32_t);
    if (budgets) {
        if (!e->stops) HIPCHK(hipMalloc((void **)&e->stops, stop_bytes));
        // stops_host is free to rewrite: every call that uploads it waits before it returns (e->dt: nb_ens_set_params waits too)
        static_assert(NB_ENS_REASON_NONE == 0 && NB_ENS_CRASH_NONE == 0, "one initial value serves both watches");
        e->stops_host.assign(2 * B, 0);
        std::copy(budgets, budgets + B, e->stops_host.begin());
        HIPCHK(hipMemcpyAsync(e->stops, e->stops_host.data(), stop_bytes, hipMemcpyHostToDevice, e->stream));
    }
    if (watch == WATCH_CRASH) {
        HIPCHK(hipMemcpyAsync(e->dt_dev, e->dt.data(), B * sizeof(double), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemsetAsync(e->crash_out, 0, B * (4 * sizeof(double) + sizeof(int32_t)), e->stream));
        HIPCHK(hipMemcpyAsync(e->prev_pos, e->pos, cnt_nd(e) * el(e), hipMemcpyDeviceToDevice, e->stream));
    }
    if (int rc = run_train(e, nmax, every, budgets ? e->stops : nullptr, watch, every ? SAMPLE_ENERGIES : 0u)) return rc;
    if (budgets) HIPCHK(hipMemcpyAsync(e->stops_host.data(), e->stops, stop_bytes, hipMemcpyDeviceToHost, e->stream));
    if (watch == WATCH_CRASH)
        if (int rc = crash_out_async(e)) return rc;
    if (int rc = history_out(e, S, kinetic, potential, on_device)) return rc;      // (waits, with S = 0 too)
    if (budgets && stop_tick) std::copy(e->stops_host.begin(), e->stops_host.begin() + B, stop_tick);
    if (budgets && why) std::copy(e->stops_host.begin() + B, e->stops_host.end(), why);
    if (watch == WATCH_CRASH) crash_results(e, flags, measures);
    if (samples) *samples = (int32_t)S;
    return NB_OK;
}

// room for one batched evaluation of the diagnostics with `num_bins` bins (buffers grow, never shrink)
int metrics_buffers(nb_ens *e, int num_bins)
{
    const size_t B = (size_t)e->cfg.members;
    if (!e->mscratch) HIPCHK(hipMalloc(&e->mscratch, nb_ens_metrics_scratch_bytes(e->cfg.members, e->cfg.n, e->is_f64)));
    if (!e->mradius) HIPCHK(hipMalloc((void **)&e->mradius, B * sizeof(double)));
    if (num_bins > e->mbins_cap) {
        // no launch reads the old results: every call that fills them copies them out and waits before it returns
        if (e->mout) { (void)hipFree(e->mout); e->mout = nullptr; }
        if (e->medges) { (void)hipFree(e->medges); e->medges = nullptr; }
        e->mbins_cap = -1;
        HIPCHK(hipMalloc((void **)&e->mout, B * (5 + 2 * (size_t)num_bins) * sizeof(double)));
        HIPCHK(hipMalloc((void **)&e->medges, B * ((size_t)num_bins + 1) * sizeof(float)));
        e->mbins_cap = num_bins;
    }
    return NB_OK;
}

// the entries a handle of nb_ens_create_ragged refuses: their kernels are one workgroup per member of the handle's n, or
// the grid modes'
int refuse_ragged(const nb_ens *e, const char *entry, const char *follow_up)
{
    if (e->sizes)
        return fail(NB_ERR_UNSUPPORTED, "%s is not implemented for members of different sizes (nb_ens_create_ragged): %s is a "
                                        "follow-up", entry, follow_up);
    return NB_OK;
}

// what both constructors ask of the shape
int check_shape(const nb_ens_config *cfg)
{
    if (cfg->members < 1 || cfg->members > NB_ENS_MAX_MEMBERS)
        return fail(NB_ERR_INVALID, "members must be in [1, %d] (got %d)", NB_ENS_MAX_MEMBERS, cfg->members);
    if (cfg->n < 1) return fail(NB_ERR_INVALID, "n must be >= 1 (got %d)", cfg->n);
    if (cfg->dim != 2 && cfg->dim != 3) return fail(NB_ERR_INVALID, "dim must be 2 or 3 (got %d)", cfg->dim);
    return NB_OK;
}

// levels: null for the cast modes, else `members` checked level counts (a grid-mode handle)
int create(nb_ens **out, const nb_ens_config *cfg, const int32_t *levels, const double *G, const double *softening_sq,
           const double *dt)
{
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
    e->cfg = *cfg;
    e->is_f64 = f64;
    e->hook = mode_hook(cfg->mode);
    const NbKnobs knobs = nb_read_knobs();
    e->lanes = knobs.small_lanes ? knobs.small_lanes : nb_small_lanes(cfg->n);     // as step_small picks them
    const int B = cfg->members;
    e->G.assign(G, G + B);
    e->eps2.assign(softening_sq, softening_sq + B);
    e->dt.assign(dt, dt + B);
    e->prm_host.resize((size_t)B * (f64 ? sizeof(EnsScalars<double>) : sizeof(EnsScalars<float>)));
    const size_t nd_bytes = cnt_nd(e) * el(e);
    hipError_t he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (he == hipSuccess) he = hipMalloc(&e->prm, e->prm_host.size());
    if (he == hipSuccess) he = hipMalloc(&e->pos, nd_bytes);
    if (he == hipSuccess) he = hipMalloc(&e->pos_alt, nd_bytes);
    if (he == hipSuccess) he = hipMalloc(&e->vel, nd_bytes);
    if (he == hipSuccess) he = hipMalloc(&e->acc, nd_bytes);
    if (he == hipSuccess) he = hipMalloc(&e->mass, cnt_n(e) * el(e));
    if (he == hipSuccess) he = hipMemsetAsync(e->acc, 0, nd_bytes, e->stream);
    if (levels) {
        e->grid = true;
        e->fq = cfg->mode != NB_CUSTOM;
        e->allow_fast = knobs.no_grid_fast ? 0 : 1;
        e->grid_blocks = nb_small_blocks(cfg->n, e->lanes);
        e->levels.assign(levels, levels + B);
        e->max_levels = *std::max_element(levels, levels + B);
        const size_t part_bytes = (size_t)B * e->grid_blocks * 2 * sizeof(double);
        // zeroed once: every evaluation puts a member's maximum and arrival counter back (grid_tables_body)
        if (he == hipSuccess) he = hipMalloc((void **)&e->tabs, (size_t)B * sizeof(GridTables));
        if (he == hipSuccess) he = hipMemsetAsync(e->tabs, 0, (size_t)B * sizeof(GridTables), e->stream);
        if (he == hipSuccess) he = hipMalloc((void **)&e->levels_dev, (size_t)B * sizeof(int));
        if (he == hipSuccess) he = hipMemcpyAsync(e->levels_dev, e->levels.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, e->stream);
        if (e->fq) {      // CUSTOM does not quantise forces: no partials, no bounds
            if (he == hipSuccess) he = hipMalloc((void **)&e->fpart, part_bytes);
            if (he == hipSuccess) he = hipMemsetAsync(e->fpart, 0, part_bytes, e->stream);
            if (he == hipSuccess) he = hipMalloc((void **)&e->fbounds, (size_t)B * 2 * sizeof(double));
            if (he == hipSuccess) he = hipMemsetAsync(e->fbounds, 0, (size_t)B * 2 * sizeof(double), e->stream);
        }
    }
    if (he != hipSuccess) {
        release(e);
        return fail(he == hipErrorOutOfMemory ? NB_ERR_OOM : NB_ERR_HIP, "ensemble allocation failed: %s", hipGetErrorString(he));
    }
    if (int rc = upload_params(e)) { release(e); return rc; }      // (waits: the level counts have left e->levels)
    *out = e;
    return NB_OK;
}

// modes[0 .. members) of a handle whose members have their own cast modes (cfg->mode: NB_FLOAT32)
int check_mode_list(const nb_ens_config *cfg, const int32_t *modes)
{
    for (int b = 0; b < cfg->members; ++b)
        if (modes[b] != NB_FLOAT32 && modes[b] != NB_BFLOAT16 && modes[b] != NB_FLOAT16)
            return fail(NB_ERR_UNSUPPORTED, "modes[%d] = %d: members of one ensemble mix the FLOAT32, BFLOAT16 and FLOAT16 modes "
                                            "only (FLOAT64 is stored differently, the grid modes need per-member tables)", b,
                        modes[b]);
    return NB_OK;
}

// the members' hooks onto the device of a freshly created handle (released on failure)
int attach_hooks(nb_ens *e, const int32_t *modes)
{
    DeviceGuard guard(e->cfg.device);
    const int B = e->cfg.members;
    e->mixed = true;
    e->hooks_host.resize(B);
    for (int b = 0; b < B; ++b) e->hooks_host[b] = mode_hook(modes[b]);
    const size_t bytes = (size_t)B * sizeof(int);
    hipError_t he = hipMalloc((void **)&e->hooks, bytes);
    if (he == hipSuccess) he = hipMemcpyAsync(e->hooks, e->hooks_host.data(), bytes, hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    if (he != hipSuccess) {
        release(e);
        return fail(he == hipErrorOutOfMemory ? NB_ERR_OOM : NB_ERR_HIP, "ensemble allocation failed: %s", hipGetErrorString(he));
    }
    return NB_OK;
}

}  // namespace

extern "C" {

int nb_ens_create(nb_ens **out, const nb_ens_config *cfg, const double *G, const double *softening_sq, const double *dt)
{
    if (!out || !cfg || !G || !softening_sq || !dt) return fail(NB_ERR_INVALID, "null argument");
    *out = nullptr;
    if (int rc = check_shape(cfg)) return rc;
    if (cfg->mode < NB_FLOAT64 || cfg->mode > NB_FLOAT16)
        return fail(NB_ERR_UNSUPPORTED, "ensembles run the FLOAT64, FLOAT32, BFLOAT16 and FLOAT16 modes (got mode %d): the grid "
                                        "modes need per-member tables", cfg->mode);
    return create(out, cfg, nullptr, G, softening_sq, dt);
}

int nb_ens_create_grid(nb_ens **out, const nb_ens_config *cfg, const int32_t *levels, const double *G, const double *softening_sq,
                       const double *dt)
{
    if (!out || !cfg || !G || !softening_sq || !dt) return fail(NB_ERR_INVALID, "null argument");
    *out = nullptr;
    if (int rc = check_shape(cfg)) return rc;
    if (cfg->mode != NB_INT8_SIM && cfg->mode != NB_INT4_SIM && cfg->mode != NB_CUSTOM)
        return fail(NB_ERR_UNSUPPORTED, "nb_ens_create_grid runs the INT8_SIM, INT4_SIM and CUSTOM modes (got mode %d): the other "
                                        "modes are nb_ens_create's", cfg->mode);
    if (cfg->mode != NB_CUSTOM && levels)
        return fail(NB_ERR_INVALID, "levels must be NULL under INT8_SIM / INT4_SIM (256 / 16 levels)");
    std::vector<int32_t> lv(cfg->members, cfg->mode == NB_INT8_SIM ? 256 : cfg->mode == NB_INT4_SIM ? 16 : 64);
    if (levels) lv.assign(levels, levels + cfg->members);
    for (int b = 0; b < cfg->members; ++b)
        if (lv[b] < 2 || lv[b] > NB_LUT_MIN)
            return fail(NB_ERR_INVALID, "levels[%d] = %d is outside [2, %d]: above it a solo run leaves the one-launch step", b,
                        lv[b], NB_LUT_MIN);
    return create(out, cfg, lv.data(), G, softening_sq, dt);
}

int nb_ens_create_grid_wide(nb_ens **out, const nb_ens_config *cfg, const int32_t *levels, const double *G,
                            const double *softening_sq, const double *dt)
{
    if (!out || !cfg || !G || !softening_sq || !dt) return fail(NB_ERR_INVALID, "null argument");
    *out = nullptr;
    if (int rc = check_shape(cfg)) return rc;
    if (cfg->mode != NB_CUSTOM)
        return fail(NB_ERR_UNSUPPORTED, "nb_ens_create_grid_wide runs the CUSTOM mode (got mode %d): INT8_SIM / INT4_SIM are "
                                        "nb_ens_create_grid's, the other modes nb_ens_create's", cfg->mode);
    std::vector<int32_t> lv(cfg->members, 64);
    if (levels) lv.assign(levels, levels + cfg->members);
    for (int b = 0; b < cfg->members; ++b)
        if (lv[b] < 2 || lv[b] > NB_MAX_LUT)
            return fail(NB_ERR_INVALID, "levels[%d] = %d is outside [2, %d]: finer grids are the solo engine's generic kernel's", b,
                        lv[b], NB_MAX_LUT);
    return create(out, cfg, lv.data(), G, softening_sq, dt);
}

int nb_ens_create_mixed(nb_ens **out, const nb_ens_config *cfg, const int32_t *modes, const double *G,
                        const double *softening_sq, const double *dt)
{
    if (!out || !cfg || !modes || !G || !softening_sq || !dt) return fail(NB_ERR_INVALID, "null argument");
    *out = nullptr;
    if (int rc = check_shape(cfg)) return rc;
    if (cfg->mode != NB_FLOAT32)
        return fail(NB_ERR_UNSUPPORTED, "nb_ens_create_mixed: cfg->mode must be NB_FLOAT32, the storage mode of every cast mode "
                                        "(got mode %d)", cfg->mode);
    if (int rc = check_mode_list(cfg, modes)) return rc;
    nb_ens *e = nullptr;
    if (int rc = create(&e, cfg, nullptr, G, softening_sq, dt)) return rc;
    if (int rc = attach_hooks(e, modes)) return rc;
    *out = e;
    return NB_OK;
}

int nb_ens_create_ragged(nb_ens **out, const nb_ens_config *cfg, const int32_t *sizes, const int32_t *modes, const double *G,
                         const double *softening_sq, const double *dt)
{
    if (!out || !cfg || !sizes || !G || !softening_sq || !dt) return fail(NB_ERR_INVALID, "null argument");
    *out = nullptr;
    if (int rc = check_shape(cfg)) return rc;
    if (cfg->mode < NB_FLOAT64 || cfg->mode > NB_FLOAT16)
        return fail(NB_ERR_UNSUPPORTED, "nb_ens_create_ragged runs the FLOAT64, FLOAT32, BFLOAT16 and FLOAT16 modes (got mode %d): "
                                        "the ragged grid modes are a follow-up", cfg->mode);
    if (modes && cfg->mode != NB_FLOAT32)
        return fail(NB_ERR_UNSUPPORTED, "nb_ens_create_ragged: with a mode list cfg->mode must be NB_FLOAT32, the storage mode of "
                                        "every cast mode (got mode %d)", cfg->mode);
    if (modes)
        if (int rc = check_mode_list(cfg, modes)) return rc;
    for (int b = 0; b < cfg->members; ++b)
        if (sizes[b] < 1 || sizes[b] > cfg->n)
            return fail(NB_ERR_INVALID, "sizes[%d] = %d is outside [1, %d]: member %d must fit the capacity cfg->n", b, sizes[b],
                        cfg->n, b);
    nb_ens *e = nullptr;
    if (int rc = create(&e, cfg, nullptr, G, softening_sq, dt)) return rc;
    if (modes)
        if (int rc = attach_hooks(e, modes)) return rc;
    DeviceGuard guard(cfg->device);
    const int B = cfg->members;
    e->sizes_host.assign(sizes, sizes + B);
    std::vector<EnsWork> work;
    e->work_items = (int)nb_plan_ragged(sizes, B, e->lanes, &work);
    static_assert(sizeof(int32_t) == sizeof(int), "the kernels read ints");
    hipError_t he = hipMalloc((void **)&e->work, work.size() * sizeof(EnsWork));
    if (he == hipSuccess) he = hipMemcpyAsync(e->work, work.data(), work.size() * sizeof(EnsWork), hipMemcpyHostToDevice, e->stream);
    // sizes last: a handle that holds them is complete
    int *dev_sizes = nullptr;
    if (he == hipSuccess) he = hipMalloc((void **)&dev_sizes, (size_t)B * sizeof(int));
    if (he == hipSuccess) he = hipMemcpyAsync(dev_sizes, e->sizes_host.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);       // (the uploads have consumed `work`)
    e->sizes = dev_sizes;
    if (he != hipSuccess) {
        release(e);
        return fail(he == hipErrorOutOfMemory ? NB_ERR_OOM : NB_ERR_HIP, "ensemble allocation failed: %s", hipGetErrorString(he));
    }
    *out = e;
    return NB_OK;
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
    if (dtype != (e->is_f64 ? NB_F64 : NB_F32))
        return fail(NB_ERR_UNSUPPORTED, "ensemble state is %s under this mode (got dtype %d): mixed dtypes and the promotion "
                                        "timeline are nb_sim's", e->is_f64 ? "fp64" : "fp32", dtype);
    DeviceGuard guard(e->cfg.device);
    if (pos) { if (int rc = copy_in(e, e->pos, pos, cnt_nd(e), on_device)) return rc; e->have_pos = true; }
    // a ragged handle: the second buffer too -- no kernel writes the rows behind a member's own, so after a swap they would
    // hold whatever the allocation held instead of the caller's padding
    if (pos && e->sizes) if (int rc = copy_in(e, e->pos_alt, pos, cnt_nd(e), on_device)) return rc;
    if (vel) { if (int rc = copy_in(e, e->vel, vel, cnt_nd(e), on_device)) return rc; e->have_vel = true; }
    if (mass) { if (int rc = copy_in(e, e->mass, mass, cnt_n(e), on_device)) return rc; e->have_mass = true; }
    HIPCHK(hipStreamSynchronize(e->stream));      // the copies have consumed the caller's buffers
    return NB_OK;
}

int nb_ens_get_state(nb_ens *e, void *pos, void *vel, void *acc, void *mass, int on_device)
{
    if (!e) return fail(NB_ERR_INVALID, "null handle");
    DeviceGuard guard(e->cfg.device);
    if (pos) if (int rc = copy_out(e, pos, e->pos, cnt_nd(e), on_device)) return rc;
    if (vel) if (int rc = copy_out(e, vel, e->vel, cnt_nd(e), on_device)) return rc;
    if (acc) if (int rc = copy_out(e, acc, e->acc, cnt_nd(e), on_device)) return rc;
    if (mass) if (int rc = copy_out(e, mass, e->mass, cnt_n(e), on_device)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return NB_OK;
}

int nb_ens_set_accelerations(nb_ens *e, const void *acc, int dtype, int on_device)
{
    if (!e || !acc) return fail(NB_ERR_INVALID, "null argument");
    if (dtype != (e->is_f64 ? NB_F64 : NB_F32)) return fail(NB_ERR_UNSUPPORTED, "acceleration dtype %d on %s state", dtype, e->is_f64 ? "fp64" : "fp32");
    DeviceGuard guard(e->cfg.device);
    if (int rc = copy_in(e, e->acc, acc, cnt_nd(e), on_device)) return rc;
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
    if (e->sizes) {
        // the probe has the capacity's shape, not the member's: a ragged member's energies are the batched kernels', which
        // give it the values of a handle of its own size (nb_ens_energy.hip)
        if (!e->have_pos || (kinetic && !e->have_vel)) return fail(NB_ERR_INVALID, "state incomplete");
        if (int rc = energy_buffers(e, 1)) return rc;
        if (int rc = launch_energy(e, 0, kinetic != nullptr)) return rc;
        return history_out(e, 1, kinetic, potential, 0);
    }
    if (!e->probe) {
        nb_config pc{};
        pc.n = c.n; pc.dim = c.dim; pc.mode = c.mode; pc.G = e->G[0]; pc.softening_sq = e->eps2[0]; pc.dt = e->dt[0];
        pc.device = c.device; pc.rank = 0; pc.nranks = 1; pc.flags = 0;
        if (int rc = nb_create(&e->probe, &pc)) return rc;
    }
    HIPCHK(hipStreamSynchronize(e->stream));         // the probe reads the members' slices on a stream of its own
    const int dtype = e->is_f64 ? NB_F64 : NB_F32;
    const size_t nd_b = (size_t)c.n * c.dim * el(e), n_b = (size_t)c.n * el(e);
    for (int b = 0; b < c.members; ++b) {
        if (int rc = nb_set_params(e->probe, e->G[b], e->eps2[b], e->dt[b])) return rc;
        if (int rc = nb_set_state(e->probe, (const char *)e->pos + b * nd_b, (const char *)e->vel + b * nd_b,
                                  (const char *)e->mass + b * n_b, dtype, 1))
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
    if (int rc = energy_buffers(e, 1)) return rc;
    if (int rc = launch_energy(e, 0, kinetic != nullptr)) return rc;
    return history_out(e, 1, kinetic, potential, on_device);
}

// run_train with samples and no stop array
int nb_ens_run_recorded(nb_ens *e, int32_t nsteps, int32_t every, double *kinetic, double *potential, int64_t capacity,
                        int on_device, int32_t *samples)
{
    if (samples) *samples = 0;
    if (int rc = check_steppable(e)) return rc;
    if (nsteps < 0) return fail(NB_ERR_INVALID, "nsteps must be >= 0 (got %d)", nsteps);
    if (every < 1) return fail(NB_ERR_INVALID, "every must be >= 1 (got %d)", every);
    return run_sampled(e, nullptr, nsteps, every, WATCH_NONE, kinetic, potential, capacity, on_device, samples, nullptr, nullptr,
                       nullptr, nullptr);
}

// run_train with the members' budgets as their stop ticks (and the watch lowering them)
int nb_ens_run_members(nb_ens *e, const int32_t *nsteps, int32_t every, int32_t watch, double *kinetic, double *potential,
                       int64_t capacity, int on_device, int32_t *samples, int32_t *stop_tick, int32_t *reason)
{
    if (samples) *samples = 0;
    if (int rc = check_steppable(e)) return rc;
    int32_t nmax = 0;
    if (int rc = check_budgets(e, nsteps, &nmax)) return rc;
    if (every < 0) return fail(NB_ERR_INVALID, "every must be >= 0 (got %d)", every);
    if (watch != 0 && watch != 1) return fail(NB_ERR_INVALID, "watch must be 0 or 1 (got %d)", watch);
    if (watch && every < 1) return fail(NB_ERR_INVALID, "the watch tests sampled ticks: it needs every >= 1");
    return run_sampled(e, nsteps, nmax, every, watch ? WATCH_EXPLOSION : WATCH_NONE, kinetic, potential, capacity, on_device,
                       samples, stop_tick, reason, nullptr, nullptr);
}

// the detector's kernel alone on the resident state: one launch, one copy-out, one wait
int nb_ens_crash_measures(nb_ens *e, const void *prev_pos, int on_device, int32_t *flags, double *measures)
{
    if (!e) return fail(NB_ERR_INVALID, "null handle");
    if (int rc = refuse_ragged(e, "nb_ens_crash_measures", "the ragged crash watch")) return rc;
    if (!e->have_pos || !e->have_vel) return fail(NB_ERR_INVALID, "state incomplete");
    DeviceGuard guard(e->cfg.device);
    const nb_ens_config &c = e->cfg;
    if (int rc = crash_buffers(e)) return rc;
    const void *prev = prev_pos;
    if (prev_pos && !on_device) {          // (the wait below: the upload has consumed prev_pos)
        if (int rc = copy_in(e, e->prev_pos, prev_pos, cnt_nd(e), 0)) return rc;
        prev = e->prev_pos;
    }
    HIPCHK(nb_launch_ens_crash(e->pos, const_cast<void *>(prev), e->vel, c.members, c.n, c.dim, e->is_f64, nullptr, nullptr,
                               nullptr, 0, 0, nullptr, nullptr, crash_flags(e), e->crash_out, e->stream));
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
    int32_t nmax = 0;
    if (int rc = check_budgets(e, nsteps, &nmax)) return rc;
    return run_sampled(e, nsteps, nmax, 1, WATCH_CRASH, kinetic, potential, capacity, on_device, samples, stop_tick, kind, flags,
                       measures);
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
    if (int rc = divergence_out(e, 1, max_pos, mean_pos, max_vel, on_device)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return NB_OK;
}

// run_train with the divergence (and, asked for, the energies) in every sample and no stop array
int nb_ens_run_diverged(nb_ens *e, int32_t nsteps, int32_t every, const int32_t *baseline, int32_t with_energies,
                        double *max_pos, double *mean_pos, double *max_vel, double *kinetic, double *potential, int64_t capacity,
                        int on_device, int32_t *samples)
{
    if (samples) *samples = 0;
    if (int rc = check_steppable(e)) return rc;
    if (nsteps < 0) return fail(NB_ERR_INVALID, "nsteps must be >= 0 (got %d)", nsteps);
    if (every < 1) return fail(NB_ERR_INVALID, "every must be >= 1 (got %d)", every);
    const int64_t S = 1 + (int64_t)(nsteps / every);
    if (capacity < S)
        return fail(NB_ERR_INVALID, "capacity of %lld samples is below the %lld of %d ticks sampled every %d",
                    (long long)capacity, (long long)S, nsteps, every);
    DeviceGuard guard(e->cfg.device);
    if (int rc = divergence_buffers(e, S)) return rc;
    if (int rc = upload_baselines(e, baseline)) return rc;      // (checks them: nothing is launched for a bad one)
    if (with_energies)
        if (int rc = energy_buffers(e, S)) return rc;
    if (int rc = run_train(e, nsteps, every, nullptr, WATCH_NONE, SAMPLE_DIVERGENCE | (with_energies ? SAMPLE_ENERGIES : 0u)))
        return rc;
    if (int rc = divergence_out(e, S, max_pos, mean_pos, max_vel, on_device)) return rc;
    if (with_energies) {
        if (int rc = history_out(e, S, kinetic, potential, on_device)) return rc;      // (waits)
    } else {
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    if (samples) *samples = (int32_t)S;
    return NB_OK;
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
    if (int rc = metrics_buffers(e, num_bins)) return rc;
    if (max_radius) HIPCHK(hipMemcpyAsync(e->mradius, max_radius, B * sizeof(double), hipMemcpyHostToDevice, e->stream));
    NbEnsMetricsArgs a{};
    a.pos = e->pos; a.vel = e->vel; a.mass = e->mass;
    a.members = c.members; a.n = c.n; a.dim = c.dim; a.is_f64 = e->is_f64;
    a.prm = e->prm;
    a.max_radius = max_radius ? e->mradius : nullptr;
    a.num_bins = num_bins;
    const long long k = (long long)((double)c.n * percentile / 100.0);     // int(len(radii) * percentile / 100), as nb_metrics
    a.kth = (int)std::min<long long>(std::max<long long>(k, 0), c.n - 1);
    a.scratch = e->mscratch;
    a.out = e->mout;
    a.edges_out = e->medges;
    HIPCHK(nb_launch_ens_metrics(a, e->stream));
    const size_t per = 5 + 2 * nb;
    std::vector<double> host(B * per);
    HIPCHK(hipMemcpyAsync(host.data(), e->mout, host.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (edges && nb > 0)
        HIPCHK(hipMemcpyAsync(edges, e->medges, B * (nb + 1) * sizeof(float), hipMemcpyDeviceToHost, e->stream));
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
    if (int rc = refuse_ragged(e, "nb_ens_quant_info", "the ragged grid modes")) return rc;
    if (!e->grid) return fail(NB_ERR_UNSUPPORTED, "quant info is only defined for the grid modes (nb_ens_create_grid)");
    DeviceGuard guard(e->cfg.device);
    const size_t B = (size_t)e->cfg.members;
    // the scalars behind the tables of every member, not the 48 KB of tables in front of them
    constexpr size_t off = offsetof(GridTables, lmin), width = sizeof(GridTables) - off;
    std::vector<char> tail(B * width);
    std::vector<double> fb(B * 2, __builtin_nan(""));
    HIPCHK(hipMemcpy2DAsync(tail.data(), width, (const char *)e->tabs + off, sizeof(GridTables), width, B, hipMemcpyDeviceToHost,
                            e->stream));
    if (e->fq) HIPCHK(hipMemcpyAsync(fb.data(), e->fbounds, B * 2 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
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
    if (int rc = refuse_ragged(e, "nb_ens_quant_bin_sums", "the ragged grid modes")) return rc;
    if (!e->grid) return fail(NB_ERR_UNSUPPORTED, "the quant-bin read-out is only defined for the grid modes (nb_ens_create_grid, "
                                                  "nb_ens_create_grid_wide)");
    if (!e->have_pos || !e->have_mass) return fail(NB_ERR_INVALID, "positions/masses not set");
    DeviceGuard guard(e->cfg.device);
    const nb_ens_config &c = e->cfg;
    const size_t B = (size_t)c.members, n = (size_t)c.n, per = 2 * n + 2, bytes = B * per * sizeof(unsigned long long);
    if (!e->bin_acc) HIPCHK(hipMalloc((void **)&e->bin_acc, cnt_nd(e) * sizeof(float)));
    if (!e->bin_out) HIPCHK(hipMalloc((void **)&e->bin_out, bytes));
    HIPCHK(hipMemsetAsync(e->bin_out, 0, bytes, e->stream));
    if (int rc = launch_tables(e, nullptr, 0)) return rc;
    HIPCHK(nb_launch_ens_grid_bins((const float *)e->pos, e->bin_acc, (const float *)e->mass, c.members, c.n, c.dim, e->prm,
                                   e->lanes, e->tabs, e->max_levels, e->bin_out, e->stream));
    std::vector<unsigned long long> host(B * per);
    HIPCHK(hipMemcpyAsync(host.data(), e->bin_out, bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (size_t b = 0; b < B; ++b) {
        const unsigned long long *h = host.data() + b * per;
        for (size_t i = 0; i < n; ++i) {
            if (sum_k) sum_k[b * n + i] = (int64_t)h[i];
            if (sum_kw) sum_kw[b * n + i] = (int64_t)h[n + i];
        }
        if (pairs) { pairs[2 * b] = (int64_t)h[2 * n]; pairs[2 * b + 1] = (int64_t)h[2 * n + 1]; }
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
