// nb_step.cpp -- kernel selection and sequencing of the hot path behind the C-ABI (include/nbody_amd.h):
//   force_eval   one evaluation of GalaxySimulation._compute_accelerations (reference simulation.py:74-118), in phases:
//                resolve_eval (dtypes, kernel, carriers: decided once), grid_prepare, launch_pairs, reduce_and_exchange,
//                force_quant_finish, fall-back kick; force_eval_generic for the dtype-faithful kernel.  Asked for with
//                an EvalRequest, answers with an EvalResult (nb_state.h); kicks are named by NbKick (nb_internal.h)
//   step_run     kick-drift-kick leapfrog steps (simulation.py:120-143), launches fused as far as each path allows
//   energy_eval  kinetic / potential energy (simulation.py:170-192)
//   bin_sums_eval  the quant-bin read-out of the production grid-mode pair loops (nb_quant_bin_sums)
// Everything is queued on the handle's own HIP stream; the only host waits are the ones the callers need.
#include <algorithm>
#include <cstring>

#include "nb_state.h"

namespace nbhost {

// ---- size thresholds of the kernel selection, in one place (measured crossovers on MI355X) ----
struct NbTuning {
    int onesided_r1_max_n = 8192;       // one-sided fp64 kernel: one target per thread up to here (parallelism-bound)
    int onesided_target_wgs = 1024;     // ... and enough source chunks for >= 4 workgroups per CU
    int prune_min_n = 8192;             // grid modes, first evaluation: pruned max-r2 search above, all-pairs scan at or below
    int track_min_n = 3072;             // grid modes: above, every evaluation after the first TRACKS the farthest pair of its
                                        // predecessor (two launches incl. the tables; the seed then always prunes).  On the
                                        // one-launch small-system path the all-pairs pass costs the same (measured INT8 / CUSTOM
                                        // N = 3000: 31.3 / 27.1 vs 31.0 / 26.7 us per step: the table construction by a single
                                        // workgroup is what is left there, not the search)
    int red_mm_max_blocks = 1024;       // INT8 / INT4: the reduction also hands out force min / max partials up to
                                        // N = 65 536 (one launch fewer: INT8 step 785.8 -> 784.2 us there; beyond, every
                                        // finish workgroup would fold thousands of them)
    int small_max_f64 = 4096;           // one-launch step: fp64 4.9 / 7.9 / 11.4 / 16.9 us per step at N = 1024 ... 4096
    int small_max_f32 = 3072;           // fp32 storage: above, the tiled path is ahead (FLOAT32) or level (INT8 / INT4)
    int small_fuse_tables_max_n = 2048; // small grid steps: max-r2 launch also builds the tables up to here
};
static const NbTuning g_tune{};

int small_max_n(bool is_f64) { return is_f64 ? g_tune.small_max_f64 : g_tune.small_max_f32; }

// targets per thread of the one-sided fp64 kernel.  Small systems are parallelism-bound, not
// throughput-bound: R = 1 doubles the workgroups (N = 1024: 27.8 -> 17.6 us per step, N = 4096:
// 32.5 -> 22.6 us)
int onesided_r(int n, const NbKnobs &knobs)
{
    if (knobs.r_onesided == 1 || knobs.r_onesided == 2 || knobs.r_onesided == 4)   // NB_R tuning knob
        return knobs.r_onesided;
    return (n <= g_tune.onesided_r1_max_n) ? 1 : 2;
}

ForceGeom onesided_geometry(const nb_config &c, const NbKnobs &knobs)
{
    const int n = c.n;
    ForceGeom g{};
    g.n = n;
    g.j_begin = (int)((int64_t)c.rank * n / c.nranks);
    g.j_end = (int)((int64_t)(c.rank + 1) * n / c.nranks);
    g.r = onesided_r(n, knobs);
    const int njr = std::max(g.j_end - g.j_begin, 1);
    const int itiles = (n + NB_BLOCK * g.r - 1) / (NB_BLOCK * g.r);
    const int max_chunks = (njr + NB_TJ - 1) / NB_TJ;
    int nch = (g_tune.onesided_target_wgs + itiles - 1) / itiles;       // aim for >= 4 workgroups per CU
    nch = std::max(1, std::min(std::min(nch, max_chunks), 64));
    int chunk = (njr + nch - 1) / nch;
    chunk = (chunk + NB_TJ - 1) / NB_TJ * NB_TJ;
    g.chunk_len = chunk;
    g.nchunks = (njr + chunk - 1) / chunk;
    return g;
}

void compute_geometry(nb_sim *s) { s->geom = onesided_geometry(s->cfg, s->knobs); }

void path_clear(nb_sim *s)
{
    for (std::string &p : s->path_part) p.clear();
    s->path_open_kd = false;
}

void path_note(nb_sim *s, int where, const char *site)
{
    if (!site || !*site) return;
    std::string &p = s->path_part[where];
    // the interior steps of a long call repeat one site: a comparison with the last token, no allocation
    const size_t len = strlen(site);
    if (p.size() >= len && p.compare(p.size() - len, len, site) == 0 && (p.size() == len || p[p.size() - len - 1] == '+')) return;
    // whole-token match: "reduce_sym:3" is not contained in "reduce_sym:3|4"
    const std::string tok = std::string("+") + site + "+";
    if (("+" + p + "+").find(tok) == std::string::npos) p += (p.empty() ? "" : "+") + std::string(site);
}

// the reported string is put together only when it is asked for
const char *path_name(nb_sim *s)
{
    static const char *const key[3] = {"open=", "mid=", "close="};
    s->step_path.clear();
    for (int k = 0; k < 3; ++k)
        if (!s->path_part[k].empty()) s->step_path += (s->step_path.empty() ? "" : " ") + (key[k] + s->path_part[k]);
    if (s->step_path.empty()) s->step_path = "none";
    return s->step_path.c_str();
}

int launch_plain_kick(nb_sim *s, bool drift, const char **site)
{
    const nb_config &c = s->cfg;
    if (s->is_f64 && s->logical[3] == NB_F32) {
        // fp32-typed accelerations on fp64 storage: the dtype-faithful variant (never the hot, uniform paths)
        const int v64 = promote(s->logical[1], NB_F32) == NB_F64;
        HIPCHK(nb_launch_kick_a32(s->pos, s->vel, s->acc, c.dt / 2, c.dt, nd(s), v64, s->logical[0] == NB_F64, drift ? 1 : 0,
                                  s->stream));
        *site = "kick_a32";
    } else if (drift) {
        HIPCHK(nb_launch_kick_drift(s->pos, s->vel, s->acc, c.dt / 2, c.dt, nd(s), s->is_f64, s->stream));
        *site = "kick_drift";
    } else {
        HIPCHK(nb_launch_axpy(s->vel, s->acc, c.dt / 2, nd(s), s->is_f64, s->stream));
        *site = "axpy";
    }
    return NB_OK;
}

int acc_logical_dtype(const nb_sim *s)
{
    // promote(promote(Q, M), P) with Q = hook output dtype (quantization.py:43-71)
    int q = s->logical[0];
    if (s->cfg.mode == NB_FLOAT64) q = NB_F64;
    else if (s->cfg.mode <= NB_FLOAT16) q = NB_F32;
    return promote(promote(promote(q, s->logical[2]), NB_F32), s->logical[0]);
}

namespace {

inline int kick_mode(bool kick, bool open) { return kick ? (open ? NB_KICK_CLOSE_OPEN : NB_KICK_CLOSE) : NB_KICK_NONE; }
inline int allow_fast(const nb_sim *s) { return s->knobs.no_grid_fast ? 0 : 1; }

// the launch that applied the kick(s) of an evaluation: "<site>:<mode>" (+ "|4": opening kick applied on read)
void site_set(EvalResult *res, const char *site, int mode, const char *tags = "")
{
    if (!(mode & NB_KICK_MODE_MASK)) { res->site[0] = 0; return; }
    snprintf(res->site, sizeof res->site, "%s:%d%s%s", site, mode & NB_KICK_MODE_MASK, (mode & NB_KICK_OPEN_ON_READ) ? "|4" : "", tags);
}

int prof_begin(nb_sim *s, int *slot, bool record = true)
{
    *slot = -1;
    if (!(s->cfg.flags & NB_FLAG_PROFILE)) return NB_OK;
    if (!s->prof_init) {
        for (int i = 0; i < PROF_RING; ++i) {
            HIPCHK(hipEventCreate(&s->ev_start[i]));
            HIPCHK(hipEventCreate(&s->ev_stop[i]));
        }
        s->prof_init = true;
    }
    if (s->prof_count == PROF_RING) {   // drain
        HIPCHK(hipStreamSynchronize(s->stream));
        for (int i = 0; i < PROF_RING; ++i) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, s->ev_start[i], s->ev_stop[i]));
            s->prof_total_ms += ms;
        }
        s->prof_launches += PROF_RING;
        s->prof_count = 0;
    }
    *slot = s->prof_count++;
    if (record) HIPCHK(hipEventRecord(s->ev_start[*slot], s->stream));
    return NB_OK;
}
// events handed to a launcher that attaches them to the dispatch itself (no barrier packets on the stream)
NbKernelEvents prof_events(nb_sim *s, int slot)
{
    NbKernelEvents ev;
    if (slot >= 0) { ev.start = s->ev_start[slot]; ev.stop = s->ev_stop[slot]; }
    return ev;
}
int prof_end(nb_sim *s, int slot)
{
    if (slot >= 0) HIPCHK(hipEventRecord(s->ev_stop[slot], s->stream));
    return NB_OK;
}

// Which evaluations take the dtype-faithful generic kernel (nb_generic.hip): dtype chains no script of the
// reference builds but its stock class accepts.
bool use_generic(const nb_sim *s)
{
    const nb_config &c = s->cfg;
    if (grid_mode(c.mode) && mode_levels(c) > NB_MAX_LUT) return true;       // fused grids beyond the table capacity
    if (s->is_f64) {
        if (c.mode == NB_FLOAT64) return false;
        if (grid_mode(c.mode)) return true;                                  // grid over an fp64 (or fp64-stored) tensor
        return s->logical[0] != NB_F64;      // cast mode before the promotion: fp32 / half positions beside fp64 tensors
    }
    return grid_mode(c.mode) && is_half(s->logical[0]);                      // grid over a half tensor
}

// ---- one force evaluation: what resolve_eval decides once, and the two things its phases hand on ----------------
struct Eval {
    bool shard = false;        // NB_FLAG_NO_COMM shard of a larger run: no collective, no force quantisation, cannot step
    bool fq = false;           // quantize_force follows the sum
    bool multi = false;        // the sum goes through a collective (comm_active)
    bool generic = false;      // use_generic: everything below is for the tuned kernels only
    int hook = HOOK_NONE;      // hook of the pair loop; fp64 storage: -1 unless a cast mode rounds fp64 positions
    int pair_dt = NB_F32;      // fp32 storage: NB_F32, or the half type of half-typed positions (first evaluation);
                               // fp64 storage: -1 for fp64 pairs, else the narrower type the positions still have
    float eps2 = 0.0f;         // softening rounded to the pair dtype
    bool used_sym = false, sym_uniform = false;   // pair-symmetric kernel; its uniform-mass variant (mass factor in `scale`)
    bool red_mm = false, x64 = false;   // the reduction hands quantize_force its min / max partials; the ranks exchange fp64 sums
    double scale = 1.0;        // launch_reduce: factor applied to the finished sums
    bool kicked = false;       // ... and by whoever applied it: the closing kick is done
};

Eval resolve_eval(const nb_sim *s)
{
    const nb_config &c = s->cfg;
    Eval e;
    e.shard = (c.flags & NB_FLAG_NO_COMM) && c.nranks > 1;
    e.fq = force_quant_mode(c) && !e.shard;
    e.multi = comm_active(s);
    e.generic = use_generic(s);
    if (e.generic) return e;
    if (s->is_f64) {
        // (grid modes on fp64 storage and cast modes before the positions are promoted take the generic path)
        e.hook = (c.mode == NB_FLOAT64) ? -1 : mode_hook(c.mode);
        e.pair_dt = (e.hook < 0 && s->logical[0] != NB_F64) ? s->logical[0] : -1;   // NB_F32 / F16 / BF16
        const bool sym_default_shape = s->sym.r == 4 || s->sym.r == 2;   // HOOK_F32PAIR instantiations
        e.used_sym = s->sym.enabled && e.hook < 0 && (e.pair_dt < 0 || (e.pair_dt == NB_F32 && sym_default_shape));
        e.sym_uniform = s->mass_uniform;
    } else {
        e.hook = mode_hook(c.mode);
        e.pair_dt = is_half(s->logical[0]) ? s->logical[0] : NB_F32;
        e.used_sym = s->sym.enabled && e.pair_dt == NB_F32;
        // grid LUT already carries G and the uniform grid kernel applies the common mass itself (reduce scale stays 1)
        e.sym_uniform = s->mass_uniform && e.hook != HOOK_GRID;
    }
    e.eps2 = (float)round_dt(e.pair_dt >= 0 ? e.pair_dt : NB_F32, c.softening_sq);
    // INT8 / INT4 on one GPU, pair-symmetric path: the reduction hands quantize_force its min / max partials (one pair
    // per workgroup of 64 particles), saving the min/max launch (4.6 of 50 us per step at N = 6000; NbTuning: up to 65 536)
    e.red_mm = e.fq && e.used_sym && !e.multi && !s->is_f64 && (c.n + 63) / 64 <= g_tune.red_mm_max_blocks && !s->knobs.no_red_mm;
    // multi-GPU INT8 / INT4 on the pair-symmetric path: the ranks exchange the UNROUNDED fp64 sums and round once,
    // (float)(sum * scale), exactly where the single-GPU reduction rounds, so the all-reduce itself adds no fp32
    // rounding of its own before quantize_force snaps the forces to their grid (a last-bit difference there is what
    // flips a force bin: measured against the single-GPU run after five steps at N = 9000 INT8, two ranks: positions
    // 1.2e-8 with the fp64 exchange, 1.2e-6 -- a flipped bin -- with fp32 partials).  Twice the bytes, so only where a
    // grid follows: the other fp32 modes differ across rank counts at the 1e-7 of their in-kernel fp32 running sums
    // either way (measured: identical with both exchanges).
    e.x64 = e.multi && e.used_sym && !s->is_f64 && e.fq && !s->knobs.no_x64;
    return e;
}

int force_eval_generic(nb_sim *s, const EvalRequest &rq, const Eval &e, EvalResult *res)
{
    const nb_config &c = s->cfg;
    const int64_t cnt = nd(s);
    if (rq.open_on_read) return fail(NB_ERR_INVALID, "internal: speculative positions on the generic path");
    // a call defers only with settled dtypes outside the grid modes, and neither takes the generic path
    if (rq.may_defer) return fail(NB_ERR_INVALID, "internal: a deferred kick on the generic path");
    const int L = mode_levels(c);
    if (grid_mode(c.mode) && L < 2) return fail(NB_ERR_INVALID, "grid levels must be >= 2 (got %d)", L);
    const int A = acc_logical_dtype(s);
    if (!s->gen_scalars) HIPCHK(hipMalloc(&s->gen_scalars, nb_generic_scalars_bytes()));
    if (grid_mode(c.mode))       // every rank scans all pairs itself: no collective for the grid bounds
        HIPCHK(nb_launch_generic_r2max(s->pos, s->is_f64, c.n, c.dim, s->logical[0], c.softening_sq, s->gen_scalars, s->stream));
    HIPCHK(nb_launch_generic_force(s->pos, s->mass, s->is_f64, s->partial, s->geom, c.dim, s->logical[0], s->logical[2], c.mode,
                                   L, c.G, c.softening_sq, s->gen_scalars, s->acc, A, s->stream));
    s->last_kernel = "generic_force_kernel";
    s->last_generic = true;
    if (e.multi)
        if (int rc = comm_allreduce_sum(s, s->acc, (size_t)cnt, s->is_f64)) return rc;
    if (e.fq) {
        // quantize_force on a tensor of dtype A (quantization.py:74-88): linear grid over its global min / max
        const bool a64 = (A == NB_F64);
        if (a64 == s->is_f64) {
            HIPCHK(nb_launch_minmax_generic(s->acc, s->is_f64, cnt, 0, 0.0, s->scalars, s->scalars + 8, s->stream));
            HIPCHK(nb_launch_grid_quantize(s->acc, s->acc, s->is_f64, cnt, L, s->scalars, s->stream));
        } else {
            // fp32-typed forces held in fp64 storage: quantise in fp32 through the staging buffer
            HIPCHK(nb_launch_convert(s->acc, NB_F64, s->staging, NB_F32, cnt, s->stream));
            HIPCHK(nb_launch_minmax_generic(s->staging, 0, cnt, 0, 0.0, s->scalars, s->scalars + 8, s->stream));
            HIPCHK(nb_launch_grid_quantize(s->staging, s->staging, 0, cnt, L, s->scalars, s->stream));
            HIPCHK(nb_launch_convert(s->staging, NB_F32, s->acc, NB_F64, cnt, s->stream));
        }
    }
    if (rq.kick) {
        HIPCHK(nb_launch_axpy(s->vel, s->acc, c.dt / 2, cnt, s->is_f64, s->stream));
        snprintf(res->site, sizeof res->site, "axpy");
    }
    s->logical[3] = A;
    s->have_acc = true;
    return NB_OK;
}

// This evaluation's grid (fp32 storage, HOOK_GRID): the maximum of r2 over all pairs, then the threshold / factor tables.
// tab->r2max_bits is 0 here: zeroed at creation, put back by grid_tables_kernel after each use.
//   tracked   after a seeding evaluation: the farthest pair of the predecessor gives the lower bound, so two launches
//             (filter, scan + tables) replace the search (exact either way, nb_grid.hip).  Single GPU or every rank
//             redundantly; not for comm-less shards, whose first evaluation is their only one.
//   small     the one-launch step's all-pairs pass; up to small_fuse_tables_max_n the same launch builds the tables
//             (measured, INT4: N = 1024 22.5 -> 18.6 us per step; N = 3000 30.8 vs 31.7: there the fused kernel's
//             arrival counter and longer source chunks cost more than the launch)
//   seeding   the pruned search (six launches, O(N) + candidates^2, no collective), else all pairs + max over the ranks
//             (the small step's evaluations above the fused size as well: one GPU, so its own block is every source)
int grid_prepare(nb_sim *s, const Eval &e, bool small)
{
    const nb_config &c = s->cfg;
    const int L = mode_levels(c);
    const float G = (float)c.G, min_val = 0.01f;
    if (L > NB_MAX_LUT || L < 2) return fail(NB_ERR_UNSUPPORTED, "grid levels must be in [2, %d] on the fused path (got %d)", NB_MAX_LUT, L);
    const bool track = !s->knobs.no_prune && !s->knobs.no_track && c.n > g_tune.track_min_n && !e.shard;
    if (track && s->prune_seeded) {
        HIPCHK(nb_launch_r2max_tracked((const float *)s->pos, c.n, c.dim, e.eps2, s->prune_cand, s->prune_idx, s->prune_state,
                                       s->tab, L, G, min_val, allow_fast(s), s->stream));
        if (L > NB_LUT_MIN)      // multi-block tables: the scan left the maximum in tab->r2max_bits
            HIPCHK(nb_launch_grid_tables(s->tab, L, G, e.eps2, min_val, nullptr, s->stream, allow_fast(s)));
        return NB_OK;
    }
    if (small && L <= NB_LUT_MIN && c.n <= g_tune.small_fuse_tables_max_n && !s->knobs.no_small_fuse) {
        HIPCHK(nb_launch_r2max_tables((const float *)s->pos, s->geom, c.dim, e.eps2, s->tab, L, G, min_val, allow_fast(s),
                                      s->stream));
        return NB_OK;
    }
    const bool prune = !small && !s->knobs.no_prune && (c.n > g_tune.prune_min_n || track);
    if (prune) {
        HIPCHK(nb_launch_r2max_pruned((const float *)s->pos, c.n, c.dim, e.eps2, s->prune_cand, s->prune_rho, s->prune_state,
                                      s->tab, s->stream));
    } else {
        ForceGeom gmax = s->geom;
        const bool scan_all = e.shard || (e.multi && g_pc.direct_only);
        if (scan_all) {   // a comm-less shard (and a rank without RCCL's max) scans every source itself
            gmax.j_begin = 0;
            gmax.j_end = c.n;
            gmax.nchunks = (c.n + gmax.chunk_len - 1) / gmax.chunk_len;
        }
        HIPCHK(nb_launch_r2max((const float *)s->pos, gmax, c.dim, e.eps2, s->tab, s->stream));
        if (e.multi && !scan_all)
            if (int rc = comm_allreduce_max_u32(s, &s->tab->r2max_bits)) return rc;
    }
    HIPCHK(nb_launch_grid_tables(s->tab, L, G, e.eps2, min_val, prune ? s->prune_state : nullptr, s->stream, allow_fast(s)));
    s->prune_seeded = prune;     // grid_tables_kernel seeded the tracked search from the pruned one's far pair
    return NB_OK;
}

// the pair sweep: partial sums into the slabs of the pair-symmetric plan, or into the one-sided kernels' source chunks
int launch_pairs(nb_sim *s, const EvalRequest &rq, const Eval &e)
{
    const nb_config &c = s->cfg;
    const auto &sp = s->sym;
    const bool grid = e.hook == HOOK_GRID;
    const int L = grid ? mode_levels(c) : 0;
    unsigned long long *bin_out = (rq.bins && grid) ? s->bin_out : nullptr;    // nb_quant_bin_sums: the same kernels, BINS = true
    int slot;
    if (!e.used_sym) {
        if (int rc = prof_begin(s, &slot)) return rc;
        if (s->is_f64)
            HIPCHK(nb_launch_force_f64((const double *)s->pos, (const double *)s->mass, s->partial, s->geom, c.dim, e.pair_dt,
                                       e.hook, c.G, c.softening_sq, e.eps2, s->stream));
        else
            HIPCHK(nb_launch_force_f32((const float *)s->pos, (const float *)s->mass, s->partial, s->geom, c.dim, e.hook,
                                       e.pair_dt, (float)c.G, e.eps2, s->tab, L, s->stream, bin_out));
        s->last_kernel = s->is_f64 ? "force_f64_kernel" : "force_f32_kernel";
        return prof_end(s, slot);
    }
    const int pa_f32 = s->is_f64 && e.pair_dt == NB_F32;
    if (!rq.packed_ready) {
        // the packed mass factor carries G, except in grid modes, whose table already does (simulation.py:101)
        const double gfac = s->is_f64 ? c.G : (grid ? 1.0 : (double)(float)c.G);
        HIPCHK(nb_launch_pack(s->pos, s->vel, s->acc, s->mass, sp.packed, c.n, sp.np, c.dim, s->is_f64, NB_PACK_NONE, 0.0, 0.0,
                              gfac, pa_f32, s->stream, 0, -1, 0, grid ? NB_FAR_OFF : NB_FAR_FORCE));
    }
    if (int rc = prof_begin(s, &slot, false)) return rc;
    if (s->is_f64) {
        HIPCHK(nb_launch_force_sym_f64((const double *)sp.packed, sp.work, sp.nwork, sp.rowslab, (double *)sp.colslab, sp.np,
                                       c.dim, sp.r, s->mass_uniform, pa_f32, c.softening_sq, s->stream, prof_events(s, slot),
                                       sp.rowsplit ? 1 : 0, s->knobs.sym_rot >= 0 ? s->knobs.sym_rot : NB_SYM_ROT_DEFAULT));
        s->last_kernel = "force_sym_kernel<double";
        return NB_OK;
    }
    // grid modes on the R = 2 tiling (N < 20 480: a few hundred short work items, one wave per SIMD): a step is bound by
    // the LATENCY of a sweep, and the general-mass kernel's four independent scalar pairs per rotation step hide the
    // log / exp chains better than the packed uniform kernel does (measured INT8 / INT4 us per step, uniform vs general:
    // N = 6000 61.7 / 55.1 vs 48.3 / 47.6, N = 12 000 100 vs 88; N = 20 000 equal; N = 65 536 0.83 vs 1.24 ms)
    const bool uniform = grid ? (s->mass_uniform && sp.r != 2) : e.sym_uniform;
    if (bin_out)
        HIPCHK(nb_launch_force_sym_f32_bins((const float *)sp.packed, sp.work, sp.nwork, sp.rowslab, (float *)sp.colslab, sp.np,
                                            c.dim, sp.r, uniform, e.eps2, s->tab, (float)c.G, (float)s->mass_value, L, bin_out,
                                            c.n, s->stream));
    else
        HIPCHK(nb_launch_force_sym_f32((const float *)sp.packed, sp.work, sp.nwork, sp.rowslab, (float *)sp.colslab, sp.np,
                                       c.dim, sp.r, uniform, e.hook, e.eps2, s->tab, (float)c.G, (float)s->mass_value, L,
                                       s->stream, prof_events(s, slot)));
    s->last_kernel = "force_sym_kernel<float";
    return NB_OK;
}

// the reduction of the partial sums with every kick it can carry (none before a collective), then the sum over the
// ranks through one of three carriers: the direct xGMI all-reduce (the reduction writes the buffer the peers read), the
// exchange of fp64 sums (Eval::x64), or the in-place RCCL all-reduce of `acc`
int reduce_and_exchange(nb_sim *s, const EvalRequest &rq, Eval &e, EvalResult *res)
{
    const nb_config &c = s->cfg;
    const int64_t cnt = nd(s);
    const bool p2p = e.multi && (e.x64 ? p2p_use_x64(s, cnt) : p2p_use(s, cnt));
    // a bin read-out (nb_quant_bin_sums) is an observer: its sums go to the staging buffer, never over the accelerations
    // the next opening kick reads
    void *red_out = p2p ? nb_p2p_data() : (rq.bins ? s->staging : s->acc);
    if (e.x64 && !p2p && !s->sums64) HIPCHK(hipMalloc((void **)&s->sums64, (size_t)cnt * sizeof(double)));
    double *sums64 = e.x64 ? (p2p ? (double *)nb_p2p_data() : s->sums64) : nullptr;
    if (p2p)
        if (int rc = p2p_claim_buffer(s)) return rc;
    const bool fuse_kick = rq.kick && !e.multi && !e.fq;
    // inside nb_step the reduction also opens the next step (one launch fewer per step, which is what small systems
    // are bound by) and, on the pair-symmetric path, repacks its positions
    int kmode = kick_mode(fuse_kick, rq.open_next);
    if (rq.open_on_read && !(fuse_kick && e.used_sym))
        return fail(NB_ERR_INVALID, "internal: a step started from speculative positions needs the kick-fusing pair-symmetric reduction");
    if (!e.used_sym) {
        HIPCHK(nb_launch_reduce(s->partial, s->geom.nchunks, cnt, red_out, s->is_f64, s->vel, c.dt / 2, kmode, s->pos, c.dt,
                                s->stream));
        site_set(res, "reduce", kmode);
    } else {
        const auto &sp = s->sym;
        // uniform-mass kernels leave out the mass factor: G*m in T arithmetic (fp32: (float)G * m)
        if (e.sym_uniform) e.scale = s->is_f64 ? c.G * s->mass_value : (double)((float)c.G * (float)s->mass_value);
        // the last step of a native call leaves the NEXT step's drifted positions in pos_alt and `packed`; a call that
        // starts from them applies its opening kick on read -- a Python loop of step() then costs force + reduction
        // per tick, no pack launch (see step_run)
        const bool spec = kmode == NB_KICK_CLOSE && rq.spec_next && !grid_mode(c.mode);
        if (spec) {
            if (!s->pos_alt) HIPCHK(hipMalloc(&s->pos_alt, (size_t)cnt * (s->is_f64 ? 8 : 4)));
            kmode = NB_KICK_CLOSE_SPEC;
        }
        if (rq.open_on_read) kmode |= NB_KICK_OPEN_ON_READ;
        HIPCHK(nb_launch_reduce_sym(sp.rowslab, sp.colslab, sp.row_slot0, sp.row_nslots, sp.col_upto, sp.tile_b, c.n, sp.np,
                                    c.dim, s->is_f64, e.scale, red_out, s->vel, c.dt / 2, kmode, s->pos, sp.packed, c.dt,
                                    s->stream, 0, -1, sums64, e.red_mm ? s->scalars + 8 : nullptr, s->pos_alt,
                                    grid_mode(c.mode) ? NB_FAR_OFF : NB_FAR_FORCE));
        site_set(res, "reduce_sym", kmode);
        if (spec) { s->spec_open = true; s->spec_kind = 2; s->spec_dt = c.dt; }
    }
    e.kicked = fuse_kick;
    res->opened = (kmode & NB_KICK_MODE_MASK) == NB_KICK_CLOSE_OPEN;
    if (p2p) {
        // every rank holds every summed element inside this kernel: the kicks (and, inside nb_step, the next step's
        // opening kick + drift + repack) ride along as they do in the single-GPU reduction -- no pack launch
        NbP2PKick kk{};
        kk.scale = e.scale;
        if (e.x64) kk.f64_to_f32 = 1;     // (force quantisation follows: its finish launch carries the kicks)
        else if (rq.kick && !e.fq && !s->knobs.no_p2p_kick) {
            kk.mode = kick_mode(true, rq.open_next);
            kk.dim = c.dim; kk.np = e.used_sym ? s->sym.np : 0;
            kk.vel = s->vel; kk.pos = s->pos; kk.packed = e.used_sym ? (void *)s->sym.packed : nullptr;
            kk.half_dt = c.dt / 2; kk.dt = c.dt;
            kk.far_lim = nb_far_limit(grid_mode(c.mode) ? NB_FAR_OFF : NB_FAR_FORCE, s->is_f64);
            e.kicked = true;
            res->opened = rq.open_next;
        }
        HIPCHK(nb_p2p_allreduce(s->acc, (size_t)cnt, s->is_f64 || e.x64, p2p_step_timeout_s(), s->stream, &kk));
        if (kk.mode != NB_KICK_NONE) site_set(res, "p2p", kk.mode);
        s->used_p2p = true;
    } else if (e.x64) {
        if (int rc = comm_allreduce_sum(s, s->sums64, (size_t)cnt, true)) return rc;
        HIPCHK(nb_launch_finish_sums64(s->sums64, e.scale, (float *)s->acc, cnt, s->stream));
    } else if (e.multi) {
        if (int rc = comm_allreduce_sum(s, s->acc, (size_t)cnt, s->is_f64)) return rc;
    }
    return NB_OK;
}

// min / max of the summed forces, then quantisation with the closing kick (and, inside nb_step, the next step's
// opening kick + drift) in the same launch
int force_quant_finish(nb_sim *s, const EvalRequest &rq, Eval &e, EvalResult *res)
{
    const nb_config &c = s->cfg;
    const int km = kick_mode(rq.kick, rq.open_next);
    if (e.red_mm)
        HIPCHK(nb_launch_force_quant_finish((float *)s->acc, nd(s), mode_levels(c), s->scalars + 8, (c.n + 63) / 64, s->scalars,
                                            s->fbins, (float *)s->vel, (float *)s->pos, c.dt / 2, c.dt, km, s->stream,
                                            (float *)s->sym.packed, s->sym.np, c.dim));
    else
        HIPCHK(nb_launch_force_quant_step((float *)s->acc, nd(s), mode_levels(c), s->scalars, s->scalars + 8, s->fbins,
                                          (float *)s->vel, (float *)s->pos, c.dt / 2, c.dt, km,
                                          e.used_sym ? (float *)s->sym.packed : nullptr, s->sym.np, c.dim, s->stream));
    const bool packed = km == NB_KICK_CLOSE_OPEN && e.used_sym;
    site_set(res, "fq_finish", km, packed ? (e.red_mm ? ",packed,red_mm" : ",packed") : (e.red_mm ? ",red_mm" : ""));
    e.kicked = rq.kick;
    res->opened = rq.open_next;
    return NB_OK;
}

}  // namespace

// one evaluation of simulation.py:74-118 and the leapfrog work the request asks for (EvalRequest / EvalResult, nb_state.h)
int force_eval(nb_sim *s, EvalRequest rq, EvalResult *result)
{
    if (!s->have_pos || !s->have_mass) return fail(NB_ERR_INVALID, "positions and masses must be set first");
    rq.open_next = rq.kick && rq.open_next;      // the next step is opened by the launch that closes this one
    EvalResult unread;
    EvalResult *res = result ? result : &unread;
    *res = EvalResult{};
    Eval e = resolve_eval(s);
    if (e.multi && !s->comm) return fail(NB_ERR_COMM, "nranks > 1 but nb_comm_init was not called");
    if (e.multi)
        if (int rc = comm_check(s)) return rc;
    if (e.shard && rq.kick) return fail(NB_ERR_INVALID, "NB_FLAG_NO_COMM handles cannot step");
    if (e.generic) return force_eval_generic(s, rq, e, res);
    s->last_generic = false;
    // the bins are decided in the pair loop: a read-out stops at the sums (reduce_and_exchange sends them to the staging
    // buffer) and leaves the force bounds, the force bins and the accelerations' dtype to the evaluation they belong to
    if (rq.bins) e.fq = e.red_mm = false;
    if (e.hook == HOOK_GRID)
        if (int rc = grid_prepare(s, e, false)) return rc;
    if (int rc = launch_pairs(s, rq, e)) return rc;
    if (int rc = reduce_and_exchange(s, rq, e, res)) return rc;
    if (e.fq)
        if (int rc = force_quant_finish(s, rq, e, res)) return rc;
    if (rq.kick && !e.kicked) {
        // no launch could carry the closing kick (RCCL all-reduce in between)
        if (rq.may_defer) res->deferred = true;
        else {
            HIPCHK(nb_launch_axpy(s->vel, s->acc, s->cfg.dt / 2, nd(s), s->is_f64, s->stream));
            snprintf(res->site, sizeof res->site, "axpy");
        }
    }
    if (rq.bins) return NB_OK;
    s->logical[3] = acc_logical_dtype(s);
    s->have_acc = true;
    return NB_OK;
}

namespace {

// ---- small systems: one launch per step (nb_small.hip) ---------------------------------------------------------
bool small_ok(const nb_sim *s)
{
    const nb_config &c = s->cfg;
    const int sdt = s->is_f64 ? NB_F64 : NB_F32;
    // fp32 storage: above 3072 the tiled path is ahead (measured us per step with 512 x 64 workgroups, one launch vs
    // tiled: FLOAT32 N = 3300 13.2 / 10.8, 3584 13.5 / 11.0, 4096 14.7 / 13.3; INT8 3584 33.2 / 35.7, 4096 35.3 / 36.5 and
    // INT4 3840 37.2 / 34.3, 4096 42.3 / 43.8 -- within the run-to-run spread of the max-r2 search; up to 3072 one
    // launch wins or ties everywhere); fp64 keeps it to 4096 (15.7 against 18.9)
    const int nmax = s->knobs.small_max > 0 ? s->knobs.small_max : (s->is_f64 ? g_tune.small_max_f64 : g_tune.small_max_f32);
    if (s->knobs.no_smalln || c.n > nmax || comm_active(s) || c.nranks != 1 || !s->have_acc) return false;
    if (grid_mode(c.mode) && (s->is_f64 || mode_levels(c) > NB_LUT_MIN || mode_levels(c) < 2)) return false;
    if (s->is_f64 != (c.mode == NB_FLOAT64)) return false;           // fp64 state under a cast mode: tuned one-sided kernel
    // masses: fp32-typed masses in an fp64 run enter the fp64 product exactly (no rounding of their own); half-typed
    // masses round the product to the half type and stay on the tuned kernels
    const bool mass_ok = s->logical[2] == sdt || (s->is_f64 && s->logical[2] == NB_F32);
    return settled(s) && mass_ok;
}

// the remaining `nsteps` steps of an nb_step call; `opened`: this step's opening kick + drift was already applied
int step_small(nb_sim *s, int nsteps, bool opened, bool first)
{
    const nb_config &c = s->cfg;
    const size_t el = s->is_f64 ? 8 : 4;
    const bool grid = grid_mode(c.mode);
    const Eval e = resolve_eval(s);
    const bool fq = e.fq;
    if (!s->pos_alt) HIPCHK(hipMalloc(&s->pos_alt, (size_t)nd(s) * el));
    if (fq && !s->small_part) HIPCHK(hipMalloc((void **)&s->small_part, 2 * (size_t)c.n * sizeof(double)));
    const int hook = mode_hook(c.mode);
    const int lanes = s->knobs.small_lanes ? s->knobs.small_lanes : nb_small_lanes(c.n);
    // A step() loop driven from Python is one nb_step(1) per tick: the last step of a call leaves the next step's
    // drifted positions in pos_alt (NB_KICK_CLOSE_SPEC); if nothing wrote state or dt since, this call takes them and applies
    // its opening kick on read -- one launch per tick instead of two (FLOAT32 us per step() call: N = 1024 9.9 -> 5.6, N = 3000 12.6 -> 10.8;
    // profiles/r03_python_step_overhead.txt)
    const bool speculate = !grid && !fq && !s->knobs.no_spec;
    bool open_on_read = false;
    if (!opened) {
        if (speculate && s->spec_open && s->spec_kind == 1 && s->spec_dt == c.dt) {
            std::swap(s->pos, s->pos_alt);
            open_on_read = true;
            path_note(s, first ? 0 : 1, "spec_read");
        } else {
            HIPCHK(nb_launch_kick_drift(s->pos, s->vel, s->acc, c.dt / 2, c.dt, nd(s), s->is_f64, s->stream));
            path_note(s, first ? 0 : 1, "kick_drift");
        }
    }
    s->spec_open = false;
    EvalResult note;
    for (int t = 0; t < nsteps; ++t) {
        const bool last = (t + 1 == nsteps);
        if (grid)
            if (int rc = grid_prepare(s, e, true)) return rc;
        // INT8 / INT4: the forces are snapped to their grid (and the kicks applied) by the finish launch
        const int closing = kick_mode(true, !last);
        const int kick = fq ? NB_KICK_NONE : ((last && speculate ? NB_KICK_CLOSE_SPEC : closing) |
                                              ((t == 0 && open_on_read) ? NB_KICK_OPEN_ON_READ : 0));
        int slot;
        if (int rc = prof_begin(s, &slot)) return rc;
        HIPCHK(nb_launch_small_step(s->pos, s->pos_alt, s->vel, s->acc, s->mass, c.n, c.dim, s->is_f64, hook, c.G,
                                    c.softening_sq, c.dt / 2, c.dt, kick, lanes, s->stream, grid ? s->tab : nullptr,
                                    fq ? s->small_part : nullptr));
        if (int rc = prof_end(s, slot)) return rc;
        site_set(&note, fq ? "fq_finish" : "small", fq ? closing : kick, fq ? ",small" : "");
        path_note(s, last ? 2 : 1, note.site);
        if (fq)      // one min / max pair per workgroup of the force launch
            HIPCHK(nb_launch_force_quant_finish((float *)s->acc, nd(s), mode_levels(c), s->small_part,
                                                nb_small_blocks(c.n, lanes), s->scalars, s->fbins,
                                                (float *)s->vel, (float *)s->pos, c.dt / 2, c.dt, closing, s->stream));
        else if (!last)
            std::swap(s->pos, s->pos_alt);
    }
    if (speculate) { s->spec_open = true; s->spec_kind = 1; s->spec_dt = c.dt; }
    s->last_kernel = "small_step_kernel";
    s->last_generic = false;
    return NB_OK;
}

}  // namespace

// `nsteps` leapfrog steps (simulation.py:120-143): v += a dt/2; x += v dt; a = force(x); v += a dt/2.
int step_run(nb_sim *s, int nsteps)
{
    EvalResult prev;                // what the previous step's evaluation left: .deferred, its closing kick; .opened: it did
                                    // this step's opening kick + drift (and, on the symmetric path, the repack)
    bool open_on_read = false;      // this call starts from the previous call's speculative positions (tiled path)
    path_clear(s);
    for (int t = 0; t < nsteps; ++t) {
        // small systems with settled dtypes: one launch per step
        if (!prev.deferred && small_ok(s)) return step_small(s, nsteps - t, prev.opened, t == 0);
        if (t == 0 && s->spec_open && s->spec_kind == 2 && s->spec_dt == s->cfg.dt && s->sym.enabled && !comm_active(s) &&
            !force_quant_mode(s->cfg) && !grid_mode(s->cfg.mode) && s->pos_alt && settled(s)) {
            std::swap(s->pos, s->pos_alt);        // positions after this step's drift; `packed` holds them as well
            prev.opened = open_on_read = true;
            path_note(s, 0, "spec_read");
        }
        s->spec_open = false;
        // opening kick + drift; on the pair-symmetric path the repack rides in the same launch
        const bool uniform_dt = settled(s);
        const bool fuse_pack = s->sym.enabled && uniform_dt && !grid_mode(s->cfg.mode);
        if (prev.opened) {
            // nothing to launch: positions and velocities were advanced by the previous reduction
        } else if (fuse_pack) {
            HIPCHK(nb_launch_pack(s->pos, s->vel, s->acc, s->mass, s->sym.packed, s->cfg.n, s->sym.np, s->cfg.dim,
                                  s->is_f64, prev.deferred ? NB_PACK_CLOSE_OPEN : NB_PACK_OPEN, s->cfg.dt / 2, s->cfg.dt,
                                  s->is_f64 ? s->cfg.G : (double)(float)s->cfg.G, 0, s->stream));
            path_note(s, t == 0 ? 0 : 1, prev.deferred ? "pack:2" : "pack:1");
        } else {
            const char *site = "";
            if (prev.deferred) {
                if (int rc = launch_plain_kick(s, false, &site)) return rc;
                path_note(s, 1, site);
            }
            if (int rc = launch_plain_kick(s, true, &site)) return rc;
            path_note(s, t == 0 ? 0 : 1, site);
        }
        // packed positions are current when this step's pack launch wrote them, or when the previous evaluation
        // opened this step on the symmetric path (its reduction / quantisation repacked them)
        EvalRequest rq;
        rq.kick = true;
        rq.packed_ready = prev.opened ? s->sym.enabled : fuse_pack;
        s->logical[1] = promote(s->logical[1], s->logical[3]);
        s->logical[0] = promote(s->logical[0], s->logical[1]);
        // a closing kick no launch of the evaluation can carry is folded into the next step's opening launch, if there is one
        rq.may_defer = (t + 1 < nsteps) && fuse_pack;
        rq.open_next = (t + 1 < nsteps) && uniform_dt;
        rq.open_on_read = (t == 0) && open_on_read;
        rq.spec_next = (t + 1 == nsteps) && uniform_dt && s->sym.enabled && !s->knobs.no_spec;
        if (int rc = force_eval(s, rq, &prev)) return rc;
        path_note(s, t + 1 < nsteps ? 1 : 2, prev.site);      // (nothing when the closing kick was deferred)
        s->logical[1] = promote(s->logical[1], s->logical[3]);
    }
    return NB_OK;
}

static const char *dtype_name(int dt)
{
    switch (dt) {
    case NB_F16: return "f16";
    case NB_BF16: return "bf16";
    case NB_F32: return "f32";
    default: return "f64";
    }
}

int energy_eval(nb_sim *s, double *kinetic, double *potential)
{
    const nb_config &c = s->cfg;
    double host[2] = {0, 0};
    bool pe_uniform = false;
    const int hp_v = is_half(s->logical[1]) ? s->logical[1] : -1;   // NB_F16 == 0: "none" is -1
    const int hp_x = is_half(s->logical[0]) ? s->logical[0] : -1;
    if (kinetic) {
        if (!s->have_vel || !s->have_mass) return fail(NB_ERR_INVALID, "velocities/masses not set");
        HIPCHK(nb_launch_kinetic(s->vel, s->mass, c.n, c.dim, s->is_f64, s->logical[1] != NB_F64, hp_v, s->logical[2], s->scratch,
                                 s->scalars + 2, s->stream));
    }
    if (potential) {
        if (!s->have_pos || !s->have_mass) return fail(NB_ERR_INVALID, "positions/masses not set");
        const auto &sp = s->sym;
        const bool pe_sym = sp.enabled && hp_x < 0 && (sp.r == 2 || sp.r == 4) && (size_t)sp.nwork <= s->scratch_elems &&
                            !s->knobs.no_pe_sym;
        if (pe_sym) {
            // same tile-pair work list as the force kernel; `packed` is scratch between force evaluations
            // uniform masses: no mass factor in the pair loop; m * m (rounded like upstream's masses[i] * masses[j], in the
            // masses' dtype) multiplies the finished sum below
            pe_uniform = s->mass_uniform;
            if (s->spec_kind == 2) s->spec_open = false;      // `packed` (the speculative next positions with it) is rewritten here
            HIPCHK(nb_launch_pack(s->pos, s->vel, s->acc, s->mass, sp.packed, c.n, sp.np, c.dim, s->is_f64, 0, 0.0, 0.0,
                                  1.0, s->is_f64 && s->logical[0] != NB_F64, s->stream, 0, -1, pe_uniform ? 1 : 0, NB_FAR_PE));
            HIPCHK(nb_launch_potential_sym(sp.packed, sp.work, sp.nwork, s->scratch, sp.np, c.dim, sp.r, s->is_f64,
                                           s->logical[0] != NB_F64, s->logical[2], c.softening_sq, pe_uniform ? 1 : 0,
                                           s->stream));
            HIPCHK(nb_launch_final_sum(s->scratch, sp.nwork, s->scalars + 3, s->stream));
            // the instantiation nb_launch_potential_sym picks (fp32 storage: always fp32 terms); the narrow-mass
            // sweep (masses carried as float) and the row-split items are branches of their own
            const bool f32t = !s->is_f64 || s->logical[0] != NB_F64;
            const bool narrow_mass = s->is_f64 && !f32t && !pe_uniform && s->logical[2] != NB_F64;
            snprintf(s->pe_kernel, sizeof s->pe_kernel, "potential_sym_kernel<%s,%d,%d,f32t=%d,uniform=%d%s%s%s>",
                     s->is_f64 ? "double" : "float", c.dim, sp.r, f32t ? 1 : 0, pe_uniform ? 1 : 0,
                     narrow_mass ? ",mass=" : "", narrow_mass ? dtype_name(s->logical[2]) : "", sp.rowsplit ? ",rowsplit" : "");
        } else {
            HIPCHK(nb_launch_potential(s->pos, s->mass, s->geom, c.dim, s->is_f64, s->logical[0] != NB_F64,
                                       s->logical[2], hp_x, c.softening_sq,
                                       (float)round_dt(hp_x >= 0 ? hp_x : NB_F32, c.softening_sq), s->scratch,
                                       s->scalars + 3, s->stream));
            // nb_launch_potential: fp32 storage and half-typed positions always take fp32 pair arithmetic; fp64 pair
            // arithmetic rounds the mass product to the masses' dtype when they are typed narrower (run-time branch)
            const bool pa_f32 = !s->is_f64 || s->logical[0] != NB_F64 || hp_x >= 0;
            const bool narrow_mass = !pa_f32 && s->logical[2] != NB_F64;
            snprintf(s->pe_kernel, sizeof s->pe_kernel, "potential_kernel<%s,%d,pa_f32=%d,hp=%s%s%s>",
                     s->is_f64 ? "double" : "float", c.dim, pa_f32 ? 1 : 0, hp_x >= 0 ? dtype_name(hp_x) : "none",
                     narrow_mass ? ",mass=" : "", narrow_mass ? dtype_name(s->logical[2]) : "");
        }
        if (comm_active(s)) {
            if (!s->comm) return fail(NB_ERR_COMM, "nranks > 1 but nb_comm_init was not called");
            if (int rc = comm_allreduce_sum(s, s->scalars + 3, 1, true)) return rc;
        }
    }
    HIPCHK(hipMemcpyAsync(host, s->scalars + 2, 2 * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (int rc = p2p_check(s)) return rc;
    if (kinetic) {
        // ke = 0.5 * (masses * v_sq).sum() in the promoted dtype of (velocities, masses)
        const int t = promote(s->logical[1], s->logical[2]);
        *kinetic = round_dt(t, round_dt(t, 0.5) * round_dt(t, host[0]));
    }
    if (potential) {
        const int t = promote(s->logical[0], s->logical[2]);
        if (pe_uniform) host[1] *= round_dt(s->logical[2], s->mass_value * s->mass_value);
        // -G * sum: a Python scalar MULTIPLYING a half tensor stays in float (torch opmath; only added scalars are
        // rounded to the tensor's dtype first)
        *potential = round_dt(t, round_dt(is_half(t) ? NB_F32 : t, -c.G) * round_dt(t, host[1]));
        // the reference multiplies by the triu mask before dividing by dist (simulation.py:189): the masked
        // entries are 0 / dist = NaN where dist == 0, i.e. on the whole diagonal when the softening rounds to
        // zero in the positions' dtype (softening 0; 1e-4 with float16 positions).  dist > 0 otherwise.
        if (c.n > 0 && round_dt(s->logical[0], c.softening_sq) == 0.0) *potential = std::nan("");
    }
    return NB_OK;
}

// Quant-bin read-out (nb_quant_bin_sums).  Runs the evaluation once more on the CURRENT positions with the BINS
// instantiation of whichever grid-mode pair loop the production path uses here -- same launch sequence up to the sums
// (max-r2, tables, uniform / general pair of launches, reduction), same control flow inside the pair loop -- and returns,
// per particle p, s1 = sum_q k(p, q) and s2 = sum_q k(p, q) ((q mod 65521) + 1) over ALL q including p itself (the
// reference's N x N bin matrix has k = 0 on the diagonal).
// An observer: the sums land in the staging buffer and there is no force quantisation, so the accelerations (the tiled
// path sums in another order than the small step: its values differ in the last bits), their dtype, the force bins and
// bounds, last_kernel and the tracked search's seed flag are what the last evaluation left.  The grid tables are rebuilt
// from the same positions (the same values); the tracked search's candidate state moves on as under any evaluation.
int bin_sums_eval(nb_sim *s, int which, int64_t *sum_k, int64_t *sum_kw, double info[8])
{
    const nb_config &c = s->cfg;
    if (s->comm) return fail(NB_ERR_UNSUPPORTED, "quant-bin read-out: not on a handle with a communicator (single GPU or NB_FLAG_NO_COMM shards)");
    if (use_generic(s)) return fail(NB_ERR_UNSUPPORTED, "quant-bin read-out: this evaluation runs on the generic per-pair path");
    const int L = mode_levels(c);
    if (L < 2 || L > NB_MAX_LUT) return fail(NB_ERR_UNSUPPORTED, "grid levels must be in [2, %d] on the fused path (got %d)", NB_MAX_LUT, L);
    const size_t words = 2 * (size_t)c.n + 2;
    if (!s->bin_out) HIPCHK(hipMalloc((void **)&s->bin_out, words * sizeof(unsigned long long)));
    HIPCHK(hipMemsetAsync(s->bin_out, 0, words * sizeof(unsigned long long), s->stream));
    const bool last_small = strcmp(s->last_kernel, "small_step_kernel") == 0;
    const bool want_small = which == 2 || (which == 0 && last_small);
    const bool seeded = s->prune_seeded;
    const char *const last_kernel = s->last_kernel;
    int path = 0, shape = 0;
    if (want_small) {
        if (!small_ok(s)) return fail(NB_ERR_INVALID, "quant-bin read-out: the one-launch small-system step does not apply to this handle "
                                                      "(size, dtypes, or no step taken yet)");
        // what step_small launches for one step, force only (do_kick = 0), forces into the staging buffer
        const int lanes = s->knobs.small_lanes ? s->knobs.small_lanes : nb_small_lanes(c.n);
        if (!s->pos_alt) HIPCHK(hipMalloc(&s->pos_alt, (size_t)nd(s) * 4));
        const int rc = grid_prepare(s, resolve_eval(s), true);
        s->prune_seeded = seeded;
        if (rc) return rc;
        HIPCHK(nb_launch_small_step(s->pos, s->pos_alt, s->vel, s->staging, s->mass, c.n, c.dim, 0, HOOK_GRID, c.G, c.softening_sq,
                                    c.dt / 2, c.dt, NB_KICK_NONE, lanes, s->stream, s->tab, nullptr, s->bin_out));
        path = 3;
        shape = lanes;
    } else {
        EvalRequest rq;
        rq.bins = true;
        const int rc = force_eval(s, rq);
        // a search the read-out seeded is run again by the next evaluation: the flag stays the last evaluation's
        s->prune_seeded = seeded;
        const bool sym = strncmp(s->last_kernel, "force_sym_kernel", 16) == 0;
        s->last_kernel = last_kernel;                // the read-out does not change what the last evaluation ran on
        if (rc) return rc;
        path = sym ? 1 : 2;
        shape = sym ? s->sym.r : 0;
    }
    std::vector<unsigned long long> host(words);
    GridTables *ht = new GridTables;
    hipError_t e = hipMemcpyAsync(host.data(), s->bin_out, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ht, s->tab, sizeof(GridTables), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    const int fast_ok = ht->fast_ok, degenerate = ht->degenerate;
    delete ht;
    HIPCHK(e);
    if (degenerate) return fail(NB_ERR_UNSUPPORTED, "quant-bin read-out: degenerate grid (lmax - lmin < 1e-10): values pass through, no bins");
    for (int i = 0; i < c.n; ++i) { sum_k[i] = (int64_t)host[i]; sum_kw[i] = (int64_t)host[(size_t)c.n + i]; }
    if (info) {
        info[0] = path;                   // 1 pair-symmetric tiles, 2 one-sided tiles, 3 one-launch small-system kernel
        info[1] = shape;                  // targets per lane (1) / lanes per target (3)
        // the uniform-mass packed kernel did the work (pair-symmetric path; the same rule force_eval applies)
        info[2] = (path == 1 && s->mass_uniform && s->sym.r != 2) ? 1 : 0;
        info[3] = fast_ok;                // the tables enabled the table-free pair path
        info[4] = (double)host[2 * (size_t)c.n];        // pair evaluations binned by the table-free estimate alone
        info[5] = (double)host[2 * (size_t)c.n + 1];    // pair evaluations binned through a threshold table
        info[6] = L;
        info[7] = 0;
    }
    return NB_OK;
}

int prof_collect(nb_sim *s, double *total_ms, int32_t *launches)
{
    HIPCHK(hipStreamSynchronize(s->stream));
    for (int i = 0; i < s->prof_count; ++i) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, s->ev_start[i], s->ev_stop[i]));
        s->prof_total_ms += ms;
    }
    s->prof_launches += s->prof_count;
    s->prof_count = 0;
    if (total_ms) *total_ms = s->prof_total_ms;
    if (launches) *launches = s->prof_launches;
    s->prof_total_ms = 0;
    s->prof_launches = 0;
    return NB_OK;
}

}  // namespace nbhost
