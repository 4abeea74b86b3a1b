// nb_grid.hip -- the bounds of the quantisation grid: which grid does this force evaluation use?
//
// The grid hook (quantization.py:91-127) needs the maximum of r2 over all pairs and, from it, the threshold / value / factor
// tables the pair loops read:
//   * the three exact searches for the fp32 maximum of r2: all pairs (r2max_kernel), pruned (prune_*_kernel), tracked
//     (track_*_kernel);
//   * the tables (grid_tables_body in named phases), alone or run by the last workgroup of a search (r2max_tables_kernel,
//     ens_r2max_tables_kernel, track_scan_kernel);
//   * the tensor-level _grid_quantize_safe through the same tables, and the d2bins read-out.
// Shared rules, one copy each: block_reduce_t0 / last_block_arrives (nb_device.h), prune_need (the distance bound of both
// pruning searches), prune_rearm (PruneState back to rest).  Two block maxima stay hand-written, each with a note:
// track_finish's (key with payload) and the tables' maxdev / maxrel pair (one barrier for both).  The three walks over a staged
// tile (r2max_block, prune_scan_kernel, track_scan_kernel) stay written out: as one function they compiled differently.
#include "nb_device.h"
#include "nb_dispatch.h"

#include <cstddef>

namespace {

using namespace nbdev;

// ------------------------------------------------------------------------------------------
// K2: global max of the fp32 r2 over (all targets) x (this rank's sources).
// quantization.py:113 needs log(max r2); the minimum is analytic (diagonal).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned int r2_order_bits(float v)
{
    // r2 >= 0 always, so the IEEE bit pattern orders like an unsigned int; any NaN maps above +inf
    return (v != v) ? 0x7fc00000u : __float_as_uint(v);
}

// all-pairs max of the fp32 r2 over this workgroup's targets and source chunk; thread 0 adds it to tab->r2max_bits
// SPLIT > 1 (small systems, R = 1): SPLIT neighbouring lanes share a target and deal a tile's sources among them --
// a thread then walks NB_TJ / SPLIT sources instead of NB_TJ, and there are SPLIT times as many workgroups.
template <int D, int R, int SPLIT = 1>
__device__ __forceinline__ void r2max_block(const float *__restrict__ pos, const ForceGeom &g, float eps2,
                                            GridTables *__restrict__ tab)
{
    static_assert(SPLIT == 1 || R == 1, "lane splitting is for one target per thread");
    __shared__ float sj[D][NB_TJ];
    __shared__ unsigned int s_red[NB_BLOCK / 64];
    const int tid = threadIdx.x;
    const int ibase = blockIdx.x * (NB_BLOCK * R / SPLIT);
    const int sub = tid % SPLIT;

    float xi[R][D];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int i = ibase + r * NB_BLOCK + tid / SPLIT;
        i = i < g.n ? i : g.n - 1;
#pragma unroll
        for (int k = 0; k < D; ++k) xi[r][k] = pos[(size_t)i * D + k];
    }
    const int j_lo = g.j_begin + blockIdx.y * g.chunk_len;
    const int j_hi = min(j_lo + g.chunk_len, g.j_end);

    unsigned int best = 0;
    for (int jt = j_lo; jt < j_hi; jt += NB_TJ) {
        // r2 is symmetric: source tiles entirely below this block's targets are covered by the
        // mirrored pairs of another block (block-uniform test, so the barriers stay matched)
        if (jt + NB_TJ <= ibase) continue;
        {
            int j = jt + tid;
            j = j < j_hi ? j : j_hi - 1;
#pragma unroll
            for (int k = 0; k < D; ++k) sj[k][tid] = pos[(size_t)j * D + k];
        }
        __syncthreads();
        const int cnt = min(NB_TJ, j_hi - jt);
#pragma unroll 8
        for (int jj = sub; jj < cnt; jj += SPLIT) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float d[D];
#pragma unroll
                for (int k = 0; k < D; ++k) d[k] = __fsub_rn(sj[k][jj], xi[r][k]);
                best = max(best, r2_order_bits(r2_f32_exact<D>(d, eps2)));
            }
        }
        __syncthreads();
    }
    // one atomic per block
    block_reduce_t0<MaxOp, NB_BLOCK / 64>(best, s_red, [&](unsigned int b) { atomicMax(&tab->r2max_bits, b); });
}

template <int D, int R>
__global__ void __launch_bounds__(NB_BLOCK)
r2max_kernel(const float *__restrict__ pos, ForceGeom g, float eps2, GridTables *__restrict__ tab)
{
    r2max_block<D, R>(pos, g, eps2, tab);
}

// ------------------------------------------------------------------------------------------
// K2 with pruning.  The pair with the largest r2 lies on the outside of the particle cloud, so a brute-force scan of all
// N^2 pairs is wasteful.  Candidates passing the test of prune_need are compacted and scanned exhaustively with the exact r2 formula.
// For a disk galaxy this keeps a few percent of the particles (~0.1 % of the pairs).
// ------------------------------------------------------------------------------------------
constexpr float NB_F32_MAX = 3.402823466e+38f;    // !(|v| <= NB_F32_MAX): v is NaN or infinite

// The distance bound of the pruned and of the tracked search: a particle i can belong to a pair with a larger r2 than the
// real pair (g, h) only if rho_i * (1 + 1e-5) >= prune_need(pos, g, h, rho_bound).
// Exactness argument (all quantities fp32; s = dx*dx + dy*dy [+ dz*dz] is r2 before eps2 is added, s_f32_exact):
//   * c = bounding-box centre, rho_i = |x_i - c|; for any pair dist(a,b) <= rho_a + rho_b <= rho_a + rho_max;
//   * (g, h) = a real pair found by two farthest-point hops (far -> g -> h), s_gh its s, LB = s_gh + eps2 its r2;
//   * fp32 addition of eps2 is monotone, so a pair whose r2 is strictly larger than LB has s > s_gh: its distance is
//     at least sqrt(s_gh), and both of its members satisfy rho >= sqrt(s_gh) - rho_max;
//   * a pair that only ties with LB need not be found: (g, h) attains the same fp32 value, and g and h always pass the
//     test with their own s_gh (rho_g >= dist(g,h) - rho_h >= sqrt(s_gh) - rho_max).  So finite input never leaves the
//     candidate list empty.
// The margins (1e-5 on each of sqrt(s_gh), rho_i and rho_max) cover the ~2e-7 relative rounding of s and of the rhos.
// They are RELATIVE to quantities that are measured directly: the bound is not sqrt(LB - eps2), whose subtraction
// returns s_gh +- half an ulp of eps2 -- far more than any margin once the softening dwarfs the cloud (a cloud of
// radius 1e-3 softenings used to lose every candidate).
// Non-finite input: a NaN or infinite coordinate makes the diagonal of torch's r2 matrix NaN (inf - inf), so the
// maximum is NaN (nan_flag).  Finite coordinates whose squares overflow leave s_gh or rho_max infinite: no bound to be had
// (inf - inf), so the result is 0, which every particle passes (rho >= 0, +inf included), and the scan covers all pairs
// (the maximum is +inf, as torch's).  A NaN rho fails the test against 0 as against any bound; it occurs only together
// with nan_flag, and with that flag set neither scan looks at the candidate list.
// rho_bound: the measured rho_max (pruned search) or the assumed bound rho_M on it (tracked search, see there).
template <int D>
__device__ __forceinline__ float prune_need(const float *__restrict__ pos, int g, int h, float rho_bound)
{
    float d[D];
#pragma unroll
    for (int k = 0; k < D; ++k) d[k] = __fsub_rn(pos[(size_t)h * D + k], pos[(size_t)g * D + k]);
    const float s_pair = s_f32_exact<D>(d);            // the pair's squared separation WITHOUT eps2
    const bool keep_all = !(s_pair <= NB_F32_MAX) || !(rho_bound <= NB_F32_MAX);
    return keep_all ? 0.0f : sqrtf(s_pair) * (1.0f - 1e-5f) - rho_bound * (1.0f + 1e-5f);
}

// The one place that lists every scratch field of PruneState and puts it back to rest (nb_api.cpp's initial state: the box
// keys at their identities, everything else 0) behind a finished search, and seeds the tracked search of the next
// evaluation: its far pair, the assumed bound on rho with the measured maximum it grew from, and whether it may run.
// Called by one thread once every other workgroup is done with *ps.  The pruned search (through the tables' last
// workgroup) dirties box_min / box_max / far / lb / count / nan_flag; the tracked search (track_finish) dirties rho_cur /
// count / nan_flag / best_i / best_j / scan_done and finds the box, far and lb fields at rest already.  c stays: it is
// the tracked searches' fixed centre, not scratch.
__device__ __forceinline__ void prune_rearm(PruneState *__restrict__ ps, int pair_i, int pair_j, float rho_m, float rho_prev,
                                            int seeded)
{
    ps->pair_i = pair_i;
    ps->pair_j = pair_j;
    ps->rho_m = rho_m;
    ps->rho_prev = rho_prev;
    ps->seeded = seeded;
    ps->rho_cur = 0u;
    ps->scan_done = 0u;
    ps->best_i = ps->best_j = 0ull;
    for (int c = 0; c < 3; ++c) { ps->box_min[c] = 0xffffffffu; ps->box_max[c] = 0u; }
    ps->far = ps->lb[0] = ps->lb[1] = 0ull;
    ps->count = 0;
    ps->nan_flag = 0;
}

// Stage 1 of the bounding box: per-block min/max of every coordinate (+ a flag for NaN / infinite ones) as ordered
// integer keys folded with atomics; the rho kernel decodes them (two launches, a few us each).
__device__ __forceinline__ unsigned int order_key(float v)
{
    const unsigned int u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);      // monotone in v for all finite values
}
__device__ __forceinline__ float order_unkey(unsigned int k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

template <int D>
__global__ void __launch_bounds__(NB_BLOCK)
prune_bbox_kernel(const float *__restrict__ pos, int n, PruneState *__restrict__ ps)
{
    __shared__ unsigned int s_mn[D][NB_BLOCK / 64], s_mx[D][NB_BLOCK / 64];
    __shared__ int s_nan;
    if (threadIdx.x == 0) s_nan = 0;
    __syncthreads();
    unsigned int mn[D], mx[D];
#pragma unroll
    for (int k = 0; k < D; ++k) { mn[k] = 0xffffffffu; mx[k] = 0u; }
    bool bad = false;
    for (int i = blockIdx.x * NB_BLOCK + threadIdx.x; i < n; i += gridDim.x * NB_BLOCK)
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const float v = pos[(size_t)i * D + k];
            bad |= !(fabsf(v) <= NB_F32_MAX);              // NaN or +-inf
            const unsigned int key = order_key(v);
            mn[k] = min(mn[k], key);
            mx[k] = max(mx[k], key);
        }
    if (bad) s_nan = 1;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        block_reduce_t0<MinOp, NB_BLOCK / 64>(mn[k], s_mn[k], [&](unsigned int a) { atomicMin(&ps->box_min[k], a); });
        block_reduce_t0<MaxOp, NB_BLOCK / 64>(mx[k], s_mx[k], [&](unsigned int b) { atomicMax(&ps->box_max[k], b); });
    }
    if (threadIdx.x == 0 && s_nan) atomicOr(&ps->nan_flag, 1);      // (behind the reductions' barriers: every thread's s_nan is in)
}

// one atomic per block instead of one per wave
__device__ __forceinline__ void block_atomic_max_u64(unsigned long long key, unsigned long long *dst)
{
    __shared__ unsigned long long s_key[NB_BLOCK / 64];
    block_reduce_t0<MaxOp, NB_BLOCK / 64>(key, s_key, [&](unsigned long long m) { if (m) atomicMax(dst, m); });
}

template <int D>
__global__ void __launch_bounds__(NB_BLOCK)
prune_rho_kernel(const float *__restrict__ pos, int n, float *__restrict__ rho, PruneState *__restrict__ ps)
{
    const int i = blockIdx.x * NB_BLOCK + threadIdx.x;
    unsigned long long key = 0ull;
    if (i == 0) {            // the centre stays put for the tracked searches that follow (PruneState::c)
#pragma unroll
        for (int k = 0; k < D; ++k) ps->c[k] = 0.5f * order_unkey(ps->box_min[k]) + 0.5f * order_unkey(ps->box_max[k]);
    }
    if (i < n) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const float c = 0.5f * order_unkey(ps->box_min[k]) + 0.5f * order_unkey(ps->box_max[k]);
            const float d = pos[(size_t)i * D + k] - c;
            s += d * d;
        }
        const float r = sqrtf(s);
        rho[i] = r;
        key = ((unsigned long long)__float_as_uint(r) << 32) | (unsigned int)i;
    }
    block_atomic_max_u64(key, &ps->far);
}

// farthest partner (by the exact fp32 r2) of the particle whose index is stored in *src_key
template <int D>
__global__ void __launch_bounds__(NB_BLOCK)
prune_hop_kernel(const float *__restrict__ pos, int n, float eps2, const unsigned long long *__restrict__ src_key,
                 unsigned long long *__restrict__ dst_key)
{
    const int f = (int)(*src_key & 0xffffffffull);
    const int j = blockIdx.x * NB_BLOCK + threadIdx.x;
    unsigned long long key = 0ull;
    if (j < n) {
        float d[D];
#pragma unroll
        for (int k = 0; k < D; ++k) d[k] = __fsub_rn(pos[(size_t)j * D + k], pos[(size_t)f * D + k]);
        key = ((unsigned long long)r2_order_bits(r2_f32_exact<D>(d, eps2)) << 32) | (unsigned int)j;
    }
    block_atomic_max_u64(key, dst_key);
}

template <int D>
__global__ void __launch_bounds__(NB_BLOCK)
prune_compact_kernel(const float *__restrict__ pos, const float *__restrict__ rho, int n, float *__restrict__ cand,
                     PruneState *__restrict__ ps)
{
    const int i = blockIdx.x * NB_BLOCK + threadIdx.x;
    if (i >= n) return;
    // the second hop's pair g -> h (indices in the low words of lb[0] / lb[1]) against the measured rho_max
    const float need = prune_need<D>(pos, (int)(ps->lb[0] & 0xffffffffull), (int)(ps->lb[1] & 0xffffffffull),
                                     __uint_as_float((unsigned int)(ps->far >> 32)));
    if (rho[i] * (1.0f + 1e-5f) >= need) {
        const int slot = atomicAdd(&ps->count, 1);
#pragma unroll
        for (int k = 0; k < D; ++k) cand[(size_t)slot * D + k] = pos[(size_t)i * D + k];
    }
}

// exhaustive exact max over the compacted candidates (count read on the device)
template <int D>
__global__ void __launch_bounds__(NB_BLOCK)
prune_scan_kernel(const float *__restrict__ cand, float eps2, const PruneState *__restrict__ ps,
                  GridTables *__restrict__ tab)
{
    __shared__ float sj[D][NB_TJ];
    __shared__ unsigned int s_red[NB_BLOCK / 64];
    const int m = ps->count;
    const int tid = threadIdx.x;
    const int ibase = blockIdx.x * NB_BLOCK;
    if (ps->nan_flag) {                          // a NaN / infinite coordinate: torch's max() would be NaN
        if (blockIdx.x == 0 && tid == 0) atomicMax(&tab->r2max_bits, 0x7fc00000u);
        return;
    }
    if (ibase >= m) return;                      // block-uniform
    const int i = min(ibase + tid, m - 1);
    float xi[D];
#pragma unroll
    for (int k = 0; k < D; ++k) xi[k] = cand[(size_t)i * D + k];
    unsigned int best = 0;
    for (int jt = ibase; jt < m; jt += NB_TJ) {  // r2 is symmetric: tiles below the block are mirrored elsewhere
        {
            const int j = min(jt + tid, m - 1);
#pragma unroll
            for (int k = 0; k < D; ++k) sj[k][tid] = cand[(size_t)j * D + k];
        }
        __syncthreads();
        const int cnt = min(NB_TJ, m - jt);
#pragma unroll 8
        for (int jj = 0; jj < cnt; ++jj) {
            float d[D];
#pragma unroll
            for (int k = 0; k < D; ++k) d[k] = __fsub_rn(sj[k][jj], xi[k]);
            best = max(best, r2_order_bits(r2_f32_exact<D>(d, eps2)));
        }
        __syncthreads();
    }
    block_reduce_t0<MaxOp, NB_BLOCK / 64>(best, s_red, [&](unsigned int b) { atomicMax(&tab->r2max_bits, b); });
}

// ------------------------------------------------------------------------------------------
// Grid tables: exact scalar form of _grid_quantize_safe (quantization.py:91-127) evaluated on
// the device once per force evaluation.  Every stage (clamp, log, -lmin, /range, *(L-1), round)
// is monotone in r2, so the bin index is a step function of the fp32 r2: thread k finds the
// smallest fp32 value whose bin is >= k by bisection over bit patterns.  Bit-identical to
// evaluating the formula per pair, with no log/div/exp in the pair loop.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float logf_cr(float t) { return (float)log((double)t); }

__device__ __forceinline__ float grid_bin_exact(float t, float min_val, float lmin, float range, float lm1)
{
    const float ts = (t < min_val) ? min_val : t;
    const float lt = logf_cr(ts);
    const float nrm = __fmul_rn(__fdiv_rn(__fsub_rn(lt, lmin), range), lm1);
    return rintf(nrm);   // half-to-even like torch.round
}

// The same bin for a t within ~1e-5 (relative) of a point c whose fp64 logarithm is known (c = exp(c_log): the result
// of exp carries the same 1e-16 the library log of t would): log t = c_log + log1p(u), u = (t - c) / c, three terms
// of the series (u^4 / 4 < 1e-21).  A dozen fp64 operations instead of a library log (~1400 cycles for a lone wave);
// the threshold search spends all its evaluations inside such a bracket.
__device__ __forceinline__ float grid_bin_near(float t, double c_log, double c_inv, float lmin, float range, float lm1)
{
    const double u = __builtin_fma((double)t, c_inv, -1.0);
    const double l1p = u * (1.0 + u * (-0.5 + u * (1.0 / 3.0)));
    const float lt = (float)(c_log + l1p);
    const float nrm = __fmul_rn(__fdiv_rn(__fsub_rn(lt, lmin), range), lm1);
    return rintf(nrm);
}

// what every phase of the tables body reads: the grid's bounds and the parameters of the pair loop's bin estimate
struct TableBounds {
    float min_val, r2max, tmin, tmax;       // clamp, the evaluation's maximum, the clamped diagonal / maximum
    float lmin, lmax, range, lm1;           // their logarithms, lmax - lmin, levels - 1
    bool degenerate;
    float est_a, est_b, est_bc;             // bin estimate log2(r2) * est_a + est_b; est_bc: centred on bin kc
    bool est_ok;
    int kc;                                 // the middle bin
};

// Phase 1: the value / factor / threshold of this thread's level (k: its level, tables_blocks: workgroups that share the
// levels), into *tab and into the workgroup's LDS copies s_lut / s_thr; s_lg2: log2 of the first / last factor.
__device__ __forceinline__ void tables_entries(GridTables *__restrict__ tab, int levels, float G, const TableBounds &b, int k,
                                               int tables_blocks, float *s_lut, float *s_thr, double *s_lg2)
{
    const float min_val = b.min_val, r2max = b.r2max, tmin = b.tmin, tmax = b.tmax;
    const float lmin = b.lmin, range = b.range, lm1 = b.lm1;
    // Small single-block tables (INT4, CUSTOM 64): the value / factor of a level and its threshold are independent
    // chains of comparable length, so they go to different lanes (threads [0, L) and [128, 128 + L)).
    const bool two_roles = tables_blocks == 1 && levels <= NB_LUT_MIN / 2;
    const int tid_l = threadIdx.x;
    const int ka = two_roles ? (tid_l < levels ? tid_l : -1) : (k < levels ? k : -1);
    const int kb = two_roles ? ((tid_l >= NB_LUT_MIN / 2 && tid_l - NB_LUT_MIN / 2 < levels) ? tid_l - NB_LUT_MIN / 2 : -1) : ka;
    const int base_l = two_roles ? 0 : (k - tid_l);          // first level of this workgroup
    if (ka >= 0) {
        // value of bin k (quantization.py:121-127) and its force factor (simulation.py:97-101)
        float v = __fdiv_rn((float)ka, lm1);
        v = __fmul_rn(v, range);
        v = __fadd_rn(v, lmin);
        float q = (float)exp((double)v);
        q = (q < min_val) ? min_val : q;
        // q^1.5 correctly rounded to fp32: q * sqrt(q) in fp64 is good to 2 ulp of fp64, 2^-29 of an fp32 spacing
        const double qd = (double)q;
        const float p = (float)(qd * __dsqrt_rn(qd));
        const float w = __fmul_rn(__fdiv_rn(1.0f, p), G);
        tab->qval[ka] = q;
        tab->lut[ka] = w;
        s_lut[ka - base_l] = w;
        if (ka == 0) s_lg2[0] = log2((double)w);
        if (ka == levels - 1) s_lg2[1] = log2((double)w);
    }
    if (kb >= 0) {
        const int k = kb;
        float thr = -__builtin_inff();
        if (k > 0 && !b.degenerate) {
            if (r2max != r2max) {
                thr = __builtin_nanf("");
            } else {
                unsigned int lo = __float_as_uint(tmin);   // bin(tmin) == 0 < k
                unsigned int hi = __float_as_uint(tmax);   // bin(tmax) == L-1 >= k
                // The edge of bin k sits near exp(lmin + (k - 1/2) range / (L-1)): bracket it within +-4e-6
                // (~70 fp32 values; the fp32 roundings of the reference's formula move the edge by ~1e-6 at most)
                // when both ends check out with the exact formula, so the bisection needs ~7 instead of ~31
                // evaluations; otherwise keep the full interval.  The result is the
                // same either way (bin is monotone in t).
                bool near = false;          // both ends of the bracket hold: every further t is within 4e-6 of `edge`
                double edge = 1.0, edge_log = 0.0, edge_inv = 1.0;
                if (range > 1e-6f) {
                    edge_log = (double)lmin + ((double)k - 0.5) * (double)range / (double)lm1;
                    edge = exp(edge_log);
                    edge_inv = 1.0 / edge;
                    const float a_lo = (float)(edge * (1.0 - 4e-6)), a_hi = (float)(edge * (1.0 + 4e-6));
                    const bool in_lo = a_lo > tmin && a_lo < tmax, in_hi = a_hi > tmin && a_hi < tmax;
                    const bool ok_lo = in_lo && grid_bin_near(a_lo, edge_log, edge_inv, lmin, range, lm1) < (float)k;
                    const bool ok_hi = in_hi && grid_bin_near(a_hi, edge_log, edge_inv, lmin, range, lm1) >= (float)k;
                    if (ok_lo) lo = __float_as_uint(a_lo);
                    if (ok_hi) hi = __float_as_uint(a_hi);
                    near = ok_lo && ok_hi;
                }
                while (hi - lo > 1u) {
                    const unsigned int mid = lo + ((hi - lo) >> 1);
                    const float bin = near ? grid_bin_near(__uint_as_float(mid), edge_log, edge_inv, lmin, range, lm1)
                                           : grid_bin_exact(__uint_as_float(mid), min_val, lmin, range, lm1);
                    if (bin >= (float)k) hi = mid; else lo = mid;
                }
                thr = __uint_as_float(hi);
            }
        }
        tab->thr[k] = thr;
        s_thr[k - base_l] = thr;
    }
}

// Phase 3 (thread 0): log2 of the force factor is affine in the bin index: fit it to the table's end points, into
// s_par = {slope, fraction of the middle bin's log2, its integer part}.  Returns whether the table-free path is still on.
__device__ __forceinline__ bool fast_path_fit(int levels, int kc, bool fast_try, const float *s_lut, const double *s_lg2,
                                              float *s_par)
{
    const double w0 = (double)s_lut[0], w1 = (double)s_lut[min(levels, NB_LUT_MIN) - 1];
    double c1 = 0.0, cm = 0.0;
    if (fast_try && w0 > 0.0 && w1 > 0.0 && w0 < 1e30 && w1 < 1e30) {
        c1 = (s_lg2[1] - s_lg2[0]) / (double)(levels - 1);
        cm = s_lg2[0] + c1 * (double)kc;            // log2 of the factor of the middle bin
    } else {
        fast_try = false;
    }
    const double tm = rint(cm);
    if (!(fabs(tm) < 100.0) || !(fabs(c1) * (double)levels < 100.0)) fast_try = false;
    s_par[0] = (float)c1;
    s_par[1] = (float)(cm - tm);
    s_par[2] = (float)tm;
    return fast_try;
}

// Phase 4 (block-uniform, all threads): the deviation of the estimate at this thread's bin edge and of the fitted factor
// from its table entry, folded into *maxdev / *maxrel (0 on entry) over the workgroup.  s_red: 16 floats.
__device__ __forceinline__ void fast_path_check(int levels, int k, const TableBounds &b, const float *s_thr, const float *s_lut,
                                                const float *s_par, float *s_red, float *maxdev, float *maxrel)
{
    float my_dev = 0.0f, my_rel = 0.0f;
    if (k < levels) {
        // the estimate exactly as the pair loop evaluates it, on both sides of the lower edge of bin k
        if (k > 0) {
            const float r = s_thr[k], rp = __uint_as_float(__float_as_uint(r) - 1u);
            const float edge = (float)(k - b.kc) - 0.5f;
            const float e1 = __builtin_fmaf(__builtin_amdgcn_logf(r), b.est_a, b.est_bc) - edge;
            const float e0 = __builtin_fmaf(__builtin_amdgcn_logf(rp), b.est_a, b.est_bc) - edge;
            my_dev = fmaxf(fabsf(e1), fabsf(e0));
            if (!(my_dev == my_dev)) my_dev = 1.0f;
        }
        const float wf = __builtin_amdgcn_exp2f(__builtin_fmaf((float)(k - b.kc), s_par[0], s_par[1]));
        const float wt = ldexpf(s_lut[k], -(int)s_par[2]);
        my_rel = fabsf(wf - wt) / wt;
        if (!(my_rel == my_rel)) my_rel = 1.0f;
    }
    // both maxima by wave shuffles + one exchange through LDS, hand-written: two block_reduce_t0 calls put a second barrier
    // and a second fold on the serial tail of every grid evaluation, +0.2 to 0.4 us per step (profiles/grid_refactor_timing.txt)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        my_dev = fmaxf(my_dev, __shfl_xor(my_dev, off, 64));
        my_rel = fmaxf(my_rel, __shfl_xor(my_rel, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { s_red[threadIdx.x >> 6] = my_dev; s_red[8 + (threadIdx.x >> 6)] = my_rel; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NB_LUT_MIN / 64; ++w) { *maxdev = fmaxf(*maxdev, s_red[w]); *maxrel = fmaxf(*maxrel, s_red[8 + w]); }
}

// Phase 6 (thread 0): the scalars of the tables, and the arrival counter and the maximum back to rest.
__device__ __forceinline__ void tables_publish(GridTables *__restrict__ tab, int levels, const TableBounds &b, bool fast_try,
                                               float maxdev, float maxrel, const float *s_par)
{
    tab->blocks_done = 0u;
    // sentinel above the last bin: NaN compares false, so a lookup can never step past L-1
    tab->thr[levels] = __builtin_nanf("");
    // fast bin estimate for the pair loop: n ~ log2(r2) * a + b with a = ln2*(L-1)/range.
    // v_log_f32 is good to ~1e-6 absolute, so for a < 1e4 the estimate is within 0.01 bins of the
    // exact (monotone) formula and rint() of it is off by at most one bin, which two threshold
    // compares repair exactly.  Narrow grids (a >= 1e4) keep the binary search.
    tab->est_a = b.est_a;
    tab->est_b = b.est_b;
    tab->use_est = b.est_ok ? 1 : 0;
    tab->lmin = b.lmin;
    tab->lmax = b.lmax;
    tab->range = b.range;
    tab->r2max = b.r2max;
    tab->degenerate = (b.range < 1e-10f) ? 1 : 0;
    tab->levels = levels;
    tab->uniform_ok = (tab->use_est && b.r2max < 1e30f) ? 1 : 0;   // false for NaN / inf r2max too
    // v_log_f32 is good to 1 ulp of its result; inside a bin the estimate can therefore dip below its value at
    // the bin's lower edge by 2 * a * ulp (taken twice here) plus the rounding of the fma (half an ulp of L)
    const float lmag = fmaxf(fabsf(__builtin_amdgcn_logf(b.tmin)), fabsf(__builtin_amdgcn_logf(b.tmax)));
    const float ulp_log = __uint_as_float((__float_as_uint(fmaxf(lmag, 1.0f)) & 0x7f800000u)) * 1.1920929e-7f;
    const float ulp_ne = __uint_as_float((__float_as_uint((float)levels) & 0x7f800000u)) * 1.1920929e-7f;
    // ... and the pair loop's estimate takes r2 from fused multiply-adds: within 4 ulp (4.8e-7 relative, 6.9e-7 in
    // log2) of the reference's separately rounded r2
    const float eta = 4.0f * b.est_a * ulp_log + ulp_ne + 8.0e-7f * b.est_a;
    const float delta = 2.0f * (maxdev + eta);
    tab->fast_ok = (fast_try && delta < 0.05f && maxrel <= 2.0e-6f) ? 1 : 0;
    tab->sure_lim = 0.5f - delta;
    tab->kc = b.kc;
    tab->tm = (int)s_par[2];
    tab->est_bc = b.est_bc;
    tab->c1 = s_par[0];
    tab->c0c = s_par[1];
    tab->fast_maxdev = maxdev;
    tab->fast_maxrel = maxrel;
    tab->r2max_bits = 0u;      // consumed (every thread read it on entry): ready for the next atomicMax round
}

// One thread per level, NB_LUT_MIN threads per block; the block that arrives last (all others have read
// tab->r2max_bits and written their entries) writes the scalars and resets the scratch for the next evaluation.
// FUSED: called by the last workgroup of r2max_tables_kernel (single-block tables, levels <= NB_LUT_MIN; the
// caller passes the finished maximum).  Otherwise the body of grid_tables_kernel (one workgroup per NB_LUT_MIN levels):
// `chunks` workgroups share the levels -- 0: the launch's gridDim.x; the batched ens_tables_wide_kernel passes the member's own.
// Phases: tables_entries -> last_block_arrives -> fast_path_fit -> fast_path_check -> prune_rearm -> tables_publish.
template <bool FUSED>
__device__ __forceinline__ void grid_tables_body(GridTables *__restrict__ tab, int levels, float G, float eps2, float min_val,
                                                 PruneState *__restrict__ ps, int allow_fast, unsigned int r2max_bits,
                                                 const double *__restrict__ bounds = nullptr, int chunks = 0)
{
    if (bounds) {                  // tensor-level hook: minimum / maximum of the tensor, found on the device
        eps2 = (float)bounds[0];
        r2max_bits = __float_as_uint((float)bounds[1]);
    }
    __shared__ int s_fast;
    __shared__ float s_thr[NB_LUT_MIN], s_lut[NB_LUT_MIN], s_red[NB_LUT_MIN], s_par[4];
    __shared__ double s_lg2[2];          // log2 of the first / last factor, taken by their own threads (off the serial tail)
    const int k = (FUSED ? 0 : blockIdx.x) * NB_LUT_MIN + threadIdx.x;
    const unsigned int nblocks = chunks ? (unsigned int)chunks : gridDim.x;      // (non-FUSED) workgroups that share the levels
    const int tables_blocks = FUSED ? 1 : nblocks;
    TableBounds b;
    b.min_val = min_val;
    b.r2max = __uint_as_float(r2max_bits);
    b.tmin = (eps2 < min_val) ? min_val : eps2;        // diagonal entries: r2 == eps2
    b.tmax = (b.r2max < min_val) ? min_val : b.r2max;
    // the two correctly rounded logarithms head every thread's dependency chain: even lanes take one, odd lanes the
    // other, and neighbours swap (all 256 threads are active here)
    const bool odd = (threadIdx.x & 1) != 0;
    const float lg_mine = logf_cr(odd ? b.tmax : b.tmin);
    const float lg_other = __shfl_xor(lg_mine, 1, 64);
    b.lmin = odd ? lg_other : lg_mine;
    b.lmax = odd ? lg_mine : lg_other;
    b.range = __fsub_rn(b.lmax, b.lmin);
    b.lm1 = (float)(levels - 1);
    b.degenerate = b.range < 1e-10f || levels > NB_MAX_LUT;

    tables_entries(tab, levels, G, b, k, tables_blocks, s_lut, s_thr, s_lg2);
    __syncthreads();               // every thread of this block has read tab->r2max_bits and written its entry
    if constexpr (!FUSED) {        // (single-block tables -- every grid up to 256 levels -- need no arrival count)
        if (nblocks > 1 && !last_block_arrives(&tab->blocks_done, nblocks)) return;
    }
    const bool fin = threadIdx.x == 0;
    // ---- table-free pair path: parameters + validation (single-block tables only: levels <= NB_LUT_MIN) ------
    const double est_a_d = 0.6931471805599453 * (double)b.lm1 / (double)b.range;
    b.est_a = (float)est_a_d;
    b.est_b = (float)(-(double)b.lmin * (double)b.lm1 / (double)b.range);
    b.est_ok = (b.range >= 1e-10f && est_a_d < 1.0e4);
    b.kc = levels / 2;
    b.est_bc = (float)(-(double)b.lmin * (double)b.lm1 / (double)b.range - (double)b.kc);
    bool fast_try = allow_fast && b.est_ok && tables_blocks == 1 && levels >= 2 && b.r2max == b.r2max && b.r2max < 1e30f;
    if (fin) s_fast = fast_path_fit(levels, b.kc, fast_try, s_lut, s_lg2, s_par) ? 1 : 0;
    __syncthreads();
    fast_try = s_fast != 0;
    float maxdev = 0.0f, maxrel = 0.0f;
    if (fast_try) fast_path_check(levels, k, b, s_thr, s_lut, s_par, s_red, &maxdev, &maxrel);
    if (fin && ps) {
        // the pruned max-r2 search is finished: seed the tracked search of the next evaluation with its far pair
        // (the second hop's pair g -> h is a real pair; the exact maximum is re-derived from the positions then) and reset its scratch
        prune_rearm(ps, (int)(ps->lb[0] & 0xffffffffull), (int)(ps->lb[1] & 0xffffffffull),
                    __uint_as_float((unsigned int)(ps->far >> 32)) * 1.005f, 0.0f, (ps->nan_flag == 0) ? 1 : 0);
    }
    if (fin) tables_publish(tab, levels, b, fast_try, maxdev, maxrel, s_par);
}

__global__ void __launch_bounds__(NB_LUT_MIN)
grid_tables_kernel(GridTables *__restrict__ tab, int levels, float G, float eps2, float min_val,
                   PruneState *__restrict__ ps, int allow_fast)
{
    grid_tables_body<false>(tab, levels, G, eps2, min_val, ps, allow_fast, tab->r2max_bits);
}

// ---- tensor-level _grid_quantize_safe (quantization.py:91-127) through the same tables ----------------------------
// The hook used to evaluate a library log twice and an exp once PER ELEMENT in fp64 (fp32 tensors: correctly rounded
// logf / expf) -- ~600 fp64 instructions per element, 200 us for a 4096 x 4096 tensor.  The bin of an element is a step
// function of its value, so: plain min / max of the tensor (log is monotone: lmin / lmax are the logs of the clamped
// extremes), the threshold / value tables for exactly these bounds (the kernel above, bounds read on the device),
// and one pass that looks every element's bin up (v_log_f32 estimate + two threshold compares, or the binary search
// for narrow grids) and writes the bin's value.  Non-finite bounds and a degenerate range keep the elementwise formula.
__global__ void __launch_bounds__(NB_LUT_MIN)
grid_tables_bounds_kernel(GridTables *__restrict__ tab, int levels, float min_val, const double *__restrict__ bounds)
{
    grid_tables_body<false>(tab, levels, 1.0f, 0.0f, min_val, nullptr, 0, 0u, bounds);
}

__global__ void __launch_bounds__(256)
grid_quantize_safe_tab_kernel(const float *__restrict__ in, float *__restrict__ out, int64_t count, int levels, float min_val,
                              const double *__restrict__ bounds, const GridTables *__restrict__ tab, int lp)
{
    extern __shared__ float s_tab[];
    float *s_thr = s_tab, *s_q = s_tab + lp + 1;
    const float mn = (float)bounds[0], mx = (float)bounds[1];
    const bool finite = fabsf(mn) < 1e30f && fabsf(mx) < 1e30f;          // false for NaN / inf as well
    if (!finite) {
        // the formula element by element, as torch evaluates it (NaN / inf propagate through lmin / lmax)
        const float tmin = (mn < min_val) ? min_val : mn, tmax = (mx < min_val) ? min_val : mx;
        const float lmin = (float)log((double)tmin), lmax = (float)log((double)tmax);
        const float range = __fsub_rn(lmax, lmin), lm1 = (float)(levels - 1);
        const bool passthrough = range < 1e-10f;
        for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < count; idx += (int64_t)gridDim.x * 256) {
            float v = in[idx];
            v = (v < min_val) ? min_val : v;
            if (!passthrough) {
                const float lt = (float)log((double)v);
                float x = __fmul_rn(__fdiv_rn(__fsub_rn(lt, lmin), range), lm1);
                const float k = rintf(x);
                x = __fadd_rn(__fmul_rn(__fdiv_rn(k, lm1), range), lmin);
                v = (float)exp((double)x);
                v = (v < min_val) ? min_val : v;
            }
            out[idx] = v;
        }
        return;
    }
    for (int k = threadIdx.x; k <= lp; k += 256) s_thr[k] = k <= levels ? tab->thr[k] : __builtin_inff();
    for (int k = threadIdx.x; k < levels; k += 256) s_q[k] = tab->qval[k];
    __syncthreads();
    if (threadIdx.x == 0) s_thr[levels] = __builtin_inff();      // the table's NaN sentinel would stop the binary search
    __syncthreads();
    const bool passthrough = tab->degenerate != 0;
    const bool use_est = tab->use_est != 0;
    const float est_a = tab->est_a, est_b = tab->est_b;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < count; idx += (int64_t)gridDim.x * 256) {
        float v = in[idx];
        v = (v < min_val) ? min_val : v;
        if (!passthrough) {
            const int k = use_est ? grid_bin_estimate(s_thr, v, est_a, est_b, levels - 1) : grid_bin_lookup(s_thr, v, lp);
            v = s_q[k];
        }
        out[idx] = v;
    }
}

// Small systems (one launch instead of two per grid evaluation): every workgroup adds its part of the all-pairs
// maximum; the LAST one to arrive (device-scope counter) reads the finished maximum and builds the tables.
constexpr int NB_R2MAX_SPLIT = 8;

// behind r2max_block, shared by the solo and the batched kernel: count this workgroup's arrival at *tab; the last of
// `arrivals` builds the tables from the finished maximum, the others return (*levels is read by the last only).  arrivals:
// the workgroups that call this for *tab in the launch -- gridDim.x * gridDim.y where every workgroup of a member works,
// the member's own count where some return before they get here (ens_r2max_tables_ragged_kernel).
// WIDE_OK (batched kernel): a grid above NB_LUT_MIN levels has multi-chunk tables, which ens_tables_wide_kernel builds from
// the maximum left in tab->r2max_bits -- the last workgroup only puts the arrival counter back for that launch.
template <bool WIDE_OK = false>
__device__ __forceinline__ void r2max_last_builds_tables(GridTables *tab, const int *levels, float G, float eps2,
                                                         float min_val, int allow_fast, unsigned int arrivals)
{
    static_assert(NB_BLOCK == NB_LUT_MIN, "the last workgroup runs the single-block tables code");
    __shared__ unsigned int s_bits;
    if (!last_block_arrives(&tab->blocks_done, arrivals)) return;
    if (WIDE_OK && *levels > NB_LUT_MIN) {
        if (threadIdx.x == 0) tab->blocks_done = 0u;
        return;
    }
    // the maximum itself through the same atomic unit that every workgroup's atomicMax went to
    if (threadIdx.x == 0) s_bits = atomicMax(&tab->r2max_bits, 0u);
    __syncthreads();
    grid_tables_body<true>(tab, *levels, G, eps2, min_val, nullptr, allow_fast, s_bits);
}

template <int D, int R>
__global__ void __launch_bounds__(NB_BLOCK)
r2max_tables_kernel(const float *__restrict__ pos, ForceGeom g, float eps2, GridTables *__restrict__ tab, int levels,
                    float G, float min_val, int allow_fast)
{
    r2max_block<D, R, NB_R2MAX_SPLIT>(pos, g, eps2, tab);
    r2max_last_builds_tables(tab, &levels, G, eps2, min_val, allow_fast, gridDim.x * gridDim.y);
}

// The same for the B members of an ensemble (nb_ens handles) in one launch: blockIdx.z is the member, blockIdx.x / .y its
// target block and source chunk as above, on the member's slice of the (B, N, D) positions.  Every member has its own
// GridTables (maximum, arrival counter, tables), its own eps2 and G (prm) and level count; the last workgroup OF A MEMBER to
// arrive builds that member's tables.  The maximum is exact and the tables a function of it alone (grid_tables_body), so
// they are the tables a solo evaluation of the member builds, however its workgroups were cut.  No workgroup waits for
// another.  A stopped member (nb_device.h) takes no further evaluation, its tables stay its last one's; all its workgroups
// return together (the test is on the member), so its arrival counter stays at rest.
template <int D, bool STOPS>
__global__ void __launch_bounds__(NB_BLOCK)
ens_r2max_tables_kernel(const float *__restrict__ pos, ForceGeom g, const EnsScalars<float> *__restrict__ prm,
                        GridTables *__restrict__ tabs, const int *__restrict__ levels, float min_val, int allow_fast,
                        const int *__restrict__ stop, int t)
{
    const int b = blockIdx.z;
    if (ens_ticks_left<STOPS>(stop, b, t) <= 0) return;
    GridTables *tab = tabs + b;
    const float G = prm[b].G, eps2 = prm[b].eps2;
    r2max_block<D, 1, NB_R2MAX_SPLIT>(pos + (size_t)b * g.n * D, g, eps2, tab);
    r2max_last_builds_tables<true>(tab, levels + b, G, eps2, min_val, allow_fast, gridDim.x * gridDim.y);
}

// The same for members of different sizes (nb_ens_create_ragged_grid; every member at most NB_LUT_MIN levels).  The launch
// grid and the source chunks are cut for the capacity g.n; member b owns the first sizes[b] rows of its slice, so its
// targets and its sources end at sizes[b].  A workgroup whose target block or source chunk starts at or beyond sizes[b]
// has no pair of the member: it returns before it touches the member's maximum or arrival counter.  The others are
// ceil(sizes[b] / targets per workgroup) * ceil(sizes[b] / chunk_len) -- the member's OWN arrival count, which the last of
// them is recognised by; no workgroup waits for another.  The maximum is exact, so maximum and tables are those of the
// member's solo run, and no padding row is read (r2max_block clamps targets and sources to the member's last star).
template <int D, bool STOPS>
__global__ void __launch_bounds__(NB_BLOCK)
ens_r2max_tables_ragged_kernel(const float *__restrict__ pos, ForceGeom g, const EnsScalars<float> *__restrict__ prm,
                               GridTables *__restrict__ tabs, const int *__restrict__ levels, float min_val, int allow_fast,
                               const int *__restrict__ stop, int t, const int *__restrict__ sizes)
{
    constexpr int PER_BLOCK = NB_BLOCK / NB_R2MAX_SPLIT;     // targets per workgroup (r2max_block)
    const int b = blockIdx.z;
    if (ens_ticks_left<STOPS>(stop, b, t) <= 0) return;
    const int n = sizes[b];
    if ((int)blockIdx.x * PER_BLOCK >= n || (int)blockIdx.y * g.chunk_len >= n) return;
    GridTables *tab = tabs + b;
    const float G = prm[b].G, eps2 = prm[b].eps2;
    const float *mine = pos + (size_t)b * g.n * D;           // (g.n: still the capacity, the stride of a slice)
    const unsigned int arrivals = (unsigned int)((n + PER_BLOCK - 1) / PER_BLOCK) * (unsigned int)((n + g.chunk_len - 1) / g.chunk_len);
    g.n = n;
    g.j_end = n;                                             // (j_begin = 0)
    r2max_block<D, 1, NB_R2MAX_SPLIT>(mine, g, eps2, tab);
    r2max_last_builds_tables(tab, levels + b, G, eps2, min_val, allow_fast, arrivals);
}

// The tables of the members above NB_LUT_MIN levels, behind ens_r2max_tables_kernel: blockIdx.y is the member, blockIdx.x
// one chunk of NB_LUT_MIN of its levels -- grid_tables_kernel's body with the member's own chunk count, so the entries, the
// NaN sentinel and the published scalars (fast_ok = 0: more than one chunk) are those of the member's solo run.  Workgroups
// of a member with single-block tables (built by the launch before), beyond a member's own chunks, or of a stopped member
// (whose maximum was not taken either) return at once.
template <bool STOPS>
__global__ void __launch_bounds__(NB_LUT_MIN)
ens_tables_wide_kernel(const EnsScalars<float> *__restrict__ prm, GridTables *__restrict__ tabs, const int *__restrict__ levels,
                       float min_val, int allow_fast, const int *__restrict__ stop, int t)
{
    const int b = blockIdx.y;
    const int L = levels[b];
    const int chunks = (L + NB_LUT_MIN - 1) / NB_LUT_MIN;
    if (L <= NB_LUT_MIN || L > NB_MAX_LUT || (int)blockIdx.x >= chunks) return;
    if (ens_ticks_left<STOPS>(stop, b, t) <= 0) return;
    GridTables *tab = tabs + b;
    grid_tables_body<false>(tab, L, prm[b].G, prm[b].eps2, min_val, nullptr, allow_fast, tab->r2max_bits, nullptr, chunks);
}

// ------------------------------------------------------------------------------------------
// Tracked max-r2 search (round 3): two launches per evaluation instead of six (+ tables).
// Exactness argument as for the pruned search above (prune_need), with the pair (g, h) being the far pair of the LAST evaluation,
// its s re-evaluated at the new positions (eps2 left out, as there), a fixed centre c, and rho_M = (last measured rho_max)
// + twice its last growth + 1e-4 of it as the bound on every rho: both members of a pair with a larger r2 satisfy
// rho >= sqrt(s_gh) - rho_M, and so do g and h themselves.  The filter pass
// measures the actual rho_max; if it exceeds rho_M (a particle left the margin) the scan simply takes ALL particles
// -- slower, still exact.  NaN and infinite coordinates poison the maximum exactly as torch's max() does (the diagonal
// holds inf - inf); where s_gh or rho_M overflows on finite coordinates every particle is a candidate.
// ------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(NB_BLOCK)
track_filter_kernel(const float *__restrict__ pos, int n, float eps2, float *__restrict__ cand, int *__restrict__ cand_idx,
                    PruneState *__restrict__ ps)
{
    __shared__ float s_need;
    __shared__ unsigned int s_rho[NB_BLOCK / 64];
    __shared__ int s_nan;
    if (threadIdx.x == 0) {
        s_need = prune_need<D>(pos, ps->pair_i, ps->pair_j, ps->rho_m);     // the far pair against the assumed bound
        s_nan = 0;
    }
    __syncthreads();
    const int i = blockIdx.x * NB_BLOCK + threadIdx.x;
    unsigned int rb = 0u;
    if (i < n) {
        float x[D], s = 0.0f;
        bool bad = false;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            x[k] = pos[(size_t)i * D + k];
            bad |= !(fabsf(x[k]) <= NB_F32_MAX);           // NaN or +-inf
            const float d = x[k] - ps->c[k];
            s += d * d;
        }
        const float r = sqrtf(s);
        if (bad) s_nan = 1;
        else rb = __float_as_uint(r);              // r >= 0 (or +inf): bit patterns order like the values
        if (!bad && r * (1.0f + 1e-5f) >= s_need) {
            const int slot = atomicAdd(&ps->count, 1);
#pragma unroll
            for (int k = 0; k < D; ++k) cand[(size_t)slot * D + k] = x[k];
            cand_idx[slot] = i;
        }
    }
    block_reduce_t0<MaxOp, NB_BLOCK / 64>(rb, s_rho, [&](unsigned int m) {
        atomicMax(&ps->rho_cur, m);
        if (s_nan) atomicOr(&ps->nan_flag, 1);
    });
}

// Tail shared by the two tracked-search kernels: block maximum of the scanned pairs -> device-wide maximum (two 64-bit
// atomics per workgroup) -> the LAST workgroup to arrive publishes the maximum, prepares the next evaluation's search
// (far pair, rho bound with its margin, clean counters) and returns true with the maximum's order bits in *bits_out.
// m: particles scanned; rho_cur / nan_flag: measured by the filter pass of this evaluation.
__device__ __forceinline__ bool track_finish(unsigned long long best_i, unsigned long long best_j, int m, float eps2,
                                             unsigned int rho_cur, int nan_flag, PruneState *__restrict__ ps,
                                             unsigned long long *s_ki, unsigned long long *s_kj, unsigned int *bits_out)
{
    const int tid = threadIdx.x;
    {
        // block maximum, hand-written: the partner index is a payload that travels with the lane that holds the maximum,
        // and block_reduce_t0 folds single values
        unsigned long long ki = best_i, kj = best_j;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long oi = __shfl_xor(ki, off, 64), oj = __shfl_xor(kj, off, 64);
            if (oi > ki) { ki = oi; kj = oj; }
        }
        if ((tid & 63) == 0) { s_ki[tid >> 6] = ki; s_kj[tid >> 6] = kj; }
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long ki = s_ki[0], kj = s_kj[0];
#pragma unroll
        for (int w = 1; w < NB_BLOCK / 64; ++w)
            if (s_ki[w] > ki) { ki = s_ki[w]; kj = s_kj[w]; }
        if (ki) {
            // two independent maxima: on an exact tie of r2 they may name particles of different pairs -- harmless, the
            // pair only provides the next evaluation's lower bound, which is re-evaluated from the positions
            atomicMax(&ps->best_i, ki);
            atomicMax(&ps->best_j, kj);
        }
    }
    if (!last_block_arrives(&ps->scan_done, gridDim.x)) return false;
    if (tid == 0) {
        const unsigned long long fi = atomicMax(&ps->best_i, 0ull), fj = atomicMax(&ps->best_j, 0ull);
        unsigned int bits = (unsigned int)(fi >> 32);
        if (m <= 0) bits = 0u;
        if (nan_flag) bits = 0x7fc00000u;                     // a NaN / infinite coordinate: torch's max() would be NaN
        // a single particle (or none scanned): the diagonal pair r2 = eps2 is the maximum
        if (bits == 0u) bits = r2_order_bits(eps2);
        *bits_out = bits;
        // next evaluation: this maximum's pair (the last one's where nothing was scanned), the measured rho_max plus margin, clean
        // counters.  Margin for the next evaluation: twice the growth rho_max showed over this step (an escaper keeps its
        // speed) + 1e-4 relative; the first tracked evaluation has no growth figure yet and keeps 0.5 %
        const float rc = __uint_as_float(rho_cur);
        const float grow = (ps->rho_prev > 0.0f) ? fmaxf(rc - ps->rho_prev, 0.0f) : 0.0025f * rc;
        prune_rearm(ps, fi ? (int)(fi & 0xffffffffull) : ps->pair_i, fi ? (int)(fj & 0xffffffffull) : ps->pair_j,
                    rc + 2.0f * grow + 1e-4f * rc, rc, (nan_flag == 0) ? 1 : 0);
    }
    __syncthreads();               // *bits_out is the whole workgroup's
    return true;
}

constexpr int NB_TRACK_BLOCKS = 128;     // scan workgroups: every one ends in up to three same-address atomics (~17 ns each)

template <int D>
__global__ void __launch_bounds__(NB_BLOCK)
track_scan_kernel(const float *__restrict__ pos, const float *__restrict__ cand, const int *__restrict__ cand_idx, int n,
                  float eps2, PruneState *__restrict__ ps, GridTables *__restrict__ tab, int levels, float G, float min_val,
                  int allow_fast, int fuse_tables)
{
    static_assert(NB_BLOCK == NB_LUT_MIN, "the last workgroup runs the single-block tables code");
    __shared__ float sj[D][NB_TJ];
    __shared__ int sji[NB_TJ];
    __shared__ unsigned long long s_ki[NB_BLOCK / 64], s_kj[NB_BLOCK / 64];
    __shared__ unsigned int s_bits;
    const int tid = threadIdx.x;
    // the filter pass measured the real rho_max: inside the assumed bound the candidates are complete, else take everyone
    const bool valid = ps->rho_cur <= __float_as_uint(ps->rho_m);
    const int m = valid ? ps->count : n;
    const float *src = valid ? cand : pos;
    const int T = (m + NB_TJ - 1) / NB_TJ;
    const long long npairs = (long long)T * (T + 1) / 2;        // tile pairs (it <= jt), row-major
    unsigned long long best_i = 0ull, best_j = 0ull;
    for (long long p = blockIdx.x; p < npairs; p += gridDim.x) {
        // p -> (it, jt): rows of lengths T, T - 1, ...; first[it] = it * T - it * (it - 1) / 2
        const double tt = 2.0 * T + 1.0;
        int it = (int)((tt - sqrt(tt * tt - 8.0 * (double)p)) * 0.5);
        it = max(0, min(it, T - 1));
        while (it > 0 && (long long)it * T - (long long)it * (it - 1) / 2 > p) --it;
        while ((long long)(it + 1) * T - (long long)(it + 1) * it / 2 <= p) ++it;
        const int jt = it + (int)(p - ((long long)it * T - (long long)it * (it - 1) / 2));
        const int i = min(it * NB_TJ + tid, m - 1), j = min(jt * NB_TJ + tid, m - 1);
        float xi[D];
#pragma unroll
        for (int k = 0; k < D; ++k) xi[k] = src[(size_t)i * D + k];
        const int ii = valid ? cand_idx[i] : i;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < D; ++k) sj[k][tid] = src[(size_t)j * D + k];
        sji[tid] = valid ? cand_idx[j] : j;
        __syncthreads();
        const int cnt = min(NB_TJ, m - jt * NB_TJ);
        unsigned int best = 0u;
        int bj = 0;
#pragma unroll 8
        for (int jj = 0; jj < cnt; ++jj) {
            float d[D];
#pragma unroll
            for (int k = 0; k < D; ++k) d[k] = __fsub_rn(sj[k][jj], xi[k]);
            const unsigned int b = r2_order_bits(r2_f32_exact<D>(d, eps2));
            bj = b > best ? jj : bj;
            best = max(best, b);
        }
        const unsigned long long ki = ((unsigned long long)best << 32) | (unsigned int)ii;
        const unsigned long long kj = ((unsigned long long)best << 32) | (unsigned int)sji[bj];
        if (ki > best_i) { best_i = ki; best_j = kj; }
    }
    const bool mine = track_finish(best_i, best_j, m, eps2, ps->rho_cur, ps->nan_flag, ps, s_ki, s_kj, &s_bits);
    if (!mine) return;
    if (!fuse_tables) {
        if (tid == 0) tab->r2max_bits = s_bits;                  // the multi-block tables kernel follows
        return;
    }
    grid_tables_body<true>(tab, levels, G, eps2, min_val, nullptr, allow_fast, s_bits);
}

// debug / parity: bin index of every pair with the tables the force kernel used
template <int D>
__global__ void __launch_bounds__(NB_BLOCK)
d2bins_kernel(const float *__restrict__ pos, int n, float eps2, const GridTables *__restrict__ tab,
              int16_t *__restrict__ bins, int i0)
{
    const int j = blockIdx.x * NB_BLOCK + threadIdx.x;
    const int i = i0 + blockIdx.y;
    if (j >= n) return;
    float d[D];
#pragma unroll
    for (int k = 0; k < D; ++k) d[k] = __fsub_rn(pos[(size_t)j * D + k], pos[(size_t)i * D + k]);
    const float r2 = r2_f32_exact<D>(d, eps2);
    int b = -1;
    if (!tab->degenerate) {
        b = 0;
        for (int k = 1; k < tab->levels; ++k) b += (tab->thr[k] <= r2) ? 1 : 0;
    }
    bins[(size_t)(i - i0) * n + j] = (int16_t)b;
}

// Launch geometry of the fused max + tables kernels.  Every workgroup ends in two atomics on one address (they serialise
// in the L2: ~25 ns each), so about one workgroup per CU, counted over all `members`, is the right number: fewer, longer
// source chunks than the force kernels use -- at least one per member, at most max_chunks.  g: targets (n) and source
// range on entry, chunk_len / nchunks set on return.
dim3 r2max_tables_grid(ForceGeom &g, int members, int max_chunks)
{
    const int per_block = NB_BLOCK / NB_R2MAX_SPLIT;
    const int gx = (g.n + per_block - 1) / per_block;
    const int njr = g.j_end - g.j_begin > 0 ? g.j_end - g.j_begin : 1;
    int nch = 256 / (gx * members);
    nch = nch < 1 ? 1 : (nch > max_chunks ? max_chunks : nch);
    int chunk = (njr + nch - 1) / nch;
    chunk = (chunk + NB_TJ - 1) / NB_TJ * NB_TJ;
    g.chunk_len = chunk;
    g.nchunks = (njr + chunk - 1) / chunk;
    return dim3(gx, g.nchunks, members);
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
hipError_t nb_launch_r2max(const float *pos, const ForceGeom &g, int dim, float eps2, GridTables *tab,
                           hipStream_t st)
{
    // small systems (the only ones that take this path by default): one target per thread, four times the
    // workgroups
    const int r = g.n <= 8192 ? 1 : 4;
    const dim3 grid((g.n + NB_BLOCK * r - 1) / (NB_BLOCK * r), g.nchunks);
    return nb::pick<2, 3>(dim, [&](auto D) {
        return nb::pick<1, 4>(r, [&](auto R) {
            hipLaunchKernelGGL((r2max_kernel<D.value, R.value>), grid, dim3(NB_BLOCK), 0, st, pos, g, eps2, tab);
            return hipGetLastError();
        });
    });
}

hipError_t nb_launch_r2max_tables(const float *pos, const ForceGeom &g, int dim, float eps2, GridTables *tab, int levels,
                                  float G, float min_val, int allow_fast, hipStream_t st)
{
    if (levels > NB_LUT_MIN) return hipErrorInvalidValue;
    ForceGeom g2 = g;
    const dim3 grid = r2max_tables_grid(g2, 1, g.nchunks);
    return nb::pick<2, 3>(dim, [&](auto D) {
        hipLaunchKernelGGL((r2max_tables_kernel<D.value, 1>), grid, dim3(NB_BLOCK), 0, st, pos, g2, eps2, tab, levels, G, min_val,
                           allow_fast);
        return hipGetLastError();
    });
}

hipError_t nb_launch_ens_r2max_tables(const float *pos, int members, int n, int dim, const void *prm, GridTables *tabs,
                                      const int *levels, float min_val, int allow_fast, const int *stop, int t, hipStream_t st,
                                      const int *sizes)
{
    if (members < 1 || members > NB_ENS_MAX_MEMBERS || n < 1 || !tabs || !levels || !prm || t < 0) return hipErrorInvalidValue;
    ForceGeom g{};
    g.n = n; g.j_begin = 0; g.j_end = n; g.r = 1;
    const dim3 grid = r2max_tables_grid(g, members, (n + NB_TJ - 1) / NB_TJ);
    return nb::pick<2, 3>(dim, [&](auto D) {
        return nb::pick_bool(stop != nullptr, [&](auto ST) {
            if (sizes) {        // the geometry is the capacity's; every member cuts its own part out of it
                hipLaunchKernelGGL((ens_r2max_tables_ragged_kernel<D.value, ST.value>), grid, dim3(NB_BLOCK), 0, st, pos, g,
                                   (const EnsScalars<float> *)prm, tabs, levels, min_val, allow_fast, stop, t, sizes);
                return hipGetLastError();
            }
            hipLaunchKernelGGL((ens_r2max_tables_kernel<D.value, ST.value>), grid, dim3(NB_BLOCK), 0, st, pos, g,
                               (const EnsScalars<float> *)prm, tabs, levels, min_val, allow_fast, stop, t);
            return hipGetLastError();
        });
    });
}

hipError_t nb_launch_ens_tables_wide(int members, int max_levels, const void *prm, GridTables *tabs, const int *levels,
                                     float min_val, int allow_fast, const int *stop, int t, hipStream_t st)
{
    if (members < 1 || members > NB_ENS_MAX_MEMBERS || !tabs || !levels || !prm || t < 0) return hipErrorInvalidValue;
    if (max_levels <= NB_LUT_MIN || max_levels > NB_MAX_LUT) return hipErrorInvalidValue;
    const dim3 grid((max_levels + NB_LUT_MIN - 1) / NB_LUT_MIN, members);
    return nb::pick_bool(stop != nullptr, [&](auto ST) {
        hipLaunchKernelGGL((ens_tables_wide_kernel<ST.value>), grid, dim3(NB_LUT_MIN), 0, st, (const EnsScalars<float> *)prm, tabs,
                           levels, min_val, allow_fast, stop, t);
        return hipGetLastError();
    });
}

hipError_t nb_launch_r2max_pruned(const float *pos, int n, int dim, float eps2, float *cand, float *rho,
                                  PruneState *ps, GridTables *tab, hipStream_t st)
{
    const int blocks = (n + NB_BLOCK - 1) / NB_BLOCK;
    const int bbox_blocks = blocks < 128 ? blocks : 128;
    // *ps is in its reset state on entry: nb_api.cpp initialises it once, grid_tables_kernel (which
    // always follows) puts it back after use -- no per-step memset / copy launches
    return nb::pick<2, 3>(dim, [&](auto D) {
        hipLaunchKernelGGL((prune_bbox_kernel<D.value>), dim3(bbox_blocks), dim3(NB_BLOCK), 0, st, pos, n, ps);
        hipLaunchKernelGGL((prune_rho_kernel<D.value>), dim3(blocks), dim3(NB_BLOCK), 0, st, pos, n, rho, ps);
        hipLaunchKernelGGL((prune_hop_kernel<D.value>), dim3(blocks), dim3(NB_BLOCK), 0, st, pos, n, eps2, &ps->far, &ps->lb[0]);
        hipLaunchKernelGGL((prune_hop_kernel<D.value>), dim3(blocks), dim3(NB_BLOCK), 0, st, pos, n, eps2, &ps->lb[0], &ps->lb[1]);
        hipLaunchKernelGGL((prune_compact_kernel<D.value>), dim3(blocks), dim3(NB_BLOCK), 0, st, pos, rho, n, cand, ps);
        hipLaunchKernelGGL((prune_scan_kernel<D.value>), dim3(blocks), dim3(NB_BLOCK), 0, st, cand, eps2, ps, tab);
        return hipGetLastError();
    });
}

hipError_t nb_launch_r2max_tracked(const float *pos, int n, int dim, float eps2, float *cand, int *cand_idx, PruneState *ps,
                                   GridTables *tab, int levels, float G, float min_val, int allow_fast, hipStream_t st)
{
    const int blocks = (n + NB_BLOCK - 1) / NB_BLOCK;
    const int fuse = levels <= NB_LUT_MIN ? 1 : 0;
    // (one launch instead of two -- every scan workgroup filtering for itself -- was measured slower at N = 6000 / 12 000:
    // 52.7 / 96.9 vs 41.8 / 73.2 us per INT8 step, profiles/r03_tracked_fused_one_launch_ab.txt)
    return nb::pick<2, 3>(dim, [&](auto D) {
        hipLaunchKernelGGL((track_filter_kernel<D.value>), dim3(blocks), dim3(NB_BLOCK), 0, st, pos, n, eps2, cand, cand_idx, ps);
        hipLaunchKernelGGL((track_scan_kernel<D.value>), dim3(NB_TRACK_BLOCKS), dim3(NB_BLOCK), 0, st, pos, cand, cand_idx, n, eps2, ps,
                           tab, levels, G, min_val, allow_fast, fuse);
        return hipGetLastError();
    });
}

hipError_t nb_launch_grid_quantize_safe_tab(const float *in, float *out, int64_t count, int levels, float min_val,
                                            const double *bounds, GridTables *tab, hipStream_t st)
{
    if (levels < 2 || levels > NB_MAX_LUT) return hipErrorInvalidValue;
    // the scalar tail of the tables (arrival counter, flags) starts from zero; the arrays are fully rewritten
    hipError_t e = hipMemsetAsync(&tab->lmin, 0, sizeof(GridTables) - offsetof(GridTables, lmin), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(grid_tables_bounds_kernel, dim3((levels + NB_LUT_MIN - 1) / NB_LUT_MIN), dim3(NB_LUT_MIN), 0, st, tab,
                       levels, min_val, bounds);
    const int lp = nb_lut_pad(levels);
    int grid = (int)((count + 1023) / 1024);
    grid = grid < 1 ? 1 : (grid > 4096 ? 4096 : grid);
    hipLaunchKernelGGL(grid_quantize_safe_tab_kernel, dim3(grid), dim3(256), (size_t)(lp + 1 + levels) * sizeof(float), st, in,
                       out, count, levels, min_val, bounds, tab, lp);
    return hipGetLastError();
}

hipError_t nb_launch_grid_tables(GridTables *tab, int levels, float G, float eps2, float min_val, PruneState *ps,
                                 hipStream_t st, int allow_fast)
{
    hipLaunchKernelGGL(grid_tables_kernel, dim3((levels + NB_LUT_MIN - 1) / NB_LUT_MIN), dim3(NB_LUT_MIN), 0, st, tab,
                       levels, G, eps2, min_val, ps, allow_fast);
    return hipGetLastError();
}

hipError_t nb_launch_d2bins(const float *pos, int n, int dim, float eps2, const GridTables *tab, int16_t *bins,
                            hipStream_t st, int i0, int i1)
{
    if (i1 < 0) i1 = n;
    const dim3 grid((n + NB_BLOCK - 1) / NB_BLOCK, i1 - i0);
    return nb::pick<2, 3>(dim, [&](auto D) {
        hipLaunchKernelGGL((d2bins_kernel<D.value>), grid, dim3(NB_BLOCK), 0, st, pos, n, eps2, tab, bins, i0);
        return hipGetLastError();
    });
}
