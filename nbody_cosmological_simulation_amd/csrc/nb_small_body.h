// nb_small_body.h -- device bodies of the one-launch small-system step (D = 2 or 3): the pair loop over LDS-staged
// source tiles, the butterfly that finishes a target's sum, and the fused closing / opening kicks (see nb_small.hip for
// the scheme).  small_step_body: the cast hooks (HOOK_NONE / HOOK_BF16 / HOOK_F16; T = double or float), or
// HOOK_AT_RUN_TIME (fp32): one of the three cast hooks as a workgroup-uniform argument (ens_step_mixed_kernel);
// small_grid_body: the grid hook (fp32, tables, bin read-out).  Included by nb_small.hip (small_step_kernel: one system
// per launch, target block = blockIdx.x), nb_ensemble.hip (ens_step_kernel / ens_grid_step_kernel: many systems per
// launch), nb_ens_ragged.hip (ens_step_ragged_kernel / ens_grid_step_ragged_kernel: systems of different sizes per launch, target block from a work list)
// and nb_ens_grid_wide.hip (ens_grid_step_wide_kernel, ens_grid_bins_kernel): the SAME code, so a member of an ensemble rounds every sum exactly as the solo step does.
#pragma once
#include "nb_device.h"

namespace {

using namespace nbdev;

constexpr int SM_TILE = 1024;     // sources per LDS tile (2048 measured: slower -- fewer workgroups per CU)

__device__ __forceinline__ double inv_r3_d(double q)
{
    const double y0 = __builtin_amdgcn_rsq(q);
    const double y02 = y0 * y0;
    const double e = __builtin_fma(-q, y02, 1.0);
    const double v = y0 * y02;
    const double c = __builtin_fma(e, 1.875, 1.5);
    return __builtin_fma(v, c * e, v);
}
__device__ __forceinline__ float inv_r3_f(float q)
{
    const float y0 = __builtin_amdgcn_rsqf(q);
    const float y02 = y0 * y0;
    const float e = __builtin_fmaf(-q, y02, 1.0f);
    const float v = y0 * y02;
    return __builtin_fmaf(v * e, 1.5f, v);
}

// One workgroup of the step: targets [blk * BS / S, (blk + 1) * BS / S) of ONE system of n particles against all of its
// sources.  The pointers are that system's own arrays ((n, D) row-major; mass (n)); the scalars are already cast to T.
// do_kick: an NbKick mode, | NB_KICK_OPEN_ON_READ (nb_internal.h); the drifted positions go to pos_out.
// part (kernel-uniform, may be null): per-workgroup {min, max} of the forces written, at part[2 blk].
// hook_rt: read under HOOK_AT_RUN_TIME only -- HOOK_NONE, HOOK_BF16 or HOOK_F16, uniform over the workgroup; the two
// rounding lines of the pair loop then test it, and every other operation is the one the compile-time hook performs.
template <typename T, int D, int HOOK, int S, int BS>
__device__ __forceinline__ void small_step_body(int blk, const T *pos_in, T *pos_out,
                                                T *vel, T *acc, const T *mass, int n,
                                                T G, T eps2, T half_dt, T dt, int do_kick, double *part,
                                                int hook_rt = HOOK_NONE)
{
    static_assert(HOOK == HOOK_NONE || HOOK == HOOK_BF16 || HOOK == HOOK_F16 || HOOK == HOOK_AT_RUN_TIME,
                  "the grid hook has its own body: small_grid_body");
    static_assert(HOOK != HOOK_AT_RUN_TIME || sizeof(T) == 4, "the cast hooks round an fp32 r2");
    const bool hook_bf16 = HOOK == HOOK_BF16 || (HOOK == HOOK_AT_RUN_TIME && hook_rt == HOOK_BF16);
    const bool hook_f16 = HOOK == HOOK_F16 || (HOOK == HOOK_AT_RUN_TIME && hook_rt == HOOK_F16);
    constexpr bool F64 = sizeof(T) == 8;
    constexpr int TG = BS / S;                       // targets per workgroup
    __shared__ T sx[D][SM_TILE];
    __shared__ T sg[SM_TILE];                        // G * m_j (fp32: the reference's (1/p * G) * m_j order is kept below)
    const int tid = threadIdx.x;
    const int grp = tid / S, l = tid % S;
    const int i_raw = blk * TG + grp;
    const bool live = i_raw < n;
    const int i = live ? i_raw : n - 1;
    // xi: the state (the drift below starts from it); xc and the LDS tile: the pair loop's copies, a coordinate beyond
    // +-FAR moved to the star's slot (stage_far, nb_device.h): a runaway star's r2 stays finite and its factor underflows
    // to 0 like the padding's
    constexpr T FAR = F64 ? (T)NB_FAR_F64 : (T)NB_FAR_F32;
    T xi[D], xc[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        xi[k] = pos_in[(size_t)i * D + k];
        xc[k] = stage_far<T>(xi[k], FAR, i);
    }
    double a[D];
#pragma unroll
    for (int k = 0; k < D; ++k) a[k] = 0.0;

    for (int j0 = 0; j0 < n; j0 += SM_TILE) {
        __syncthreads();
        // entries past the end, up to the pair loop's stride: padding (far away, massless)
        constexpr int STRIDE = S;
        const int cnt_ld = min(SM_TILE, (min(SM_TILE, n - j0) + STRIDE - 1) / STRIDE * STRIDE);
        // (a "flat" variant -- consecutive threads reading consecutive elements of the (N, D) array and scattering them
        // into the component arrays -- measured slower on the same box: 6.8 vs 5.4 us per step at N = 1024 fp64)
        for (int t = tid; t < cnt_ld; t += BS) {
            const int j = j0 + t;
            if (j < n) {
#pragma unroll
                for (int k = 0; k < D; ++k) sx[k][t] = stage_far<T>(pos_in[(size_t)j * D + k], FAR, j);
                sg[t] = F64 ? (T)(G * mass[j]) : mass[j];
            } else {
#pragma unroll
                for (int k = 0; k < D; ++k) sx[k][t] = F64 ? (T)1e150 : (T)1e18;
                sg[t] = (T)0;
            }
        }
        __syncthreads();
        const int cnt_up = cnt_ld;                   // padding entries are harmless
#pragma unroll 4
        for (int jj = l; jj < cnt_up; jj += S) {
            T d[D];
            if constexpr (F64) {
#pragma unroll
                for (int k = 0; k < D; ++k) d[k] = sx[k][jj] - xc[k];
                double q = __builtin_fma(d[D - 1], d[D - 1], eps2);
#pragma unroll
                for (int k = D - 2; k >= 0; --k) q = __builtin_fma(d[k], d[k], q);
                const double w = inv_r3_d(q) * sg[jj];
#pragma unroll
                for (int k = 0; k < D; ++k) a[k] = __builtin_fma(w, d[k], a[k]);
            } else {
#pragma unroll
                for (int k = 0; k < D; ++k) d[k] = __fsub_rn(sx[k][jj], xc[k]);
                float q = r2_f32_exact<D>(d, eps2);
                if (hook_bf16) q = round_bf16(q);
                if (hook_f16) q = round_f16(q);
                float w = __fmul_rn(inv_r3_f(q), G);
                if (hook_f16) w = (q == __builtin_inff()) ? 0.0f : w;      // pow(inf) = inf -> G / inf = 0 upstream
                w = __fmul_rn(w, sg[jj]);
#pragma unroll
                for (int k = 0; k < D; ++k) a[k] += (double)__fmul_rn(w, d[k]);
            }
        }
    }
    // the S lanes of a target: fixed butterfly
#pragma unroll
    for (int off = S / 2; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < D; ++k) a[k] += __shfl_xor(a[k], off, 64);
    }
    __shared__ double s_mm[BS / 16][2];        // min / max of this workgroup's force components (`part`)
    double lo = __builtin_inf(), hi = -__builtin_inf();
    if (live && l == 0) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const size_t idx = (size_t)i * D + k;
            const T ak = (T)a[k];
            const T a_prev = (do_kick & NB_KICK_OPEN_ON_READ) ? acc[idx] : (T)0;     // (read before this evaluation's force replaces it)
            acc[idx] = ak;
            const double av = (double)ak;              // NaN-propagating like torch's min() / max()
            lo = (av != av || lo != lo) ? __builtin_nan("") : (av < lo ? av : lo);
            hi = (av != av || hi != hi) ? __builtin_nan("") : (av > hi ? av : hi);
            const int kmode = do_kick & NB_KICK_MODE_MASK;
            if (kmode != NB_KICK_NONE) {
                T v = vel[idx];
                if (do_kick & NB_KICK_OPEN_ON_READ) v = axpy_rn<T>(v, a_prev, half_dt);     // this step's opening kick, deferred (see below)
                v = axpy_rn<T>(v, ak, half_dt);                          // closing kick (simulation.py:141)
                if (kmode == NB_KICK_CLOSE_OPEN) {
                    v = axpy_rn<T>(v, ak, half_dt);                      // next step's opening kick (:132)
                    pos_out[idx] = axpy_rn<T>(xi[k], v, dt);             // ... and drift (:135)
                } else if (kmode == NB_KICK_CLOSE_SPEC) {
                    // last step of a native call: velocities stay at the closing kick (what a reader must see), but the
                    // positions the NEXT step would drift to go to pos_out -- if the next nb_step finds the state
                    // untouched it takes them and applies its opening kick here on read (NB_KICK_OPEN_ON_READ): a Python loop of
                    // step() costs one launch per step instead of two
                    const T vo = axpy_rn<T>(v, ak, half_dt);
                    pos_out[idx] = axpy_rn<T>(xi[k], vo, dt);
                }
                vel[idx] = v;
            }
        }
    }
    if (part) {                                      // kernel-uniform
        if (l == 0) { s_mm[grp][0] = lo; s_mm[grp][1] = hi; }    // dead targets hold (+inf, -inf): neutral
        __syncthreads();
        if (tid == 0) {
            double mn = s_mm[0][0], mx = s_mm[0][1];
            for (int g = 1; g < TG; ++g) {
                const double a0 = s_mm[g][0], a1 = s_mm[g][1];
                mn = (a0 != a0 || mn != mn) ? __builtin_nan("") : (a0 < mn ? a0 : mn);
                mx = (a1 != a1 || mx != mx) ? __builtin_nan("") : (a1 > mx ? a1 : mx);
            }
            part[2 * (size_t)blk] = mn;
            part[2 * (size_t)blk + 1] = mx;
        }
    }
}

// The grid hook (INT8 / INT4 / CUSTOM up to NB_LUT_MIN levels; fp32 state): the same workgroup of the step with the
// evaluation's tables (*tab: nb_grid.hip grid_tables_body) staged in LDS and a pair's factor taken table-free when no
// pair of its WAVE sits on a bin edge -- so a pair's factor depends on which pairs share its wave,
// and every caller keeps the lane layout: BS threads, S lanes per target, four sources per lane and iteration.
// BINS: the same body with the quant-bin read-out -- per-target integer checksums s1 = sum_j k,
// s2 = sum_j k ((j mod 65521) + 1) of the bin every pair was given, by whichever route the production code took
// (table-free estimate / wave ballot / threshold fallback); bin_out = {s1[n], s2[n], {table-free pairs, table pairs}}.
// part (kernel-uniform; INT8 / INT4): per-workgroup {min, max} of the forces written, at part[2 blk].
// WIDE (ens_grid_step_wide_kernel: CUSTOM members of up to NB_MAX_LUT levels): the tables live in the launch's dynamic LDS
// instead -- wide_tabs = 2 (wide_cap + 1) floats, wide_cap the padded size (nb_lut_pad) of the launch's widest member --
// and the binary search walks the member's OWN padded size.  A grid above NB_LUT_MIN levels has fast_ok = 0 (multi-chunk
// tables, nb_grid.hip) and takes the estimate or the search, as on the solo tiled path; one of up to NB_LUT_MIN levels
// performs the operations of the fixed-size body in the same order.  Lane layout and source order are the same either way.
template <int D, int S, bool BINS, int BS, bool WIDE = false>
__device__ __forceinline__ void small_grid_body(int blk, const float *pos_in, float *pos_out, float *vel, float *acc,
                                                const float *mass, int n, float G, float eps2, float half_dt, float dt,
                                                int do_kick, const GridTables *tab, double *part,
                                                unsigned long long *bin_out, float *wide_tabs = nullptr,
                                                int wide_cap = NB_LUT_MIN)
{
    using T = float;
    constexpr bool F64 = sizeof(T) == 8;
    constexpr int TG = BS / S;                       // targets per workgroup
    __shared__ T sx[D][SM_TILE];
    __shared__ T sg[SM_TILE];                        // G * m_j (fp32: the reference's (1/p * G) * m_j order is kept below)
    // grid hook (INT8 / INT4 / CUSTOM up to 256 levels): the evaluation's tables (nb_grid.hip grid_tables_kernel)
    __shared__ float s_thr_fix[WIDE ? 1 : NB_LUT_MIN + 1], s_lut_fix[WIDE ? 1 : NB_LUT_MIN + 1];
    float *const s_thr = WIDE ? wide_tabs : s_thr_fix;
    float *const s_lut = WIDE ? wide_tabs + wide_cap + 1 : s_lut_fix;
    const int tid = threadIdx.x;
    bool g_fast = false, g_est = false, g_deg = false;
    float est_a = 0.0f, est_b = 0.0f, est_bc = 0.0f, sure_lim = 0.0f, c1 = 0.0f, c0c = 0.0f, kcf = 0.0f;
    int g_levels = 0, g_tm = 0;
    g_levels = tab->levels;
    int lp = NB_LUT_MIN;                             // the member's padded table size (nb_lut_pad), never above the launch's
    if constexpr (WIDE) {
        g_levels = min(g_levels, wide_cap);
        while (lp < g_levels) lp <<= 1;
    }
    for (int k = tid; k <= lp; k += BS) {
        s_thr[k] = (k <= g_levels) ? tab->thr[k] : __builtin_inff();     // thr[levels] = NaN sentinel, +inf padding
        s_lut[k] = (k < g_levels) ? tab->lut[k] : 0.0f;
    }
    g_fast = tab->fast_ok != 0;
    g_est = tab->use_est != 0;
    g_deg = tab->degenerate != 0;
    est_a = tab->est_a; est_b = tab->est_b; est_bc = tab->est_bc; sure_lim = tab->sure_lim;
    c1 = tab->c1; c0c = tab->c0c; kcf = (float)tab->kc; g_tm = tab->tm;
    const int grp = tid / S, l = tid % S;
    const int i_raw = blk * TG + grp;
    const bool live = i_raw < n;
    const int i = live ? i_raw : n - 1;
    T xi[D];
#pragma unroll
    for (int k = 0; k < D; ++k) xi[k] = pos_in[(size_t)i * D + k];
    double a[D];
#pragma unroll
    for (int k = 0; k < D; ++k) a[k] = 0.0;
    long long b1 = 0, b2 = 0, bfast = 0, bexact = 0;     // BINS only

    for (int j0 = 0; j0 < n; j0 += SM_TILE) {
        __syncthreads();
        // entries past the end, up to the pair loop's stride: padding (far away, massless)
        constexpr int STRIDE = 4 * S;
        const int cnt_ld = min(SM_TILE, (min(SM_TILE, n - j0) + STRIDE - 1) / STRIDE * STRIDE);
        // (a "flat" variant -- consecutive threads reading consecutive elements of the (N, D) array and scattering them
        // into the component arrays -- measured slower on the same box: 6.8 vs 5.4 us per step at N = 1024 fp64)
        for (int t = tid; t < cnt_ld; t += BS) {
            const int j = j0 + t;
            if (j < n) {
#pragma unroll
                for (int k = 0; k < D; ++k) sx[k][t] = pos_in[(size_t)j * D + k];
                sg[t] = F64 ? (T)(G * mass[j]) : mass[j];
            } else {
#pragma unroll
                for (int k = 0; k < D; ++k) sx[k][t] = F64 ? (T)1e150 : (T)1e18;
                sg[t] = (T)0;
            }
        }
        __syncthreads();
        const int cnt_up = cnt_ld;                   // padding entries are harmless
        // four sources per iteration: independent log / exp chains in flight, ONE edge test for all of them
        constexpr int U = 4;
        for (int jj = l; jj < cnt_up; jj += U * S) {
            float dd[U][D], q[U], w[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int k = 0; k < D; ++k) dd[u][k] = __fsub_rn(sx[k][jj + u * S], xi[k]);
                q[u] = r2_f32_exact<D>(dd[u], eps2);
            }
            // (1 / q_k^1.5) * G of each pair's bin: table-free when no pair of the wave sits on a bin edge
            // (DESIGN.md section 4.3), else floor(estimate) + one threshold compare, else binary search
            int kb[U];                 // BINS: the bin each pair was given
            bool kexact = true;
            if (g_deg) {
#pragma unroll
                for (int u = 0; u < U; ++u) { w[u] = __fmul_rn(inv_r3_f(q[u] < 0.01f ? 0.01f : q[u]), G); kb[u] = 0; }
            } else if (g_fast) {
                float kf[U], dev = 0.0f;
                bool bad = false;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const float ne = __builtin_fmaf(__builtin_amdgcn_logf(q[u]), est_a, est_bc);
                    kf[u] = __builtin_rintf(ne);
                    const float dv = __builtin_fabsf(ne - kf[u]);
                    bad |= !(dv <= sure_lim);                                 // also true for NaN
                    dev = __builtin_fmaxf(dev, dv);
                }
                if (__builtin_amdgcn_ballot_w64(bad) != 0ull) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        kb[u] = grid_bin_floor_estimate(s_thr, q[u], est_a, est_b, g_levels - 2);
                        w[u] = s_lut[kb[u]];
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < U; ++u) {        // max(): softening^2 below the grid's floor
                        const float kc_ = __builtin_fmaxf(kf[u], -kcf);
                        w[u] = ldexpf(__builtin_amdgcn_exp2f(__builtin_fmaf(kc_, c1, c0c)), g_tm);
                        if constexpr (BINS) kb[u] = (int)__builtin_fminf(kc_ + kcf, 1e6f);
                    }
                    kexact = false;
                }
            } else if (g_est) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    kb[u] = grid_bin_floor_estimate(s_thr, q[u], est_a, est_b, g_levels - 2);
                    w[u] = s_lut[kb[u]];
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    kb[u] = grid_bin_lookup(s_thr, q[u], lp);
                    w[u] = s_lut[kb[u]];
                }
            }
            if constexpr (BINS) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int j = j0 + jj + u * S;
                    if (j < n) {             // padding entries of the tile take part in no pair
                        b1 += kb[u];
                        b2 += (long long)kb[u] * (j % 65521 + 1);
                        if (kexact) ++bexact; else ++bfast;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float wm = __fmul_rn(w[u], sg[jj + u * S]);
#pragma unroll
                for (int k = 0; k < D; ++k) a[k] += (double)__fmul_rn(wm, dd[u][k]);
            }
        }
    }
    // the S lanes of a target: fixed butterfly
#pragma unroll
    for (int off = S / 2; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < D; ++k) a[k] += __shfl_xor(a[k], off, 64);
    }
    if constexpr (BINS) {
#pragma unroll
        for (int off = S / 2; off >= 1; off >>= 1) {
            b1 += __shfl_xor(b1, off, 64);
            b2 += __shfl_xor(b2, off, 64);
            bfast += __shfl_xor(bfast, off, 64);
            bexact += __shfl_xor(bexact, off, 64);
        }
        if (live && l == 0) {
            bin_out[i] = (unsigned long long)b1;
            bin_out[(size_t)n + i] = (unsigned long long)b2;
            atomicAdd(&bin_out[2 * (size_t)n], (unsigned long long)bfast);
            atomicAdd(&bin_out[2 * (size_t)n + 1], (unsigned long long)bexact);
        }
    }
    __shared__ double s_mm[BS / 16][2];        // INT8 / INT4: min / max of this workgroup's force components
    double lo = __builtin_inf(), hi = -__builtin_inf();
    if (live && l == 0) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const size_t idx = (size_t)i * D + k;
            const T ak = (T)a[k];
            const T a_prev = (do_kick & NB_KICK_OPEN_ON_READ) ? acc[idx] : (T)0;     // (read before this evaluation's force replaces it)
            acc[idx] = ak;
            const double av = (double)ak;              // NaN-propagating like torch's min() / max()
            lo = (av != av || lo != lo) ? __builtin_nan("") : (av < lo ? av : lo);
            hi = (av != av || hi != hi) ? __builtin_nan("") : (av > hi ? av : hi);
            const int kmode = do_kick & NB_KICK_MODE_MASK;
            if (kmode != NB_KICK_NONE) {
                T v = vel[idx];
                if (do_kick & NB_KICK_OPEN_ON_READ) v = axpy_rn<T>(v, a_prev, half_dt);     // this step's opening kick, deferred (see below)
                v = axpy_rn<T>(v, ak, half_dt);                          // closing kick (simulation.py:141)
                if (kmode == NB_KICK_CLOSE_OPEN) {
                    v = axpy_rn<T>(v, ak, half_dt);                      // next step's opening kick (:132)
                    pos_out[idx] = axpy_rn<T>(xi[k], v, dt);             // ... and drift (:135)
                } else if (kmode == NB_KICK_CLOSE_SPEC) {
                    // last step of a native call: velocities stay at the closing kick (what a reader must see), but the
                    // positions the NEXT step would drift to go to pos_out -- if the next nb_step finds the state
                    // untouched it takes them and applies its opening kick here on read (NB_KICK_OPEN_ON_READ): a Python loop of
                    // step() costs one launch per step instead of two
                    const T vo = axpy_rn<T>(v, ak, half_dt);
                    pos_out[idx] = axpy_rn<T>(xi[k], vo, dt);
                }
                vel[idx] = v;
            }
        }
    }
    if (part) {                                      // kernel-uniform
        if (l == 0) { s_mm[grp][0] = lo; s_mm[grp][1] = hi; }    // dead targets hold (+inf, -inf): neutral
        __syncthreads();
        if (tid == 0) {
            double mn = s_mm[0][0], mx = s_mm[0][1];
            for (int g = 1; g < TG; ++g) {
                const double a0 = s_mm[g][0], a1 = s_mm[g][1];
                mn = (a0 != a0 || mn != mn) ? __builtin_nan("") : (a0 < mn ? a0 : mn);
                mx = (a1 != a1 || mx != mx) ? __builtin_nan("") : (a1 > mx ? a1 : mx);
            }
            part[2 * (size_t)blk] = mn;
            part[2 * (size_t)blk + 1] = mx;
        }
    }
}

}  // namespace
