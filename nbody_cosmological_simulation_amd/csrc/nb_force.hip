// nb_force.hip -- all-pairs softened-gravity kernels for gfx950 (MI355X, CDNA4).
//
// Replaces GalaxySimulation._compute_accelerations (reference simulation.py:74-118) and the
// per-pair part of quantize_distance_squared (quantization.py:21-71).
//
// Decomposition (DESIGN.md "force kernel"):
//   grid  = (target tiles) x (source chunks); block = 256 threads = 4 wavefronts of 64.
//   Each thread keeps R targets in registers; the block walks its source chunk in tiles of
//   NB_TJ particles staged in LDS with one coalesced load per thread; the inner loop reads the
//   tile with wave-uniform (broadcast, conflict-free) ds_reads.
//   Every (tile, chunk) block writes an fp64 partial sum per target to its own slab;
//   reduce_kernel (nb_misc.hip) adds the slabs in fixed order -> run-to-run bit reproducible,
//   no atomics.
//   The path is VALU-bound (arithmetic intensity ~0.135*N flop/B), so the
//   inner loop is written for minimum instruction count: one v_rsq + a fused second-order
//   correction instead of sqrt/div/pow, no self-interaction mask (d == 0 kills the diagonal
//   term exactly as the reference's (1 - eye) multiply does, NaN cases included).
#include "nb_device.h"
#include "nb_dispatch.h"

#include <hip/hip_fp16.h>

#include <cstdlib>

namespace {

using namespace nbdev;

// ------------------------------------------------------------------------------------------
// q^(-3/2) kernels
// ------------------------------------------------------------------------------------------

// fp64:  returns gm * q^(-3/2).  y0 = v_rsq_f64(q) (about 2^-26 relative), then with
// e = 1 - q*y0^2 :  q^(-3/2) = y0^3 * (1-e)^(-3/2) = y0^3 * (1 + e*(3/2 + 15/8 e) + O(e^3)).
// The neglected term is < 2^-70; the result carries ~1.5 ulp of rounding, the same order as the
// reference's pow -> reciprocal -> *G -> *m chain (simulation.py:97-105).
__device__ __forceinline__ double inv_r3_f64(double q, double gm)
{
    const double y0 = __builtin_amdgcn_rsq(q);
    const double y02 = y0 * y0;
    const double e = __builtin_fma(-q, y02, 1.0);
    const double u = y0 * gm;
    const double v = u * y02;
    const double c = __builtin_fma(e, 1.875, 1.5);
    const double ce = c * e;
    return __builtin_fma(v, ce, v);
}

// fp32:  q^(-3/2) from v_rsq_f32 (1 ulp) plus one Newton step, then cubed.
__device__ __forceinline__ float inv_r3_f32(float q)
{
    const float y0 = __builtin_amdgcn_rsqf(q);
    const float t = q * y0;
    const float e = __builtin_fmaf(-t, y0, 1.0f);
    const float y = __builtin_fmaf(0.5f * y0, e, y0);
    return (y * y) * y;
}

// PA: arithmetic type of diff / r2.  NB_F32 normally; NB_F16 / NB_BF16 for the first evaluation on
// half-typed state tensors (omega_point_test.py:722-733): every op of simulation.py:83-86 rounds to
// the half type, the D-term sum accumulates in float and rounds once (torch opmath), eps2 enters
// as a half scalar.
template <int PA> __device__ __forceinline__ float round_pa(float x)
{
    if (PA == NB_F16) return round_f16(x);
    if (PA == NB_BF16) return round_bf16(x);
    return x;
}
template <int D, int PA>
__device__ __forceinline__ float r2_half_state(const float *xi, const float *xj, float eps2_pa, float *d)
{
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        d[k] = round_pa<PA>(__fsub_rn(xj[k], xi[k]));
        const float sq = round_pa<PA>(__fmul_rn(d[k], d[k]));
        s = (k == 0) ? sq : __fadd_rn(s, sq);
    }
    s = round_pa<PA>(s);
    return round_pa<PA>(__fadd_rn(s, eps2_pa));
}

// ------------------------------------------------------------------------------------------
// fp64 state (FLOAT64 mode).  PA_F32: diff and r2 in fp32 (first evaluation on fp32-typed
// positions), everything after the hook in fp64.
// ------------------------------------------------------------------------------------------
// QHOOK != HOOK_NONE: fp64 positions under FLOAT32 / BFLOAT16 / FLOAT16 mode (omega_point_test.py
// :722-733 builds such sims): diff and r2 in fp64 in the reference's op order, the hook casts r2
// to fp32 (and through the half type), q^1.5 and G/. stay fp32, the product with the fp64 mass and
// everything after it is fp64 again (torch promotion).
// PAIR: -1 = fp64 pair arithmetic; NB_F32 / NB_F16 / NB_BF16 = the dtype the positions are typed as
// (first evaluation before the state has been promoted to fp64).
template <int D, int R, int PAIR, int QHOOK = -1>
__global__ void __launch_bounds__(NB_BLOCK)
force_f64_kernel(const double *__restrict__ pos, const double *__restrict__ mass,
                 double *__restrict__ partial, ForceGeom g, double G, double eps2, float eps2_f)
{
    __shared__ double sj[D + 1][NB_TJ];
    // targets and source tiles are the pair loop's own copies: a coordinate beyond +-FAR is moved to the star's slot
    // (stage_far, nb_device.h); the fp32 limit and slots wherever r2 is formed in or cast to fp32
    constexpr double FAR = (PAIR < 0 && QHOOK < 0) ? NB_FAR_F64 : (double)NB_FAR_F32;

    const int tid = threadIdx.x;
    const int ibase = blockIdx.x * (NB_BLOCK * R);

    double xi[R][D];
    double acc[R][D];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int i = ibase + r * NB_BLOCK + tid;
        i = i < g.n ? i : g.n - 1;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            xi[r][k] = stage_far<double>(pos[(size_t)i * D + k], FAR, i);
            acc[r][k] = 0.0;
        }
    }

    const int j_lo = g.j_begin + blockIdx.y * g.chunk_len;
    const int j_hi = min(j_lo + g.chunk_len, g.j_end);

    for (int jt = j_lo; jt < j_hi; jt += NB_TJ) {
        {
            int j = jt + tid;
            j = j < j_hi ? j : j_hi - 1;
#pragma unroll
            for (int k = 0; k < D; ++k) sj[k][tid] = stage_far<double>(pos[(size_t)j * D + k], FAR, j);
            sj[D][tid] = (QHOOK >= 0) ? mass[j] : G * mass[j];
        }
        __syncthreads();
        const int cnt = min(NB_TJ, j_hi - jt);
#pragma unroll 4
        for (int jj = 0; jj < cnt; ++jj) {
            double xj[D];
#pragma unroll
            for (int k = 0; k < D; ++k) xj[k] = sj[k][jj];
            const double gm = sj[D][jj];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double d[D];
                double q;
                if (QHOOK >= 0) {
#pragma unroll
                    for (int k = 0; k < D; ++k) d[k] = __dsub_rn(xj[k], xi[r][k]);
                    double s2 = __dadd_rn(__dmul_rn(d[0], d[0]), __dmul_rn(d[1], d[1]));
                    if (D == 3) s2 = __dadd_rn(s2, __dmul_rn(d[2], d[2]));
                    float q32 = (float)__dadd_rn(s2, eps2);
                    if (QHOOK == HOOK_BF16) q32 = round_bf16(q32);
                    if (QHOOK == HOOK_F16) q32 = round_f16(q32);
                    float wq = inv_r3_f32(q32) * (float)G;
                    if (QHOOK == HOOK_F16) wq = (q32 == __builtin_inff()) ? 0.0f : wq;
                    const double w = __dmul_rn((double)wq, gm);
#pragma unroll
                    for (int k = 0; k < D; ++k) acc[r][k] = __builtin_fma(w, d[k], acc[r][k]);
                    continue;
                }
                if (PAIR == NB_F32) {
                    float df[D];
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        df[k] = __fsub_rn((float)xj[k], (float)xi[r][k]);
                        d[k] = (double)df[k];
                    }
                    q = (double)r2_f32_exact<D>(df, eps2_f);
                } else if (PAIR == NB_F16 || PAIR == NB_BF16) {
                    float xif[D], xjf[D], df[D];
#pragma unroll
                    for (int k = 0; k < D; ++k) { xif[k] = (float)xi[r][k]; xjf[k] = (float)xj[k]; }
                    q = (double)r2_half_state<D, PAIR>(xif, xjf, eps2_f, df);     // eps2_f already half-rounded
#pragma unroll
                    for (int k = 0; k < D; ++k) d[k] = (double)df[k];
                } else {
#pragma unroll
                    for (int k = 0; k < D; ++k) d[k] = xj[k] - xi[r][k];
                    q = __builtin_fma(d[D - 1], d[D - 1], eps2);
#pragma unroll
                    for (int k = D - 2; k >= 0; --k) q = __builtin_fma(d[k], d[k], q);
                }
                const double w = inv_r3_f64(q, gm);
#pragma unroll
                for (int k = 0; k < D; ++k) acc[r][k] = __builtin_fma(w, d[k], acc[r][k]);
            }
        }
        __syncthreads();
    }

    double *out = partial + (size_t)blockIdx.y * g.n * D;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = ibase + r * NB_BLOCK + tid;
        if (i < g.n) {
#pragma unroll
            for (int k = 0; k < D; ++k) out[(size_t)i * D + k] = acc[r][k];
        }
    }
}

// ------------------------------------------------------------------------------------------
// fp32 state (FLOAT32 / BFLOAT16 / FLOAT16 / INT8 / INT4 / CUSTOM modes)
// ------------------------------------------------------------------------------------------
// BINS: the same body with the quant-bin read-out (per-target integer checksums s1 = sum_j k, s2 = sum_j k ((j mod
// 65521) + 1), see nb_force_sym_kernel.h BinDbg), added to bin_out = {s1[n], s2[n], {0, table pairs}} with atomics.
template <int D, int R, int HOOK, int PA = NB_F32, bool BINS = false>
__global__ void __launch_bounds__(NB_BLOCK)
force_f32_kernel(const float *__restrict__ pos, const float *__restrict__ mass,
                 double *__restrict__ partial, ForceGeom g, float G, float eps2,
                 const GridTables *__restrict__ tab, int lp, unsigned long long *__restrict__ bin_out)
{
    __shared__ float sj[D + 1][NB_TJ];
    extern __shared__ float s_tables[];        // grid hook: thr[lp + 1], lut[lp + 1] (nb_lut_lds_bytes)
    float *s_thr = s_tables, *s_lut = s_tables + lp + 1;

    const int tid = threadIdx.x;
    const int ibase = blockIdx.x * (NB_BLOCK * R);
    bool degenerate = false, use_est = false;
    float est_a = 0.0f, est_b = 0.0f;
    int est_kmax = 0;

    if (HOOK == HOOK_GRID) {
        for (int k = tid; k < lp; k += NB_BLOCK) {
            s_thr[k] = (k < tab->levels) ? tab->thr[k] : __builtin_inff();
            s_lut[k] = (k < tab->levels) ? tab->lut[k] : 0.0f;
        }
        degenerate = tab->degenerate != 0;
        use_est = tab->use_est != 0;
        est_a = tab->est_a;
        est_b = tab->est_b;
        est_kmax = tab->levels - 2;
    }

    // the pair loop's copies: a coordinate beyond +-FAR is moved to the star's slot (stage_far, nb_device.h); not in the grid modes,
    // whose tables come from the unclamped maximum of r2
    const float FAR = (HOOK == HOOK_GRID) ? __builtin_inff() : NB_FAR_F32;
    float xi[R][D];
    double acc[R][D];
    long long b1[BINS ? R : 1], b2[BINS ? R : 1], bcount = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int i = ibase + r * NB_BLOCK + tid;
        i = i < g.n ? i : g.n - 1;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            xi[r][k] = stage_far<float>(pos[(size_t)i * D + k], FAR, i);
            acc[r][k] = 0.0;
        }
        if constexpr (BINS) b1[r] = b2[r] = 0;
    }

    const int j_lo = g.j_begin + blockIdx.y * g.chunk_len;
    const int j_hi = min(j_lo + g.chunk_len, g.j_end);

    for (int jt = j_lo; jt < j_hi; jt += NB_TJ) {
        {
            int j = jt + tid;
            j = j < j_hi ? j : j_hi - 1;
#pragma unroll
            for (int k = 0; k < D; ++k) sj[k][tid] = stage_far<float>(pos[(size_t)j * D + k], FAR, j);
            sj[D][tid] = mass[j];
        }
        __syncthreads();
        const int cnt = min(NB_TJ, j_hi - jt);
        // fp32 running sums over one tile only; the tile sums are folded into fp64 accumulators
        // so the error of an N-term fp32 sum stays at the level of torch's cascade summation.
        float tacc[R][D];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int k = 0; k < D; ++k) tacc[r][k] = 0.0f;

#pragma unroll 4
        for (int jj = 0; jj < cnt; ++jj) {
            float xj[D];
#pragma unroll
            for (int k = 0; k < D; ++k) xj[k] = sj[k][jj];
            const float mj = sj[D][jj];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float d[D];
                float r2;
                if (PA == NB_F32) {
#pragma unroll
                    for (int k = 0; k < D; ++k) d[k] = __fsub_rn(xj[k], xi[r][k]);
                    r2 = r2_f32_exact<D>(d, eps2);
                } else {
                    r2 = r2_half_state<D, PA>(xi[r], xj, eps2, d);
                }
                float wq;   // (1 / q^1.5) * G   (simulation.py:97-101)
                if (HOOK == HOOK_GRID) {
                    if (!degenerate) {
                        // floor estimate + one threshold compare (nb_device.h) when the tables allow it,
                        // else the 8-step binary search: both give the exact bin
                        const int kb = use_est ? grid_bin_floor_estimate(s_thr, r2, est_a, est_b, est_kmax)
                                               : grid_bin_lookup(s_thr, r2, lp);
                        wq = s_lut[kb];
                        if constexpr (BINS) {
                            b1[r] += kb;
                            b2[r] += (long long)kb * ((jt + jj) % 65521 + 1);
                            ++bcount;
                        }
                    } else {
                        const float q = (r2 < 0.01f) ? 0.01f : r2;     // clamp keeps NaN
                        wq = inv_r3_f32(q) * G;
                    }
                } else {
                    float q = r2;
                    if (HOOK == HOOK_BF16) q = round_bf16(r2);
                    if (HOOK == HOOK_F16) q = round_f16(r2);
                    wq = inv_r3_f32(q) * G;
                    // fp16 overflow: q = +inf -> pow = inf -> 1/inf = 0 upstream (rsq-based form gives NaN)
                    if (HOOK == HOOK_F16) wq = (q == __builtin_inff()) ? 0.0f : wq;
                }
                const float w = wq * mj;                                // simulation.py:105
#pragma unroll
                for (int k = 0; k < D; ++k) tacc[r][k] = __builtin_fmaf(w, d[k], tacc[r][k]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int k = 0; k < D; ++k) acc[r][k] += (double)tacc[r][k];
        __syncthreads();
    }

    double *out = partial + (size_t)blockIdx.y * g.n * D;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = ibase + r * NB_BLOCK + tid;
        if (i < g.n) {
#pragma unroll
            for (int k = 0; k < D; ++k) out[(size_t)i * D + k] = acc[r][k];
            if constexpr (BINS) {
                atomicAdd(&bin_out[i], (unsigned long long)b1[r]);
                atomicAdd(&bin_out[(size_t)g.n + i], (unsigned long long)b2[r]);
            }
        }
    }
    if constexpr (BINS) {
        // clamped duplicate targets (i >= n) counted pairs too: report only this thread's live ones
        int live = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) live += (ibase + r * NB_BLOCK + tid < g.n) ? 1 : 0;
        atomicAdd(&bin_out[2 * (size_t)g.n + 1], (unsigned long long)(bcount / R * live));
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
constexpr int R_F32 = 2;
template <int V>
using ic = std::integral_constant<int, V>;     // a fixed template argument beside picked ones

hipError_t nb_launch_force_f64(const double *pos, const double *mass, double *partial, const ForceGeom &g,
                               int dim, int pair_dt, int qhook, double G, double eps2_py, float eps2_pair,
                               hipStream_t st)
{
    // pair_dt: -1 (fp64 pairs) or the dtype the positions are typed as (NB_F32 / NB_F16 / NB_BF16)
    const bool cast = qhook >= 0, typed = !cast && (pair_dt == NB_F32 || pair_dt == NB_F16 || pair_dt == NB_BF16);
    const int r = (pair_dt >= 0 || cast) ? 2 : g.r;   // the special variants are compiled for R = 2 only
    const dim3 grid((g.n + NB_BLOCK * r - 1) / (NB_BLOCK * r), g.nchunks);
    return nb::pick<2, 3>(dim, [&](auto D) {
        auto launch = [&](auto R, auto PA, auto QH) {
            hipLaunchKernelGGL((force_f64_kernel<D.value, R.value, PA.value, QH.value>), grid, dim3(NB_BLOCK), 0, st, pos, mass,
                               partial, g, G, eps2_py, eps2_pair);
            return hipGetLastError();
        };
        if (cast) return nb::pick<HOOK_NONE, HOOK_BF16, HOOK_F16>(qhook, [&](auto QH) { return launch(ic<2>{}, ic<-1>{}, QH); });
        if (typed) return nb::pick<NB_F32, NB_F16, NB_BF16>(pair_dt, [&](auto PA) { return launch(ic<2>{}, PA, ic<-1>{}); });
        return nb::pick<1, 2, 4>(g.r == 1 || g.r == 2 ? g.r : 4, [&](auto R) { return launch(R, ic<-1>{}, ic<-1>{}); });
    });
}

hipError_t nb_launch_force_f32(const float *pos, const float *mass, double *partial, const ForceGeom &g,
                               int dim, int hook, int pa, float G, float eps2, const GridTables *tab, int levels,
                               hipStream_t st, unsigned long long *bin_out)
{
    const int lp = hook == HOOK_GRID ? nb_lut_pad(levels) : 0;
    const size_t lds = hook == HOOK_GRID ? nb_lut_lds_bytes(levels) : 0;
    // small systems are parallelism-bound: one target per thread doubles the workgroups (like the fp64 kernel)
    const int r = g.n <= 8192 ? 1 : R_F32;
    const dim3 grid((g.n + NB_BLOCK * r - 1) / (NB_BLOCK * r), g.nchunks);
    return nb::pick<2, 3>(dim, [&](auto D) {
        return nb::pick<1, R_F32>(r, [&](auto R) {
            auto launch = [&](auto H, auto PA, auto BINS) {
                hipLaunchKernelGGL((force_f32_kernel<D.value, R.value, H.value, PA.value, BINS.value>), grid, dim3(NB_BLOCK), lds,
                                   st, pos, mass, partial, g, G, eps2, tab, lp, bin_out);
                return hipGetLastError();
            };
            if (bin_out) {           // bin read-out of the grid hook (nb_quant_bin_sums): same body, BINS = true
                if (hook != HOOK_GRID || pa != NB_F32) return hipErrorInvalidValue;
                return launch(ic<HOOK_GRID>{}, ic<NB_F32>{}, std::true_type{});
            }
            if (pa != NB_F32) {
                // half-typed state: cast hooks only (a grid over a half tensor is not implemented); whatever is not fp16 runs
                // as bf16, and a hook that is neither none nor bf16 as fp16
                if (hook == HOOK_GRID) return hipErrorInvalidValue;
                return nb::pick<NB_F16, NB_BF16>(pa == NB_F16 ? NB_F16 : NB_BF16, [&](auto PA) {
                    return nb::pick<HOOK_NONE, HOOK_BF16, HOOK_F16>(hook == HOOK_NONE || hook == HOOK_BF16 ? hook : HOOK_F16,
                                                                    [&](auto H) { return launch(H, PA, std::false_type{}); });
                });
            }
            return nb::pick<HOOK_NONE, HOOK_BF16, HOOK_F16, HOOK_GRID>(
                hook, [&](auto H) { return launch(H, ic<NB_F32>{}, std::false_type{}); });
        });
    });
}
