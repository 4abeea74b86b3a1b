// nb_small_body.h -- device body of the one-launch small-system step for the cast hooks (HOOK_NONE / HOOK_BF16 /
// HOOK_F16; T = double or float; D = 2 or 3): the pair loop over LDS-staged source tiles, the butterfly that finishes a
// target's sum, and the fused closing / opening kicks (see nb_small.hip for the scheme).  Included by nb_small.hip
// (small_step_kernel: one system per launch, target block = blockIdx.x) and nb_ensemble.hip (ens_step_kernel: many
// systems per launch, member = blockIdx.y): the SAME code, so a member of an ensemble rounds every sum exactly as the
// solo step does.  The grid-hook body (tables, bin read-out) stays in nb_small.hip.
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

template <typename T> __device__ __forceinline__ T axpy_sep(T a, T b, T s);      // a + b*s, two roundings like torch
template <> __device__ __forceinline__ double axpy_sep<double>(double a, double b, double s) { return __dadd_rn(a, __dmul_rn(b, s)); }
template <> __device__ __forceinline__ float axpy_sep<float>(float a, float b, float s) { return __fadd_rn(a, __fmul_rn(b, s)); }

// One workgroup of the step: targets [blk * BS / S, (blk + 1) * BS / S) of ONE system of n particles against all of its
// sources.  The pointers are that system's own arrays ((n, D) row-major; mass (n)); the scalars are already cast to T.
// do_kick: an NbKick mode, | NB_KICK_OPEN_ON_READ (nb_internal.h); the drifted positions go to pos_out.
// part (kernel-uniform, may be null): per-workgroup {min, max} of the forces written, at part[2 blk].
template <typename T, int D, int HOOK, int S, int BS>
__device__ __forceinline__ void small_step_body(int blk, const T *pos_in, T *pos_out,
                                                T *vel, T *acc, const T *mass, int n,
                                                T G, T eps2, T half_dt, T dt, int do_kick, double *part)
{
    static_assert(HOOK == HOOK_NONE || HOOK == HOOK_BF16 || HOOK == HOOK_F16, "the grid hook keeps its own body");
    constexpr bool F64 = sizeof(T) == 8;
    constexpr int TG = BS / S;                       // targets per workgroup
    __shared__ T sx[D][SM_TILE];
    __shared__ T sg[SM_TILE];                        // G * m_j (fp32: the reference's (1/p * G) * m_j order is kept below)
    const int tid = threadIdx.x;
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
#pragma unroll 4
        for (int jj = l; jj < cnt_up; jj += S) {
            T d[D];
            if constexpr (F64) {
#pragma unroll
                for (int k = 0; k < D; ++k) d[k] = sx[k][jj] - xi[k];
                double q = __builtin_fma(d[D - 1], d[D - 1], eps2);
#pragma unroll
                for (int k = D - 2; k >= 0; --k) q = __builtin_fma(d[k], d[k], q);
                const double w = inv_r3_d(q) * sg[jj];
#pragma unroll
                for (int k = 0; k < D; ++k) a[k] = __builtin_fma(w, d[k], a[k]);
            } else {
#pragma unroll
                for (int k = 0; k < D; ++k) d[k] = __fsub_rn(sx[k][jj], xi[k]);
                float q = r2_f32_exact<D>(d, eps2);
                if (HOOK == HOOK_BF16) q = round_bf16(q);
                if (HOOK == HOOK_F16) q = round_f16(q);
                float w = __fmul_rn(inv_r3_f(q), G);
                if (HOOK == HOOK_F16) w = (q == __builtin_inff()) ? 0.0f : w;      // pow(inf) = inf -> G / inf = 0 upstream
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
                if (do_kick & NB_KICK_OPEN_ON_READ) v = axpy_sep<T>(v, a_prev, half_dt);     // this step's opening kick, deferred (see below)
                v = axpy_sep<T>(v, ak, half_dt);                          // closing kick (simulation.py:141)
                if (kmode == NB_KICK_CLOSE_OPEN) {
                    v = axpy_sep<T>(v, ak, half_dt);                      // next step's opening kick (:132)
                    pos_out[idx] = axpy_sep<T>(xi[k], v, dt);             // ... and drift (:135)
                } else if (kmode == NB_KICK_CLOSE_SPEC) {
                    // last step of a native call: velocities stay at the closing kick (what a reader must see), but the
                    // positions the NEXT step would drift to go to pos_out -- if the next nb_step finds the state
                    // untouched it takes them and applies its opening kick here on read (NB_KICK_OPEN_ON_READ): a Python loop of
                    // step() costs one launch per step instead of two
                    const T vo = axpy_sep<T>(v, ak, half_dt);
                    pos_out[idx] = axpy_sep<T>(xi[k], vo, dt);
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
