// nb_ens_energy.hip -- kinetic and potential energy of every member of an ensemble in two launches (nb_ens_energies /
// nb_ens_run_recorded, include/nbody_amd.h).
//
//   ens_energy_partials_kernel   grid (tile pairs, members).  The member's N stars are cut into tiles of EE_TILE; a
//       workgroup takes one tile pair (ti <= tj) of the upper triangle, so every unordered pair of stars is evaluated
//       once.  Thread t owns target ti * EE_TILE + t and streams the column tile from LDS (all lanes read the same entry:
//       a broadcast).  A diagonal tile pair takes i < j only and adds its stars' kinetic terms.  Entries past N are
//       predicated out (never multiplied away: 0 * inf cannot appear).  Every workgroup writes its {pe, ke} to its own
//       slot part[member][tile pair]: no atomics, no counters, no fences.
//   ens_energy_finish_kernel     one wave per member adds the member's slots in a fixed order (lane l takes slots l,
//       l + 64, ...; then a fixed butterfly), applies -G and 0.5 and writes sample `s` of the history.
//
// The kernel boundary is the only synchronisation between the two.  Terms (simulation.py:170-192):
//   fp64   m_i m_j * rsqrt(r2 + eps2): v_rsq_f64 + one Newton step, y = y0 (1 + e / 2), e = 1 - q y0^2 (as pe_sweep_f64;
//          the neglected 3 e^2 / 8 is < 5e-15 relative)
//   fp32   the upstream op order, one rounding per operation: difference, square, sum, + eps2, root, mass product,
//          quotient; each term is added into an fp64 sum
//   kinetic  m * (sum_k v_k^2) in T, one rounding per operation, added into an fp64 sum
#include "nb_device.h"
#include "nb_dispatch.h"
#include "nb_internal.h"

namespace {

using namespace nbdev;

constexpr int EE_TILE = NB_ENS_ENERGY_TILE;      // stars per tile = threads per workgroup
constexpr int EE_WAVES = EE_TILE / 64;

template <int D>
__device__ __forceinline__ double pair_term(const double (&d)[D], double eps2, double mi, double mj)
{
    double q = __builtin_fma(d[D - 1], d[D - 1], eps2);
#pragma unroll
    for (int k = D - 2; k >= 0; --k) q = __builtin_fma(d[k], d[k], q);
    const double y0 = __builtin_amdgcn_rsq(q);
    const double e = __builtin_fma(-(q * y0), y0, 1.0);
    const double c = __builtin_fma(e, 0.5, 1.0);
    return (mi * mj) * (y0 * c);
}

// RAGGED (sizes: nb_device.h): n is the stride of a member's slice and ntiles the grid's; the member cuts its OWN stars into
// tiles, the workgroups past its own tile pairs return, and its slots are the first of its gridDim.x: the {pe, ke} a
// handle of that size alone would write, in the same slots
template <typename T, int D, bool RAGGED>
__global__ void __launch_bounds__(EE_TILE)
ens_energy_partials_kernel(const T *__restrict__ pos, const T *__restrict__ vel /* null: no kinetic terms */,
                           const T *__restrict__ mass, int n, int ntiles, const EnsScalars<T> *__restrict__ prm,
                           double *__restrict__ part, const int *__restrict__ sizes)
{
    __shared__ T sx[D][EE_TILE];
    __shared__ T sm[EE_TILE];
    __shared__ double s_red[2][EE_WAVES];
    const int b = blockIdx.y;                        // member: uniform per workgroup
    const int tid = threadIdx.x;
    const size_t stride = (size_t)n;                 // stars of a member's slice
    if constexpr (RAGGED) {
        n = ens_member_count<true>(sizes, b, 1, n);
        ntiles = (n + EE_TILE - 1) / EE_TILE;
        if ((int)blockIdx.x >= ntiles * (ntiles + 1) / 2) return;
    }
    // blockIdx.x -> (ti, tj), ti <= tj: row ti of the upper triangle holds ntiles - ti pairs
    int ti = 0, rem = blockIdx.x;
    while (rem >= ntiles - ti) { rem -= ntiles - ti; ++ti; }
    const int tj = ti + rem;
    const bool diag = ti == tj;
    const T eps2 = prm[b].eps2;
    const T *p = pos + (size_t)b * stride * D;
    const T *m = mass + (size_t)b * stride;

    const int j0 = tj * EE_TILE;
    const int cnt = min(EE_TILE, n - j0);            // >= 1: tj < ntiles
    // the pair loop's copies (stage_far_pe, nb_device.h): an infinite coordinate becomes NaN, as upstream's masked diagonal
    // makes the energy; the fp64 term's q^(-1/2) = y0 (1 + e / 2) needs a finite q, so far coordinates move to the star's slot
    constexpr T FAR = sizeof(T) == 8 ? (T)NB_FAR_F64 : (T)__builtin_inff();
    if (tid < cnt) {
#pragma unroll
        for (int k = 0; k < D; ++k) sx[k][tid] = stage_far_pe<T>(p[(size_t)(j0 + tid) * D + k], FAR, j0 + tid);
        sm[tid] = m[j0 + tid];
    }
    const int i = ti * EE_TILE + tid;
    const bool live = i < n;
    const int ic = live ? i : n - 1;
    T xi[D];
#pragma unroll
    for (int k = 0; k < D; ++k) xi[k] = stage_far_pe<T>(p[(size_t)ic * D + k], FAR, ic);
    const T mi = m[ic];
    __syncthreads();

    // two chains: a single accumulator would serialise the adds
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
    for (int jj = 0; jj < cnt; ++jj) {
        const bool take = live && (!diag || jj > tid);
        double term;
        if constexpr (sizeof(T) == 8) {
            double d[D];
#pragma unroll
            for (int k = 0; k < D; ++k) d[k] = sx[k][jj] - xi[k];
            term = pair_term<D>(d, eps2, mi, sm[jj]);
        } else {
            float d[D];
#pragma unroll
            for (int k = 0; k < D; ++k) d[k] = __fsub_rn(sx[k][jj], xi[k]);
            const float dist = __builtin_sqrtf(r2_f32_exact<D>(d, eps2));
            term = (double)__fdiv_rn(__fmul_rn(mi, sm[jj]), dist);
        }
        const double add = take ? term : 0.0;
        if (jj & 1) s1 += add;
        else s0 += add;
    }
    double pe = s0 + s1;

    double ke = 0.0;
    if (diag && live && vel) {
        const T *v = vel + ((size_t)b * stride + i) * D;
        if constexpr (sizeof(T) == 8) {
            double v2 = __dmul_rn(v[0], v[0]);
#pragma unroll
            for (int k = 1; k < D; ++k) v2 = __dadd_rn(v2, __dmul_rn(v[k], v[k]));
            ke = __dmul_rn(mi, v2);
        } else {
            float v2 = __fmul_rn(v[0], v[0]);
#pragma unroll
            for (int k = 1; k < D; ++k) v2 = __fadd_rn(v2, __fmul_rn(v[k], v[k]));
            ke = (double)__fmul_rn(mi, v2);
        }
    }

#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        pe += __shfl_xor(pe, off, 64);
        ke += __shfl_xor(ke, off, 64);
    }
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = pe; s_red[1][tid >> 6] = ke; }
    __syncthreads();
    if (tid == 0) {
        double tp = s_red[0][0], tk = s_red[1][0];
#pragma unroll
        for (int w = 1; w < EE_WAVES; ++w) { tp += s_red[0][w]; tk += s_red[1][w]; }
        double *slot = part + ((size_t)b * gridDim.x + blockIdx.x) * 2;
        slot[0] = tp;
        slot[1] = tk;
    }
}

// RAGGED: npairs is the stride of a member's slots, of which it adds its own first pairs(sizes[b])
template <typename T, bool RAGGED>
__global__ void __launch_bounds__(64)
ens_energy_finish_kernel(const double *__restrict__ part, int npairs, int members, const EnsScalars<T> *__restrict__ prm,
                         double *__restrict__ kinetic, double *__restrict__ potential, int64_t sample,
                         const int *__restrict__ sizes)
{
    const int b = blockIdx.x;
    const double *slots = part + (size_t)b * npairs * 2;
    if constexpr (RAGGED) {
        const int ntiles = (ens_member_count<true>(sizes, b, 1, 0) + EE_TILE - 1) / EE_TILE;
        npairs = ntiles * (ntiles + 1) / 2;
    }
    double pe = 0.0, ke = 0.0;
    for (int s = threadIdx.x; s < npairs; s += 64) {
        pe += slots[2 * s];
        ke += slots[2 * s + 1];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        pe += __shfl_xor(pe, off, 64);
        ke += __shfl_xor(ke, off, 64);
    }
    if (threadIdx.x == 0) {
        const EnsScalars<T> sc = prm[b];
        double u = -(double)sc.G * pe;
        // the upstream multiplies by the upper-triangle mask BEFORE dividing by the distance (simulation.py:189): the
        // masked entries are 0 / dist, which is 0 / 0 = NaN on the whole diagonal when eps2 is zero in T
        if (sc.eps2 == (T)0) u = __builtin_nan("");
        kinetic[sample * members + b] = 0.5 * ke;
        potential[sample * members + b] = u;
    }
}

}  // namespace

int nb_ens_energy_pairs(int n)
{
    const int ntiles = (n + EE_TILE - 1) / EE_TILE;
    return ntiles * (ntiles + 1) / 2;
}

hipError_t nb_launch_ens_energy(const void *pos, const void *vel, const void *mass, int members, int n, int dim, int is_f64,
                                const void *prm, double *part, double *kinetic, double *potential, int64_t sample,
                                hipStream_t st, const int *sizes)
{
    if (members < 1 || members > NB_ENS_MAX_MEMBERS || n < 1 || (dim != 2 && dim != 3)) return hipErrorInvalidValue;
    if (!pos || !mass || !prm || !part || !kinetic || !potential || sample < 0) return hipErrorInvalidValue;
    const int ntiles = (n + EE_TILE - 1) / EE_TILE, npairs = nb_ens_energy_pairs(n);
    const dim3 grid(npairs, members);
    return nb::pick_real(is_f64, [&](auto real) {
        using T = typename decltype(real)::type;
        const EnsScalars<T> *p = (const EnsScalars<T> *)prm;
        return nb::pick_bool(sizes != nullptr, [&](auto RG) {
            const hipError_t err = nb::pick<2, 3>(dim, [&](auto D) {
                hipLaunchKernelGGL((ens_energy_partials_kernel<T, D.value, RG.value>), grid, dim3(EE_TILE), 0, st, (const T *)pos,
                                   (const T *)vel, (const T *)mass, n, ntiles, p, part, sizes);
                return hipGetLastError();
            });
            if (err != hipSuccess) return err;
            hipLaunchKernelGGL((ens_energy_finish_kernel<T, RG.value>), dim3(members), dim3(64), 0, st, (const double *)part, npairs,
                               members, p, kinetic, potential, sample, sizes);
            return hipGetLastError();
        });
    });
}
