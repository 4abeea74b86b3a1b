// nb_ensemble.hip -- many small systems per launch (nb_ens handles, include/nbody_amd.h).
//
// A system of a few hundred to a few thousand particles is one small_step_kernel launch per step (nb_small.hip) that
// fills a fraction of the chip: N = 1024 is 128 workgroups on 256 CUs, N = 256 is 32.  A sweep over B independent systems
// of the same shape (parameter scans, seeds) is B such latency-bound launches per tick.  Here the B systems advance in ONE
// launch: gridDim.y = B, blockIdx.y picks the member, and every workgroup runs the solo step's body (nb_small_body.h) on
// its member's slice of contiguous (B, N, D) / (B, N) buffers with the member's own scalars.  No arithmetic crosses
// members, and a member's sums are rounded in the solo order (same lanes per target, same workgroup size).
// The grid modes (INT8 / INT4 / CUSTOM) run small_grid_body the same way, each member with its own tables
// (ens_grid_step_kernel); their max-r2 + tables launch is ens_r2max_tables_kernel (nb_force.hip) and the INT8 / INT4 force
// snap ens_force_quant_finish_kernel (nb_misc.hip).
#include "nb_small_body.h"
#include "nb_internal.h"

namespace {

using namespace nbdev;

// scalars of one member, already cast to T on the host as nb_launch_small_step casts the solo step's
template <typename T>
struct EnsScalars {
    T G, eps2, half_dt, dt;
};
static_assert(sizeof(EnsScalars<double>) == NB_ENS_PARAM_WORDS * 8 && sizeof(EnsScalars<float>) == NB_ENS_PARAM_WORDS * 4,
              "the host fills NB_ENS_PARAM_WORDS elements per member");

template <typename T, int D, int HOOK, int S, int BS>
__global__ void __launch_bounds__(BS)
ens_step_kernel(const T *__restrict__ pos_in, T *__restrict__ pos_out, T *__restrict__ vel, T *__restrict__ acc,
                const T *__restrict__ mass, int n, const EnsScalars<T> *__restrict__ prm, int do_kick)
{
    const int b = blockIdx.y;                        // member: uniform per workgroup
    const EnsScalars<T> p = prm[b];
    const size_t o = (size_t)b * n;
    small_step_body<T, D, HOOK, S, BS>(blockIdx.x, pos_in + o * D, pos_out + o * D, vel + o * D, acc + o * D, mass + o, n,
                                       p.G, p.eps2, p.half_dt, p.dt, do_kick, nullptr);
}

// grid hook: member b reads the tables its own max-r2 launch built (tabs[b]); under INT8 / INT4 (part != null) it leaves
// one {min, max} pair of its forces per workgroup at part[(b * gridDim.x + blockIdx.x) * 2]
template <int D, int S, int BS>
__global__ void __launch_bounds__(BS)
ens_grid_step_kernel(const float *__restrict__ pos_in, float *__restrict__ pos_out, float *__restrict__ vel,
                     float *__restrict__ acc, const float *__restrict__ mass, int n, const EnsScalars<float> *__restrict__ prm,
                     int do_kick, const GridTables *__restrict__ tabs, double *__restrict__ part)
{
    const int b = blockIdx.y;
    const EnsScalars<float> p = prm[b];
    const size_t o = (size_t)b * n;
    small_grid_body<D, S, false, BS>(blockIdx.x, pos_in + o * D, pos_out + o * D, vel + o * D, acc + o * D, mass + o, n, p.G,
                                     p.eps2, p.half_dt, p.dt, do_kick, tabs + b,
                                     part ? part + (size_t)b * 2 * gridDim.x : nullptr, nullptr);
}

// opening kick + drift of a run (simulation.py:132,135) for every member with its own dt: v += a dt/2; x += v dt
constexpr int EK_BLOCK = 256;
template <typename T>
__global__ void __launch_bounds__(EK_BLOCK)
ens_kick_drift_kernel(T *__restrict__ pos, T *__restrict__ vel, const T *__restrict__ acc, int count /* n * D */,
                      const EnsScalars<T> *__restrict__ prm)
{
    const int b = blockIdx.y;
    const T half_dt = prm[b].half_dt, dt = prm[b].dt;
    const size_t o = (size_t)b * count;
    for (int k = blockIdx.x * EK_BLOCK + threadIdx.x; k < count; k += gridDim.x * EK_BLOCK) {
        const T v = axpy_sep<T>(vel[o + k], acc[o + k], half_dt);
        vel[o + k] = v;
        pos[o + k] = axpy_sep<T>(pos[o + k], v, dt);
    }
}

template <typename T, int D, int HOOK>
hipError_t launch_e(const T *pos_in, T *pos_out, T *vel, T *acc, const T *mass, int members, int n, const void *prm,
                    int do_kick, int lanes, hipStream_t st)
{
    const EnsScalars<T> *p = (const EnsScalars<T> *)prm;
#define NB_ENS(SS)                                                                                                         \
    do {                                                                                                                   \
        if (nb_small_block(n) == 512)                                                                                      \
            hipLaunchKernelGGL((ens_step_kernel<T, D, HOOK, SS, 512>), dim3((n + 512 / SS - 1) / (512 / SS), members),     \
                               dim3(512), 0, st, pos_in, pos_out, vel, acc, mass, n, p, do_kick);                          \
        else                                                                                                               \
            hipLaunchKernelGGL((ens_step_kernel<T, D, HOOK, SS, 256>), dim3((n + 256 / SS - 1) / (256 / SS), members),     \
                               dim3(256), 0, st, pos_in, pos_out, vel, acc, mass, n, p, do_kick);                          \
    } while (0)
    if (lanes == 64) NB_ENS(64);
    else if (lanes == 32) NB_ENS(32);
    else NB_ENS(16);
#undef NB_ENS
    return hipGetLastError();
}

template <int D>
hipError_t launch_g(const float *pos_in, float *pos_out, float *vel, float *acc, const float *mass, int members, int n,
                    const void *prm, int do_kick, int lanes, const GridTables *tabs, double *part, hipStream_t st)
{
    const EnsScalars<float> *p = (const EnsScalars<float> *)prm;
#define NB_ENSG(SS)                                                                                                        \
    do {                                                                                                                   \
        if (nb_small_block(n) == 512)                                                                                      \
            hipLaunchKernelGGL((ens_grid_step_kernel<D, SS, 512>), dim3((n + 512 / SS - 1) / (512 / SS), members),         \
                               dim3(512), 0, st, pos_in, pos_out, vel, acc, mass, n, p, do_kick, tabs, part);              \
        else                                                                                                               \
            hipLaunchKernelGGL((ens_grid_step_kernel<D, SS, 256>), dim3((n + 256 / SS - 1) / (256 / SS), members),         \
                               dim3(256), 0, st, pos_in, pos_out, vel, acc, mass, n, p, do_kick, tabs, part);              \
    } while (0)
    if (lanes == 64) NB_ENSG(64);
    else if (lanes == 32) NB_ENSG(32);
    else NB_ENSG(16);
#undef NB_ENSG
    return hipGetLastError();
}

}  // namespace

hipError_t nb_launch_ens_step(const void *pos_in, void *pos_out, void *vel, void *acc, const void *mass, int members, int n,
                              int dim, int is_f64, int hook, const void *prm, int do_kick, int lanes, hipStream_t st)
{
    if (dim != 2 && dim != 3) return hipErrorInvalidValue;
    if (members < 1 || members > NB_ENS_MAX_MEMBERS || n < 1) return hipErrorInvalidValue;
    if ((do_kick & NB_KICK_MODE_MASK) == NB_KICK_CLOSE_SPEC || (do_kick & NB_KICK_OPEN_ON_READ)) return hipErrorInvalidValue;
    if (is_f64) {
        if (hook != HOOK_NONE) return hipErrorInvalidValue;
        if (dim == 2) return launch_e<double, 2, HOOK_NONE>((const double *)pos_in, (double *)pos_out, (double *)vel, (double *)acc, (const double *)mass, members, n, prm, do_kick, lanes, st);
        return launch_e<double, 3, HOOK_NONE>((const double *)pos_in, (double *)pos_out, (double *)vel, (double *)acc, (const double *)mass, members, n, prm, do_kick, lanes, st);
    }
    if (hook != HOOK_NONE && hook != HOOK_BF16 && hook != HOOK_F16) return hipErrorInvalidValue;
#define NB_EF(DD, HH) launch_e<float, DD, HH>((const float *)pos_in, (float *)pos_out, (float *)vel, (float *)acc, (const float *)mass, members, n, prm, do_kick, lanes, st)
    if (dim == 2) {
        if (hook == HOOK_BF16) return NB_EF(2, HOOK_BF16);
        if (hook == HOOK_F16) return NB_EF(2, HOOK_F16);
        return NB_EF(2, HOOK_NONE);
    }
    if (hook == HOOK_BF16) return NB_EF(3, HOOK_BF16);
    if (hook == HOOK_F16) return NB_EF(3, HOOK_F16);
    return NB_EF(3, HOOK_NONE);
#undef NB_EF
}

int nb_ens_grid_blocks(int n, int lanes) { return (n + nb_small_block(n) / lanes - 1) / (nb_small_block(n) / lanes); }

hipError_t nb_launch_ens_grid_step(const float *pos_in, float *pos_out, float *vel, float *acc, const float *mass, int members,
                                   int n, int dim, const void *prm, int do_kick, int lanes, const GridTables *tabs, double *part,
                                   hipStream_t st)
{
    if (dim != 2 && dim != 3) return hipErrorInvalidValue;
    if (members < 1 || members > NB_ENS_MAX_MEMBERS || n < 1 || !tabs) return hipErrorInvalidValue;
    if (lanes != 16 && lanes != 32 && lanes != 64) return hipErrorInvalidValue;
    const int km = do_kick & NB_KICK_MODE_MASK;
    if (km == NB_KICK_CLOSE_SPEC || (do_kick & NB_KICK_OPEN_ON_READ)) return hipErrorInvalidValue;
    if (part && km != NB_KICK_NONE) return hipErrorInvalidValue;      // INT8 / INT4: the finish launch carries the kicks
    if (dim == 2) return launch_g<2>(pos_in, pos_out, vel, acc, mass, members, n, prm, do_kick, lanes, tabs, part, st);
    return launch_g<3>(pos_in, pos_out, vel, acc, mass, members, n, prm, do_kick, lanes, tabs, part, st);
}

hipError_t nb_launch_ens_kick_drift(void *pos, void *vel, const void *acc, int members, int n, int dim, int is_f64,
                                    const void *prm, hipStream_t st)
{
    if (members < 1 || members > NB_ENS_MAX_MEMBERS || n < 1 || (dim != 2 && dim != 3)) return hipErrorInvalidValue;
    const int count = n * dim;
    const dim3 grid((count + EK_BLOCK - 1) / EK_BLOCK, members);
    if (is_f64)
        hipLaunchKernelGGL((ens_kick_drift_kernel<double>), grid, dim3(EK_BLOCK), 0, st, (double *)pos, (double *)vel,
                           (const double *)acc, count, (const EnsScalars<double> *)prm);
    else
        hipLaunchKernelGGL((ens_kick_drift_kernel<float>), grid, dim3(EK_BLOCK), 0, st, (float *)pos, (float *)vel,
                           (const float *)acc, count, (const EnsScalars<float> *)prm);
    return hipGetLastError();
}
