// nb_ensemble.hip -- many small systems per launch (nb_ens handles, include/nbody_amd.h).
//
// A system of a few hundred to a few thousand particles is one small_step_kernel launch per step (nb_small.hip) that
// fills a fraction of the chip: N = 1024 is 128 workgroups on 256 CUs, N = 256 is 32.  A sweep over B independent systems
// of the same shape (parameter scans, seeds) is B such latency-bound launches per tick.  Here the B systems advance in ONE
// launch: gridDim.y = B, blockIdx.y picks the member, and every workgroup runs the solo step's body (nb_small_body.h) on
// its member's slice of contiguous (B, N, D) / (B, N) buffers with the member's own scalars.  No arithmetic crosses
// members, and a member's sums are rounded in the solo order (same lanes per target, same workgroup size).
// The grid modes (INT8 / INT4 / CUSTOM) run small_grid_body the same way, each member with its own tables
// (ens_grid_step_kernel); their max-r2 + tables launch is ens_r2max_tables_kernel (nb_grid.hip) and the INT8 / INT4 force
// snap ens_force_quant_finish_kernel (nb_misc.hip).
//
// Members of different sizes (nb_ens_create_ragged) have their own step kernel over a work list, nb_ens_ragged.hip; of the
// kernels here they launch the kick + drift with `sizes` (its RAGGED instantiation, nb_device.h).
//
// Per-member stops (nb_ens_run_members): every kernel of the tick path takes `stop` and the launch's tick index t and comes
// in two instantiations, with and without the array; nb_device.h states the rule and implements it (ens_ticks_left).
#include "nb_dispatch.h"
#include "nb_small_body.h"
#include "nb_internal.h"

namespace {

using namespace nbdev;

template <typename T, int D, int HOOK, int S, int BS, bool STOPS>
__global__ void __launch_bounds__(BS)
ens_step_kernel(const T *__restrict__ pos_in, T *__restrict__ pos_out, T *__restrict__ vel, T *__restrict__ acc,
                const T *__restrict__ mass, int n, const EnsScalars<T> *__restrict__ prm, int do_kick,
                const int *__restrict__ stop, int t)
{
    const int b = blockIdx.y;                        // member: uniform per workgroup
    const EnsScalars<T> p = prm[b];
    const size_t o = (size_t)b * n;
    const int left = ens_ticks_left<STOPS>(stop, b, t);
    if (STOPS && left <= 1) {
        ens_carry_positions<T, D, S, BS>(blockIdx.x, pos_in + o * D, pos_out + o * D, n);
        if (left <= 0) return;
        do_kick = ens_kick_mode(left, do_kick);
    }
    small_step_body<T, D, HOOK, S, BS>(blockIdx.x, pos_in + o * D, pos_out + o * D, vel + o * D, acc + o * D, mass + o, n,
                                       p.G, p.eps2, p.half_dt, p.dt, do_kick, nullptr);
}

// Members of different cast modes in one launch (nb_ens_create_mixed; fp32 state): ens_step_kernel<float, ...> with the
// hook read per member from hooks[b] (HOOK_NONE / HOOK_BF16 / HOOK_F16) instead of compiled in.  The body is the same
// small_step_body with the hook as a workgroup-uniform argument: member b performs the operations of the uniform kernel of
// its hook, in the same order, on one copy of the LDS tile.
template <int D, int S, int BS, bool STOPS>
__global__ void __launch_bounds__(BS)
ens_step_mixed_kernel(const float *__restrict__ pos_in, float *__restrict__ pos_out, float *__restrict__ vel,
                      float *__restrict__ acc, const float *__restrict__ mass, int n, const EnsScalars<float> *__restrict__ prm,
                      int do_kick, const int *__restrict__ hooks, const int *__restrict__ stop, int t)
{
    const int b = blockIdx.y;                        // member: uniform per workgroup
    const EnsScalars<float> p = prm[b];
    const size_t o = (size_t)b * n;
    const int left = ens_ticks_left<STOPS>(stop, b, t);
    if (STOPS && left <= 1) {
        ens_carry_positions<float, D, S, BS>(blockIdx.x, pos_in + o * D, pos_out + o * D, n);
        if (left <= 0) return;
        do_kick = ens_kick_mode(left, do_kick);
    }
    small_step_body<float, D, HOOK_AT_RUN_TIME, S, BS>(blockIdx.x, pos_in + o * D, pos_out + o * D, vel + o * D, acc + o * D,
                                                       mass + o, n, p.G, p.eps2, p.half_dt, p.dt, do_kick, nullptr, hooks[b]);
}

// grid hook: member b reads the tables its own max-r2 launch built (tabs[b]); under INT8 / INT4 (part != null) it leaves
// one {min, max} pair of its forces per workgroup at part[(b * gridDim.x + blockIdx.x) * 2]
template <int D, int S, int BS, bool STOPS>
__global__ void __launch_bounds__(BS)
ens_grid_step_kernel(const float *__restrict__ pos_in, float *__restrict__ pos_out, float *__restrict__ vel,
                     float *__restrict__ acc, const float *__restrict__ mass, int n, const EnsScalars<float> *__restrict__ prm,
                     int do_kick, const GridTables *__restrict__ tabs, double *__restrict__ part,
                     const int *__restrict__ stop, int t)
{
    const int b = blockIdx.y;
    const EnsScalars<float> p = prm[b];
    const size_t o = (size_t)b * n;
    const int left = ens_ticks_left<STOPS>(stop, b, t);
    if (STOPS && left <= 1) {
        if (!part) ens_carry_positions<float, D, S, BS>(blockIdx.x, pos_in + o * D, pos_out + o * D, n);   // (INT8 / INT4: no ping-pong)
        if (left <= 0) return;
        do_kick = ens_kick_mode(left, do_kick);
    }
    small_grid_body<D, S, false, BS>(blockIdx.x, pos_in + o * D, pos_out + o * D, vel + o * D, acc + o * D, mass + o, n, p.G,
                                     p.eps2, p.half_dt, p.dt, do_kick, tabs + b,
                                     part ? part + (size_t)b * 2 * gridDim.x : nullptr, nullptr);
}

// opening kick + drift of a run (simulation.py:132,135) for every member with its own dt: v += a dt/2; x += v dt
constexpr int EK_BLOCK = 256;
// RAGGED (sizes, dim: nb_device.h): count is the stride of a member's slice, of which it owns the first sizes[b] * dim
template <typename T, bool STOPS, bool RAGGED>
__global__ void __launch_bounds__(EK_BLOCK)
ens_kick_drift_kernel(T *__restrict__ pos, T *__restrict__ vel, const T *__restrict__ acc, int count /* n * D */,
                      const EnsScalars<T> *__restrict__ prm, const int *__restrict__ stop, int t,
                      const int *__restrict__ sizes, int dim)
{
    const int b = blockIdx.y;
    if (ens_ticks_left<STOPS>(stop, b, t) <= 0) return;      // the member opens no further tick
    const T half_dt = prm[b].half_dt, dt = prm[b].dt;
    const size_t o = (size_t)b * count;
    const int mine = ens_member_count<RAGGED>(sizes, b, dim, count);
    for (int k = blockIdx.x * EK_BLOCK + threadIdx.x; k < mine; k += gridDim.x * EK_BLOCK) {
        const T v = axpy_rn<T>(vel[o + k], acc[o + k], half_dt);
        vel[o + k] = v;
        pos[o + k] = axpy_rn<T>(pos[o + k], v, dt);
    }
}

}  // namespace

hipError_t nb_ens_step_check(const EnsStepArgs &a, int do_kick, int t)
{
    if (a.members < 1 || a.members > NB_ENS_MAX_MEMBERS || a.n < 1 || t < 0) return hipErrorInvalidValue;
    const int km = do_kick & NB_KICK_MODE_MASK;
    if (km == NB_KICK_CLOSE_SPEC || (do_kick & NB_KICK_OPEN_ON_READ)) return hipErrorInvalidValue;
    if (a.part && km != NB_KICK_NONE) return hipErrorInvalidValue;      // INT8 / INT4: the finish launch carries the kicks
    return hipSuccess;
}

hipError_t nb_launch_ens_step(const EnsStepArgs &a, int do_kick, const int *stop, int t, hipStream_t st)
{
    if (hipError_t err = nb_ens_step_check(a, do_kick, t)) return err;
    return nb::pick<2, 3>(a.dim, [&](auto D) {
        auto launch = [&](auto real, auto H) {
            using T = typename decltype(real)::type;
            return nb::pick_small_step<512, 256>(a.lanes, nb_small_block(a.n), stop != nullptr, [&](auto S, auto BS, auto ST) {
                hipLaunchKernelGGL((ens_step_kernel<T, D.value, H.value, S.value, BS.value, ST.value>),
                                   dim3(nb_small_blocks(a.n, a.lanes), a.members), dim3(BS.value), 0, st, (const T *)a.pos_in,
                                   (T *)a.pos_out, (T *)a.vel, (T *)a.acc, (const T *)a.mass, a.n, (const EnsScalars<T> *)a.prm,
                                   do_kick, stop, t);
                return hipGetLastError();
            });
        };
        if (a.is_f64) return nb::pick<HOOK_NONE>(a.hook, [&](auto H) { return launch(nb::real_tag<double>{}, H); });
        return nb::pick<HOOK_NONE, HOOK_BF16, HOOK_F16>(a.hook, [&](auto H) { return launch(nb::real_tag<float>{}, H); });
    });
}

hipError_t nb_launch_ens_step_mixed(const EnsStepArgs &a, int do_kick, const int *stop, int t, hipStream_t st)
{
    if (hipError_t err = nb_ens_step_check(a, do_kick, t)) return err;
    if (a.is_f64 || !a.hooks) return hipErrorInvalidValue;
    return nb::pick<2, 3>(a.dim, [&](auto D) {
        return nb::pick_small_step<512, 256>(a.lanes, nb_small_block(a.n), stop != nullptr, [&](auto S, auto BS, auto ST) {
            hipLaunchKernelGGL((ens_step_mixed_kernel<D.value, S.value, BS.value, ST.value>),
                               dim3(nb_small_blocks(a.n, a.lanes), a.members), dim3(BS.value), 0, st, (const float *)a.pos_in,
                               (float *)a.pos_out, (float *)a.vel, (float *)a.acc, (const float *)a.mass, a.n,
                               (const EnsScalars<float> *)a.prm, do_kick, a.hooks, stop, t);
            return hipGetLastError();
        });
    });
}

hipError_t nb_launch_ens_grid_step(const EnsStepArgs &a, int do_kick, const int *stop, int t, hipStream_t st)
{
    if (hipError_t err = nb_ens_step_check(a, do_kick, t)) return err;
    if (a.is_f64 || !a.tabs) return hipErrorInvalidValue;
    return nb::pick<2, 3>(a.dim, [&](auto D) {
        return nb::pick_small_step<512, 256>(a.lanes, nb_small_block(a.n), stop != nullptr, [&](auto S, auto BS, auto ST) {
            hipLaunchKernelGGL((ens_grid_step_kernel<D.value, S.value, BS.value, ST.value>),
                               dim3(nb_small_blocks(a.n, a.lanes), a.members), dim3(BS.value), 0, st, (const float *)a.pos_in,
                               (float *)a.pos_out, (float *)a.vel, (float *)a.acc, (const float *)a.mass, a.n,
                               (const EnsScalars<float> *)a.prm, do_kick, a.tabs, a.part, stop, t);
            return hipGetLastError();
        });
    });
}

hipError_t nb_launch_ens_kick_drift(void *pos, void *vel, const void *acc, int members, int n, int dim, int is_f64,
                                    const void *prm, const int *stop, int t, hipStream_t st, const int *sizes)
{
    if (members < 1 || members > NB_ENS_MAX_MEMBERS || n < 1 || (dim != 2 && dim != 3) || t < 0) return hipErrorInvalidValue;
    const int count = n * dim;
    const dim3 grid((count + EK_BLOCK - 1) / EK_BLOCK, members);
    return nb::pick_real(is_f64, [&](auto real) {
        using T = typename decltype(real)::type;
        return nb::pick_bool(stop != nullptr, [&](auto ST) {
            return nb::pick_bool(sizes != nullptr, [&](auto RG) {
                hipLaunchKernelGGL((ens_kick_drift_kernel<T, ST.value, RG.value>), grid, dim3(EK_BLOCK), 0, st, (T *)pos, (T *)vel,
                                   (const T *)acc, count, (const EnsScalars<T> *)prm, stop, t, sizes, dim);
                return hipGetLastError();
            });
        });
    });
}
