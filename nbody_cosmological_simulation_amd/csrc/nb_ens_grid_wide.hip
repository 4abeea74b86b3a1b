// nb_ens_grid_wide.hip -- the pair sweep of a CUSTOM ensemble with members above NB_LUT_MIN levels (nb_ens_create_grid_wide)
// and the bin read-out of the grid-mode ensembles (nb_ens_quant_bin_sums): ens_grid_step_kernel (nb_ensemble.hip) with the
// tables of small_grid_body (nb_small_body.h) in dynamic LDS, and both sweeps with BINS = true.
// A file of its own: with these kernels -- and their dynamic LDS -- in nb_ensemble.hip, the 24 ens_grid_step_kernel
// instantiations there came out with other wait counts and registers (the same arithmetic); apart, that file compiles to
// the code it compiled to before.
#include "nb_dispatch.h"
#include "nb_small_body.h"
#include "nb_internal.h"

namespace {

using namespace nbdev;

// CUSTOM members of up to NB_MAX_LUT levels (nb_ens_create_grid_wide, launched when a member exceeds NB_LUT_MIN): the same
// kernel with the tables in dynamic LDS, 2 (cap + 1) floats with cap = nb_lut_pad of the launch's widest member -- at most
// 32 776 bytes beside the 16 KiB source tile (D = 3) -- so the workgroups per CU follow the grid actually used.  Every
// member stages its own padded size; CUSTOM only, so there are no force bounds (`part`).
template <int D, int S, int BS, bool STOPS>
__global__ void __launch_bounds__(BS)
ens_grid_step_wide_kernel(const float *__restrict__ pos_in, float *__restrict__ pos_out, float *__restrict__ vel,
                          float *__restrict__ acc, const float *__restrict__ mass, int n,
                          const EnsScalars<float> *__restrict__ prm, int do_kick, const GridTables *__restrict__ tabs, int cap,
                          const int *__restrict__ stop, int t)
{
    extern __shared__ float s_wide_tabs[];
    const int b = blockIdx.y;
    const EnsScalars<float> p = prm[b];
    const size_t o = (size_t)b * n;
    const int left = ens_ticks_left<STOPS>(stop, b, t);
    if (STOPS && left <= 1) {
        ens_carry_positions<float, D, S, BS>(blockIdx.x, pos_in + o * D, pos_out + o * D, n);
        if (left <= 0) return;
        do_kick = ens_kick_mode(left, do_kick);
    }
    small_grid_body<D, S, false, BS, true>(blockIdx.x, pos_in + o * D, pos_out + o * D, vel + o * D, acc + o * D, mass + o, n,
                                           p.G, p.eps2, p.half_dt, p.dt, do_kick, tabs + b, nullptr, nullptr, s_wide_tabs, cap);
}

// The bin read-out of a grid-mode ensemble (nb_ens_quant_bin_sums): the two kernels above with BINS = true, forces only
// (NB_KICK_NONE, no stops, no force bounds) -- `acc` is the caller's scratch, and member b's sums and pair counts go to
// bin_out + b (2 n + 2), zeroed by the caller.
template <int D, int S, int BS, bool WIDE>
__global__ void __launch_bounds__(BS)
ens_grid_bins_kernel(const float *__restrict__ pos_in, float *__restrict__ acc, const float *__restrict__ mass, int n,
                     const EnsScalars<float> *__restrict__ prm, const GridTables *__restrict__ tabs, int cap,
                     unsigned long long *__restrict__ bin_out)
{
    extern __shared__ float s_wide_tabs[];
    const int b = blockIdx.y;
    const EnsScalars<float> p = prm[b];
    const size_t o = (size_t)b * n;
    small_grid_body<D, S, true, BS, WIDE>(blockIdx.x, pos_in + o * D, nullptr, nullptr, acc + o * D, mass + o, n, p.G, p.eps2,
                                          p.half_dt, p.dt, NB_KICK_NONE, tabs + b, nullptr, bin_out + (size_t)b * (2 * (size_t)n + 2),
                                          WIDE ? s_wide_tabs : nullptr, cap);
}

}  // namespace

hipError_t nb_launch_ens_grid_step_wide(const EnsStepArgs &a, int do_kick, const int *stop, int t, hipStream_t st)
{
    if (hipError_t err = nb_ens_step_check(a, do_kick, t)) return err;
    if (a.is_f64 || !a.tabs || a.max_levels < 2 || a.max_levels > NB_MAX_LUT) return hipErrorInvalidValue;
    const int cap = nb_lut_pad(a.max_levels);
    return nb::pick<2, 3>(a.dim, [&](auto D) {
        return nb::pick_small_step<512, 256>(a.lanes, nb_small_block(a.n), stop != nullptr, [&](auto S, auto BS, auto ST) {
            hipLaunchKernelGGL((ens_grid_step_wide_kernel<D.value, S.value, BS.value, ST.value>),
                               dim3(nb_small_blocks(a.n, a.lanes), a.members), dim3(BS.value), nb_lut_lds_bytes(a.max_levels), st,
                               (const float *)a.pos_in, (float *)a.pos_out, (float *)a.vel, (float *)a.acc, (const float *)a.mass,
                               a.n, (const EnsScalars<float> *)a.prm, do_kick, a.tabs, cap, stop, t);
            return hipGetLastError();
        });
    });
}

hipError_t nb_launch_ens_grid_bins(const float *pos, float *acc, const float *mass, int members, int n, int dim, const void *prm,
                                   int lanes, const GridTables *tabs, int max_levels, unsigned long long *bin_out, hipStream_t st)
{
    if (members < 1 || members > NB_ENS_MAX_MEMBERS || n < 1 || !tabs || !acc || !bin_out) return hipErrorInvalidValue;
    if (max_levels < 2 || max_levels > NB_MAX_LUT) return hipErrorInvalidValue;
    const bool wide = max_levels > NB_LUT_MIN;
    const int cap = nb_lut_pad(max_levels);
    return nb::pick<2, 3>(dim, [&](auto D) {
        return nb::pick_small_step<512, 256>(lanes, nb_small_block(n), wide, [&](auto S, auto BS, auto W) {
            hipLaunchKernelGGL((ens_grid_bins_kernel<D.value, S.value, BS.value, W.value>),
                               dim3(nb_small_blocks(n, lanes), members), dim3(BS.value), wide ? nb_lut_lds_bytes(max_levels) : 0,
                               st, pos, acc, mass, n, (const EnsScalars<float> *)prm, tabs, cap, bin_out);
            return hipGetLastError();
        });
    });
}
