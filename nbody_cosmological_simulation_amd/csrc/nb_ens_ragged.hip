// nb_ens_ragged.hip -- members of different sizes in one launch per tick (nb_ens_create_ragged, include/nbody_amd.h).
//
// The handle is an ordinary nb_ens whose n is the CAPACITY, the largest member: member b lives at offset b * capacity of the
// (B, capacity, D) / (B, capacity) buffers and owns the first sizes[b] rows; the rows behind them are padding that no kernel
// reads or writes.  A (blocks, members) grid sized for the capacity would launch capacity / 8 workgroups for a member of 16
// stars, so the launch runs over a 1-D list of work items instead (nb_plan_ragged, nb_plan.cpp): workgroup w reads
// work[w] = {member, blk} and runs the solo step's body (nb_small_body.h) on targets [blk * TG, (blk + 1) * TG) of that
// member with the member's own n and scalars.  The list holds the largest members first, blk ascending within a member:
// workgroups are dispatched in index order and a large member's workgroup streams more sources, so the tick ends with the
// short items.
//
// Why ONE workgroup size serves every member bit for bit: in small_step_body a target's sum depends on S (lane l takes
// sources l, l + S, ... of every SM_TILE tile, then the fixed butterfly over the S lanes), on SM_TILE and on the member's n
// -- not on BS, which only decides which targets share a workgroup and how the threads split the staging of a tile that
// holds the same values either way.  A solo run takes 256 threads for n in 2049 .. 3072 and 512 elsewhere; the member's
// bits are the same under NB_ENS_RAGGED_BLOCK (512) at every size.
//
// The hook is compiled in (a uniform handle) or HOOK_AT_RUN_TIME with hooks[member] (a mode list), as ens_step_kernel and
// ens_step_mixed_kernel have it; the stop rule is theirs (nb_device.h), with blk from the work item.
//
// The grid modes (nb_ens_create_ragged_grid: INT8 / INT4 / CUSTOM up to NB_LUT_MIN levels) run small_grid_body over the
// same work list (ens_grid_step_ragged_kernel), member b with its own tables.  There a pair's factor depends on which
// pairs share its WAVE (the table-free path's ballot), so the argument above needs one more line: a wave is 64 / S
// consecutive targets over all their sources, and its first target is a multiple of 64 / S at 256 and at 512 threads
// alike -- the set of pairs in a wave, hence every factor, is the solo run's at either workgroup size.
#include "nb_dispatch.h"
#include "nb_small_body.h"
#include "nb_internal.h"

namespace {

using namespace nbdev;

constexpr int ER_BLOCK = NB_ENS_RAGGED_BLOCK;

// waves per SIMD: 8, what ens_step_kernel / ens_step_mixed_kernel come out at by themselves (at most 55 VGPRs).  Left to
// itself the compiler gives the fp64 instantiations here 84 - 96 VGPRs (the four unrolled pairs interleaved) and 5 waves
// per SIMD: two 512-thread workgroups per CU instead of four.  With the attribute they have ens_step_kernel's registers
// (profiles/ensemble_ragged_step_resources.txt); no instantiation spills.
template <typename T, int D, int HOOK, int S, bool STOPS>
__global__ void __launch_bounds__(ER_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8)))
ens_step_ragged_kernel(const T *__restrict__ pos_in, T *__restrict__ pos_out, T *__restrict__ vel, T *__restrict__ acc,
                       const T *__restrict__ mass, int cap, const int *__restrict__ sizes, const EnsWork *__restrict__ work,
                       const EnsScalars<T> *__restrict__ prm, int do_kick, const int *__restrict__ hooks,
                       const int *__restrict__ stop, int t)
{
    const EnsWork w = work[blockIdx.x];              // member and target block: uniform per workgroup
    const int b = w.member;
    const int n = ens_member_count<true>(sizes, b, 1, cap);
    const EnsScalars<T> p = prm[b];
    const size_t o = (size_t)b * cap;
    const int left = ens_ticks_left<STOPS>(stop, b, t);
    if (STOPS && left <= 1) {
        ens_carry_positions<T, D, S, ER_BLOCK>(w.blk, pos_in + o * D, pos_out + o * D, n);
        if (left <= 0) return;
        do_kick = ens_kick_mode(left, do_kick);
    }
    int hook_rt = HOOK_NONE;
    if constexpr (HOOK == HOOK_AT_RUN_TIME) hook_rt = hooks[b];
    small_step_body<T, D, HOOK, S, ER_BLOCK>(w.blk, pos_in + o * D, pos_out + o * D, vel + o * D, acc + o * D, mass + o, n,
                                             p.G, p.eps2, p.half_dt, p.dt, do_kick, nullptr, hook_rt);
}

// grid hook over the work list: ens_grid_step_kernel's arguments and stop rule (nb_ensemble.hip) with the member, its size
// and its target block from the work item.  Under INT8 / INT4 (part != null) workgroup w.blk of member b leaves its
// {min, max} pair at part[(b * stride + w.blk) * 2], stride = nb_ens_ragged_blocks(cap, lanes): a member uses the first
// ceil(sizes[b] / (ER_BLOCK / S)) pairs of its row.  BINS (nb_ens_quant_bin_sums; without stops, kicks or bounds): acc is
// the caller's scratch, and member b's read-out goes to bin_out + b (2 cap + 2), laid out for the member's OWN n --
// {s1[n], s2[n], {table-free pairs, table pairs}} -- the words behind them are not written.
// waves per SIMD: 8, as the cast kernel above; ens_grid_step_kernel comes out there at 512 threads by itself
// (profiles/ensemble_ragged_grid_step_resources.txt).
template <int D, int S, bool STOPS, bool BINS>
__global__ void __launch_bounds__(ER_BLOCK)
ens_grid_step_ragged_kernel(const float *__restrict__ pos_in, float *__restrict__ pos_out, float *__restrict__ vel,
                            float *__restrict__ acc, const float *__restrict__ mass, int cap, const int *__restrict__ sizes,
                            const EnsWork *__restrict__ work, const EnsScalars<float> *__restrict__ prm, int do_kick,
                            const GridTables *__restrict__ tabs, double *__restrict__ part, int stride,
                            unsigned long long *__restrict__ bin_out, const int *__restrict__ stop, int t)
{
    static_assert(!(BINS && STOPS), "the bin read-out is an observer: no member is stopped for it");
    const EnsWork w = work[blockIdx.x];              // member and target block: uniform per workgroup
    const int b = w.member;
    const int n = ens_member_count<true>(sizes, b, 1, cap);
    const EnsScalars<float> p = prm[b];
    const size_t o = (size_t)b * cap;
    const int left = ens_ticks_left<STOPS>(stop, b, t);
    if (STOPS && left <= 1) {
        if (!part) ens_carry_positions<float, D, S, ER_BLOCK>(w.blk, pos_in + o * D, pos_out + o * D, n);   // (INT8 / INT4: no ping-pong)
        if (left <= 0) return;
        do_kick = ens_kick_mode(left, do_kick);
    }
    small_grid_body<D, S, BINS, ER_BLOCK>(w.blk, pos_in + o * D, pos_out + o * D, vel + o * D, acc + o * D, mass + o, n, p.G,
                                          p.eps2, p.half_dt, p.dt, do_kick, tabs + b,
                                          part ? part + (size_t)b * 2 * stride : nullptr,
                                          BINS ? bin_out + (size_t)b * (2 * (size_t)cap + 2) : nullptr);
}

}  // namespace

hipError_t nb_launch_ens_step_ragged(const EnsStepArgs &a, int do_kick, const int *stop, int t, hipStream_t st)
{
    if (hipError_t err = nb_ens_step_check(a, do_kick, t)) return err;       // (a.n: the capacity)
    if (!a.sizes || !a.work || a.items < 1) return hipErrorInvalidValue;
    if (a.hook == HOOK_AT_RUN_TIME && (a.is_f64 || !a.hooks)) return hipErrorInvalidValue;
    return nb::pick<2, 3>(a.dim, [&](auto D) {
        auto launch = [&](auto real, auto H) {
            using T = typename decltype(real)::type;
            // ONE workgroup size: the ladder's block is not a choice here
            return nb::pick_small_step<ER_BLOCK>(a.lanes, ER_BLOCK, stop != nullptr, [&](auto S, auto, auto ST) {
                hipLaunchKernelGGL((ens_step_ragged_kernel<T, D.value, H.value, S.value, ST.value>), dim3(a.items), dim3(ER_BLOCK),
                                   0, st, (const T *)a.pos_in, (T *)a.pos_out, (T *)a.vel, (T *)a.acc, (const T *)a.mass, a.n,
                                   a.sizes, a.work, (const EnsScalars<T> *)a.prm, do_kick, a.hooks, stop, t);
                return hipGetLastError();
            });
        };
        if (a.is_f64) return nb::pick<HOOK_NONE>(a.hook, [&](auto H) { return launch(nb::real_tag<double>{}, H); });
        return nb::pick<HOOK_NONE, HOOK_BF16, HOOK_F16, HOOK_AT_RUN_TIME>(a.hook, [&](auto H) {
            return launch(nb::real_tag<float>{}, H);
        });
    });
}

hipError_t nb_launch_ens_grid_step_ragged(const EnsStepArgs &a, int do_kick, const int *stop, int t, hipStream_t st)
{
    if (hipError_t err = nb_ens_step_check(a, do_kick, t)) return err;       // (a.n: the capacity)
    if (!a.sizes || !a.work || a.items < 1 || a.is_f64 || !a.tabs) return hipErrorInvalidValue;
    if (a.max_levels < 2 || a.max_levels > NB_LUT_MIN) return hipErrorInvalidValue;
    return nb::pick<2, 3>(a.dim, [&](auto D) {
        return nb::pick_small_step<ER_BLOCK>(a.lanes, ER_BLOCK, stop != nullptr, [&](auto S, auto, auto ST) {
            hipLaunchKernelGGL((ens_grid_step_ragged_kernel<D.value, S.value, ST.value, false>), dim3(a.items), dim3(ER_BLOCK), 0,
                               st, (const float *)a.pos_in, (float *)a.pos_out, (float *)a.vel, (float *)a.acc,
                               (const float *)a.mass, a.n, a.sizes, a.work, (const EnsScalars<float> *)a.prm, do_kick, a.tabs,
                               a.part, nb_ens_ragged_blocks(a.n, a.lanes), nullptr, stop, t);
            return hipGetLastError();
        });
    });
}

hipError_t nb_launch_ens_grid_bins_ragged(const EnsStepArgs &a, float *acc, unsigned long long *bin_out, hipStream_t st)
{
    if (a.members < 1 || a.members > NB_ENS_MAX_MEMBERS || a.n < 1 || !acc || !bin_out) return hipErrorInvalidValue;
    if (!a.sizes || !a.work || a.items < 1 || a.is_f64 || !a.tabs) return hipErrorInvalidValue;
    if (a.max_levels < 2 || a.max_levels > NB_LUT_MIN) return hipErrorInvalidValue;
    return nb::pick<2, 3>(a.dim, [&](auto D) {
        return nb::pick<64, 32, 16>(a.lanes, [&](auto S) {
            hipLaunchKernelGGL((ens_grid_step_ragged_kernel<D.value, S.value, false, true>), dim3(a.items), dim3(ER_BLOCK), 0, st,
                               (const float *)a.pos_in, nullptr, nullptr, acc, (const float *)a.mass, a.n, a.sizes, a.work,
                               (const EnsScalars<float> *)a.prm, (int)NB_KICK_NONE, a.tabs, nullptr, 0, bin_out, nullptr, 0);
            return hipGetLastError();
        });
    });
}
