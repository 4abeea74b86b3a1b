// nb_small.hip -- one launch per leapfrog step for small systems (N up to a few thousand).
//
// Small systems are bound by LATENCY, not throughput: a force launch, a reduction launch and the kernel boundaries
// between them (~1.5 us each, /opt/skills/guides/MI355X_MICROARCH.md "boundary") cost more than the arithmetic
// (N = 1024: 0.5 M pairs = 0.3 us of the chip's VALU time).  A grid barrier inside a persistent kernel costs 4-10 us
// on this machine (same guide, "barrier-xcd"), i.e. MORE than a kernel boundary, so the step is not made persistent;
// instead the whole step is ONE launch with no cross-workgroup reduction at all:
//   * S lanes of a wavefront share one target and split the sources between them (S = 16 / 32 / 64 by size), so a
//     target's sum is finished by a fixed butterfly of wave shuffles -- no slabs, no second kernel;
//   * every workgroup stages the sources through LDS in tiles of 1024 (coalesced loads; lanes of a group read
//     consecutive entries, groups read the same entries: conflict-free broadcasts);
//   * the lane that holds a finished sum applies the closing half kick and, inside nb_step, the NEXT step's opening
//     kick + drift, writing the new positions to a second buffer (other workgroups still read the old ones): the
//     positions ping-pong between two buffers, one launch per step.
// One-sided (each ordered pair evaluated), which at these sizes is free: the chip is mostly idle.
// Arithmetic per pair is that of the tuned kernels (fp64: v_rsq_f64 + second-order correction; fp32: reference op
// order for r2 without fma, cast hooks, v_rsq_f32 + first-order correction, fp32 products summed in fp64).
#include "nb_device.h"
#include "nb_dispatch.h"
#include "nb_small_body.h"

#include <cstdlib>

namespace {

using namespace nbdev;

// the pair loop, butterfly and kicks (and SM_TILE, inv_r3_*): nb_small_body.h, shared with the batched steps of
// nb_ensemble.hip -- small_step_body for the cast hooks, small_grid_body for the grid hook

// do_kick: an NbKick mode, | NB_KICK_OPEN_ON_READ (nb_internal.h); the drifted positions go to pos_out
// BINS (grid hook only): the same body with the quant-bin read-out into bin_out (small_grid_body).
// BS: threads per workgroup.  Every workgroup streams ALL sources through its LDS, so the L2 -> LDS traffic of a step is
// N^2 * 24 B / (targets per workgroup): 512 threads (8 targets of 64 lanes) halve it against 256; used up to N = 2048,
// where all workgroups still run in one round (nb_small_block).
template <typename T, int D, int HOOK, int S, bool BINS = false, int BS = NB_BLOCK>
__global__ void __launch_bounds__(BS)
small_step_kernel(const T *__restrict__ pos_in, T *__restrict__ pos_out, T *__restrict__ vel, T *__restrict__ acc,
                  const T *__restrict__ mass, int n, T G, T eps2, T half_dt, T dt, int do_kick,
                  const GridTables *__restrict__ tab, double *__restrict__ part, unsigned long long *__restrict__ bin_out)
{
    if constexpr (HOOK != HOOK_GRID) {
        small_step_body<T, D, HOOK, S, BS>(blockIdx.x, pos_in, pos_out, vel, acc, mass, n, G, eps2, half_dt, dt, do_kick, part);
    } else {
        static_assert(sizeof(T) == 4, "the grid hook runs on fp32 state");
        small_grid_body<D, S, BINS, BS>(blockIdx.x, pos_in, pos_out, vel, acc, mass, n, G, eps2, half_dt, dt, do_kick, tab, part,
                                        bin_out);
    }
}

template <typename T, int D, int HOOK, bool BINS = false>
hipError_t launch_s(const void *pos_in, void *pos_out, void *vel, void *acc, const void *mass, int n, double G, double eps2,
                    double half_dt, double dt, int do_kick, int lanes, hipStream_t st, const GridTables *tab = nullptr,
                    double *part = nullptr, unsigned long long *bin_out = nullptr)
{
    return nb::pick<64, 32, 16>(lanes, [&](auto S) {
        return nb::pick<512, 256>(nb_small_block(n), [&](auto BS) {
            hipLaunchKernelGGL((small_step_kernel<T, D, HOOK, S.value, BINS, BS.value>), dim3(nb_small_blocks(n, lanes)),
                               dim3(BS.value), 0, st, (const T *)pos_in, (T *)pos_out, (T *)vel, (T *)acc, (const T *)mass, n, (T)G,
                               (T)eps2, (T)half_dt, (T)dt, do_kick, tab, part, bin_out);
            return hipGetLastError();
        });
    });
}

}  // namespace

// lanes per target by size: enough lanes to keep a lane's source loop short, few enough that the source tiles every
// workgroup re-reads from L2 stay small (N^2 * S * 0.1 bytes per step)
// threads per workgroup of the one-launch step (see small_step_kernel): NB_SMALL_BLOCK overrides (A/B)
int nb_small_block(int n)
{
    static const int forced = getenv("NB_SMALL_BLOCK") ? atoi(getenv("NB_SMALL_BLOCK")) : 0;
    if (forced == 256 || forced == 512) return forced;
    // measured fp64 us per step, 256 / 512 / 1024 threads: N = 1024 5.4 / 5.2 / -, 2048 8.4 / 7.5 / -, 2500 10.9 / 11.3 / 11.3,
    // 3000 11.9 / 12.5 / 12.4, 4096 17.2 / 17.4 / 24.8: the larger workgroup wins while all of them fit the chip in one round
    // ... and again above N = 3072 (fp64 only gets there), with 64 lanes per target: N = 4096 15.7 (512 x 64) vs 17.2
    // (256 x 32) / 17.9 (256 x 64)
    return (n <= 2048 || n > 3072) ? 512 : 256;
}

// workgroups of the one-launch step: nb_small_block(n) / lanes targets each.  The force-bound partials (`part`) hold one
// {min, max} pair per workgroup, so whoever sizes or reads them takes the count from here
int nb_small_blocks(int n, int lanes)
{
    const int targets = nb_small_block(n) / lanes;
    return (n + targets - 1) / targets;
}

int nb_small_lanes(int n)
{
    // measured (fp32, us per step at N = 1024 / 2048 / 3000 / 4096): 16 lanes 6.8 / 11.4 / 15.9 / 20.5, 32 lanes
    // 5.4 / 8.5 / 12.5 / 15.5, 64 lanes 4.7 / 7.5 / 10.3 / 15.8 (two-launch path: 8.0 / 9.5 / 11.5 / 16.0);
    // fp64: 64 lanes 4.9 / 7.9 / 11.4 / 17.2, 32 lanes 5.5 / 8.8 / 13.3 / 16.9 (two-launch path: 8.3 / 12.5 / 19.1 / 21.3)
    return 64;       // (32 lanes above N = 3072 with 256-thread workgroups until round 3; 512 x 64 is ahead there now)
}

hipError_t nb_launch_small_step(const void *pos_in, void *pos_out, void *vel, void *acc, const void *mass, int n, int dim,
                                int is_f64, int hook, double G, double eps2, double half_dt, double dt, int do_kick, int lanes,
                                hipStream_t st, const GridTables *tab, double *part, unsigned long long *bin_out)
{
    if (bin_out && hook != HOOK_GRID) return hipErrorInvalidValue;
    if (hook == HOOK_GRID && (is_f64 || !tab)) return hipErrorInvalidValue;
    // fp32 state: G and eps2 are rounded to fp32 here; a hook the fp32 kernels do not compile in runs as none
    const double g = is_f64 ? G : (double)(float)G, e = is_f64 ? eps2 : (double)(float)eps2;
    const int h = (hook == HOOK_BF16 || hook == HOOK_F16) ? hook : HOOK_NONE;
    return nb::pick<2, 3>(dim, [&](auto D) {
        if (hook == HOOK_GRID)      // bin_out: the bin read-out (nb_quant_bin_sums), the same kernel body with BINS = true
            return nb::pick_bool(bin_out != nullptr, [&](auto B) {
                return launch_s<float, D.value, HOOK_GRID, B.value>(pos_in, pos_out, vel, acc, mass, n, g, e, half_dt, dt, do_kick,
                                                                    lanes, st, tab, part, bin_out);
            });
        if (is_f64) return launch_s<double, D.value, HOOK_NONE>(pos_in, pos_out, vel, acc, mass, n, g, e, half_dt, dt, do_kick, lanes, st);
        return nb::pick<HOOK_NONE, HOOK_BF16, HOOK_F16>(h, [&](auto H) {
            return launch_s<float, D.value, H.value>(pos_in, pos_out, vel, acc, mass, n, g, e, half_dt, dt, do_kick, lanes, st);
        });
    });
}
