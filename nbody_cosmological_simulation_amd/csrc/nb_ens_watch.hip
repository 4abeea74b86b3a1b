// nb_ens_watch.hip -- the explosion watch of an ensemble run (nb_ens_run_members with watch = 1, include/nbody_amd.h).
//
// The reference's stability sweep (stability_test.py:94-105) steps a system check_interval ticks, then asks
// detect_explosion (:34-61) whether it has "exploded", and stops it there.  Here that question is answered on the device for
// every member at every sampled tick, behind the two energy launches of the tick, and the answer is a write to the member's
// entry of the stop array that every later launch of the tick path reads (nb_device.h): the host never looks.
//
//   ens_watch_kernel   grid (members), one workgroup per member.  A member that has stopped before this tick, or was
//       halted, is skipped.  The others scan their n * D positions and velocities for a non-finite value (all exponent bits
//       of the storage type set), fold the flag over the workgroup, and thread 0 applies the reference's three criteria in
//       the reference's order with E0 = sample 0 and E = this sample of the history, kinetic + potential in double as
//       get_total_energy() adds them.  The comparisons are the reference's expressions, so a NaN energy trips nothing.
//
// The kernel boundary is the only synchronisation: the energies were written by the launch in front, and the launches
// behind this one read the stop it writes.
#include "nb_device.h"
#include "nb_dispatch.h"

namespace {

using namespace nbdev;

constexpr int EW_THREADS = 256;

// RAGGED (sizes, dim: nb_device.h): count is the stride of a member's slice, of which it scans its own sizes[b] * dim
template <typename T, bool RAGGED>
__global__ void __launch_bounds__(EW_THREADS)
ens_watch_kernel(const T *__restrict__ pos, const T *__restrict__ vel, int count /* n * D */, int members,
                 const double *__restrict__ kinetic, const double *__restrict__ potential, int64_t sample, int t,
                 int *__restrict__ stop, int *__restrict__ reason, const int *__restrict__ sizes, int dim)
{
    __shared__ int s_bad[EW_THREADS / 64];
    const int b = blockIdx.x;                        // member: uniform per workgroup
    if (!ens_still_running(stop, reason, b, t)) return;
    const size_t o = (size_t)b * count;
    const int mine = ens_member_count<RAGGED>(sizes, b, dim, count);
    bool bad = false;
    for (int k = threadIdx.x; k < mine; k += EW_THREADS) {
        const T x = pos[o + k], v = vel[o + k];
        bad = bad || non_finite(x) || non_finite(v);
    }
    const bool wave_bad = __builtin_amdgcn_ballot_w64(bad) != 0ull;
    if ((threadIdx.x & 63) == 0) s_bad[threadIdx.x >> 6] = wave_bad ? 1 : 0;
    __syncthreads();
    if (threadIdx.x != 0) return;
    int any = 0;
#pragma unroll
    for (int w = 0; w < EW_THREADS / 64; ++w) any |= s_bad[w];
    const double e0 = kinetic[b] + potential[b];
    const double e = kinetic[sample * members + b] + potential[sample * members + b];
    int r = NB_ENS_REASON_NONE;
    if (any) r = NB_ENS_REASON_NONFINITE;
    else if (fabs(e0) > 1e-10 && fabs(e - e0) / fabs(e0) > 10.0) r = NB_ENS_REASON_ENERGY;
    else if (e0 < 0 && e > fabs(e0)) r = NB_ENS_REASON_UNBOUND;
    if (r != NB_ENS_REASON_NONE) {
        stop[b] = t;
        reason[b] = r;
    }
}

}  // namespace

hipError_t nb_launch_ens_watch(const void *pos, const void *vel, int members, int n, int dim, int is_f64, const double *kinetic,
                               const double *potential, int64_t sample, int t, int *stop, int *reason, hipStream_t st,
                               const int *sizes)
{
    if (members < 1 || members > NB_ENS_MAX_MEMBERS || n < 1 || (dim != 2 && dim != 3)) return hipErrorInvalidValue;
    if (!pos || !vel || !kinetic || !potential || !stop || !reason || sample < 1 || t < 1) return hipErrorInvalidValue;
    return nb::pick_real(is_f64, [&](auto real) {
        using T = typename decltype(real)::type;
        return nb::pick_bool(sizes != nullptr, [&](auto RG) {
            hipLaunchKernelGGL((ens_watch_kernel<T, RG.value>), dim3(members), dim3(EW_THREADS), 0, st, (const T *)pos,
                               (const T *)vel, n * dim, members, kinetic, potential, sample, t, stop, reason, sizes, dim);
            return hipGetLastError();
        });
    });
}
