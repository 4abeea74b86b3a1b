// nb_ens_diverge.hip -- divergence between the members of an ensemble (nb_ens_divergence / nb_ens_run_diverged,
// include/nbody_amd.h).
//
// The reference's comparison loops (reality_glitch_tests.py:148-256 MultiverseSim, omega_point_test.py:665-766 _test_point)
// step two or three simulations side by side and read (a.positions - b.positions).abs().max().item(), .mean().item() and
// the same maximum of the velocities back after every tick.  Here every member b is compared with the member baseline[b]
// of the same ensemble on the device, behind the energy launches and the watch of a sampled tick, into a history that is
// copied out once at the end of the run: the host never looks in between.
//
//   ens_divergence_kernel<T, D>   grid (members), one workgroup of 256 threads per member b.  Thread t walks elements
//       k = t, t + 256, ... of the member's n * D positions and velocities and forms |pos[b][k] - pos[base][k]| and
//       |vel[b][k] - vel[base][k]| in T, one subtraction each (the reference's expressions).  Three results:
//         max |d position|, max |d velocity|: torch's max() -- NaN if any element is NaN (inf - inf included), else the
//             largest value, +inf an ordinary one: a NaN flag rides beside a maximum over the non-NaN values;
//         mean |d position|: every thread adds its elements in ascending k into a double, a fixed butterfly folds the
//             wave, the four waves fold in wave order through LDS and thread 0 divides by n * D in double: the same bits
//             run to run, NaN if any term is.
//       Thread 0 writes the three to sample `sample` of the history (index sample * members + b of each array).
//       baseline[b] == b is no special case: exact zeros, or NaN for a member that holds a NaN, as torch gives them.
//
// The kernel boundary is the only synchronisation: the state was written by the launches in front.
#include "nb_device.h"
#include "nb_dispatch.h"

namespace {

using namespace nbdev;

constexpr int ED_THREADS = 256, ED_WAVES = ED_THREADS / 64;

// torch's max(): a NaN wins, else the larger
template <typename T>
struct NanMax {
    T m;            // over the non-NaN values seen (differences are >= 0: starts at 0)
    bool nan;
    __device__ __forceinline__ void take(T x)
    {
        nan |= (x != x);
        m = x > m ? x : m;
    }
};

template <typename T>
__device__ __forceinline__ T wave_max_plain(T m)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const T o = __shfl_xor(m, off, 64);
        m = o > m ? o : m;
    }
    return m;
}

// RAGGED (sizes: nb_device.h): n is the stride of a member's slice; the member compares its own sizes[b] * D elements with
// its baseline's (of the same size: the host has checked) and divides the mean by that count
template <typename T, int D, bool RAGGED>
__global__ void __launch_bounds__(ED_THREADS)
ens_divergence_kernel(const T *__restrict__ pos, const T *__restrict__ vel, int n, int members,
                      const int *__restrict__ baseline, int64_t sample, double *__restrict__ max_pos,
                      double *__restrict__ mean_pos, double *__restrict__ max_vel, const int *__restrict__ sizes)
{
    __shared__ T s_max[ED_WAVES][2];
    __shared__ double s_sum[ED_WAVES];
    __shared__ int s_nan[ED_WAVES];
    const int b = blockIdx.x;                        // member: uniform per workgroup
    int base = baseline[b];
    if ((unsigned)base >= (unsigned)members) base = b;     // (the host has checked the range: never read outside the state)
    const size_t o = (size_t)b * (n * D), ob = (size_t)base * (n * D);
    const int count = ens_member_count<RAGGED>(sizes, b, D, n * D);
    NanMax<T> mp{(T)0, false}, mv{(T)0, false};
    double sum = 0.0;
    for (int k = threadIdx.x; k < count; k += ED_THREADS) {
        const T dp = (T)fabs(pos[o + k] - pos[ob + k]);
        const T dv = (T)fabs(vel[o + k] - vel[ob + k]);
        mp.take(dp);
        mv.take(dv);
        sum += (double)dp;
    }
    mp.m = wave_max_plain(mp.m);
    mv.m = wave_max_plain(mv.m);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);     // fixed butterfly: every lane the same bits
    const int wave_nan = (__builtin_amdgcn_ballot_w64(mp.nan) != 0ull ? 1 : 0) | (__builtin_amdgcn_ballot_w64(mv.nan) != 0ull ? 2 : 0);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        s_max[w][0] = mp.m; s_max[w][1] = mv.m;
        s_sum[w] = sum;
        s_nan[w] = wave_nan;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    T m_pos = s_max[0][0], m_vel = s_max[0][1];
    double total = s_sum[0];
    int f = s_nan[0];
#pragma unroll
    for (int w = 1; w < ED_WAVES; ++w) {             // wave order
        m_pos = s_max[w][0] > m_pos ? s_max[w][0] : m_pos;
        m_vel = s_max[w][1] > m_vel ? s_max[w][1] : m_vel;
        total += s_sum[w];
        f |= s_nan[w];
    }
    const size_t at = (size_t)sample * members + b;
    max_pos[at] = (f & 1) ? __builtin_nan("") : (double)m_pos;
    max_vel[at] = (f & 2) ? __builtin_nan("") : (double)m_vel;
    mean_pos[at] = total / (double)count;            // a NaN term has made the sum NaN
}

}  // namespace

hipError_t nb_launch_ens_divergence(const void *pos, const void *vel, int members, int n, int dim, int is_f64, const int *baseline,
                                    int64_t sample, double *max_pos, double *mean_pos, double *max_vel, hipStream_t st,
                                    const int *sizes)
{
    if (members < 1 || members > NB_ENS_MAX_MEMBERS || n < 1 || sample < 0) return hipErrorInvalidValue;
    if (!pos || !vel || !baseline || !max_pos || !mean_pos || !max_vel) return hipErrorInvalidValue;
    return nb::pick_real(is_f64, [&](auto real) {
        using T = typename decltype(real)::type;
        return nb::pick<2, 3>(dim, [&](auto D) {
            return nb::pick_bool(sizes != nullptr, [&](auto RG) {
                hipLaunchKernelGGL((ens_divergence_kernel<T, D.value, RG.value>), dim3(members), dim3(ED_THREADS), 0, st,
                                   (const T *)pos, (const T *)vel, n, members, baseline, sample, max_pos, mean_pos, max_vel, sizes);
                return hipGetLastError();
            });
        });
    });
}
