// nb_ens_crash.hip -- the crash-point detector of an ensemble (nb_ens_crash_measures / nb_ens_run_crash_watched,
// include/nbody_amd.h).
//
// The reference's crash-point finders (crash_point_test.py:142-466) step a system one tick, then ask detect_crash (:46-139)
// whether it has "crashed": eight whole-array reductions read back one by one and six criteria in a fixed order, two of
// them about the motion since the previous tick.  Here the reductions and the decision are made on the device for every
// member, behind the two energy launches of the tick, and the answer is a write to the member's entry of the stop array that
// every later launch of the tick path reads (nb_device.h): the host never looks.
//
//   ens_crash_kernel<T, D>   grid (members), one workgroup of 256 threads per member.  Every thread walks the member's stars
//       with stride 256: D positions, D previous positions, D velocities.  It keeps a NaN and an Inf flag (exponent and
//       mantissa bits of the storage type; positions and velocities, not the previous positions) and four running maxima:
//       the squared norms of pos - prev, vel and pos -- (c0*c0 + c1*c1) + c2*c2, separate multiplies and adds in that
//       order, as torch's (x ** 2).sum(dim=-1) adds a last dimension of 2 or 3 -- and |v_k| over all components.  Waves
//       fold by shuffles, the four waves through LDS; thread 0 takes ONE correctly rounded root per maximum in T (the root
//       is monotone: the root of the maximum is the maximum of the roots), widens to double and writes the member's flags
//       and measures {max_displacement, max_abs_velocity, max_speed, max_radius}.
//
//       stop == nullptr: measure only.  Every member is measured against the previous positions given (none: displacement
//       0); nothing else is written.
//       stop given (tick t): a member with stop[b] < t, or already halted, is skipped: its flags and measures stay those of
//       its last check.  The others also store their positions into the previous-position buffer, each thread the stars it
//       has just read, and thread 0 applies the reference's six criteria in the reference's order, in double, with the
//       member's dt as given, E = kinetic + potential of this sample and E_prev of the sample before.  The comparisons are
//       the reference's expressions: a NaN ratio trips nothing and a zero E_prev of either sign skips the energy test.  A
//       hit writes stop[b] = t and the kind.
//
// The kernel boundary is the only synchronisation: the energies were written by the launch in front, and the launches
// behind this one read the stop it writes.
#include "nb_device.h"
#include "nb_dispatch.h"

namespace {

using namespace nbdev;

constexpr int EC_THREADS = 256, EC_WAVES = EC_THREADS / 64;

template <typename T, int D>
__device__ __forceinline__ T norm2(const T (&c)[D])
{
    T s = add_rn(mul_rn(c[0], c[0]), mul_rn(c[1], c[1]));
    if constexpr (D == 3) s = add_rn(s, mul_rn(c[2], c[2]));
    return s;
}

// a NaN candidate is not taken (a member with a NaN is outside the measures' contract)
template <typename T>
__device__ __forceinline__ T take_max(T m, T x) { return x > m ? x : m; }

template <typename T>
__device__ __forceinline__ T wave_max(T m)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = take_max(m, __shfl_xor(m, off, 64));
    return m;
}

template <typename T, int D>
__global__ void __launch_bounds__(EC_THREADS)
ens_crash_kernel(const T *__restrict__ pos, T *prev, const T *__restrict__ vel, int n, int members,
                 const double *__restrict__ dt, const double *__restrict__ kinetic, const double *__restrict__ potential,
                 int64_t sample, int t, int *__restrict__ stop, int *__restrict__ kind, int *__restrict__ flags,
                 double *__restrict__ measures)
{
    __shared__ T s_max[EC_WAVES][4];
    __shared__ int s_flag[EC_WAVES];
    const int b = blockIdx.x;                        // member: uniform per workgroup
    const bool watch = stop != nullptr;
    if (watch && !ens_still_running(stop, kind, b, t)) return;
    const size_t o = (size_t)b * n * D;
    bool nan = false, inf = false;
    T m_disp2 = 0, m_absv = 0, m_speed2 = 0, m_rad2 = 0;
    for (int i = threadIdx.x; i < n; i += EC_THREADS) {
        const size_t k = o + (size_t)i * D;
        T x[D], v[D], d[D];
#pragma unroll
        for (int c = 0; c < D; ++c) {
            x[c] = pos[k + c];
            v[c] = vel[k + c];
            d[c] = prev ? x[c] - prev[k + c] : (T)0;
            classify(x[c], nan, inf);
            classify(v[c], nan, inf);
            m_absv = take_max(m_absv, (T)fabs(v[c]));
        }
        if (watch) {
#pragma unroll
            for (int c = 0; c < D; ++c) prev[k + c] = x[c];       // read above by this thread, by no other
        }
        m_disp2 = take_max(m_disp2, norm2<T, D>(d));
        m_speed2 = take_max(m_speed2, norm2<T, D>(v));
        m_rad2 = take_max(m_rad2, norm2<T, D>(x));
    }
    m_disp2 = wave_max(m_disp2);
    m_absv = wave_max(m_absv);
    m_speed2 = wave_max(m_speed2);
    m_rad2 = wave_max(m_rad2);
    const int wave_flags = (__builtin_amdgcn_ballot_w64(nan) != 0ull ? 1 : 0) | (__builtin_amdgcn_ballot_w64(inf) != 0ull ? 2 : 0);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        s_max[w][0] = m_disp2; s_max[w][1] = m_absv; s_max[w][2] = m_speed2; s_max[w][3] = m_rad2;
        s_flag[w] = wave_flags;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int f = 0;
#pragma unroll
    for (int w = 0; w < EC_WAVES; ++w) {
        f |= s_flag[w];
        m_disp2 = take_max(m_disp2, s_max[w][0]);
        m_absv = take_max(m_absv, s_max[w][1]);
        m_speed2 = take_max(m_speed2, s_max[w][2]);
        m_rad2 = take_max(m_rad2, s_max[w][3]);
    }
    const double max_disp = (double)sqrt_rn(m_disp2), max_absv = (double)m_absv;
    const double max_speed = (double)sqrt_rn(m_speed2), max_radius = (double)sqrt_rn(m_rad2);
    flags[b] = f;
    measures[4 * b + 0] = max_disp;
    measures[4 * b + 1] = max_absv;
    measures[4 * b + 2] = max_speed;
    measures[4 * b + 3] = max_radius;
    if (!watch) return;
    // detect_crash (crash_point_test.py:46-139), criterion by criterion
    const double e = kinetic[sample * members + b] + potential[sample * members + b];
    const double e_prev = kinetic[(sample - 1) * members + b] + potential[(sample - 1) * members + b];
    int r = NB_ENS_CRASH_NONE;
    if (f & 1) r = NB_ENS_CRASH_NAN;
    else if (f & 2) r = NB_ENS_CRASH_INF;
    else if (max_disp > max_absv * dt[b] * 10 && max_disp > 1.0) r = NB_ENS_CRASH_TELEPORT;
    else if (max_speed > 100.0) r = NB_ENS_CRASH_VELOCITY;
    else {
        bool hit = false;
        if (e_prev != 0) {
            const double ratio = fabs(e / e_prev);
            hit = ratio > 100 || ratio < 0.01;
        }
        if (hit) r = NB_ENS_CRASH_ENERGY;
        else if (max_radius > 1000) r = NB_ENS_CRASH_RADIUS;
    }
    if (r != NB_ENS_CRASH_NONE) {
        stop[b] = t;
        kind[b] = r;
    }
}

}  // namespace

hipError_t nb_launch_ens_crash(const void *pos, void *prev, const void *vel, int members, int n, int dim, int is_f64,
                               const double *dt, const double *kinetic, const double *potential, int64_t sample, int t, int *stop,
                               int *kind, int *flags, double *measures, hipStream_t st)
{
    if (members < 1 || members > NB_ENS_MAX_MEMBERS || n < 1) return hipErrorInvalidValue;
    if (!pos || !vel || !flags || !measures) return hipErrorInvalidValue;
    if (stop && (!prev || !kind || !dt || !kinetic || !potential || sample < 1 || t < 1)) return hipErrorInvalidValue;
    return nb::pick_real(is_f64, [&](auto real) {
        using T = typename decltype(real)::type;
        return nb::pick<2, 3>(dim, [&](auto D) {
            hipLaunchKernelGGL((ens_crash_kernel<T, D.value>), dim3(members), dim3(EC_THREADS), 0, st, (const T *)pos, (T *)prev,
                               (const T *)vel, n, members, dt, kinetic, potential, sample, t, stop, kind, flags, measures);
            return hipGetLastError();
        });
    });
}
