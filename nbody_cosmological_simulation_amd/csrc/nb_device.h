// nb_device.h -- device-side helpers shared by the kernels: the exact-arithmetic primitives that the bit-for-bit
// contracts rest on, the per-member stop rule of the ensemble tick path, and the fp32 r2 / grid-bin helpers of the force
// kernels.
#pragma once
#include <climits>

#include "nb_internal.h"

namespace nbdev {

// ---- exact arithmetic: one correctly rounded operation each, never contracted whatever the build's flags ----------------
template <typename T> __device__ __forceinline__ T mul_rn(T a, T b);
template <> __device__ __forceinline__ float mul_rn<float>(float a, float b) { return __fmul_rn(a, b); }
template <> __device__ __forceinline__ double mul_rn<double>(double a, double b) { return __dmul_rn(a, b); }
template <typename T> __device__ __forceinline__ T add_rn(T a, T b);
template <> __device__ __forceinline__ float add_rn<float>(float a, float b) { return __fadd_rn(a, b); }
template <> __device__ __forceinline__ double add_rn<double>(double a, double b) { return __dadd_rn(a, b); }
template <typename T> __device__ __forceinline__ T div_rn(T a, T b);
template <> __device__ __forceinline__ float div_rn<float>(float a, float b) { return __fdiv_rn(a, b); }
template <> __device__ __forceinline__ double div_rn<double>(double a, double b) { return __ddiv_rn(a, b); }
// sqrtf, not __fsqrt_rn: the latter compiles to the bare v_sqrt_f32 -- 1 ulp -- on this toolchain, sqrtf carries the fix-up
// to correct rounding.  Solo and batched diagnostics agree star by star only because both take THIS root.
template <typename T> __device__ __forceinline__ T sqrt_rn(T x);
template <> __device__ __forceinline__ float sqrt_rn<float>(float x) { return __builtin_sqrtf(x); }
template <> __device__ __forceinline__ double sqrt_rn<double>(double x) { return __dsqrt_rn(x); }
// torch semantics: `a + b * s` is two rounded operations (no fused multiply-add), with the Python scalar cast to the
// tensor dtype first
template <typename T> __device__ __forceinline__ T axpy_rn(T a, T b, T s) { return add_rn<T>(a, mul_rn<T>(b, s)); }

// sort keys: radii are >= +0 or NaN, so their bit patterns order like the values; NaN goes last (torch.sort's rule)
template <typename A> struct KeyOf;
template <> struct KeyOf<float> {
    typedef unsigned type;
    static __device__ __forceinline__ unsigned make(float x) { return x != x ? 0xffffffffu : __float_as_uint(x); }
    static __device__ __forceinline__ float back(unsigned k) { return __uint_as_float(k); }   // all-ones is a NaN
};
template <> struct KeyOf<double> {
    typedef unsigned long long type;
    static __device__ __forceinline__ unsigned long long make(double x)
    { return x != x ? ~0ull : (unsigned long long)__double_as_longlong(x); }
    static __device__ __forceinline__ double back(unsigned long long k) { return __longlong_as_double((long long)k); }
};

// the bit tests of the explosion watch (any exponent-all-ones value) and of the crash-point detector (NaN and Inf told
// apart), side by side: two questions, not one
__device__ __forceinline__ bool non_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ bool non_finite(double x) { return ((unsigned int)__double2hiint(x) & 0x7ff00000u) == 0x7ff00000u; }
__device__ __forceinline__ void classify(float x, bool &nan, bool &inf)
{
    const unsigned int u = __float_as_uint(x);
    if ((u & 0x7f800000u) == 0x7f800000u) {
        if (u & 0x007fffffu) nan = true; else inf = true;
    }
}
__device__ __forceinline__ void classify(double x, bool &nan, bool &inf)
{
    const unsigned int hi = (unsigned int)__double2hiint(x);
    if ((hi & 0x7ff00000u) == 0x7ff00000u) {
        if ((hi & 0x000fffffu) | (unsigned int)__double2loint(x)) nan = true; else inf = true;
    }
}

// ---- far coordinates: moved where a pair loop's copy is staged, never per pair -------------------------
// Upstream's G / r2 ** 1.5 is exactly 0 once r2 has overflowed to +inf; the kernels' rsqrt-based q^(-3/2) and q^(-1/2) are
// inf * 0 = NaN there.  So the COPY of a coordinate that a pair loop reads (the packed arrays, an LDS tile, the target
// registers; never the state) is moved when it lies beyond +-L: star p's far coordinate goes to the slot +-far_slot(p), the
// way the spread padding is placed.  Slots lie above L and above every padding coordinate (fp32: L 1.2e18, padding 1e18,
// slots 1.5e18 .. 4.5e18; fp64: L 1.2e153, spread padding up to 1.03e153, slots 1.5e153 .. 3e153) and below
// sqrt(MAX / (4 D)), D = 3 (5.32e18, 3.87e153), so r2 = sum of D squares of differences <= 2 max-slot stays finite.  A
// star beyond L is at least 2e17 (2e152) from every star inside L and every slot is at least 3e17 (3e152) from every
// star inside L and from the padding: far past the distance where r^3 overflows (fp32 7e12, fp64 5.6e102), so the factor
// is 0 upstream and underflows to exactly 0 here, before and after the move.  Two stars beyond L get different slots:
//   fp64  1.5e153 + 1e146 p (p mod 1.5e7): any two slots are >= 1e146 apart, factor exactly 0
//   fp32  1.5e18 + 2e15 (p mod 1500) + 1e12 (p / 1500 mod 2000): exactly 0 unless p = p' (mod 1500); then the two stars
//         are >= 7e11 apart (1e12 less the rounding to fp32) and their mutual factor is at most (7e11)^-3 (upstream: 0) -- never the O(1) factor that
//         two stars clamped onto one value would get from their other coordinates
// What is lost: two stars beyond L whose true separation is below the r^3 overflow distance (fp32 numbers there are
// 1.4e11 and more apart, so that means equal or neighbouring values; fp64: equal values) interact upstream and not here.
// NaN stays NaN and +-inf stays +-inf (the comparisons are false for NaN).  L: NB_FAR_F64 / NB_FAR_F32 (nb_internal.h), by
// the type of the PAIR arithmetic, not of the storage; lim = +inf switches the staging off.
template <typename T> __device__ __forceinline__ T far_slot(int p);
template <> __device__ __forceinline__ float far_slot<float>(int p)
{
    return (float)(1.5e18 + 2e15 * (double)(p % 1500) + 1e12 * (double)((p / 1500) % 2000));
}
template <> __device__ __forceinline__ double far_slot<double>(int p) { return 1.5e153 + 1e146 * (double)(p % 15000000); }
// the slot follows the pair arithmetic like the limit does: fp64 storage under the fp32 limit takes the fp32 slots
template <typename T> __device__ __forceinline__ T far_slot_for(T lim, int p)
{
    if constexpr (sizeof(T) == 4) return far_slot<float>(p);
    else return lim < (T)1e100 ? (T)far_slot<float>(p) : far_slot<double>(p);
}
// star p's coordinate x as the pair loop is to see it (the same value wherever star p is staged, as target or as source)
template <typename T> __device__ __forceinline__ T stage_far(T x, T lim, int p)
{
    if (x > lim && !non_finite(x)) return far_slot_for<T>(lim, p);
    if (x < -lim && !non_finite(x)) return -far_slot_for<T>(lim, p);
    return x;
}
// the same for a potential-energy kernel, where upstream's masked diagonal makes the sum NaN as soon as one coordinate is
// infinite (dist_ii = sqrt(inf - inf)): +-inf becomes NaN, which every pair of that star then carries into the sum
template <typename T> __device__ __forceinline__ T stage_far_pe(T x, T lim, int p)
{
    return non_finite(x) ? (T)__builtin_nanf("") : stage_far<T>(x, lim, p);
}

// ---- per-member stops of the ensemble tick path (nb_ens_run_members) -----------------------------------------------------
// Every kernel of the tick path takes `stop` (device, one int per member, or null: no member ever stops) and the launch's
// tick index t = ticks the call has already closed.  The kernels come in two instantiations, STOPS = false for a launch
// without the array: its code is what it was before there were stops.  (One kernel with a run-time null test was measured
// first, N = 1024 on an MI355X: the test sits in front of the loads of the other kernel arguments, a scalar-memory round
// trip of its own in every launch, +0.3 to +0.9 us per launch.)  With STOPS a workgroup reads its member's stop once:
// left = stop[b] - t ticks are still the member's.
//   left <= 0   the member is done: the workgroup returns
//   left == 1   this launch closes the member's last tick: it gets NB_KICK_CLOSE whatever the launch's mode is
//   else        the launch's own mode
// Where the positions ping-pong, a member on its last tick (left == 1) or just stopped (left == 0: budget 0, or halted by
// the watch kernel behind the previous launch) also gets its positions carried into the second buffer, bit for bit, so
// that both buffers hold a stopped member's final positions whatever the host swaps later: carry where left <= 1.
// (The step kernels write that test as `STOPS && left <= 1`: the front end then drops the block from the instantiation
// without stops, which keeps it the code of before instruction for instruction, not only byte for byte.)
template <bool STOPS>
__device__ __forceinline__ int ens_ticks_left(const int *__restrict__ stop, int b, int t)
{
    if constexpr (STOPS) return stop[b] - t;
    else return INT_MAX;
}
// the kick mode of a member with `left` >= 1 ticks under a launch of mode `kick`
__device__ __forceinline__ int ens_kick_mode(int left, int kick)
{
    return (left == 1 && kick != NB_KICK_NONE) ? NB_KICK_CLOSE : kick;
}
// a stopped member's positions into the second buffer: the targets of target block `blk` (the workgroup's own: nobody else
// writes or reads them there) of a member of n stars
template <typename T, int D, int S, int BS>
__device__ __forceinline__ void ens_carry_positions(int blk, const T *__restrict__ pos_in, T *__restrict__ pos_out, int n)
{
    constexpr int PER = BS / S * D;                  // elements of this workgroup's targets
    const int k = blk * PER + threadIdx.x;
    if (threadIdx.x < PER && k < n * D) pos_out[k] = pos_in[k];
}

// ---- members of different sizes (nb_ens_create_ragged) ----------------------------------------------------------------------
// A ragged handle's buffers are strided by the capacity; member b owns the first sizes[b] rows of its slice and no kernel
// touches the rest.  Every kernel of the tick path that needs the member's own count takes `sizes` (device, one int per
// member, or null) and comes in two instantiations, as with `stop`: RAGGED = false for a launch without the array, whose
// code is what it was before there were sizes.  per: elements per row (D, or 1 for stars); count: what a member of a
// uniform handle has, rows of the stride * per.
template <bool RAGGED>
__device__ __forceinline__ int ens_member_count(const int *__restrict__ sizes, int b, int per, int count)
{
    if constexpr (RAGGED) return sizes[b] * per;
    else return count;
}

// the watch kernels behind a sampled tick t (nb_ens_watch.hip, nb_ens_crash.hip): the member has not stopped before this
// tick and no earlier check halted it (halted: its reason / kind, 0 = none)
__device__ __forceinline__ bool ens_still_running(const int *stop, const int *halted, int b, int t)
{
    return stop[b] >= t && halted[b] == 0;
}

// ---- workgroup reductions and the arrival count (the grid's bounds, nb_grid.hip) -----------------------------------------
// Integer max / min, and fmaxf of values that are never NaN, do not depend on the order of the operands: whatever order
// the lanes, the waves and the workgroups are folded in, the result has the same bits.
struct MaxOp {
    static __device__ __forceinline__ unsigned int apply(unsigned int a, unsigned int b) { return max(a, b); }
    static __device__ __forceinline__ unsigned long long apply(unsigned long long a, unsigned long long b) { return b > a ? b : a; }
    static __device__ __forceinline__ float apply(float a, float b) { return fmaxf(a, b); }
};
struct MinOp {
    static __device__ __forceinline__ unsigned int apply(unsigned int a, unsigned int b) { return min(a, b); }
};
// Op over the WAVES * 64 threads of the workgroup (all of them call it): butterfly inside the wave, one slot per wave,
// thread 0 folds the slots in wave order and hands the result to use(result): the result exists on THREAD 0 ONLY, and
// what is done with it (the workgroup's one atomic, as a rule) stands in the same branch as the fold.  Contains one
// barrier, between the slot stores and the fold; the caller owes a barrier before it writes `slots` again.
template <typename Op, int WAVES, typename T, typename F>
__device__ __forceinline__ void block_reduce_t0(T v, T *slots, F &&use)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = Op::apply(v, __shfl_xor(v, off, 64));
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        v = slots[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v = Op::apply(v, slots[w]);
        use(v);
    }
}

// "The last workgroup to arrive does the rest": every thread of every workgroup calls it once per launch when the
// workgroup's results are written (behind a barrier of the caller's where more than thread 0 wrote them); thread 0 fences
// and counts the arrival at *counter, and the answer -- true in the one workgroup that arrives as number `total`, which
// then sees what all the others wrote -- is block-uniform (one barrier inside).  The last workgroup puts *counter back.
__device__ __forceinline__ bool last_block_arrives(unsigned int *counter, unsigned int total)
{
    __shared__ int s_last;
    if (threadIdx.x == 0) {
        __threadfence();
        s_last = (atomicAdd(counter, 1u) == total - 1) ? 1 : 0;
    }
    __syncthreads();
    return s_last != 0;
}

// ---- the force kernels' helpers ------------------------------------------------------------------------------------------

__device__ __forceinline__ float round_bf16(float x) { return (float)(__bf16)x; }
__device__ __forceinline__ float round_f16(float x) { return (float)(_Float16)x; }

// mass_prod = masses[i] * masses[j] keeps the masses' dtype upstream (simulation.py:185): fp32-typed masses give an
// fp32-rounded product even when the positions are fp64, half-typed masses (omega_point_test.py:722-733 keeps them
// half while the rest of the state is promoted) a product rounded to that half type.  mass_dt: nb_dtype of the masses.
__device__ __forceinline__ float mass_prod_f32(float mi, float mj, int mass_dt)
{
    float p = __fmul_rn(mi, mj);                       // exact for half inputs (11 + 11 bits)
    if (mass_dt == NB_F16) p = (float)(_Float16)p;
    else if (mass_dt == NB_BF16) p = (float)(__bf16)p;
    return p;
}

// r2 exactly as the reference's fp32 tensors produce it: (dx*dx + dy*dy [+ dz*dz]) + eps2, one
// rounding per operation, no fused multiply-add (simulation.py:86).
// s_f32_exact: the sum of squares before eps2 joins it (the max-r2 searches take their distance bound from it: eps2
// added and subtracted again would leave half an ulp of eps2 in place of a small separation).
template <int D>
__device__ __forceinline__ float s_f32_exact(const float *d)
{
    float s = __fadd_rn(__fmul_rn(d[0], d[0]), __fmul_rn(d[1], d[1]));
    if (D == 3) s = __fadd_rn(s, __fmul_rn(d[2], d[2]));
    return s;
}

template <int D>
__device__ __forceinline__ float r2_f32_exact(const float *d, float eps2)
{
    return __fadd_rn(s_f32_exact<D>(d), eps2);
}

// bin index = number of thresholds <= r2 (branch-free binary search over the LDS table)
// lp: table size (power of two, entries beyond the levels hold +inf)
__device__ __forceinline__ int grid_bin_lookup(const float *thr, float r2, int lp)
{
    int k = 0;
    for (int step = lp >> 1; step >= 1; step >>= 1)
        k += (thr[k + step] <= r2) ? step : 0;
    return k;
}

// Exact bin from an estimate: k0 = rint(log2(r2)*a + b) is within one bin of the true index
// (grid_tables_kernel guarantees it when tab->use_est), thr[k0] / thr[k0+1] settle it.
__device__ __forceinline__ int grid_bin_estimate(const float *thr, float r2, float est_a, float est_b, int lmax_bin)
{
    const float ne = __builtin_fmaf(__builtin_amdgcn_logf(r2), est_a, est_b);
    int k0 = (int)(ne + 0.5f);
    k0 = min(max(k0, 0), lmax_bin);
    const float lo = thr[k0], hi = thr[k0 + 1];
    return k0 - ((r2 < lo) ? 1 : 0) + ((r2 >= hi) ? 1 : 0);
}

// Floor form of the estimate: with k0 = floor(estimate) the exact bin is k0 or k0 + 1, so ONE
// threshold (thr[k0+1]) settles it.  kmax = levels - 2.
__device__ __forceinline__ int grid_bin_floor_estimate(const float *thr, float r2, float est_a, float est_b, int kmax)
{
    const float ne = __builtin_fmaf(__builtin_amdgcn_logf(r2), est_a, est_b);
    int k0 = (int)ne;
    k0 = min(max(k0, 0), kmax);
    return k0 + ((r2 >= thr[k0 + 1]) ? 1 : 0);
}

// Same guarantee, one LDS access: with k0 = floor(estimate) the exact bin is k0 or k0 + 1 (the exact
// index is rint() of a value the estimate tracks to << 0.5), so a record {thr[k0+1], lut[k0], lut[k0+1]}
// decides it with one compare.  Returns the force factor (1/q^1.5)*G of the exact bin.
__device__ __forceinline__ float grid_w_estimate(const float4 *rec, float r2, float est_a, float est_b, int kmax)
{
    const float ne = __builtin_fmaf(__builtin_amdgcn_logf(r2), est_a, est_b);
    int k0 = (int)ne;                       // truncation; negative estimates clamp to bin 0 below
    k0 = min(max(k0, 0), kmax);
    const float4 rc = rec[k0];
    return (r2 >= rc.x) ? rc.z : rc.y;
}

}  // namespace nbdev
