// nb_ens_metrics.hip -- the four galaxy diagnostics of nb_metrics.hip for every member of an ensemble in ONE launch
// (nb_ens_metrics, include/nbody_amd.h).  nb_metrics.hip is the specification: the arithmetic below follows it operation
// by operation in the state dtype A (correctly rounded sqrt and divide, no contraction), so every per-star decision --
// radial bin, bound flag, order statistic -- is the one a solo evaluation of that member takes.
//
//   ens_metrics_kernel   grid (members), one workgroup of 64 .. 1024 threads per member; P = N rounded up to a power of
//       two, threads = clamp(P / 2, 64, 1024), so a thread owns at most 4 stars (i = tid + q * threads) and at most 4
//       consecutive sorted positions.
//         1  per star: r, |v|, vt; fp64 sums of m, (A)(x m), |v| and the NaN-propagating max r        (registers)
//         2  centre of mass in A, mean |v|, R_b, the member's float32 edges                           (LDS, 1 KiB)
//         3  per star: r_com, radial bin (count of edges <= r, as metrics_decide_kernel), (|v| - mean)^2
//         4  bitonic sort of the r keys in LDS -> r_kth
//         5  bitonic sort of (r_com key, index) in the same LDS: the composite order is the unique stable one
//         6  fp64 inclusive scan of the masses in that order (4 per thread, wave scan by shuffles, wave totals in
//            order), enc = (A)prefix, escape test
//         7  one wave per bin (b = wave, wave + waves, ...): fp64 sum of the bin's vt and its count, lanes strided
//            over the stars, then a fixed butterfly
//       Keys are the bit patterns, NaN -> all-ones (KeyOf, nb_device.h).  Padding up to P carries all-ones keys and
//       indices >= N: it sorts after every NaN star and is never read as a star (positions >= N are skipped).
//       vt, |v| and the bin index of every star cross threads through the member's slice of a global scratch buffer
//       (written before a workgroup barrier, read after it); nothing else leaves the workgroup until the outputs.
//       No rocPRIM, no atomics, no counters or fences between workgroups.  Every sum is added in a fixed order.
//
// LDS: P * (sizeof(key) + 4) bytes of dynamic LDS for the sorts (48 KiB at N = 4096 fp64, 32 KiB at N = 3072 fp32) beside
// the static arrays below.  -Rpass-analysis=kernel-resource-usage, gfx950 (static LDS only; scratch 0 everywhere):
//   ens_metrics_kernel<float, 2>    VGPRs 68   static LDS 1160 B   scratch 0   occupancy 7 waves / SIMD
//   ens_metrics_kernel<float, 3>    VGPRs 74   static LDS 1160 B   scratch 0   occupancy 6
//   ens_metrics_kernel<double, 2>   VGPRs 96   static LDS 1160 B   scratch 0   occupancy 5
//   ens_metrics_kernel<double, 3>   VGPRs 96   static LDS 1160 B   scratch 0   occupancy 5
#include "nb_device.h"
#include "nb_dispatch.h"

namespace {

using namespace nbdev;

constexpr int EM_MAX_THREADS = 1024;
constexpr int EM_WAVES = EM_MAX_THREADS / 64;
constexpr int EM_SPT = 4;                        // stars (and sorted positions) per thread, at most

struct SumOp {
    static __device__ __forceinline__ double apply(double a, double b) { return a + b; }
};
struct NanMaxOp {          // NaN-propagating like torch.max(): a NaN radius poisons the maximum
    static __device__ __forceinline__ double apply(double a, double b)
    { return (a != a || b != b) ? __builtin_nan("") : (a > b ? a : b); }
};

// fixed-order reduction over the workgroup: butterfly inside a wave, then the wave results in wave order; every thread
// gets the result.  All threads of the workgroup call it.
template <typename Op>
__device__ __forceinline__ double block_reduce(double v, double *s_red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = Op::apply(v, __shfl_xor(v, off, 64));
    const int waves = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = s_red[0];
    for (int w = 1; w < waves; ++w) r = Op::apply(r, s_red[w]);
    __syncthreads();
    return r;
}

// ascending bitonic sort of s_key[0 .. P) (PAIRS: of the composite (s_key, s_idx)); P a power of two.  Ends on a barrier.
template <typename K, bool PAIRS>
__device__ __forceinline__ void bitonic_sort(K *s_key, int *s_idx, int P)
{
    const int half = P >> 1;
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < half; t += blockDim.x) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const bool up = (lo & k) == 0;
                const K a = s_key[lo], b = s_key[hi];
                bool gt = a > b;
                if constexpr (PAIRS) {
                    const int ia = s_idx[lo], ib = s_idx[hi];
                    gt = gt || (a == b && ia > ib);
                    if (gt == up) { s_key[lo] = b; s_key[hi] = a; s_idx[lo] = ib; s_idx[hi] = ia; }
                } else {
                    if (gt == up) { s_key[lo] = b; s_key[hi] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// out_d per member: [0] max r, [1] r_kth, [2] bound count, [3] dispersion, [4] max_radius used, [5 + b] mean of bin b,
// [5 + nb + b] its count; out_e per member: nb + 1 float edges
template <typename A, int D>
__global__ void __launch_bounds__(EM_MAX_THREADS)
ens_metrics_kernel(const A *__restrict__ pos, const A *__restrict__ vel, const A *__restrict__ mass, int n, int P,
                   const EnsScalars<A> *__restrict__ prm, const double *__restrict__ max_radius /* null: own max r */,
                   int num_bins, int kth, A *star_vt, A *star_vm, int *star_bin,
                   double *__restrict__ out_d, float *__restrict__ out_e)
{
    typedef typename KeyOf<A>::type K;
    extern __shared__ unsigned long long s_dyn[];          // P keys, then P indices
    K *s_key = (K *)s_dyn;
    int *s_idx = (int *)(s_key + P);
    __shared__ double s_red[EM_WAVES];
    __shared__ float s_edges[256];
    __shared__ double s_glob[4];                           // com[0..2], r_kth

    const int b = blockIdx.x;                              // member: uniform per workgroup
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, waves = nt >> 6;
    const A *p = pos + (size_t)b * n * D;
    const A *u = vel + (size_t)b * n * D;
    const A *m = mass + (size_t)b * n;
    A *vt_s = star_vt + (size_t)b * n;
    A *vm_s = star_vm + (size_t)b * n;
    int *bin_s = star_bin + (size_t)b * n;
    double *od = out_d + (size_t)b * (5 + 2 * num_bins);
    float *oe = out_e + (size_t)b * (num_bins + 1);

    // ---- 1: per star
    A x[EM_SPT][D], r[EM_SPT], vm[EM_SPT];
    double mx = -1.0, sm = 0.0, sx[3] = {0.0, 0.0, 0.0}, sv = 0.0;
#pragma unroll
    for (int q = 0; q < EM_SPT; ++q) {
        const int i = tid + q * nt;
        r[q] = (A)0; vm[q] = (A)0;
#pragma unroll
        for (int k = 0; k < D; ++k) x[q][k] = (A)0;
        if (i < n) {
            A v[D];
#pragma unroll
            for (int k = 0; k < D; ++k) { x[q][k] = p[(size_t)i * D + k]; v[k] = u[(size_t)i * D + k]; }
            A r2 = x[q][0] * x[q][0], v2 = v[0] * v[0];
#pragma unroll
            for (int k = 1; k < D; ++k) { r2 = r2 + x[q][k] * x[q][k]; v2 = v2 + v[k] * v[k]; }   // -ffp-contract=off: no fma
            r[q] = sqrt_rn<A>(r2);
            vm[q] = sqrt_rn<A>(v2);
            A cr = x[q][0] * v[1] - x[q][1] * v[0];
            cr = cr < (A)0 ? -cr : cr;
            const A rc = (r[q] < (A)0.1) ? (A)0.1 : r[q];        // clamp(min=0.1); NaN stays NaN
            vt_s[i] = div_rn<A>(cr, rc);
            vm_s[i] = vm[q];
            const A mi = m[i];
            mx = NanMaxOp::apply((double)r[q], mx);
            sm += (double)mi;
#pragma unroll
            for (int k = 0; k < D; ++k) sx[k] += (double)(A)(x[q][k] * mi);
            sv += (double)vm[q];
        }
    }
    mx = block_reduce<NanMaxOp>(mx, s_red);
    sm = block_reduce<SumOp>(sm, s_red);
#pragma unroll
    for (int k = 0; k < D; ++k) sx[k] = block_reduce<SumOp>(sx[k], s_red);
    sv = block_reduce<SumOp>(sv, s_red);

    // ---- 2: centre of mass in A, mean |v|, the member's edges
    const A tm = (A)sm;
    A com[D];
#pragma unroll
    for (int k = 0; k < D; ++k) com[k] = div_rn<A>((A)sx[k], tm);
    const double mean = sv / (double)n;
    const double R = max_radius ? max_radius[b] : mx;
    if (num_bins > 0) {
        // torch.linspace(0, R, num_bins + 1) in float32 as metrics_finish_sums_kernel restates it: step * i below the
        // middle, ONE fused end - step * (steps - 1 - i) from it on
        const float end = (float)R;
        const int steps = num_bins + 1;
        const float step = __fdiv_rn(end, (float)(steps - 1));
        for (int i = tid; i < steps; i += nt) {
            const float e = (i < steps / 2) ? __fmul_rn(step, (float)i) : __fmaf_rn(-step, (float)(steps - i - 1), end);
            s_edges[i] = e;
            oe[i] = e;
        }
    }
    __syncthreads();

    // ---- 3: per star: r_com key, radial bin, squared deviation of |v|
    K key_rc[EM_SPT];
    double ss = 0.0;
#pragma unroll
    for (int q = 0; q < EM_SPT; ++q) {
        const int i = tid + q * nt;
        key_rc[q] = ~(K)0;
        if (i < n) {
            A s = (A)0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const A d = x[q][k] - com[k];
                s = (k == 0) ? d * d : s + d * d;
            }
            key_rc[q] = KeyOf<A>::make(sqrt_rn<A>(s));
            // bin c - 1 holds edge_{c-1} <= r < edge_c (metrics.py:65); r is compared in A against the float32 edges
            int bin = -1;
            if (num_bins > 0) {
                int c = 0;
                for (int e = 0; e <= num_bins; ++e) c += ((A)s_edges[e] <= r[q]) ? 1 : 0;
                bin = (c >= 1 && c <= num_bins) ? c - 1 : -1;
            }
            bin_s[i] = bin;
            const double d = (double)vm[q] - mean;
            ss += d * d;
        }
    }
    ss = block_reduce<SumOp>(ss, s_red);

    // ---- 4: the order statistic of the radii
    for (int i = tid; i < P; i += nt) s_key[i] = ~(K)0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < EM_SPT; ++q) {
        const int i = tid + q * nt;
        if (i < n) s_key[i] = KeyOf<A>::make(r[q]);
    }
    __syncthreads();
    bitonic_sort<K, false>(s_key, s_idx, P);
    if (tid == 0) s_glob[3] = (double)KeyOf<A>::back(s_key[kth]);
    __syncthreads();

    // ---- 5: stable order by distance from the centre of mass
    for (int i = tid; i < P; i += nt) { s_key[i] = ~(K)0; s_idx[i] = i; }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < EM_SPT; ++q) {
        const int i = tid + q * nt;
        if (i < n) s_key[i] = key_rc[q];
    }
    __syncthreads();
    bitonic_sort<K, true>(s_key, s_idx, P);

    // ---- 6: enclosed mass = inclusive prefix sum of the masses in that order, in fp64; escape test
    int who[EM_SPT];
    double pre[EM_SPT], t = 0.0;
    const int k0 = tid * EM_SPT;
#pragma unroll
    for (int q = 0; q < EM_SPT; ++q) {
        who[q] = k0 + q < n ? s_idx[k0 + q] : -1;
        if (who[q] >= n) who[q] = -1;                      // (padding sorts behind every star: never taken)
        if (who[q] >= 0) t += (double)m[who[q]];
        pre[q] = t;
    }
    double inc = t;                                        // inclusive scan of the thread totals inside the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double y = __shfl_up(inc, off, 64);
        if (lane >= off) inc += y;
    }
    if (lane == 63) s_red[wave] = inc;
    __syncthreads();
    double base = 0.0;
    for (int w = 0; w < wave; ++w) base += s_red[w];
    base += inc - t;
    __syncthreads();                                       // s_red is read: the next reduction may write it
    const A g2 = (A)2 * prm[b].G;                          // (A)(2.0 * G) of metrics_decide_kernel: doubling is exact
    int nbound = 0;
#pragma unroll
    for (int q = 0; q < EM_SPT; ++q) {
        const int i = who[q];
        if (i < 0) continue;
        const A enc = (A)(base + pre[q]);
        const A rci = KeyOf<A>::back(s_key[k0 + q]);
        const A rcc = (rci < (A)0.1) ? (A)0.1 : rci;
        const A vesc = sqrt_rn<A>(div_rn<A>(g2 * enc, rcc));
        nbound += (vm_s[i] < vesc) ? 1 : 0;
    }
    const double bound = block_reduce<SumOp>((double)nbound, s_red);      // (ends on a barrier: s_red is free again)

    // ---- 7: bin means and counts, one wave per bin
    for (int bb = wave; bb < num_bins; bb += waves) {
        double s = 0.0;
        int c = 0;
        for (int i = lane; i < n; i += 64)
            if (bin_s[i] == bb) { s += (double)vt_s[i]; ++c; }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            s += __shfl_xor(s, off, 64);
            c += __shfl_xor(c, off, 64);
        }
        if (lane == 0) {
            od[5 + bb] = c > 0 ? (double)(A)(s / (double)c) : __builtin_nan("");
            od[5 + num_bins + bb] = (double)c;
        }
    }
    if (tid == 0) {
        od[0] = mx;
        od[1] = s_glob[3];
        od[2] = bound;
        od[3] = n > 1 ? (double)(A)__dsqrt_rn(ss / (double)(n - 1)) : __builtin_nan("");
        od[4] = R;
    }
}

}  // namespace

size_t nb_ens_metrics_scratch_bytes(int members, int n, int is_f64)
{
    return (size_t)members * n * (2 * (is_f64 ? 8 : 4) + 4);
}

hipError_t nb_launch_ens_metrics(const NbEnsMetricsArgs &a, hipStream_t st)
{
    if (a.members < 1 || a.members > NB_ENS_MAX_MEMBERS || a.n < 1 || a.n > 4096 || (a.dim != 2 && a.dim != 3))
        return hipErrorInvalidValue;
    if (a.num_bins < 0 || a.num_bins > 255 || a.kth < 0 || a.kth >= a.n) return hipErrorInvalidValue;
    if (!a.pos || !a.vel || !a.mass || !a.prm || !a.scratch || !a.out || !a.edges_out) return hipErrorInvalidValue;
    int P = 1;
    while (P < a.n) P <<= 1;
    int threads = P / 2;
    threads = threads < 64 ? 64 : (threads > EM_MAX_THREADS ? EM_MAX_THREADS : threads);
    const size_t count = (size_t)a.members * a.n;
    return nb::pick_real(a.is_f64, [&](auto real) {
        using A = typename decltype(real)::type;
        using K = typename KeyOf<A>::type;
        const size_t lds = (size_t)P * (sizeof(K) + sizeof(int));
        A *vt = (A *)a.scratch, *vm = vt + count;
        int *bin = (int *)(vm + count);
        return nb::pick<2, 3>(a.dim, [&](auto D) {
            hipLaunchKernelGGL((ens_metrics_kernel<A, D.value>), dim3(a.members), dim3(threads), lds, st, (const A *)a.pos,
                               (const A *)a.vel, (const A *)a.mass, a.n, P, (const EnsScalars<A> *)a.prm, a.max_radius,
                               a.num_bins, a.kth, vt, vm, bin, a.out, a.edges_out);
            return hipGetLastError();
        });
    });
}
