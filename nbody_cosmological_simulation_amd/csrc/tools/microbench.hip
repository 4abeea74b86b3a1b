// microbench.hip -- instruction-rate and accuracy probes that size the force kernel's budget
// on gfx950 (DESIGN.md "instruction budget").  Not part of the library; built by
// csrc/Makefile target `tools`, run on the GPU box:  ./microbench.bin > gpurun_out/microbench.txt
// (`./microbench.bin rot 3`: only the DPP value check and the rotation-cost table, three times)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../nb_force_sym_kernel.h"     // sweep<>, inv_r3_sym, LdsRot: the rotation-cost rows run the library's own pair loop

#define CHECK(x)                                                                        \
    do {                                                                                \
        hipError_t e = (x);                                                             \
        if (e != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); exit(1); } \
    } while (0)

constexpr int ITERS = 4096;
constexpr int UNROLL = 8;

// Each op kernel keeps UNROLL independent chains per lane so issue rate, not latency, is measured.
enum { OP_FMA64, OP_MUL64, OP_ADD64, OP_RSQ64, OP_RCP64, OP_SQRT64, OP_CVT64_32, OP_CVT32_64, OP_FMA32, OP_RSQ32,
       OP_MFMA64_4, OP_MFMA64_4_FMA6, OP_FMA64_X6, OP_PKFMA32, OP_PKFMA32_RSQ, OP_MIX_PAIR, OP_NOPS };
const char *OP_NAMES[] = {"v_fma_f64", "v_mul_f64", "v_add_f64", "v_rsq_f64", "v_rcp_f64", "v_sqrt_f64",
                          "v_cvt_f32_f64", "v_cvt_f64_f32", "v_fma_f32", "v_rsq_f32",
                          "mfma_f64_4x4x4", "mfma4x4x4+6fma", "6 x v_fma_f64", "v_pk_fma_f32", "pk_fma+2rsq_f32",
                          "pair_body_f64"};

template <int OP>
__global__ void __launch_bounds__(256) op_kernel(double *out, double seed)
{
    double a[UNROLL], g[UNROLL][6];
    float f[UNROLL], h[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        a[u] = seed + threadIdx.x * 1e-3 + u;
        f[u] = (float)a[u];
        h[u] = f[u] + 0.5f;
#pragma unroll
        for (int k = 0; k < 6; ++k) g[u][k] = a[u] + k;
    }
    const double b = 1.0000001, c = 1e-9;
    for (int it = 0; it < ITERS; ++it) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            if (OP == OP_FMA64) a[u] = __builtin_fma(a[u], b, c);
            if (OP == OP_MUL64) a[u] = a[u] * b;
            if (OP == OP_ADD64) a[u] = a[u] + c;
            if (OP == OP_RSQ64) a[u] = __builtin_amdgcn_rsq(a[u]);
            if (OP == OP_RCP64) a[u] = __builtin_amdgcn_rcp(a[u]);
            if (OP == OP_SQRT64) a[u] = __builtin_amdgcn_sqrt(a[u]);
            if (OP == OP_CVT64_32) { f[u] = (float)a[u]; asm volatile("" : "+v"(f[u])); a[u] += 0; }
            if (OP == OP_CVT32_64) { a[u] = (double)f[u]; asm volatile("" : "+v"(a[u])); }
            if (OP == OP_FMA32) f[u] = __builtin_fmaf(f[u], 1.0000001f, 1e-9f);
            if (OP == OP_RSQ32) f[u] = __builtin_amdgcn_rsqf(f[u]);
            if (OP == OP_PKFMA32 || OP == OP_PKFMA32_RSQ) {
                typedef float f2v __attribute__((ext_vector_type(2)));
                f2v t = {f[u], h[u]};
                t = __builtin_elementwise_fma(t, f2v{1.0000001f, 0.9999999f}, f2v{1e-9f, 2e-9f});
                if (OP == OP_PKFMA32_RSQ) { t.x = __builtin_amdgcn_rsqf(t.x); t.y = __builtin_amdgcn_rsqf(t.y); }
                f[u] = t.x; h[u] = t.y;
            }
            // matrix pipe: does v_mfma_f64_4x4x4_4b overlap with VALU FMAs of the same and of other waves?
            if (OP == OP_MFMA64_4 || OP == OP_MFMA64_4_FMA6) a[u] = __builtin_amdgcn_mfma_f64_4x4x4f64(b, c, a[u], 0, 0, 0);
            if (OP == OP_MFMA64_4_FMA6 || OP == OP_FMA64_X6) {
#pragma unroll
                for (int k = 0; k < 6; ++k) g[u][k] = __builtin_fma(g[u][k], b, c);
            }
        }
    }
    double s = 0;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        s += a[u] + f[u] + h[u];
        if (OP == OP_MFMA64_4_FMA6 || OP == OP_FMA64_X6)
#pragma unroll
            for (int k = 0; k < 6; ++k) s += g[u][k];
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// the fp64 pair body of nb_force.hip (13 VALU + 1 rsq per pair), operands in registers
__global__ void __launch_bounds__(256) pair_kernel(double *out, double seed)
{
    double xi = seed + threadIdx.x * 1e-3, yi = seed * 0.5 + threadIdx.x * 2e-3;
    double ax = 0, ay = 0;
    double xj = 0.25, yj = 0.75;
    const double eps2 = 0.01, gm = 1e-3;
    for (int it = 0; it < ITERS; ++it) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const double dx = xj - xi, dy = yj - yi;
            double q = __builtin_fma(dy, dy, eps2);
            q = __builtin_fma(dx, dx, q);
            const double y0 = __builtin_amdgcn_rsq(q);
            const double y02 = y0 * y0;
            const double e = __builtin_fma(-q, y02, 1.0);
            const double uu = y0 * gm;
            const double v = uu * y02;
            const double cc = __builtin_fma(e, 1.875, 1.5);
            const double ce = cc * e;
            const double w = __builtin_fma(v, ce, v);
            ax = __builtin_fma(w, dx, ax);
            ay = __builtin_fma(w, dy, ay);
            xj += 1e-3; yj -= 1e-3;       // 2 extra adds per pair: subtracted in the report
        }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = ax + ay;
}

// ---- what the rotation step of the pair-symmetric fp64 sweep costs (nb_force_sym_kernel.h: sweep<double, 2, 4, 4>, uniform
// masses, off-diagonal: 14 VALU + rsq per pair, 16 pairs per step).  ROT_BPERMUTE and ROT_LDS run the library's own sweep<>
// (two ds_bpermute_b32 per pair, or the LDS hand-off of LdsRot: 0.75 wide LDS instructions per pair); ROT_NONE is the same
// pair body with the source data and accumulators staying where they are (made opaque to the compiler once per slot, so
// that nothing is hoisted: no instruction is emitted for that).  ROT_DPP keeps the ring for the positions and moves the
// accumulators with DPP (SYM_ROT_DPP: one v_mov_b32_dpp per pair, 0.25 ds_read_b128); ROT_DPPALL moves the positions by
// DPP too (SYM_ROT_DPPALL: two v_mov_b32_dpp per pair, no LDS instruction in the step loop).
enum { ROT_NONE, ROT_BPERMUTE, ROT_LDS, ROT_DPP, ROT_DPPALL };
constexpr int rot_mode(int m) { return m == ROT_LDS ? SYM_ROT_LDS : m == ROT_DPP ? SYM_ROT_DPP : m == ROT_DPPALL ? SYM_ROT_DPPALL : SYM_ROT_LANES; }
constexpr int ROT_SWEEPS = 64;      // sweeps of 64 steps per launch: 65 536 pairs per lane

template <int MODE>
__global__ void __launch_bounds__(256, 4) sweep_rot_kernel(double *out, double seed)
{
    constexpr int R = 4, D = 2;
    __shared__ d2 s_ring[R][128];
    __shared__ d2 s_mail[4][R][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double xi[R][D], gi[R], ai[R][D], xj[R][D], gj[R], aj[R][D];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        gi[r] = gj[r] = 1.0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            xi[r][k] = seed + threadIdx.x * 1e-3 + r + 0.5 * k;
            xj[r][k] = 0.25 + lane * 2e-3 + 0.75 * r + 0.125 * k;
            ai[r][k] = aj[r][k] = 0.0;
        }
    }
    if (MODE == ROT_LDS || MODE == ROT_DPP) {      // the ring as force_sym_kernel stages it: 64 entries per slot, repeated
        const int r = threadIdx.x >> 6;
        const d2 v = {0.25 + lane * 2e-3 + 0.75 * r, 0.25 + lane * 2e-3 + 0.75 * r + 0.125};
        s_ring[r][lane] = v;
        s_ring[r][lane + 64] = v;
        __syncthreads();
    }
    const LdsRot lr{&s_ring[0][lane], nullptr, &s_mail[wave][0][lane], &s_mail[wave][0][(lane + 1) & 63]};
    const int rot_addr = ((lane + 1) & 63) << 2;
    const GridArgs ga{};
    BinDbg<R, R, false> bd;
    const double eps2 = 0.01;
    for (int o = 0; o < ROT_SWEEPS; ++o) {
        if constexpr (MODE == ROT_NONE) {
            double c15 = 1.5, c1875 = 1.875;
            asm volatile("" : "+v"(c15), "+s"(c1875));
#pragma unroll 1
            for (int s = 0; s < 64; ++s) {
#pragma unroll
                for (int rj = 0; rj < R; ++rj) {
#pragma unroll
                    for (int ri = 0; ri < R; ++ri) {
                        const double dx = xj[rj][0] - xi[ri][0], dy = xj[rj][1] - xi[ri][1];
                        const double q = __builtin_fma(dx, dx, __builtin_fma(dy, dy, eps2));
                        const double w = inv_r3_sym(q, c15, c1875);
                        ai[ri][0] = __builtin_fma(w, dx, ai[ri][0]);
                        ai[ri][1] = __builtin_fma(w, dy, ai[ri][1]);
                        aj[rj][0] = __builtin_fma(-w, dx, aj[rj][0]);
                        aj[rj][1] = __builtin_fma(-w, dy, aj[rj][1]);
                    }
                    asm volatile("" : "+v"(xj[rj][0]), "+v"(xj[rj][1]), "+v"(aj[rj][0]), "+v"(aj[rj][1]));
                }
            }
        } else {
            sweep<double, D, R, R, false, true, HOOK_NONE, 0, false, rot_mode(MODE)>(xi, gi, ai, xj, gj, aj, eps2, rot_addr, ga, 64, bd, lr);
        }
    }
    double s = 0;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < D; ++k) s += ai[r][k] + aj[r][k];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// ---- does dpp_rol1 (nb_force_sym_kernel.h) hand lane l the value of lane (l + 1) & 63, as the mailbox read does, bit for
// bit?  One wave; after `rotations` rotations lane l writes what it holds.
__global__ void __launch_bounds__(64) dpp_rol_check_kernel(const double *in, double *out, int rotations)
{
    double v = in[threadIdx.x];
    for (int r = 0; r < rotations; ++r) v = dpp_rol1(v);
    out[threadIdx.x] = v;
}

static bool dpp_rol_check()
{
    // two patterns per lane: the lane id in both words (direction), and fp64 values that a move through an fp64 ALU
    // could alter -- a NaN with a payload (quiet and signalling), -0.0, a denormal, infinities, ordinary numbers
    unsigned long long hin[2][64], hout[64];
    for (int l = 0; l < 64; ++l) {
        hin[0][l] = ((unsigned long long)(0x1000 + l) << 32) | (unsigned)l;
        unsigned long long b;
        switch (l % 8) {
        case 0: b = 0x7ff8dead0000beefull; break;                     // quiet NaN with a payload
        case 1: b = 0x7ff0000000c0ffeeull; break;                     // signalling NaN
        case 2: b = 0x8000000000000000ull; break;                     // -0.0
        case 3: b = 0x0000000000000123ull; break;                     // denormal
        case 4: b = 0xfff0000000000000ull; break;                     // -inf
        case 5: b = 0xfff8000000000001ull; break;                     // negative NaN
        default: { const double d = 1.0 / 3.0 + l; __builtin_memcpy(&b, &d, 8); }
        }
        hin[1][l] = b + ((unsigned long long)l << 8);                 // distinct in every lane (the payload / mantissa bits)
    }
    double *din, *dout;
    CHECK(hipMalloc(&din, 64 * 8));
    CHECK(hipMalloc(&dout, 64 * 8));
    bool ok = true;
    for (int pat = 0; pat < 2; ++pat) {
        CHECK(hipMemcpy(din, hin[pat], 64 * 8, hipMemcpyHostToDevice));
        const int rots[] = {1, 64, 21};
        for (int nr : rots) {
            hipLaunchKernelGGL(dpp_rol_check_kernel, dim3(1), dim3(64), 0, 0, din, dout, nr);
            CHECK(hipMemcpy(hout, dout, 64 * 8, hipMemcpyDeviceToHost));
            int bad = 0;
            for (int l = 0; l < 64; ++l) bad += hout[l] != hin[pat][(l + nr) & 63];
            printf("dpp wave_rol:1 check, pattern %d, %2d rotation(s): lane l holds lane (l + %d) & 63 bit for bit: %s", pat, nr, nr & 63,
                   bad ? "FAIL" : "pass");
            if (bad) {
                int from_prev = 0;
                for (int l = 0; l < 64; ++l) from_prev += hout[l] == hin[pat][(l - nr) & 63];
                printf(" (%d lanes wrong; %d lanes hold lane (l - %d) & 63; lane 0 holds %016llx)", bad, from_prev, nr & 63, hout[0]);
                ok = false;
            }
            printf("\n");
        }
    }
    CHECK(hipFree(din));
    CHECK(hipFree(dout));
    printf("dpp wave_rol:1 value check: %s\n", ok ? "PASS" : "FAIL");
    return ok;
}

__global__ void rsq_accuracy_kernel(const double *x, double *y_rsq, double *y_r3, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double q = x[i];
    y_rsq[i] = __builtin_amdgcn_rsq(q);
    const double y0 = y_rsq[i];
    const double y02 = y0 * y0;
    const double e = __builtin_fma(-q, y02, 1.0);
    const double v = y0 * y02;
    const double cc = __builtin_fma(e, 1.875, 1.5);
    y_r3[i] = __builtin_fma(v, cc * e, v);
}

template <typename K>
double time_kernel(K launch, int reps)
{
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    launch();
    CHECK(hipDeviceSynchronize());
    CHECK(hipEventRecord(a));
    for (int r = 0; r < reps; ++r) launch();
    CHECK(hipEventRecord(b));
    CHECK(hipEventSynchronize(b));
    float ms;
    CHECK(hipEventElapsedTime(&ms, a, b));
    return ms / reps;
}

// ./microbench.bin            every table once
// ./microbench.bin rot [K]    the DPP value check and the rotation-cost table K times (its own spread), nothing else
int main(int argc, char **argv)
{
    const bool rot_only = argc > 1 && !strcmp(argv[1], "rot");
    const int rot_reps = rot_only && argc > 2 ? atoi(argv[2]) : 1;
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    const double clk_ghz = prop.clockRate * 1e-6;
    printf("device %s (%s)  CUs %d  clock %.3f GHz\n", prop.name, prop.gcnArchName, cus, clk_ghz);
    double *out;
    const int blocks_per_cu[] = {1, 2, 4};
    CHECK(hipMalloc(&out, sizeof(double) * 256 * cus * 8));

    // ~150 ms of fp64 FMAs first: the chip needs tens of ms to reach its sustained clock
    for (int r = 0; r < 300; ++r) hipLaunchKernelGGL(op_kernel<OP_FMA64>, dim3(cus * 4), dim3(256), 0, 0, out, 1.5);
    CHECK(hipDeviceSynchronize());
    {   // the clock this run holds under fp64 load: a v_fma_f64 issues every 4 cycles per SIMD (four waves per SIMD)
        const double ms = time_kernel([&]() { hipLaunchKernelGGL(op_kernel<OP_FMA64>, dim3(cus * 4), dim3(256), 0, 0, out, 1.5); }, 5);
        const double cyc = ms * 1e-3 * clk_ghz * 1e9 / ((double)ITERS * UNROLL * 4);
        printf("clock held under fp64 load: %.3f GHz (v_fma_f64 at %.2f nominal cycles, 4 real); cycles below are at the NOMINAL clock\n",
               clk_ghz * 4.0 / cyc, cyc);
    }

    if (!rot_only) printf("\n# issue rate: cycles per wave64 instruction per SIMD (at nominal clock), by waves/SIMD\n");
    if (!rot_only) printf("%-16s %10s %10s %10s\n", "op", "1 wave", "2 waves", "4 waves");
    for (int op = 0; op <= OP_MIX_PAIR && !rot_only; ++op) {
        printf("%-16s", OP_NAMES[op]);
        for (int bpc : blocks_per_cu) {
            const int grid = cus * bpc;   // 256 threads = 4 waves = 1 wave per SIMD per block
            auto launch = [&]() {
                switch (op) {
#define CASE(O) case O: hipLaunchKernelGGL(op_kernel<O>, dim3(grid), dim3(256), 0, 0, out, 1.5); break;
                    CASE(OP_FMA64) CASE(OP_MUL64) CASE(OP_ADD64) CASE(OP_RSQ64) CASE(OP_RCP64) CASE(OP_SQRT64)
                    CASE(OP_CVT64_32) CASE(OP_CVT32_64) CASE(OP_FMA32) CASE(OP_RSQ32)
                    CASE(OP_MFMA64_4) CASE(OP_MFMA64_4_FMA6) CASE(OP_FMA64_X6) CASE(OP_PKFMA32) CASE(OP_PKFMA32_RSQ)
#undef CASE
                case OP_MIX_PAIR: hipLaunchKernelGGL(pair_kernel, dim3(grid), dim3(256), 0, 0, out, 1.5); break;
                }
            };
            const double ms = time_kernel(launch, 5);
            const double instr_per_simd = (double)ITERS * UNROLL * bpc;   // wave-instructions per SIMD
            const double cyc = ms * 1e-3 * clk_ghz * 1e9 / instr_per_simd;
            printf(" %10.2f", cyc);
        }
        if (op == OP_MIX_PAIR) printf("   <- cycles per PAIR-instruction group (13 VALU + rsq + 2 adds)");
        printf("\n");
    }

    // rotation cost of the pair-symmetric fp64 sweep, in the units of pair_body_f64 above; v_fma_f64 once more right before
    // them gives the clock these rows held (an fp64 FMA issues every 4 cycles per SIMD)
    printf("\n");
    const bool dpp_ok = dpp_rol_check();
    const char *rot_names[] = {"v_fma_f64", "pair_sym_f64", "pair_sym+bperm", "pair_sym+ldsrot", "pair_sym+dpp", "pair_sym+dppall"};
    double fma_cyc4 = 4.0;
    for (int rep = 0; rep < rot_reps; ++rep) {
        printf("\n# rotation cost: cycles per PAIR (14 VALU + rsq, sweep<double, 2, 4, 4> uniform off-diagonal) per SIMD at nominal clock\n");
        printf("%-16s %10s %10s %10s\n", "op", "1 wave", "2 waves", "4 waves");
        for (int row = 0; row < 6; ++row) {
            printf("%-16s", rot_names[row]);
            for (int bpc : blocks_per_cu) {
                const int grid = cus * bpc;
                auto launch = [&]() {
                    switch (row) {
                    case 0: hipLaunchKernelGGL(op_kernel<OP_FMA64>, dim3(grid), dim3(256), 0, 0, out, 1.5); break;
                    case 1: hipLaunchKernelGGL(sweep_rot_kernel<ROT_NONE>, dim3(grid), dim3(256), 0, 0, out, 1.5); break;
                    case 2: hipLaunchKernelGGL(sweep_rot_kernel<ROT_BPERMUTE>, dim3(grid), dim3(256), 0, 0, out, 1.5); break;
                    case 3: hipLaunchKernelGGL(sweep_rot_kernel<ROT_LDS>, dim3(grid), dim3(256), 0, 0, out, 1.5); break;
                    case 4: hipLaunchKernelGGL(sweep_rot_kernel<ROT_DPP>, dim3(grid), dim3(256), 0, 0, out, 1.5); break;
                    case 5: hipLaunchKernelGGL(sweep_rot_kernel<ROT_DPPALL>, dim3(grid), dim3(256), 0, 0, out, 1.5); break;
                    }
                };
                const double ms = time_kernel(launch, 5);
                const double per_simd = row == 0 ? (double)ITERS * UNROLL * bpc : (double)ROT_SWEEPS * 64 * 16 * bpc;
                const double cyc = ms * 1e-3 * clk_ghz * 1e9 / per_simd;
                if (row == 0 && bpc == 4) fma_cyc4 = cyc;
                printf(" %10.2f", cyc);
            }
            if (row == 2) printf("   <- + 2 ds_bpermute_b32 per pair");
            if (row == 3) printf("   <- + 0.75 ds_read_b128 / ds_write_b128 per pair");
            if (row == 4) printf("   <- + 0.25 ds_read_b128 + 1 v_mov_b32_dpp per pair");
            if (row == 5) printf("   <- + 2 v_mov_b32_dpp per pair");
            printf("\n");
        }
        printf("clock held (4 cycles per v_fma_f64 at 4 waves): %.3f GHz of %.3f nominal -> real cycles = nominal x %.3f\n",
               clk_ghz * 4.0 / fma_cyc4, clk_ghz, 4.0 / fma_cyc4);
    }
    if (rot_only) return dpp_ok ? 0 : 1;

    // accuracy of v_rsq_f64 and of the corrected q^-1.5
    const int n = 1 << 20;
    std::vector<double> hx(n), hr(n), h3(n);
    srand(1);
    for (int i = 0; i < n; ++i) hx[i] = exp((rand() / (double)RAND_MAX) * 40.0 - 20.0);
    double *dx, *dr, *d3;
    CHECK(hipMalloc(&dx, n * 8)); CHECK(hipMalloc(&dr, n * 8)); CHECK(hipMalloc(&d3, n * 8));
    CHECK(hipMemcpy(dx, hx.data(), n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(rsq_accuracy_kernel, dim3(n / 256), dim3(256), 0, 0, dx, dr, d3, n);
    CHECK(hipMemcpy(hr.data(), dr, n * 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h3.data(), d3, n * 8, hipMemcpyDeviceToHost));
    long double e1 = 0, e3 = 0;
    for (int i = 0; i < n; ++i) {
        const long double t1 = 1.0L / sqrtl((long double)hx[i]);
        const long double t3 = t1 * t1 * t1;
        e1 = fmaxl(e1, fabsl((hr[i] - t1) / t1));
        e3 = fmaxl(e3, fabsl((h3[i] - t3) / t3));
    }
    printf("\n# accuracy over %d log-uniform samples in [e^-20, e^20]\n", n);
    printf("v_rsq_f64 max rel err      = %.3Le  (2^%.1Lf)\n", e1, log2l(e1));
    printf("corrected q^-1.5 max rel err = %.3Le  (%.2Lf ulp of fp64)\n", e3, e3 / 1.1102230246251565e-16L);
    return 0;
}
