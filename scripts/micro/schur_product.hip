// Times the persistent local BA's per-workgroup Schur product S = Yt^T Yt (4x4 register blocks, nblk upper blocks x KS splits of the K range,
// the kernel's form until the product moved to the f64 matrix pipe, now schur_item_product.hpp beside this file; schur_product_mfma.hip times the
// two against each other) WITHOUT the rest of a trial: one workgroup of 256 threads (one wave per SIMD) on every CU, a random panel in LDS, the loop
// the kernel had before the hand-pipelined one (form 0: four rows per iteration, clamped row index, 1.0 / 0.0 row mask, the compiler's own
// schedule) against schur_item_product (form 1).  Per form: shader clocks (s_memtime) of the best of `reps` repetitions on workgroup 0, the
// wall clock (100 MHz) over all repetitions, and the two results compared bit for bit.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I ucoslam-cv3_amd/csrc -I include scripts/micro/schur_product.hip ucoslam-cv3_amd/csrc/ctx.hip -o scripts/micro/schur_product.bin
#include <hip/hip_runtime.h>
#include "ba.hip"
#include "schur_item_product.hpp"
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

__device__ __forceinline__ long long now_clk() { long long t; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory"); return t; }

constexpr int kYS = 6 * 8 + 2;   // the <8> kernel's panel row

template <int FORM>
__global__ __launch_bounds__(256) void k(const double* panel, double* out, int krows, int nb4, int nblk, int KS, long long* clk, int reps) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ unsigned char s_blk[160][2];
    __builtin_amdgcn_s_setprio(3);
    constexpr int YS = kYS;
    double* Yt = lds;
    double* U = lds + krows * YS;
    const int tid = threadIdx.x, OFF_CAM = nblk * 16;
    for (int i = tid; i < krows * YS; i += 256) Yt[i] = panel[i];
    for (int t = tid; t < nblk; t += 256) { int bi = 0, rem = t; while (rem >= nb4 - bi) { rem -= nb4 - bi; ++bi; } s_blk[t][0] = bi; s_blk[t][1] = bi + rem; }
    long long best = 1ll << 60, wall = 0;
    for (int r = 0; r < reps; r++) {
        __syncthreads();
        const long long w0 = wall_clock64();
        const long long t0 = now_clk();
        const int nitems = nblk * KS;
        const int kc = (krows + KS - 1) / KS;
        for (int item = tid; item < nitems; item += 256) {
            const int kt = item / nblk, bq = item - kt * nblk;
            const int bi = s_blk[bq][0], bj = s_blk[bq][1];
            const int kbeg = kt * kc, kend = min(krows, kbeg + kc);
            double acc4[16];
#pragma unroll
            for (int i = 0; i < 16; i++) acc4[i] = 0;
            if (FORM == 0) {
                const double* ra = Yt + 4 * bi, * rb = Yt + 4 * bj;
                for (int kk0 = kbeg; kk0 < kend; kk0 += 4) {
                    double2 a01[4], a23[4], b01[4], b23[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int kk = kk0 + u < kend ? kk0 + u : kbeg;
                        a01[u] = *reinterpret_cast<const double2*>(ra + kk * YS); a23[u] = *reinterpret_cast<const double2*>(ra + kk * YS + 2);
                        b01[u] = *reinterpret_cast<const double2*>(rb + kk * YS); b23[u] = *reinterpret_cast<const double2*>(rb + kk * YS + 2);
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const double z = kk0 + u < kend ? 1.0 : 0.0;
                        const double av[4] = {a01[u].x * z, a01[u].y * z, a23[u].x * z, a23[u].y * z}, bv[4] = {b01[u].x, b01[u].y, b23[u].x, b23[u].y};
#pragma unroll
                        for (int rr = 0; rr < 4; rr++)
#pragma unroll
                            for (int c = 0; c < 4; c++) acc4[rr * 4 + c] = fma(av[rr], bv[c], acc4[rr * 4 + c]);
                    }
                }
            } else if (FORM == 1) {
                schur_item_product<YS>(Yt + kbeg * YS + 4 * bi, Yt + kbeg * YS + 4 * bj, kend - kbeg, acc4);
            } else if (FORM == 2) {   // the FMAs alone: one group's operands, fetched once, multiplied as often as the split has groups
                const double* ra = Yt + kbeg * YS + 4 * bi, * rb = Yt + kbeg * YS + 4 * bj;
                double av[4][4], bv[4][4];
#pragma unroll
                for (int u = 0; u < 4; u++)
#pragma unroll
                    for (int c = 0; c < 4; c++) { av[u][c] = ra[u * YS + c]; bv[u][c] = rb[u * YS + c]; }
                for (int g = 0; g < (kend - kbeg) >> 2; g++) {
#pragma unroll
                    for (int u = 0; u < 4; u++)
#pragma unroll
                        for (int rr = 0; rr < 4; rr++)
#pragma unroll
                            for (int c = 0; c < 4; c++) acc4[rr * 4 + c] = fma(av[u][rr], bv[u][c], acc4[rr * 4 + c]);
                    asm volatile("" ::: "memory");
                }
            } else {   // the reads alone: the same sixteen ds_read_b128 per group, waited for a group at a time, nothing multiplied
                typedef __attribute__((address_space(3))) const double* lds_cptr;
                unsigned pa = (unsigned)(size_t)(lds_cptr)(Yt + kbeg * YS + 4 * bi), pb = (unsigned)(size_t)(lds_cptr)(Yt + kbeg * YS + 4 * bj);
                ba_d2 x0, x1, x2, x3;
                for (int g = 0; g < (kend - kbeg) >> 2; g++) {
#define RD(off) asm volatile("ds_read_b128 %0, %4 offset:%6\n\tds_read_b128 %1, %4 offset:%7\n\tds_read_b128 %2, %5 offset:%6\n\tds_read_b128 %3, %5 offset:%7" \
                             : "=&v"(x0), "=&v"(x1), "=&v"(x2), "=&v"(x3) : "v"(pa), "v"(pb), "n"(off), "n"((off) + 16))
                    RD(0); RD(YS * 8); RD(2 * YS * 8); RD(3 * YS * 8);
#undef RD
                    pa += 4 * YS * 8; pb += 4 * YS * 8;
                }
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3));
                acc4[0] = x0.x + x1.x + x2.x + x3.x;
            }
#pragma unroll
            for (int i = 0; i < 16; i++) U[kt * OFF_CAM + bq * 16 + i] = acc4[i];
        }
        __syncthreads();   // (the kernel's barrier behind the product: the slowest wave counts)
        const long long t1 = now_clk();
        const long long w1 = wall_clock64();
        if (t1 - t0 < best) best = t1 - t0;
        wall += w1 - w0;
    }
    if (blockIdx.x == 0) {
        if (tid == 0) { clk[0] = best; clk[1] = wall; }
        for (int i = tid; i < KS * OFF_CAM; i += 256) out[i] = U[i];
    }
}

template <int FORM>
void run(const std::vector<double>& panel, int krows, int nfree, int KS, int ncu, std::vector<double>& res, long long (&c)[2], int reps) {
    const int n = 6 * nfree, nb4 = (n + 3) / 4, nblk = nb4 * (nb4 + 1) / 2;
    double *dP, *dO; long long* dc;
    (void)hipMalloc(&dP, panel.size() * 8); (void)hipMalloc(&dO, (size_t)KS * nblk * 16 * 8); (void)hipMalloc(&dc, 64);
    (void)hipMemcpy(dP, panel.data(), panel.size() * 8, hipMemcpyHostToDevice);
    (void)hipMemset(dc, 0, 64);
    const size_t lds = ((size_t)krows * kYS + (size_t)KS * nblk * 16) * 8;
    const size_t lds_one_per_cu = lds > 96 * 1024 ? lds : 96 * 1024;   // more than half a CU's 160 KB: one workgroup per CU
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k<FORM>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_one_per_cu);
    hipLaunchKernelGGL(k<FORM>, dim3(ncu), dim3(256), lds_one_per_cu, 0, dP, dO, krows, nb4, nblk, KS, dc, reps);
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) { printf("launch failed: %s\n", hipGetErrorString(e)); exit(2); }
    (void)hipMemcpy(c, dc, sizeof(c), hipMemcpyDeviceToHost);
    res.resize((size_t)KS * nblk * 16);
    (void)hipMemcpy(res.data(), dO, res.size() * 8, hipMemcpyDeviceToHost);
    (void)hipFree(dP); (void)hipFree(dO); (void)hipFree(dc);
}

int shape(int krows, int nfree, int KS, int ncu) {
    const int n = 6 * nfree, nb4 = (n + 3) / 4, nblk = nb4 * (nb4 + 1) / 2, kc = (krows + KS - 1) / KS, reps = 200;
    std::mt19937 rng(krows * 131 + nfree); std::normal_distribution<double> N(0, 1);
    std::vector<double> panel((size_t)krows * kYS, 0.0);
    for (int r = 0; r < krows; r++) for (int j = 0; j < n; j++) panel[(size_t)r * kYS + j] = N(rng);   // (columns n .. YS-1 stay zero, as in the kernel)
    std::vector<double> r0, r1; long long c0[2], c1[2];
    run<0>(panel, krows, nfree, KS, ncu, r0, c0, reps);
    run<1>(panel, krows, nfree, KS, ncu, r1, c1, reps);
    std::vector<double> r2; long long c2[2], c3[2];
    run<2>(panel, krows, nfree, KS, ncu, r2, c2, reps);
    run<3>(panel, krows, nfree, KS, ncu, r2, c3, reps);
    const bool same = r0.size() == r1.size() && std::memcmp(r0.data(), r1.data(), r0.size() * 8) == 0;
    // a reference in the same order of additions: the partial of split kt, rows ascending, one fma per row
    size_t bad = 0;
    for (int kt = 0; kt < KS; kt++) {
        int bq = 0;
        for (int bi = 0; bi < nb4; bi++) for (int bj = bi; bj < nb4; bj++, bq++)
            for (int r = 0; r < 4; r++) for (int cc = 0; cc < 4; cc++) {
                double s = 0;
                for (int kk = kt * kc; kk < std::min(krows, kt * kc + kc); kk++) s = std::fma(panel[(size_t)kk * kYS + 4 * bi + r], panel[(size_t)kk * kYS + 4 * bj + cc], s);
                const double got = r1[((size_t)kt * nblk + bq) * 16 + r * 4 + cc];
                bad += std::memcmp(&s, &got, 8) != 0;
            }
    }
    printf("krows %3d nblk %3d KS %d kc %2d (%d workgroups): bounds, whole groups only (+ index arithmetic, stores, barrier): FMAs alone %6lld clocks, reads alone %6lld clocks\n", krows, nblk, KS, kc, ncu, c2[0], c3[0]);
    printf("krows %3d nblk %3d KS %d kc %2d (%d workgroups): parent loop %6lld clocks best (%.2f us at 2.4 GHz), %.3f us mean wall | pipelined %6lld clocks best (%.2f us), %.3f us mean wall | bitwise equal %s | against the host's ordered sum: %zu of %zu differ\n",
           krows, nblk, KS, kc, ncu, c0[0], c0[0] / 2400.0, c0[1] * 0.01 / reps, c1[0], c1[0] / 2400.0, c1[1] * 0.01 / reps, same ? "yes" : "NO", bad, r1.size());
    return !same || bad != 0;
}

int main() {
    hipDeviceProp_t p; (void)hipGetDeviceProperties(&p, 0);
    const int ncu = p.multiProcessorCount;
    int bad = 0;
    bad += shape(96, 8, 3, ncu);    // the headline: 10 keyframes (8 free) x 3000 points
    bad += shape(32, 6, 3, ncu);    // 33 landmarks, six free keyframes: kc 11, a tail of three rows, a last split of ten
    bad += shape(96, 8, 3, 1);      // a lone workgroup (no other CU on the clock / power budget)
    printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
