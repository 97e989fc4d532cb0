// Times the two forms of the persistent local BA's per-workgroup Schur product S = Yt^T Yt (ba_persist.hpp) WITHOUT the rest of a trial, in the
// product's real shape: one workgroup of 256 threads (one wave per SIMD) on every CU, a random panel in LDS,
//   form 0: schur_item_product — vector FMA on 4x4 register blocks, nblk upper blocks x KS splits of the K range (KS as the plan chose it),
//   form 1: schur_product_mfma — v_mfma_f64_16x16x4_f64 on the upper 16x16 tiles, operands from LDS a k-step ahead, accumulators used
//           round-robin, written out from the MFMA C layout into the same 4x4-block partial format (one K-split slot per wave up to three
//           tile rows, tiles dealt to the waves from four on),
// each with its write-out and the barrier behind it.  Per form: shader clocks (s_memtime) of the best of `reps` repetitions on workgroup 0, the
// wall clock (100 MHz) over all repetitions and the shader clock the run held (clocks / wall time over all repetitions).  The two results
// (K-splits added in order, as the kernel's store loop does) are compared element by element over the upper triangle.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I ucoslam-cv3_amd/csrc -I include scripts/micro/schur_product_mfma.hip ucoslam-cv3_amd/csrc/ctx.hip -o scripts/micro/schur_product_mfma.bin
#include <hip/hip_runtime.h>
#include "ba.hip"
#include "schur_item_product.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

__device__ __forceinline__ long long now_clk() { long long t; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory"); return t; }

template <int NF, int FORM>
__global__ __launch_bounds__(256) void k(const double* panel, double* out, int krows, int nb4, int nblk, int KS, int ntt, long long* clk, int reps) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ unsigned char s_blk[600][2];
    __builtin_amdgcn_s_setprio(3);
    constexpr int YS = 6 * NF + 2;
    double* Yt = lds;
    double* U = lds + krows * YS;
    const int tid = threadIdx.x, lane = tid & 63, wvu = __builtin_amdgcn_readfirstlane(tid >> 6), OFF_CAM = nblk * 16;
    for (int i = tid; i < krows * YS; i += 256) Yt[i] = panel[i];
    for (int t = tid; t < nblk; t += 256) { int bi = 0, rem = t; while (rem >= nb4 - bi) { rem -= nb4 - bi; ++bi; } s_blk[t][0] = bi; s_blk[t][1] = bi + rem; }
    long long best = 1ll << 60, wall = 0, total = 0;
    for (int r = 0; r < reps; r++) {
        __syncthreads();
        const long long w0 = wall_clock64();
        const long long t0 = now_clk();
        if (FORM == 0) {
            const int nitems = nblk * KS;
            const int kc = (krows + KS - 1) / KS;
            for (int item = tid; item < nitems; item += 256) {
                const int kt = item / nblk, bq = item - kt * nblk;
                const int bi = s_blk[bq][0], bj = s_blk[bq][1];
                const int kbeg = kt * kc, kend = min(krows, kbeg + kc);
                double acc4[16];
#pragma unroll
                for (int i = 0; i < 16; i++) acc4[i] = 0;
                schur_item_product<YS>(Yt + kbeg * YS + 4 * bi, Yt + kbeg * YS + 4 * bj, kend - kbeg, acc4);
#pragma unroll
                for (int i = 0; i < 16; i++) U[kt * OFF_CAM + bq * 16 + i] = acc4[i];
            }
        } else {
            schur_product_mfma<NF>(Yt, krows, ntt, U, OFF_CAM, nb4, wvu, lane);
        }
        __syncthreads();   // (the kernel's barrier behind the product: the slowest wave counts)
        const long long t1 = now_clk();
        const long long w1 = wall_clock64();
        if (t1 - t0 < best) best = t1 - t0;
        wall += w1 - w0; total += t1 - t0;
    }
    if (blockIdx.x == 0) {
        if (tid == 0) { clk[0] = best; clk[1] = wall; clk[2] = total; }
        const int ksl = FORM == 0 ? KS : schur_mfma_splits(ntt);
        for (int i = tid; i < OFF_CAM; i += 256) {   // the splits added in order, as the kernel's store loop sends them
            double v = U[i];
            for (int kt = 1; kt < ksl; kt++) v += U[kt * OFF_CAM + i];
            out[i] = v;
        }
    }
}

template <int NF, int FORM>
void run(const std::vector<double>& panel, int krows, int nfree, int KS, int ncu, std::vector<double>& res, long long (&c)[3], int reps) {
    constexpr int YS = 6 * NF + 2;
    const int n = 6 * nfree, nb4 = (n + 3) / 4, nblk = nb4 * (nb4 + 1) / 2, ntt = (n + 15) / 16;
    const int slots = std::max(KS, schur_mfma_splits(ntt));
    double *dP, *dO; long long* dc;
    (void)hipMalloc(&dP, panel.size() * 8); (void)hipMalloc(&dO, (size_t)nblk * 16 * 8); (void)hipMalloc(&dc, 64);
    (void)hipMemcpy(dP, panel.data(), panel.size() * 8, hipMemcpyHostToDevice);
    (void)hipMemset(dc, 0, 64);
    (void)hipMemset(dO, 0, (size_t)nblk * 16 * 8);
    const size_t lds = ((size_t)krows * YS + (size_t)slots * nblk * 16) * 8;
    const size_t lds_one_per_cu = lds > 96 * 1024 ? lds : 96 * 1024;   // more than half a CU's 160 KB: one workgroup per CU
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k<NF, FORM>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_one_per_cu);
    hipLaunchKernelGGL((k<NF, FORM>), dim3(ncu), dim3(256), lds_one_per_cu, 0, dP, dO, krows, nb4, nblk, KS, ntt, dc, reps);
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) { printf("launch failed: %s\n", hipGetErrorString(e)); exit(2); }
    (void)hipMemcpy(c, dc, sizeof(c), hipMemcpyDeviceToHost);
    res.resize((size_t)nblk * 16);
    (void)hipMemcpy(res.data(), dO, res.size() * 8, hipMemcpyDeviceToHost);
    (void)hipFree(dP); (void)hipFree(dO); (void)hipFree(dc);
}

// the K-splits plan_persist chooses for the 4x4 form
int plan_ks(int krows, int n, int nblk) {
    int KS = 1, best = 1 << 30;
    for (int ks = 1; ks <= 6; ks++) {
        if (ks > 1 && ks * nblk * 16 > (n + 1) * (n + 1) + 1452) break;
        const int rounds = (nblk * ks + 255) / 256, depth = ((krows + ks - 1) / ks + 3) & ~3;
        if (rounds * depth < best) { best = rounds * depth; KS = ks; }
    }
    return KS;
}

template <int NF>
int shape(int krows, int nfree, int ncu) {
    constexpr int YS = 6 * NF + 2;
    const int n = 6 * nfree, nb4 = (n + 3) / 4, nblk = nb4 * (nb4 + 1) / 2, ntt = (n + 15) / 16, KS = plan_ks(krows, n, nblk), reps = 200;
    std::mt19937 rng(krows * 131 + nfree); std::normal_distribution<double> N(0, 1);
    std::vector<double> panel((size_t)krows * YS, 0.0);
    for (int r = 0; r < krows; r++) for (int j = 0; j < n; j++) panel[(size_t)r * YS + j] = N(rng);   // (columns n .. YS-1 stay zero, as in the kernel)
    std::vector<double> r0, r1; long long c0[3], c1[3];
    run<NF, 0>(panel, krows, nfree, KS, ncu, r0, c0, reps);
    run<NF, 1>(panel, krows, nfree, KS, ncu, r1, c1, reps);
    // element by element over the upper triangle, relative to sqrt(S_ii S_jj) (an entry itself may cancel to nearly nothing); the words
    // of the diagonal blocks' lower halves and of the columns n .. 4 nb4 - 1 must be the same too (both forms write every word of the partial)
    auto at = [&](const std::vector<double>& v, int row, int col) { const int bi = row >> 2, bj = col >> 2; return v[(size_t)(bi * nb4 - bi * (bi - 1) / 2 + (bj - bi)) * 16 + (row & 3) * 4 + (col & 3)]; };
    double rel = 0, rel_host = 0; size_t pad_bad = 0;
    for (int i = 0; i < 4 * nb4; i++) for (int j = (i & ~3); j < 4 * nb4; j++) {
        const double a = at(r0, i, j), b = at(r1, i, j);
        if (j < i || j >= n || i >= n) { pad_bad += !(std::fabs(a - b) <= 1e-12 * std::sqrt(std::fabs(at(r0, std::min(i, j), std::min(i, j)) * at(r0, std::max(i, j), std::max(i, j)))) ); continue; }
        long double s = 0;
        for (int kk = 0; kk < krows; kk++) s += (long double)panel[(size_t)kk * YS + i] * panel[(size_t)kk * YS + j];
        const double sc = std::sqrt(at(r0, i, i) * at(r0, j, j));
        rel = std::max(rel, std::fabs(a - b) / sc);
        rel_host = std::max(rel_host, std::fabs(b - (double)s) / sc);
    }
    const double mhz0 = c0[2] / (c0[1] * 0.01), mhz1 = c1[2] / (c1[1] * 0.01);
    printf("<%2d> krows %3d n %2d ntt %d (%3d workgroups): 4x4 vector form (KS %d) %6lld clocks best, %.3f us mean wall, %.0f MHz held | MFMA form (%d slot%s) %6lld clocks best, %.3f us mean wall, %.0f MHz held | "
           "largest relative difference %.2e (MFMA against a long-double sum %.2e), padding words that differ: %zu\n",
           NF, krows, n, ntt, ncu, KS, c0[0], c0[1] * 0.01 / reps, mhz0, schur_mfma_splits(ntt), schur_mfma_splits(ntt) > 1 ? "s" : "", c1[0], c1[1] * 0.01 / reps, mhz1, rel, rel_host, pad_bad);
    return !(rel < 1e-13) || !(rel_host < 1e-13) || pad_bad != 0;
}

int main() {
    hipDeviceProp_t p; (void)hipGetDeviceProperties(&p, 0);
    const int ncu = p.multiProcessorCount;
    int bad = 0;
    bad += shape<8>(96, 8, ncu);     // the headline: 10 keyframes (8 free) x 3000 points, six tiles, six k-steps per wave
    bad += shape<8>(96, 8, 1);       // a lone workgroup (no other CU on the clock / power budget)
    bad += shape<8>(48, 8, ncu);     // three k-steps per wave
    bad += shape<8>(32, 6, ncu);     // n = 36: three tile rows, the last partly used; two k-steps per wave
    bad += shape<8>(32, 3, ncu);     // n = 18: two tile rows
    bad += shape<8>(32, 2, ncu);     // n = 12: one tile
    bad += shape<8>(32, 1, ncu);     // n = 6
    bad += shape<16>(48, 9, ncu);    // <16>: four tile rows, ten tiles dealt 3 3 2 2
    bad += shape<16>(48, 13, ncu);   // five tile rows, fifteen tiles
    bad += shape<16>(48, 16, ncu);   // six tile rows, 21 tiles dealt 6 5 5 5
    printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
