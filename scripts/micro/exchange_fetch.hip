// Times the two fetches of the persistent local BA's exchange (ba_persist.hpp) WITHOUT the rest of a trial: G workgroups of 256 threads,
// one per CU.  Every round each workgroup sends a partial of `nelem` tagged elements with tst() in the `part` layout
// ([slice][workgroup][SL], as phase1 does), runs the A batch (reduce_slices' indexing: slice g of every workgroup, HG source groups, up to
// eight sources per thread in one batch of loads), sends its reduced slice to `red` with tst() and runs the B batch (element tid + u * 256
// of the reduced vector).  G, SL and nelem are what plan_ba gives for the window; HG as the kernel derives it.
// Forms of the fetch (a compile-time choice HERE only; the kernel has one form):
//   a   two 8-byte agent-scope atomic loads per element, a failed poll re-issues the whole batch   (the kernel before this file existed)
//   b   one 16-byte sc1 buffer load per element (tld_raw), a failed poll re-issues the whole batch
//   bm  b + a failed poll re-issues only the elements whose tag has not matched                     (the kernel now)
//   c   bm + slices padded to a multiple of 8 elements (128 bytes) in `part` and `red`
// `delay`: wall-clock ticks (10 ns) every workgroup idles between its stores and its first poll.  0: the poll also waits for the slowest
// sender; 300: the data are there when the poll is issued (the kernel's case: DESIGN 4.3, hand-offs, measurement (i)) and the time is the
// batch's own.  Per form: shader clocks (s_memtime) of workgroup 0, best and mean over the rounds, barrier behind the batch included
// (the slowest wave counts); the mean over all workgroups; and the fetched values of all rounds folded into one word per thread, which
// must be bitwise equal between the forms.  Every spin is bounded: 50 ms without a match and the launch gives up (reported, exit 2).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I ucoslam-cv3_amd/csrc -I include scripts/micro/exchange_fetch.hip ucoslam-cv3_amd/csrc/ctx.hip -o scripts/micro/exchange_fetch.bin
#include <hip/hip_runtime.h>
#include "ba.hip"
#include <cstdio>
#include <cstring>
#include <vector>

__device__ __forceinline__ long long now_clk() { long long t; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory"); return t; }

struct XArgs {
    pword* part; pword* red; unsigned* abort_word;
    int G, SL, SLP, HG, nelem, rounds, delay;
    long long* clk;            // [G][4]: A best, A sum, B best, B sum
    unsigned long long* fold;  // [G][256]
};

__device__ __forceinline__ double payload(int g, int i, int r) {   // exact in a double, sums of 256 of them too
    return (double)(((unsigned)g * 2654435761u ^ (unsigned)i * 40503u ^ (unsigned)r * 2246822519u) & 0xFFFFFu) * 0.125;
}

template <bool WIDE, bool MASK>
__global__ __launch_bounds__(256) void k(XArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ int s_abort;
    double* R = lds;
    const int tid = threadIdx.x, g = blockIdx.x, G = a.G, SL = a.SL, SLP = a.SLP, HG = a.HG;
    const trsrc_t rs_part = trsrc(a.part), rs_red = trsrc(a.red);
    if (tid == 0) s_abort = 0;
    __syncthreads();
    auto give_up = [&](long long& t0) -> bool {
        if (t0 < 63) { ++t0; return false; }
        if (t0 == 63) t0 = wall_clock64();
        if (__hip_atomic_load(a.abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u || wall_clock64() - t0 > 5000000ll) {
            s_abort = 1;
            __hip_atomic_store(a.abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return true;
        }
        __builtin_amdgcn_s_sleep(1);
        return false;
    };
    auto fetch = [&](const pword* base, trsrc_t rs, size_t i) -> TWord {
        if (WIDE) return tld_raw(rs, i);
        TWord w;
        w.lo = __hip_atomic_load(base + 2 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        w.hi = __hip_atomic_load(base + 2 * i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return w;
    };
    auto tload8 = [&](const pword* base, trsrc_t rs, size_t first, size_t stride, int cnt, unsigned tag, double (&v)[8]) {
        long long t0 = 0;
        unsigned todo = (1u << cnt) - 1u;
        const unsigned all = todo;
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = 0.0;
        for (;;) {
            tpoll_begin();
            TWord w[8];
#pragma unroll
            for (int u = 0; u < 8; u++) if ((todo >> u) & 1u) w[u] = fetch(base, rs, first + u * stride);
#pragma unroll
            for (int u = 0; u < 8; u++) if (((todo >> u) & 1u) && tok(w[u], tag)) { v[u] = tval(w[u]); todo &= ~(1u << u); }
            if (!todo || give_up(t0)) return;
            if (!MASK) todo = all;
        }
    };
    const unsigned sl_inv = (unsigned)(0x100000000ull / (unsigned)SL) + 1u;
    auto div_sl = [&](int i) -> int { return (int)__umulhi((unsigned)i, sl_inv); };
    auto part_at = [&](int i) -> size_t { const int sl = div_sl(i); return ((size_t)sl * G + g) * SLP + (i - sl * SL); };
    auto red_at = [&](int i) -> size_t { const int sl = div_sl(i); return (size_t)sl * SLP + (i - sl * SL); };
    long long bestA = 1ll << 60, bestB = 1ll << 60, sumA = 0, sumB = 0;
    unsigned long long fold = 0;
    for (int r = 0; r < a.rounds; r++) {
        const unsigned tagA = (1u << 12) | (unsigned)(2 * r + 1), tagB = (1u << 12) | (unsigned)(2 * r + 2);
        for (int i = tid; i < a.nelem; i += 256) tst(a.part, part_at(i), payload(g, i, r), tagA);
        if (a.delay) { const long long w0 = wall_clock64(); while (wall_clock64() - w0 < a.delay) __builtin_amdgcn_s_sleep(8); }
        __syncthreads();
        const long long t0 = now_clk();
        const size_t src = (size_t)g * G * SLP;
        for (int idx = tid; idx < SL * HG; idx += 256) {
            const int hg = div_sl(idx), e = idx - hg * SL;
            const bool used = g * SL + e < a.nelem;
            double s = 0.0;
            for (int h = hg; used && h < G; h += 8 * HG) {
                double v[8];
                const int cnt = min(8, (G - h + HG - 1) / HG);
                tload8(a.part, rs_part, src + (size_t)h * SLP + e, (size_t)HG * SLP, cnt, tagA, v);
#pragma unroll
                for (int u = 0; u < 8; u++) if (u < cnt) s += v[u];
            }
            R[idx] = s;
        }
        __syncthreads();
        const long long t1 = now_clk();
        if (s_abort) break;
        for (int e = tid; e < SL; e += 256) {
            double s = R[e];
            for (int hg = 1; hg < HG; hg++) s += R[hg * SL + e];
            if (g * SL + e < a.nelem) tst(a.red, (size_t)g * SLP + e, s, tagB);
        }
        if (a.delay) { const long long w0 = wall_clock64(); while (wall_clock64() - w0 < a.delay) __builtin_amdgcn_s_sleep(8); }
        __syncthreads();
        const long long t2 = now_clk();
        for (int b0 = 0; b0 < a.nelem; b0 += 8 * 256) {
            double rv[8];
            const int left = a.nelem - b0 - tid;
            const int cnt = left <= 0 ? 0 : min(8, (left + 255) / 256);
            // (padded slices: the elements a thread fetches are the same, their addresses follow the slices)
            if (SLP == SL) tload8(a.red, rs_red, (size_t)(b0 + tid), 256, cnt, tagB, rv);
            else {   // no common stride: element by element through the same batch (first = 0, the offsets ride in a table)
                long long tt = 0;
                unsigned todo = (1u << cnt) - 1u;
#pragma unroll
                for (int u = 0; u < 8; u++) rv[u] = 0.0;
                size_t at[8];
#pragma unroll
                for (int u = 0; u < 8; u++) at[u] = u < cnt ? red_at(b0 + tid + u * 256) : 0;
                for (;;) {
                    tpoll_begin();
                    TWord w[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) if ((todo >> u) & 1u) w[u] = fetch(a.red, rs_red, at[u]);
#pragma unroll
                    for (int u = 0; u < 8; u++) if (((todo >> u) & 1u) && tok(w[u], tagB)) { rv[u] = tval(w[u]); todo &= ~(1u << u); }
                    if (!todo || give_up(tt)) break;
                }
            }
#pragma unroll
            for (int u = 0; u < 8; u++) fold = fold * 0x9E3779B97F4A7C15ull + (unsigned long long)__double_as_longlong(rv[u]);
        }
        __syncthreads();
        const long long t3 = now_clk();
        if (s_abort) break;
        if (r >= 8) {   // (the first rounds fill the TLBs)
            bestA = min(bestA, t1 - t0); sumA += t1 - t0;
            bestB = min(bestB, t3 - t2); sumB += t3 - t2;
        }
    }
    if (tid == 0) { a.clk[4 * g] = bestA; a.clk[4 * g + 1] = sumA; a.clk[4 * g + 2] = bestB; a.clk[4 * g + 3] = sumB; }
    a.fold[(size_t)g * 256 + tid] = fold;
}

struct Res { double A0_best, A0_mean, B0_best, B0_mean, A_all, B_all; std::vector<unsigned long long> fold; bool gave_up; };

template <bool WIDE, bool MASK>
Res run(int G, int SL, int SLP, int HG, int nelem, int rounds, int delay) {
    XArgs a{};
    const size_t npart = (size_t)G * G * SLP, nred = (size_t)G * SLP;
    (void)hipMalloc(&a.part, npart * 16 + 256); (void)hipMalloc(&a.red, nred * 16 + 256); (void)hipMalloc(&a.abort_word, 64);
    (void)hipMalloc(&a.clk, (size_t)G * 4 * 8); (void)hipMalloc(&a.fold, (size_t)G * 256 * 8);
    (void)hipMemset(a.part, 0, npart * 16 + 256); (void)hipMemset(a.red, 0, nred * 16 + 256); (void)hipMemset(a.abort_word, 0, 64);
    a.G = G; a.SL = SL; a.SLP = SLP; a.HG = HG; a.nelem = nelem; a.rounds = rounds; a.delay = delay;
    const size_t lds = 96 * 1024;   // more than half a CU's 160 KB: one workgroup per CU
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k<WIDE, MASK>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((k<WIDE, MASK>), dim3(G), dim3(256), lds, 0, a);
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) { printf("launch failed: %s\n", hipGetErrorString(e)); exit(2); }
    std::vector<long long> c((size_t)G * 4);
    Res r;
    r.fold.resize((size_t)G * 256);
    unsigned ab = 0;
    (void)hipMemcpy(c.data(), a.clk, c.size() * 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(r.fold.data(), a.fold, r.fold.size() * 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&ab, a.abort_word, 4, hipMemcpyDeviceToHost);
    r.gave_up = ab != 0;
    const double n = rounds - 8;
    r.A0_best = (double)c[0]; r.A0_mean = c[1] / n; r.B0_best = (double)c[2]; r.B0_mean = c[3] / n;
    r.A_all = 0; r.B_all = 0;
    for (int g = 0; g < G; g++) { r.A_all += c[4 * g + 1] / n / G; r.B_all += c[4 * g + 3] / n / G; }
    (void)hipFree(a.part); (void)hipFree(a.red); (void)hipFree(a.abort_word); (void)hipFree(a.clk); (void)hipFree(a.fold);
    return r;
}

int window(int K, int nfree, int P, int lw, int ncu) {
    BAPlanIn in{}; in.K = K; in.P = P; in.E = P * K; in.nfree = nfree; in.stereo = false; in.persist_ok = true; in.markers = false;
    BAKnobs kn; if (lw > 0) kn.lw = lw;
    BALimits lim{}; lim.cus = ncu; lim.max_lds = 160 * 1024; lim.packed_static = 0;
    const BAPlan pl = plan_ba(in, kn, lim);
    if (pl.form != kFormPersist) { printf("%d keyframes x %d points: not the persistent form on %d CUs, skipped\n", K, P, ncu); return 0; }
    const int G = pl.ps.G, SL = pl.ps.SL, nelem = pl.ps.nelem, HG = std::max(1, std::min(G, kPThreads / SL)), SLP = (SL + 7) & ~7, rounds = 208;
    printf("%d keyframes (%d free) x %d points: G %d, Lw %d, nelem %d, SL %d (padded %d), HG %d, sources per thread <= %d; part %.1f KB fetched per workgroup, red %.1f KB\n",
           K, nfree, P, G, pl.ps.Lw, nelem, SL, SLP, HG, (G + HG - 1) / HG, G * SL * 16 / 1024.0, nelem * 16 / 1024.0);
    int bad = 0;
    for (int delay : {300, 0}) {
        printf("  idle between stores and first poll: %.1f us%s\n", delay * 0.01, delay ? " (the data are there when the poll is issued)" : " (the poll waits for the slowest sender)");
        std::vector<unsigned long long> ref;
        for (int rep = 0; rep < 3; rep++) {
            Res r[4] = {run<false, false>(G, SL, SL, HG, nelem, rounds, delay), run<true, false>(G, SL, SL, HG, nelem, rounds, delay),
                        run<true, true>(G, SL, SL, HG, nelem, rounds, delay), run<true, true>(G, SL, SLP, HG, nelem, rounds, delay)};
            const char* name[4] = {"a  8-byte x 2     ", "b  16-byte        ", "bm 16-byte + mask ", "c  bm + 128-B pad "};
            for (int f = 0; f < 4; f++) {
                if (ref.empty()) ref = r[f].fold;
                const bool same = ref == r[f].fold;
                bad += !same || r[f].gave_up;
                printf("    rep %d %s: A batch %6.0f best %7.1f mean clocks (all workgroups %7.1f) | B batch %6.0f best %7.1f mean (all workgroups %7.1f) | values bitwise equal %s%s\n",
                       rep, name[f], r[f].A0_best, r[f].A0_mean, r[f].A_all, r[f].B0_best, r[f].B0_mean, r[f].B_all, same ? "yes" : "NO", r[f].gave_up ? " | GAVE UP" : "");
            }
        }
    }
    return bad;
}

int main() {
    hipDeviceProp_t p; (void)hipGetDeviceProperties(&p, 0);
    const int ncu = p.multiProcessorCount;
    printf("%d CUs; s_memtime clocks\n", ncu);
    int bad = 0;
    bad += window(10, 8, 3000, 0, ncu);    // the headline: G = 94
    bad += window(10, 8, 2048, 8, ncu);    // the fan-in extreme: G = 256, smallest SL
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
