// Test hooks of the reduced-system solves (uh_ba_debug_solve; included at the end of ba.hip, inside its anonymous namespace): every kernel here
// loads a system the caller gives into the layout one production form expects, calls the device functions that form's production caller calls,
// in a workgroup of that caller's size, and hands back x, the factor as the form leaves it and the failure verdict.  No arithmetic of a
// solve is restated here; what is restated is each caller's glue around the calls (who publishes the verdict, which barrier follows).
//
// A: (n + 1) x (n + 1) doubles, row stride ld = n + 1 (odd: n = 6 nfree): the lower triangle of S in rows 0 .. n - 1, b in row n, and a
// NaN in every other word — production never initialises those words, so a form that reads one into a result shows it.
#pragma once

// Forms 1-4: the system in LDS with row stride ld, n + 1 <= 128 rows.
//   PERSIST: the persistent kernel's call sequence (ba_persist.hpp, "Factorisation and back substitution"), kPThreads threads, the panel
//            buffer directly behind the matrix (where an odd ld * ld leaves it 8 bytes off a 16-byte boundary);
//   else:    solve_body<true>'s, kFusedThreads threads, the panel buffer a static array.
template <bool PERSIST>
__global__ __launch_bounds__(PERSIST ? kPThreads : kFusedThreads) void ba_dbg_solve_rowlane_kernel(double* A, double* xg, int* failg, int nfree) {
    constexpr int NT = PERSIST ? kPThreads : kFusedThreads;
    constexpr int kDbgFree = 21;   // 127 rows: the two-rows-per-lane form's limit
    extern __shared__ __attribute__((aligned(16))) double dbg_lds[];
    __shared__ short s_pair[kDbgFree * (kDbgFree + 1) / 2][2];
    __shared__ double s_x[6 * kDbgFree + 2];
    __shared__ double s_zero[2];
    __shared__ int s_flag;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = 6 * nfree, ld = n + 1, npairs = nfree * (nfree + 1) / 2;
    double* const M = dbg_lds;
    for (int i = tid; i < ld * ld; i += NT) M[i] = A[i];
    for (int t = tid; t < npairs; t += NT) {   // the s1-major pair list, as both callers build it
        int s1 = 0, rem = t;
        while (rem >= nfree - s1) { rem -= nfree - s1; ++s1; }
        s_pair[t][0] = (short)s1; s_pair[t][1] = (short)(s1 + rem);
    }
    for (int i = tid; i < n; i += NT) s_x[i] = __builtin_nan("");
    if (tid == 0) { s_flag = 1; s_zero[0] = 0.0; }
    __syncthreads();
    if constexpr (PERSIST) {
        double (*const s_w)[121][6] = reinterpret_cast<double (*)[121][6]>(M + (size_t)ld * ld);
        if (n + 1 <= 64) {
            const int wvu = __builtin_amdgcn_readfirstlane(wv);
            const bool failed = ldlt_rowlane_v2<false>(M, n, ld, nfree, npairs, s_pair, &s_w[0][0][0]);
            if (wvu == 0) {
                if (!failed) backsolve_v2(M, n, ld, s_x, s_zero);
                else if (lane < n) s_x[lane] = 0.0;
                if (lane == 0) s_flag = failed ? 0 : 1;
            }
            __syncthreads();
        } else {
            const bool failed = ldlt_bordered_lds(M, n, ld, nfree, npairs, s_pair, s_w);
            if (failed && lane == 0) s_flag = 0;
            __syncthreads();
            if (s_flag) backsolve2_lds(M, n, ld, s_x);
            else for (int i = tid; i < n; i += NT) s_x[i] = 0.0;
            __syncthreads();
        }
    } else {
        __shared__ double s_w_store[2][129][6];
        double (*s_w)[121][6] = reinterpret_cast<double (*)[121][6]>(&s_w_store[0][0][0]);
        const bool failed = ldlt_bordered_lds(M, n, ld, nfree, npairs, s_pair, s_w);
        if (failed && tid == 0) s_flag = 0;
        __syncthreads();
        if (s_flag) {
            if (n <= 64) backsolve1_fused(M, n, ld, s_x, xg);
            else backsolve2_fused<NT>(M, n, ld, s_x, xg);
        } else {
            for (int i = tid; i < n; i += NT) { xg[i] = 0.0; s_x[i] = 0.0; }
        }
        __syncthreads();
    }
    for (int i = tid; i < n; i += NT) xg[i] = s_x[i];
    for (int i = tid; i < ld * ld; i += NT) A[i] = M[i];
    if (tid == 0) *failg = s_flag ? 0 : 1;
}

// Forms 5, 6: ldlt_solve_mfma_lds on the packed triangle in LDS (PACKED, kPackedThreads; the scratch block behind the triangle as
// solve_body places it) or on A itself, in HBM (kHbmThreads; the scratch block a static array).
template <bool PACKED>
__global__ __launch_bounds__(PACKED ? kPackedThreads : kHbmThreads) void ba_dbg_solve_mfma_kernel(double* A, double* xg, int* failg, int nfree) {
    constexpr int NT = PACKED ? kPackedThreads : kHbmThreads;
    extern __shared__ __attribute__((aligned(16))) double dbg_lds[];
    __shared__ double s_x[6 * (PACKED ? kPackedFree : kMaxFree)];
    __shared__ __attribute__((aligned(16))) double s_aux_hbm[PACKED ? 2 : kLdltAux];
    __shared__ int s_ok;
    const int tid = threadIdx.x;
    const int n = 6 * nfree, ld = n + 1;
    auto M = [&]() { if constexpr (PACKED) return dbg_lds; else return A; }();   // (the address space is known at compile time, as in solve_body)
    double* s_aux = s_aux_hbm;
    if constexpr (PACKED) {
        for (int i = tid; i < ld * ld; i += NT) { const int r = i / ld, c = i - r * ld; if (c <= r) M[(size_t)r * (r + 1) / 2 + c] = A[i]; }
        s_aux = dbg_lds + ((((size_t)(n + 1) * (n + 2) / 2) + 1) & ~(size_t)1);
    }
    for (int i = tid; i < n; i += NT) s_x[i] = __builtin_nan("");
    if (tid == 0) s_ok = 1;
    __syncthreads();
    const bool failed = ldlt_solve_mfma_lds<PACKED>(M, n, ld, s_aux, s_x);
    if (failed && tid == 0) s_ok = 0;
    __syncthreads();
    const int ok = s_ok;
    for (int i = tid; i < n; i += NT) xg[i] = ok ? s_x[i] : 0.0;
    if constexpr (PACKED) {
        for (int i = tid; i < ld * ld; i += NT) { const int r = i / ld, c = i - r * ld; if (c <= r) A[i] = M[(size_t)r * (r + 1) / 2 + c]; }
    }
    if (tid == 0) *failg = ok ? 0 : 1;
}

// form 7: a state whose pass is not finished, for the wide kernels' "phase == 2: nothing to do" test
__global__ __launch_bounds__(64) void ba_dbg_state_kernel(BAState* st) {
    if (threadIdx.x < 2) { BAState s{}; s.phase = 0; s.solve_ok = 1; st[threadIdx.x] = s; }
}
