// Dense blocked LDL^T with forward and back substitution for the pose-graph optimiser (posegraph.hip): fp64, no pivoting (g2o's
// LinearSolverEigen is an exact LDL^T as well), panel width 64.  The method is the wide bundle adjustment's (ba.hip, ba_ldlw_*), stated
// again here so that nothing the bundle adjustment runs depends on this module.
//
// Layout: S is (n + 1) x ld row-major with ld = n + 1; only the lower triangle of rows 0..n-1 is read; row n (the border row) holds the
// right-hand side b and leaves the factorisation as z = D^-1 L^-1 b, so the forward substitution costs nothing extra.  After
// pgl::factor_and_solve's launches x holds the solution and *fail is 1 where a pivot was zero or not finite (g2o: solve() returns false).
//
// An essential graph is sparse and, with keyframes in temporal order, mostly banded, so most of a panel's rows are exactly zero.  The panel
// kernel notes per group of 64 rows (one wave; panels start at multiples of 64, so groups and update tiles coincide) whether the panel's
// columns hold anything there, does nothing for an empty group, and the trailing update leaves out every tile whose row group or column
// group is empty.  What is left out would have subtracted exact zeros, so the factors are those of the full dense form.
#pragma once
#include <hip/hip_runtime.h>

namespace pgl {

constexpr int kNB = 64;

struct Sys {
    double* S;    // (n + 1) x ld
    double* Y;    // (n + 1) x kNB: L_rk D of the current panel
    double* x;    // n
    int* group_nz; // (n + 1 + 63) / 64: whether the 64-row group holds anything in the current panel's columns
    int* fail;
    int n;
    size_t ld;
};

// diagonal block [k0, k0 + nb): one workgroup, block in LDS; afterwards S holds L (strict lower) and d (diagonal) of the block
__global__ __launch_bounds__(256) void diag_kernel(Sys w, int k0, int nb) {
    __shared__ double A[kNB][kNB + 1];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    const size_t ld = w.ld;
    if (tid == 0) s_bad = 0;
    for (int e = tid; e < nb * nb; e += 256) { const int i = e / nb, c = e - i * nb; if (c <= i) A[i][c] = w.S[(size_t)(k0 + i) * ld + k0 + c]; }
    __syncthreads();
    for (int j = 0; j < nb; j++) {
        const double dj = A[j][j];
        if (dj == 0.0 || !isfinite(dj)) { if (tid == 0) s_bad = 1; }
        const double inv = 1.0 / dj;
        // A[i][c] -= (A[i][j] / d_j) * A[c][j], j < c <= i   (A[.][j] still holds L d_j)
        const int m = nb - 1 - j;
        for (int e = tid; e < m * m; e += 256) {
            const int i = j + 1 + e / m, c = j + 1 + e % m;
            if (c <= i) A[i][c] = fma(-(A[i][j] * inv), A[c][j], A[i][c]);
        }
        __syncthreads();
        for (int i = j + 1 + tid; i < nb; i += 256) A[i][j] *= inv;
        __syncthreads();
    }
    for (int e = tid; e < nb * nb; e += 256) { const int i = e / nb, c = e - i * nb; if (c <= i) w.S[(size_t)(k0 + i) * ld + k0 + c] = A[i][c]; }
    if (tid == 0 && s_bad) *w.fail = 1;
}

// panel rows r in [k0 + nb, n] (the border row included), one per thread: Y_r = A_rk Lkk^-T (= L_rk D), L_rk = Y_r D^-1
__global__ __launch_bounds__(256) void panel_kernel(Sys w, int k0, int nb) {
    __shared__ double Lk[kNB][kNB + 1];
    const int tid = threadIdx.x;
    const size_t ld = w.ld;
    for (int e = tid; e < nb * nb; e += 256) { const int i = e / nb, c = e - i * nb; if (c <= i) Lk[i][c] = w.S[(size_t)(k0 + i) * ld + k0 + c]; }
    __syncthreads();
    const int r = k0 + nb + blockIdx.x * 256 + tid;
    const bool live = r <= w.n;
    double y[kNB];
    bool nz = false;
#pragma unroll
    for (int j = 0; j < kNB; j++) { y[j] = (live && j < nb) ? w.S[(size_t)r * ld + k0 + j] : 0.0; nz |= y[j] != 0.0; }
    const bool group = __any(nz) != 0;   // the wave's 64 rows: k0 + nb is a multiple of 64 whenever rows are left, so this is row group r / 64
    if ((tid & 63) == 0 && live) w.group_nz[r >> 6] = group ? 1 : 0;
    if (!live || !group) return;   // an empty group stays as it is: zeros in S, and nobody reads its Y
#pragma unroll
    for (int j = 0; j < kNB; j++) {
        if (j < nb) {
            double a = y[j];
#pragma unroll
            for (int t = 0; t < j; t++) a = fma(-y[t], Lk[j][t], a);
            y[j] = a;
        }
    }
#pragma unroll
    for (int j = 0; j < kNB; j++) {
        if (j < nb) { w.Y[(size_t)r * kNB + j] = y[j]; w.S[(size_t)r * ld + k0 + j] = y[j] / Lk[j][j]; }
    }
}

// trailing update A_rc -= sum_t L_rt Y_ct over 64 x 64 tiles with tile column <= tile row; rows and columns start at k1 = k0 + nb,
// the border row n is the last row and has no column.  256 threads, 4 x 4 outputs each, both operand tiles staged in LDS.
__global__ __launch_bounds__(256) void update_kernel(Sys w, int k0, int nb) {
    int tr = (int)((sqrt(8.0 * blockIdx.x + 1.0) - 1.0) * 0.5);
    while ((tr + 1) * (tr + 2) / 2 <= (int)blockIdx.x) ++tr;
    while (tr * (tr + 1) / 2 > (int)blockIdx.x) --tr;
    const int tc = blockIdx.x - tr * (tr + 1) / 2;
    const int k1 = k0 + nb, r0 = k1 + 64 * tr, c0 = k1 + 64 * tc;
    if (!w.group_nz[r0 >> 6] || !w.group_nz[c0 >> 6]) return;   // the tile's product is exactly zero
    __shared__ double Ls[64][kNB + 1], Ys[64][kNB + 1];
    const int tid = threadIdx.x;
    const size_t ld = w.ld;
    for (int e = tid; e < 64 * nb; e += 256) {
        const int i = e / nb, t = e - i * nb;
        const int r = r0 + i, c = c0 + i;
        Ls[i][t] = r <= w.n ? w.S[(size_t)r * ld + k0 + t] : 0.0;
        Ys[i][t] = c < w.n ? w.Y[(size_t)c * kNB + t] : 0.0;
    }
    __syncthreads();
    const int ti = (tid >> 4) * 4, tj = (tid & 15) * 4;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = 0;
    for (int t = 0; t < nb; t++) {
        double l[4], y[4];
#pragma unroll
        for (int a = 0; a < 4; a++) { l[a] = Ls[ti + a][t]; y[a] = Ys[tj + a][t]; }
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) acc[a][b] = fma(l[a], y[b], acc[a][b]);
    }
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int r = r0 + ti + a, c = c0 + tj + b;
            if (r <= w.n && c < w.n && c <= r) w.S[(size_t)r * ld + c] -= acc[a][b];
        }
}

// L^T x = z, one launch per panel from the last one upwards: every workgroup solves the panel's unit upper triangle for itself,
// workgroup 0 stores it in x, then each workgroup takes 256 earlier rows: z_r -= sum_c L[k0 + c][r] x_c
__global__ __launch_bounds__(256) void back_kernel(Sys w, int k0, int nb) {
    __shared__ double xs[kNB];
    __shared__ double Lk[kNB][kNB + 1];
    const int tid = threadIdx.x;
    const size_t ld = w.ld;
    for (int e = tid; e < nb * nb; e += 256) { const int i = e / nb, c = e - i * nb; if (c < i) Lk[i][c] = w.S[(size_t)(k0 + i) * ld + k0 + c]; }
    double* z = w.S + (size_t)w.n * ld;
    if (tid < nb) xs[tid] = z[k0 + tid];
    __syncthreads();
    if (tid < 64) {   // one wave: x_i = z_i - sum_{j > i} L_ji x_j, from the last row of the panel upwards
        double x = tid < nb ? xs[tid] : 0.0;
        for (int j = nb - 1; j > 0; j--) {
            const double xj = __shfl(x, j);
            if (tid < j) x = fma(-Lk[j][tid], xj, x);
        }
        if (tid < nb) xs[tid] = x;
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid < nb) w.x[k0 + tid] = xs[tid];
    const int r = blockIdx.x * 256 + tid;
    if (r < k0) {
        double a = z[r];
        for (int c = 0; c < nb; c++) a = fma(-w.S[(size_t)(k0 + c) * ld + r], xs[c], a);
        z[r] = a;
    }
}

// enqueue the factorisation of S and both substitutions on `st`
inline void factor_and_solve(const Sys& w, hipStream_t st) {
    const int n = w.n;
    for (int k0 = 0; k0 < n; k0 += kNB) {
        const int nb = n - k0 < kNB ? n - k0 : kNB, rows = n + 1 - (k0 + nb);   // rows behind the panel, border row included
        hipLaunchKernelGGL(diag_kernel, dim3(1), dim3(256), 0, st, w, k0, nb);
        hipLaunchKernelGGL(panel_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, w, k0, nb);
        const int ntile = (rows + 63) / 64;
        if (k0 + nb < n) hipLaunchKernelGGL(update_kernel, dim3(ntile * (ntile + 1) / 2), dim3(256), 0, st, w, k0, nb);
    }
    for (int k0 = ((n - 1) / kNB) * kNB; k0 >= 0; k0 -= kNB) {
        const int nb = n - k0 < kNB ? n - k0 : kNB;
        const int g = (k0 + 255) / 256;
        hipLaunchKernelGGL(back_kernel, dim3(g > 0 ? g : 1), dim3(256), 0, st, w, k0, nb);
    }
}

}  // namespace pgl
