// Loop-closure pose graph on the device: loopClosurePathOptimizationg2o (src/optimization/graphoptsim3.cpp:74-168), g2o's Levenberg over
// VertexSim3Expmap / EdgeSim3 (typesg2o.h:673-749) on the essential graph of all keyframes.  All of it is fp64.
//
//   set-up      float poses -> Sim3 (Eigen's matrix -> quaternion, sign rule, normalize), per-edge measurements Sjw * Siw^-1
//   linearise   one wave per edge, one error evaluation per lane: the current one and +- delta on the 7 + 7 coordinates (g2o's numeric
//               central differences, base_binary_edge.hpp:165-233), columns as scalar * (e+ - e-), then the edge's part of
//               constructQuadraticForm into a per-edge record
//   assemble    no atomics: per vertex / per vertex pair the incident records are summed in edge order into the lower triangle of a
//               dense system with a border row for b (dense_ldlt.hpp)
//   solve       blocked LDL^T, forward and back substitution (dense_ldlt.hpp)
//   update      trial estimates Sim3(x) * estimate (x[6] zeroed IN x when the scale is fixed, as oplusImpl does), then trial errors
//   decide      optimization_algorithm_levenberg.cpp:58-150 and the outer loop of sparse_optimizer.cpp:366-436 on the device; the host
//               reads the decision once per Levenberg trial to know what to enqueue next
//   results     [sR | t/s] rounded to float for EVERY vertex, and the Sim3 state
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <map>
#include "common.hpp"
#include "dense_ldlt.hpp"
#include "reduce.hpp"
#include "sim3.hpp"

namespace {

constexpr int kMaxIters = UH_POSEGRAPH_MAX_ITERS;
constexpr int kRec = 161;   // per-edge record: A'OA (49) | A'OB (49) | B'OB (49) | A'(-Oe) (7) | B'(-Oe) (7)

struct PGState {
    double lambda, ni, cur_chi, tmp_chi, rho, chi2_before;
    float prev_f, cur_f;
    int cur;      // which of the two estimate buffers is the current one
    int iter;     // outer iterations done
    int qmax;
    int started;  // Levenberg trials started in this iteration
    int next;     // 0: another trial, 1: another iteration, 2: done
    int pad;
    int trials[kMaxIters];
};

struct PG {
    int n, E, na, N;          // poses, edges, active free vertices, 7 * na
    int idx_new, idx_old, fix_scale, max_iters;
    double lambda_init, delta;
    const float* pose_in;     // n x 16, then expected_pose_new (16)
    double* est[2];           // n x 8
    double* meas;             // E x 8
    const int* edge_i; const int* edge_j; const double* edge_w;
    const int* slot;          // n: index in the system, -1 for the fixed vertex and for vertices without edges
    double* rec;              // E x kRec
    double* chi_cur; double* chi_trial;   // E
    double* dbg_err; double* dbg_J;       // E x 7, E x 98 (Ji | Jj)
    const int* v_ptr; const int* v_item;        // per system vertex: incident (edge * 2 + end) in edge order
    const int* pair_hi; const int* pair_lo; const int* pair_ptr; const int* pair_item;   // per vertex pair: (edge * 2 + transposed)
    double* b;                // N
    float* out_pose; double* out_state;
    PGState* st;
    pgl::Sys sys;
};

__global__ __launch_bounds__(256) void pg_setup_kernel(PG p) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < p.n) {
        double s[8];
        sim3::from_pose(p.pose_in + 16 * (size_t)(t == p.idx_new ? p.n : t), s);
#pragma unroll
        for (int k = 0; k < 8; k++) { p.est[0][8 * (size_t)t + k] = s[k]; p.est[1][8 * (size_t)t + k] = s[k]; }
    }
    if (t < p.E) {
        const int i = p.edge_i[t], j = p.edge_j[t];
        const bool closing = (i == p.idx_new && j == p.idx_old) || (j == p.idx_new && i == p.idx_old);
        double Siw[8], Sjw[8], Swi[8], Sji[8];
        sim3::from_pose(p.pose_in + 16 * (size_t)((closing && i == p.idx_new) ? p.n : i), Siw);
        sim3::from_pose(p.pose_in + 16 * (size_t)((closing && j == p.idx_new) ? p.n : j), Sjw);
        sim3::inverse(Siw, Swi);
        sim3::mul(Sjw, Swi, Sji);
#pragma unroll
        for (int k = 0; k < 8; k++) p.meas[8 * (size_t)t + k] = Sji[k];
    }
    if (t == 0) {
        PGState& st = *p.st;
        st.lambda = 0; st.ni = 2; st.cur_chi = 0; st.tmp_chi = 0; st.rho = 0; st.chi2_before = 0;
        st.prev_f = FLT_MAX; st.cur_f = FLT_MAX;
        st.cur = 0; st.iter = 0; st.qmax = 0; st.started = 0; st.next = 2; st.pad = 0;
        for (int k = 0; k < kMaxIters; k++) st.trials[k] = 0;
    }
}

// grid = E, one wave per edge
__global__ __launch_bounds__(64) void pg_lin_kernel(PG p, int dbg) {
    __shared__ double s_e[29][7];
    __shared__ double s_J[7][14];
    const int e = blockIdx.x, lane = threadIdx.x;
    const int cur = p.st->cur;
    const int i = p.edge_i[e], j = p.edge_j[e];
    const bool free_i = p.slot[i] >= 0, free_j = p.slot[j] >= 0;
    const double w = p.edge_w[e];
    if (lane < 29) {
        double si[8], sj[8], C[8];
#pragma unroll
        for (int k = 0; k < 8; k++) { si[k] = p.est[cur][8 * (size_t)i + k]; sj[k] = p.est[cur][8 * (size_t)j + k]; C[k] = p.meas[8 * (size_t)e + k]; }
        if (lane > 0) {
            const int c = (lane - 1) % 14, a = c % 7;
            const double step = lane <= 14 ? p.delta : -p.delta;
            double u[7], base[8], moved[8];
#pragma unroll
            for (int k = 0; k < 7; k++) u[k] = k == a ? step : 0.0;
#pragma unroll
            for (int k = 0; k < 8; k++) base[k] = c < 7 ? si[k] : sj[k];
            sim3::oplus(base, u, p.fix_scale != 0, moved);
#pragma unroll
            for (int k = 0; k < 8; k++) { if (c < 7) si[k] = moved[k]; else sj[k] = moved[k]; }
        }
        double err[7];
        sim3::edge_error(C, si, sj, err);
#pragma unroll
        for (int k = 0; k < 7; k++) s_e[lane][k] = err[k];
    }
    __syncthreads();
    const double scalar = 1 / (2 * p.delta);
    for (int q = lane; q < 98; q += 64) {
        const int k = q / 14, c = q - 14 * k;
        const bool fr = c < 7 ? free_i : free_j;
        s_J[k][c] = fr ? scalar * (s_e[1 + c][k] - s_e[15 + c][k]) : 0.0;
    }
    __syncthreads();
    if (dbg) {
        if (lane < 7) p.dbg_err[7 * (size_t)e + lane] = s_e[0][lane];
        for (int q = lane; q < 98; q += 64) {   // Ji (7 x 7 row-major) then Jj
            const int m = q / 49, r = (q - 49 * m) / 7, c = q - 49 * m - 7 * r;
            p.dbg_J[98 * (size_t)e + q] = s_J[r][7 * m + c];
        }
    }
    // constructQuadraticForm (base_binary_edge.hpp:83-122) with information w * I7: AtO = A' * Omega, omega_r = -Omega e
    double* rec = p.rec + (size_t)kRec * e;
    for (int q = lane; q < kRec; q += 64) {
        double v = 0;
        if (q < 147) {
            const int m = q / 49, a = (q - 49 * m) / 7, c = q - 49 * m - 7 * a;
            const int ca = m == 2 ? 7 + a : a, cc = m == 0 ? c : 7 + c;
#pragma unroll
            for (int k = 0; k < 7; k++) v += (s_J[k][ca] * w) * s_J[k][cc];
        } else {
            const int c = q - 147;
#pragma unroll
            for (int k = 0; k < 7; k++) v += s_J[k][c] * (-(w * s_e[0][k]));
        }
        rec[q] = v;
    }
    if (lane == 0) {
        double chi = 0;
#pragma unroll
        for (int k = 0; k < 7; k++) chi += s_e[0][k] * (w * s_e[0][k]);
        p.chi_cur[e] = chi;
    }
}

// grid = na, 64 threads: the diagonal block (lambda added) and b of one system vertex
__global__ __launch_bounds__(64) void pg_assemble_diag_kernel(PG p) {
    const int s = blockIdx.x, q = threadIdx.x;
    if (q >= 56) return;
    const double lambda = p.st->lambda;
    const size_t ld = p.sys.ld;
    double v = 0;
    if (q < 49) {
        const int a = q / 7, c = q - 7 * a;
        if (c > a) return;
        // g2o's solver reads the upper triangle of the block: entry (c, a) for the lower position (a, c)
        for (int it = p.v_ptr[s]; it < p.v_ptr[s + 1]; it++) {
            const int item = p.v_item[it];
            v += p.rec[(size_t)kRec * (item >> 1) + ((item & 1) ? 98 : 0) + 7 * c + a];
        }
        if (a == c) v += lambda;
        p.sys.S[(size_t)(7 * s + a) * ld + 7 * s + c] = v;
    } else {
        const int a = q - 49;
        for (int it = p.v_ptr[s]; it < p.v_ptr[s + 1]; it++) {
            const int item = p.v_item[it];
            v += p.rec[(size_t)kRec * (item >> 1) + 147 + ((item & 1) ? 7 : 0) + a];
        }
        p.b[7 * s + a] = v;
        p.sys.S[(size_t)p.N * ld + 7 * s + a] = v;
    }
}

// grid = pairs, 64 threads: the off-diagonal block of two system vertices joined by at least one edge
__global__ __launch_bounds__(64) void pg_assemble_pair_kernel(PG p) {
    const int pr = blockIdx.x, q = threadIdx.x;
    if (q >= 49) return;
    const int a = q / 7, c = q - 7 * a;
    double v = 0;
    for (int it = p.pair_ptr[pr]; it < p.pair_ptr[pr + 1]; it++) {
        const int item = p.pair_item[it];
        v += p.rec[(size_t)kRec * (item >> 1) + 49 + ((item & 1) ? 7 * c + a : 7 * a + c)];
    }
    p.sys.S[(size_t)(7 * p.pair_hi[pr] + a) * p.sys.ld + 7 * p.pair_lo[pr] + c] = v;
}

// one thread per pose: the trial estimate.  A failed factorisation leaves x = 0 (the trial is rejected whatever x holds).
__global__ __launch_bounds__(256) void pg_update_kernel(PG p) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= p.n) return;
    const int cur = p.st->cur, trial = cur ^ 1;
    const int s = p.slot[v];
    double a[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; k++) a[k] = p.est[cur][8 * (size_t)v + k];
    if (s >= 0) {
        double* x = p.sys.x + 7 * (size_t)s;
        if (*p.sys.fail) { for (int k = 0; k < 7; k++) x[k] = 0.0; }
        if (p.fix_scale) x[6] = 0.0;
        double u[7];
#pragma unroll
        for (int k = 0; k < 7; k++) u[k] = x[k];
        sim3::oplus(a, u, p.fix_scale != 0, o);
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) o[k] = a[k];
    }
#pragma unroll
    for (int k = 0; k < 8; k++) p.est[trial][8 * (size_t)v + k] = o[k];
}

// one thread per edge: chi2 at the trial estimates
__global__ __launch_bounds__(64) void pg_trial_chi_kernel(PG p) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= p.E) return;
    const int trial = p.st->cur ^ 1;
    const int i = p.edge_i[e], j = p.edge_j[e];
    const double w = p.edge_w[e];
    double si[8], sj[8], C[8], err[7];
#pragma unroll
    for (int k = 0; k < 8; k++) { si[k] = p.est[trial][8 * (size_t)i + k]; sj[k] = p.est[trial][8 * (size_t)j + k]; C[k] = p.meas[8 * (size_t)e + k]; }
    sim3::edge_error(C, si, sj, err);
    double chi = 0;
#pragma unroll
    for (int k = 0; k < 7; k++) chi += err[k] * (w * err[k]);
    p.chi_trial[e] = chi;
}

// fixed order: every thread adds its elements in index order, then the block sum of reduce.hpp
__device__ double ordered_sum(const double* v, int n, double* s_red) {
    double a = 0;
    for (int k = threadIdx.x; k < n; k += kRedThreads) a += v[k];
    return block_sum(a, s_red);
}

// one workgroup.  mode 0: an outer iteration begins behind its linearisation; mode 1: a Levenberg trial has been evaluated
__global__ __launch_bounds__(kRedThreads) void pg_decide_kernel(PG p, int mode) {
    __shared__ double s_red[kRedThreads / 64];
    PGState& st = *p.st;
    if (mode == 0) {
        const double chi = ordered_sum(p.chi_cur, p.E, s_red);
        if (threadIdx.x != 0) return;
        const float h = st.prev_f; st.prev_f = st.cur_f; st.cur_f = h;   // swap(prevChi2, curChi2)
        st.cur_chi = chi;
        if (st.iter == 0) { st.lambda = p.lambda_init; st.ni = 2; st.chi2_before = chi; }
        st.qmax = 0; st.started = 0; st.rho = 0;
        st.next = 0;
        return;
    }
    const double tmp_real = ordered_sum(p.chi_trial, p.E, s_red);
    const double lambda = st.lambda;
    double part = 0;
    for (int k = threadIdx.x; k < p.N; k += kRedThreads) { const double x = p.sys.x[k]; part += x * (lambda * x + p.b[k]); }
    double scale = block_sum(part, s_red);
    if (threadIdx.x != 0) return;
    const double tmp = *p.sys.fail ? DBL_MAX : tmp_real;
    st.tmp_chi = tmp_real;
    st.started++;
    double rho = st.cur_chi - tmp;
    scale += 1e-3;
    rho /= scale;
    bool brk = false;
    if (rho > 0 && isfinite(tmp)) {
        const double h = 2 * rho - 1;
        double alpha = 1. - (h * h) * h;
        alpha = fmin(alpha, 2. / 3.);
        const double f = fmax(1. / 3., alpha);
        st.lambda *= f;
        st.ni = 2;
        st.cur_chi = tmp;
        st.cur ^= 1;   // discardTop: the trial is the estimate
    } else {
        st.lambda *= st.ni;
        st.ni *= 2;
        if (!isfinite(st.lambda)) brk = true;
    }
    if (!brk) st.qmax++;
    st.rho = rho;
    if (!brk && rho < 0 && st.qmax < 10) { st.next = 0; return; }
    const bool terminate = st.qmax == 10 || rho == 0 || !isfinite(st.lambda);
    st.trials[st.iter] = st.started;
    st.cur_f = (float)tmp_real;   // the chi2 of the last evaluated trial, accepted or not
    const float diff = st.prev_f - st.cur_f;
    st.iter++;
    st.next = (st.iter < p.max_iters && !terminate && diff > 0.f) ? 1 : 2;
}

__global__ __launch_bounds__(256) void pg_results_kernel(PG p) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= p.n) return;
    const int cur = p.st->cur;
    double a[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { a[k] = p.est[cur][8 * (size_t)v + k]; p.out_state[8 * (size_t)v + k] = a[k]; }
    float M[16];
    sim3::to_pose(a, M);
#pragma unroll
    for (int k = 0; k < 16; k++) p.out_pose[16 * (size_t)v + k] = M[k];
}

}  // namespace

struct uh_posegraph {
    uh_ctx* ctx = nullptr;
    uh::DevBuf arena;
    uh::DevBuf dbg_arena;   // uh_posegraph_debug_solve
    bool have = false;
    int n = 0, E = 0;
    std::vector<float> poses;
    std::vector<double> state, dbg_err, dbg_J, meas;
    PGState fin{};
};

extern "C" {

int uh_posegraph_check_problem(const uh_posegraph_problem* pr, const uh_posegraph_params* pa) {
    UH_REQUIRE(pr, "uh_posegraph: NULL problem");
    UH_REQUIRE(pr->n_poses >= 1 && pr->pose_f2g && pr->expected_pose_new, "uh_posegraph: no poses or a NULL pose array");
    if (pr->n_poses > UH_POSEGRAPH_MAX_POSES) {
        uh::set_error("uh_posegraph: %d poses exceed the cap of %d (the dense system would not fit)", pr->n_poses, UH_POSEGRAPH_MAX_POSES);
        return UH_ECAPACITY;
    }
    UH_REQUIRE(pr->n_edges >= 0 && (pr->n_edges == 0 || (pr->edge_i && pr->edge_j)), "uh_posegraph: bad edge arrays");
    UH_REQUIRE(pr->idx_new >= 0 && pr->idx_new < pr->n_poses && pr->idx_old >= 0 && pr->idx_old < pr->n_poses, "uh_posegraph: idx_new / idx_old out of range");
    UH_REQUIRE(pr->idx_new != pr->idx_old, "uh_posegraph: idx_new == idx_old");
    for (int e = 0; e < pr->n_edges; e++) {
        const int i = pr->edge_i[e], j = pr->edge_j[e];
        UH_REQUIRE(i >= 0 && i < pr->n_poses && j >= 0 && j < pr->n_poses, "uh_posegraph: edge %d (%d, %d) out of range", e, i, j);
        UH_REQUIRE(i != j, "uh_posegraph: edge %d joins pose %d with itself", e, i);
        UH_REQUIRE(!pr->edge_weight || std::isfinite(pr->edge_weight[e]), "uh_posegraph: edge %d has a non-finite weight", e);
    }
    if (pa) {
        UH_REQUIRE(pa->max_iters >= 0 && pa->max_iters <= UH_POSEGRAPH_MAX_ITERS, "uh_posegraph: max_iters outside 0..%d", UH_POSEGRAPH_MAX_ITERS);
        UH_REQUIRE(pa->lambda_init >= 0 && std::isfinite(pa->lambda_init), "uh_posegraph: bad lambda_init");
        UH_REQUIRE(pa->fd_delta >= 0 && std::isfinite(pa->fd_delta), "uh_posegraph: bad fd_delta");
    }
    return UH_OK;
}

int uh_posegraph_create(uh_ctx* ctx, uh_posegraph** out) {
    UH_REQUIRE(ctx && out, "uh_posegraph_create: NULL argument");
    uh_posegraph* g = new uh_posegraph();
    g->ctx = ctx;
    *out = g;
    return UH_OK;
}

void uh_posegraph_destroy(uh_posegraph* g) { delete g; }

int uh_posegraph_optimize(uh_posegraph* g, const uh_posegraph_problem* pr, const uh_posegraph_params* pa) {
    UH_REQUIRE(g, "uh_posegraph_optimize: NULL handle");
    g->have = false;
    if (const int rc = uh_posegraph_check_problem(pr, pa)) return rc;
    const int n = pr->n_poses, E = pr->n_edges;
    hipStream_t st = g->ctx->stream;
    UH_HIP_CHECK(hipSetDevice(g->ctx->device));

    // the system's vertices: every free vertex that has an edge, in index order; incident records per vertex and per pair in edge order
    std::vector<int> slot(n, -1), deg(n, 0);
    for (int e = 0; e < E; e++) { deg[pr->edge_i[e]]++; deg[pr->edge_j[e]]++; }
    int na = 0;
    for (int v = 0; v < n; v++) if (deg[v] && v != pr->idx_old) slot[v] = na++;
    const int N = 7 * na;
    std::vector<int> v_ptr(na + 1, 0), v_item;
    std::vector<std::vector<int>> inc(na);
    std::map<std::pair<int, int>, std::vector<int>> pairs;
    for (int e = 0; e < E; e++) {
        const int si = slot[pr->edge_i[e]], sj = slot[pr->edge_j[e]];
        if (si >= 0) inc[si].push_back(2 * e);
        if (sj >= 0) inc[sj].push_back(2 * e + 1);
        if (si >= 0 && sj >= 0) pairs[{std::max(si, sj), std::min(si, sj)}].push_back(2 * e + (si < sj ? 1 : 0));   // row block si, column block sj: transposed into the lower triangle when si < sj
    }
    for (int s = 0; s < na; s++) { v_ptr[s + 1] = v_ptr[s] + (int)inc[s].size(); v_item.insert(v_item.end(), inc[s].begin(), inc[s].end()); }
    std::vector<int> pair_hi, pair_lo, pair_ptr(1, 0), pair_item;
    for (const auto& kv : pairs) {
        pair_hi.push_back(kv.first.first); pair_lo.push_back(kv.first.second);
        pair_item.insert(pair_item.end(), kv.second.begin(), kv.second.end());
        pair_ptr.push_back((int)pair_item.size());
    }
    const int np = (int)pair_hi.size();
    std::vector<double> w(E);
    for (int e = 0; e < E; e++) w[e] = pr->edge_weight ? (double)pr->edge_weight[e] : 1.0;

    // one arena, carved front to back
    uh::Layout L;
    const size_t o_pose = L.take<float>(16 * ((size_t)n + 1)), o_est0 = L.take<double>(8 * (size_t)n), o_est1 = L.take<double>(8 * (size_t)n);
    const size_t o_meas = L.take<double>(8 * (size_t)E), o_ei = L.take<int>(E), o_ej = L.take<int>(E), o_ew = L.take<double>(E), o_slot = L.take<int>(n);
    const size_t o_rec = L.take<double>((size_t)kRec * E), o_cc = L.take<double>(E), o_ct = L.take<double>(E);
    const size_t o_de = L.take<double>(7 * (size_t)E), o_dj = L.take<double>(98 * (size_t)E);
    const size_t o_vp = L.take<int>(na + 1), o_vi = L.take<int>(v_item.size()), o_ph = L.take<int>(np), o_pl = L.take<int>(np), o_pp = L.take<int>(np + 1), o_pi = L.take<int>(pair_item.size());
    const size_t o_b = L.take<double>(N), o_x = L.take<double>(N), o_fail = L.take<int>(1), o_st = L.take<PGState>(1), o_gz = L.take<int>((N + 64) / 64 + 1);
    const size_t o_op = L.take<float>(16 * (size_t)n), o_os = L.take<double>(8 * (size_t)n);
    const size_t ld = (size_t)N + 1;
    const size_t o_Y = L.take<double>(ld * pgl::kNB), o_S = L.take<double>(ld * ld);
    if (const int rc = g->arena.reserve(L.off + 256)) return rc;
    char* base = g->arena.as<char>();

    PG p{};
    p.n = n; p.E = E; p.na = na; p.N = N;
    p.idx_new = pr->idx_new; p.idx_old = pr->idx_old; p.fix_scale = pr->fix_scale ? 1 : 0;
    p.max_iters = (pa && pa->max_iters) ? pa->max_iters : 20;
    p.lambda_init = (pa && pa->lambda_init > 0) ? pa->lambda_init : 1e-16;
    p.delta = (double)((pa && pa->fd_delta > 0) ? pa->fd_delta : 1e-9f);   // g2o: cst(_delta_der), a float member widened
    p.pose_in = (const float*)(base + o_pose);
    p.est[0] = (double*)(base + o_est0); p.est[1] = (double*)(base + o_est1);
    p.meas = (double*)(base + o_meas);
    p.edge_i = (const int*)(base + o_ei); p.edge_j = (const int*)(base + o_ej); p.edge_w = (const double*)(base + o_ew);
    p.slot = (const int*)(base + o_slot);
    p.rec = (double*)(base + o_rec); p.chi_cur = (double*)(base + o_cc); p.chi_trial = (double*)(base + o_ct);
    p.dbg_err = (double*)(base + o_de); p.dbg_J = (double*)(base + o_dj);
    p.v_ptr = (const int*)(base + o_vp); p.v_item = (const int*)(base + o_vi);
    p.pair_hi = (const int*)(base + o_ph); p.pair_lo = (const int*)(base + o_pl); p.pair_ptr = (const int*)(base + o_pp); p.pair_item = (const int*)(base + o_pi);
    p.b = (double*)(base + o_b);
    p.out_pose = (float*)(base + o_op); p.out_state = (double*)(base + o_os);
    p.st = (PGState*)(base + o_st);
    p.sys.S = (double*)(base + o_S); p.sys.Y = (double*)(base + o_Y); p.sys.x = (double*)(base + o_x); p.sys.fail = (int*)(base + o_fail); p.sys.group_nz = (int*)(base + o_gz);
    p.sys.n = N; p.sys.ld = ld;

#define PG_UP(off, ptr, bytes) do { if ((bytes) > 0) UH_HIP_CHECK(hipMemcpyAsync(base + (off), (ptr), (bytes), hipMemcpyHostToDevice, st)); } while (0)
    PG_UP(o_pose, pr->pose_f2g, 64 * (size_t)n);
    PG_UP(o_pose + 64 * (size_t)n, pr->expected_pose_new, 64);
    PG_UP(o_ei, pr->edge_i, 4 * (size_t)E); PG_UP(o_ej, pr->edge_j, 4 * (size_t)E); PG_UP(o_ew, w.data(), 8 * (size_t)E);
    PG_UP(o_slot, slot.data(), 4 * (size_t)n);
    PG_UP(o_vp, v_ptr.data(), 4 * (size_t)(na + 1)); PG_UP(o_vi, v_item.data(), 4 * v_item.size());
    PG_UP(o_ph, pair_hi.data(), 4 * (size_t)np); PG_UP(o_pl, pair_lo.data(), 4 * (size_t)np);
    PG_UP(o_pp, pair_ptr.data(), 4 * (size_t)(np + 1)); PG_UP(o_pi, pair_item.data(), 4 * pair_item.size());
#undef PG_UP
    UH_HIP_CHECK(hipStreamSynchronize(st));   // the host vectors above end with this call

    UH_LAUNCH(g->ctx, pg_setup_kernel, dim3(uh_div_up(std::max(n, E), 256)), dim3(256), 0, p);
    PGState hs{};
    hs.next = 2;
    if (na > 0 && p.max_iters > 0) {
        bool first = true;
        for (;;) {
            UH_LAUNCH(g->ctx, pg_lin_kernel, dim3(E), dim3(64), 0, p, first ? 1 : 0);
            UH_LAUNCH(g->ctx, pg_decide_kernel, dim3(1), dim3(kRedThreads), 0, p, 0);
            first = false;
            do {
                UH_HIP_CHECK(hipMemsetAsync(p.sys.S, 0, ld * ld * sizeof(double), st));
                UH_HIP_CHECK(hipMemsetAsync(p.sys.fail, 0, sizeof(int), st));
                UH_LAUNCH(g->ctx, pg_assemble_diag_kernel, dim3(na), dim3(64), 0, p);
                if (np) UH_LAUNCH(g->ctx, pg_assemble_pair_kernel, dim3(np), dim3(64), 0, p);
                {
                    uh::ProfScope ps(g->ctx, "pg_ldlt");
                    pgl::factor_and_solve(p.sys, st);
                }
                UH_LAUNCH(g->ctx, pg_update_kernel, dim3(uh_div_up(n, 256)), dim3(256), 0, p);
                UH_LAUNCH(g->ctx, pg_trial_chi_kernel, dim3(uh_div_up(E, 64)), dim3(64), 0, p);
                UH_LAUNCH(g->ctx, pg_decide_kernel, dim3(1), dim3(kRedThreads), 0, p, 1);
                UH_HIP_CHECK(hipMemcpyAsync(&hs, p.st, sizeof(PGState), hipMemcpyDeviceToHost, st));
                UH_HIP_CHECK(hipStreamSynchronize(st));
            } while (hs.next == 0);
            if (hs.next != 1) break;
        }
    }
    UH_LAUNCH(g->ctx, pg_results_kernel, dim3(uh_div_up(n, 256)), dim3(256), 0, p);
    g->poses.resize(16 * (size_t)n); g->state.resize(8 * (size_t)n);
    g->dbg_err.assign(7 * (size_t)E, 0.0); g->dbg_J.assign(98 * (size_t)E, 0.0); g->meas.resize(8 * (size_t)E);
    UH_HIP_CHECK(hipMemcpyAsync(g->poses.data(), p.out_pose, 64 * (size_t)n, hipMemcpyDeviceToHost, st));
    UH_HIP_CHECK(hipMemcpyAsync(g->state.data(), p.out_state, 64 * (size_t)n, hipMemcpyDeviceToHost, st));
    UH_HIP_CHECK(hipMemcpyAsync(&g->fin, p.st, sizeof(PGState), hipMemcpyDeviceToHost, st));
    if (E > 0) {
        UH_HIP_CHECK(hipMemcpyAsync(g->meas.data(), p.meas, 64 * (size_t)E, hipMemcpyDeviceToHost, st));
        if (na > 0 && p.max_iters > 0) {
            UH_HIP_CHECK(hipMemcpyAsync(g->dbg_err.data(), p.dbg_err, 56 * (size_t)E, hipMemcpyDeviceToHost, st));
            UH_HIP_CHECK(hipMemcpyAsync(g->dbg_J.data(), p.dbg_J, 784 * (size_t)E, hipMemcpyDeviceToHost, st));
        }
    }
    UH_HIP_CHECK(hipStreamSynchronize(st));
    UH_HIP_CHECK(hipGetLastError());
    g->n = n; g->E = E;
    g->have = true;
    return UH_OK;
}

int uh_posegraph_get_results(uh_posegraph* g, float* poses_out, double* state_out, uh_posegraph_info* info, int32_t* trials_out) {
    UH_REQUIRE(g && g->have, "uh_posegraph_get_results: no optimisation has run");
    if (poses_out) std::memcpy(poses_out, g->poses.data(), g->poses.size() * sizeof(float));
    if (state_out) std::memcpy(state_out, g->state.data(), g->state.size() * sizeof(double));
    if (info) {
        info->iterations = g->fin.iter;
        info->lambda = g->fin.lambda;
        info->chi2_before = g->fin.chi2_before;
        info->chi2_after = g->fin.cur_chi;
    }
    if (trials_out) for (int k = 0; k < g->fin.iter; k++) trials_out[k] = g->fin.trials[k];
    return UH_OK;
}

int uh_posegraph_debug_linearisation(uh_posegraph* g, double* err_out, double* Ji_out, double* Jj_out, double* meas_out) {
    UH_REQUIRE(g && g->have, "uh_posegraph_debug_linearisation: no optimisation has run");
    for (int e = 0; e < g->E; e++) {
        if (err_out) std::memcpy(err_out + 7 * (size_t)e, g->dbg_err.data() + 7 * (size_t)e, 56);
        if (Ji_out) std::memcpy(Ji_out + 49 * (size_t)e, g->dbg_J.data() + 98 * (size_t)e, 392);
        if (Jj_out) std::memcpy(Jj_out + 49 * (size_t)e, g->dbg_J.data() + 98 * (size_t)e + 49, 392);
        if (meas_out) std::memcpy(meas_out + 8 * (size_t)e, g->meas.data() + 8 * (size_t)e, 64);
    }
    return UH_OK;
}

// test hook: pgl::factor_and_solve on a system the caller gives, laid out and cleared as uh_posegraph_optimize does it
int uh_posegraph_debug_solve(uh_posegraph* g, int n, const double* S, const double* bv, double* x, double* LD, int* failed) {
    UH_REQUIRE(g && S && bv && x && failed, "uh_posegraph_debug_solve: NULL argument");
    UH_REQUIRE(n >= 1 && n <= 4096, "uh_posegraph_debug_solve: n = %d outside 1..4096", n);
    UH_HIP_CHECK(hipSetDevice(g->ctx->device));
    hipStream_t st = g->ctx->stream;
    const size_t ld = (size_t)n + 1;
    std::vector<double> A(ld * ld, 0.0);   // (the optimiser clears S before every assembly)
    for (int r = 0; r < n; r++) for (int c = 0; c <= r; c++) A[r * ld + c] = S[(size_t)r * n + c];
    for (int c = 0; c < n; c++) A[n * ld + c] = bv[c];
    uh::Layout L;
    const size_t o_x = L.take<double>(n), o_fail = L.take<int>(1), o_gz = L.take<int>((n + 64) / 64 + 1), o_Y = L.take<double>(ld * pgl::kNB), o_S = L.take<double>(ld * ld);
    if (const int rc = g->dbg_arena.reserve(L.off + 256)) return rc;
    char* base = g->dbg_arena.as<char>();
    pgl::Sys w{};
    w.S = (double*)(base + o_S); w.Y = (double*)(base + o_Y); w.x = (double*)(base + o_x); w.fail = (int*)(base + o_fail); w.group_nz = (int*)(base + o_gz);
    w.n = n; w.ld = ld;
    UH_HIP_CHECK(hipMemcpyAsync(w.S, A.data(), ld * ld * sizeof(double), hipMemcpyHostToDevice, st));
    UH_HIP_CHECK(hipMemsetAsync(w.x, 0xFF, (size_t)n * sizeof(double), st));   // (NaN: an x the solve did not write shows)
    UH_HIP_CHECK(hipMemsetAsync(w.fail, 0, sizeof(int), st));
    pgl::factor_and_solve(w, st);
    UH_HIP_CHECK(hipGetLastError());
    int hfail = 0;
    UH_HIP_CHECK(hipMemcpyAsync(x, w.x, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    UH_HIP_CHECK(hipMemcpyAsync(&hfail, w.fail, sizeof(int), hipMemcpyDeviceToHost, st));
    if (LD) UH_HIP_CHECK(hipMemcpyAsync(LD, w.S, ld * ld * sizeof(double), hipMemcpyDeviceToHost, st));
    UH_HIP_CHECK(hipStreamSynchronize(st));
    *failed = hfail ? 1 : 0;
    return UH_OK;
}

}  // extern "C"
