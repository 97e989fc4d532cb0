// TEST INFRASTRUCTURE ONLY — the loop-closure pose graph (src/optimization/graphoptsim3.cpp:74-168) on the REAL reference g2o (the core
// objects that `make -C oracle ref` leaves in oracle/_ref/obj/; built by tests/golden/make_posegraph_golden.py into oracle/_ref/, never
// into git).
//
// The reference's own graph types (src/optimization/typesg2o.h:673-749) cannot be compiled without OpenCV, so this driver restates the two
// it needs on g2o's base classes: the Sim3 vertex (oplus: update[6] zeroed IN THE CALLER'S BUFFER when the scale is fixed, then
// Sim3(update) * estimate) and the seven-row edge (error = log(C * Si * Sj^-1)), which has no linearizeOplus of its own, so g2o's numeric
// central differences run on both vertices (base_binary_edge.hpp:165-233) with _delta_der, a float member, at g2o's 1e-9 unless the
// caller sets another one.  The graph is graphoptsim3.cpp's: one vertex per pose from the float 4x4 (the new keyframe from the expected
// pose, the old one fixed), one edge per pair with measurement Sjw * Siw^-1 from the input poses (the closing edge with the expected
// pose), information weight * I7, Levenberg with lambda_init 1e-16 on BlockSolver_7_3 + LinearSolverEigen.  Sim3, its exp and log, the
// numeric Jacobian, the Levenberg loop and the solver are g2o's own code.
//
// delta_der (test only): 0 = g2o's own step, else the value _delta_der is set to.  jitter (test only): 0 = off; 1..8 multiply the
// measurements' translations by 1 +- 1e-12 per axis, bit 0 / 1 / 2 of (jitter - 1) choosing the sign for x / y / z — what the numeric
// Jacobian at step 1e-9 makes of such a change shows how far the reference pins itself.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "g2o/core/base_binary_edge.h"
#include "g2o/core/base_vertex.h"
#include "g2o/core/block_solver.h"
#include "g2o/core/batch_stats.h"
#include "g2o/core/optimization_algorithm_levenberg.h"
#include "g2o/core/sparse_optimizer.h"
#include "g2o/solvers/eigen/linear_solver_eigen.h"
#include "g2o/types/slam3d/se3quat.h"
#include "g2o/types/sim3/sim3.h"

namespace {

class SimVertex : public g2o::BaseVertex<7, g2o::Sim3> {   // VertexSim3Expmap
   public:
    EIGEN_MAKE_ALIGNED_OPERATOR_NEW
    bool fix_scale = false;
    bool read(std::istream&) override { return false; }
    bool write(std::ostream&) const override { return false; }
    void setToOriginImpl() override { _estimate = g2o::Sim3(); }
    void oplusImpl(const number_t* u) override {
        number_t* x = const_cast<number_t*>(u);   // the zero is written THROUGH the const pointer: the solver's own vector sees it
        if (fix_scale) x[6] = 0;
        g2o::Vector7 step;
        for (int k = 0; k < 7; k++) step[k] = x[k];
        setEstimate(g2o::Sim3(step) * estimate());
    }
};

class SimEdge : public g2o::BaseBinaryEdge<7, g2o::Sim3, SimVertex, SimVertex> {   // EdgeSim3
   public:
    EIGEN_MAKE_ALIGNED_OPERATOR_NEW
    bool read(std::istream&) override { return false; }
    bool write(std::ostream&) const override { return false; }
    void set_delta_der(float d) { _delta_der = d; }
    void computeError() override {
        const g2o::Sim3& a = static_cast<const SimVertex*>(_vertices[0])->estimate();
        const g2o::Sim3& b = static_cast<const SimVertex*>(_vertices[1])->estimate();
        _error = (_measurement * a * b.inverse()).log();
    }
};

g2o::Sim3 get_sim3(const float* M) {   // getSim3(T, 1)
    Eigen::Matrix<double, 3, 3> R;
    R << M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10];
    Eigen::Matrix<double, 3, 1> t;
    t << M[3], M[7], M[11];
    return g2o::Sim3(R, t, 1);
}

void put_state(const g2o::Sim3& S, double* o) {
    o[0] = S.rotation().x(); o[1] = S.rotation().y(); o[2] = S.rotation().z(); o[3] = S.rotation().w();
    o[4] = S.translation()[0]; o[5] = S.translation()[1]; o[6] = S.translation()[2];
    o[7] = S.scale();
}

}  // namespace

struct posegraph_ref_in {
    int32_t n, E, idx_new, idx_old, fix_scale, max_iters, jitter;
    float delta_der;
    const float* poses; const int32_t* edge_i; const int32_t* edge_j; const float* edge_w; const float* expected;
};
struct posegraph_ref_out {
    float* poses;       // n x 16
    double* state;      // n x 8
    int32_t* iters;     // 1
    int32_t* trials;    // max_iters
    double* info;       // lambda, chi2 before, chi2 after
    double* lin_err;    // E x 7
    double* lin_Ji;     // E x 49 row-major, zero where vertex 0 is fixed
    double* lin_Jj;     // E x 49
    double* meas;       // E x 8
    double* seconds;    // 1: optimize() alone
};

extern "C" int posegraph_ref_optimize(const posegraph_ref_in* in, posegraph_ref_out* out) {
    const int n = in->n, E = in->E;
    g2o::SparseOptimizer opt;
    auto linearSolver = g2o::make_unique<g2o::LinearSolverEigen<g2o::BlockSolver_7_3::PoseMatrixType>>();
    auto* solver = new g2o::OptimizationAlgorithmLevenberg(g2o::make_unique<g2o::BlockSolver_7_3>(std::move(linearSolver)));
    opt.setAlgorithm(solver);
    solver->setUserLambdaInit(1e-16);
    opt.setVerbose(false);
    opt.setComputeBatchStatistics(true);   // for the count of Levenberg trials only
    std::vector<SimVertex*> vs(n);
    for (int k = 0; k < n; k++) {
        auto* v = new SimVertex();
        v->setEstimate(get_sim3(k == in->idx_new ? in->expected : in->poses + 16 * k));
        v->setFixed(k == in->idx_old);
        v->setId(k);
        v->setMarginalized(false);
        v->fix_scale = in->fix_scale != 0;
        opt.addVertex(v);
        vs[k] = v;
    }
    std::vector<SimEdge*> es(E);
    for (int e = 0; e < E; e++) {
        const int i = in->edge_i[e], j = in->edge_j[e];
        const bool closing = (i == in->idx_new && j == in->idx_old) || (j == in->idx_new && i == in->idx_old);
        // both ends from the INPUT poses; only on the closing edge does the new keyframe stand where the detector expects it
        const g2o::Sim3 first = get_sim3((closing && i == in->idx_new) ? in->expected : in->poses + 16 * i);
        const g2o::Sim3 second = get_sim3((closing && j == in->idx_new) ? in->expected : in->poses + 16 * j);
        g2o::Sim3 rel = second * first.inverse();
        if (in->jitter > 0) {
            const int s = in->jitter - 1;
            for (int a = 0; a < 3; a++) rel.translation()[a] *= 1 + (((s >> a) & 1) ? -1e-12 : 1e-12);
        }
        auto* ed = new SimEdge();
        if (in->delta_der > 0) ed->set_delta_der(in->delta_der);
        ed->setVertex(0, vs[i]);
        ed->setVertex(1, vs[j]);
        ed->setMeasurement(rel);
        const float weight = in->edge_w ? in->edge_w[e] : 1.f;   // a float times the identity, as the reference forms it
        ed->information() = weight * Eigen::Matrix<double, 7, 7>::Identity();
        opt.addEdge(ed);
        es[e] = ed;
    }
    for (int k = 0; k < in->max_iters; k++) out->trials[k] = 0;
    out->info[0] = out->info[1] = out->info[2] = 0;
    out->iters[0] = 0;
    out->seconds[0] = 0;
    if (E > 0) {
        opt.initializeOptimization();
        opt.computeActiveErrors();
        out->info[1] = opt.activeChi2();
        for (int e = 0; e < E; e++) {   // the first linearisation, read off the edges (the Jacobian workspace is shared, so each edge is read at once)
            es[e]->linearizeOplus(opt.jacobianWorkspace());
            put_state(es[e]->measurement(), out->meas + 8 * e);
            for (int r = 0; r < 7; r++) {
                out->lin_err[7 * e + r] = es[e]->error()(r);
                for (int c = 0; c < 7; c++) {
                    out->lin_Ji[49 * e + 7 * r + c] = vs[in->edge_i[e]]->fixed() ? 0.0 : es[e]->jacobianOplusXi()(r, c);
                    out->lin_Jj[49 * e + 7 * r + c] = vs[in->edge_j[e]]->fixed() ? 0.0 : es[e]->jacobianOplusXj()(r, c);
                }
            }
        }
        const double t0 = g2o::get_monotonic_time();
        const int it = opt.optimize(in->max_iters);
        out->seconds[0] = g2o::get_monotonic_time() - t0;
        out->iters[0] = it;
        for (int k = 0; k < it && k < (int)opt.batchStatistics().size(); k++) out->trials[k] = opt.batchStatistics()[k].levenbergIterations;
        out->info[0] = solver->currentLambda();
        opt.computeActiveErrors();
        out->info[2] = opt.activeChi2();
    }
    for (int k = 0; k < n; k++) {
        const g2o::Sim3 S = vs[k]->estimate();
        put_state(S, out->state + 8 * k);
        Eigen::Matrix3d eigR = S.rotation().toRotationMatrix();
        Eigen::Vector3d eigt = S.translation();
        const double s = S.scale();
        eigt *= (1. / s);
        eigR *= s;
        float* M = out->poses + 16 * k;
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) M[4 * r + c] = eigR(r, c);
            M[4 * r + 3] = eigt(r);
        }
        M[12] = M[13] = M[14] = 0.f; M[15] = 1.f;
    }
    return 0;
}
