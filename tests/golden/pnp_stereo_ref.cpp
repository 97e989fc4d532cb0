// TEST INFRASTRUCTURE ONLY — the pose-only PnP with stereo / RGB-D observations, on the REAL reference g2o (the core objects that
// `make -C oracle ref` leaves in oracle/_ref/obj/; built by tests/golden/make_pnp_stereo_golden.py into oracle/_ref/, never into git).
//
// The reference's own graph types (src/optimization/typesg2o.h) cannot be compiled without OpenCV, so this driver restates the two
// pose-only edges on g2o's BaseUnaryEdge with the expressions of typesg2o.h:521-650 (the stereo edge's cam_project rounds 1/z to float,
// its Jacobian uses the double 1/z) and runs the loop of PnPSolver::solvePnp (pnpsolver.cpp:116-409, no markers): edges built per match
// by depth (:205-276: kp_ur = x - mbf / depth in float, robust weight doubled, Huber sqrt(7.815)), four rounds of optimize(10) from the
// input pose, relabelling against each edge's own MaxChi (5.99 / 7.815), robust kernels dropped from the third round, early stop below
// 10 inliers.  The solver stack (Levenberg, block solver, Eigen LDLT, SE3 exp, robustification) is g2o's own code.
//
// Two entry points on the one graph: pnp_stereo_ref_solve (tests/golden/pnp_stereo_golden.npz) and pnp_hard_ref_solve
// (tests/golden/pnp_hard_golden.npz), which also reports the Levenberg trials of every iteration and can jitter the map points.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "g2o/core/base_unary_edge.h"
#include "g2o/core/base_vertex.h"
#include "g2o/core/batch_stats.h"
#include "g2o/core/block_solver.h"
#include "g2o/core/hyper_graph_action.h"
#include "g2o/core/optimization_algorithm_levenberg.h"
#include "g2o/core/robust_kernel.h"
#include "g2o/core/sparse_optimizer.h"
#include "g2o/solvers/eigen/linear_solver_eigen.h"
#include "g2o/types/slam3d/se3quat.h"

namespace {

class PoseVertex : public g2o::BaseVertex<6, g2o::SE3Quat> {   // VertexSE3Expmap: exp(update) * estimate
   public:
    EIGEN_MAKE_ALIGNED_OPERATOR_NEW
    bool read(std::istream&) override { return false; }
    bool write(std::ostream&) const override { return false; }
    void setToOriginImpl() override { _estimate = g2o::SE3Quat(); }
    void oplusImpl(const number_t* u) override {
        Eigen::Map<const g2o::Vector6> d(u);
        setEstimate(g2o::SE3Quat::exp(d) * estimate());
    }
};

class MonoEdge : public g2o::BaseUnaryEdge<2, Eigen::Vector2d, PoseVertex> {   // EdgeSE3ProjectXYZOnlyPose
   public:
    EIGEN_MAKE_ALIGNED_OPERATOR_NEW
    Eigen::Vector3d Xw;
    double fx = 1, fy = 1, cx = 0, cy = 0;
    bool read(std::istream&) override { return false; }
    bool write(std::ostream&) const override { return false; }
    void computeError() override {
        const Eigen::Vector3d c = static_cast<const PoseVertex*>(_vertices[0])->estimate().map(Xw);
        Eigen::Vector2d res;
        res[0] = (c[0] / c[2]) * fx + cx;
        res[1] = (c[1] / c[2]) * fy + cy;
        _error = _measurement - res;
    }
    void linearizeOplus() override {
        const Eigen::Vector3d c = static_cast<const PoseVertex*>(_vertices[0])->estimate().map(Xw);
        const double x = c[0], y = c[1], invz = 1.0 / c[2], invz_2 = invz * invz;
        _jacobianOplusXi(0, 0) = x * y * invz_2 * fx;
        _jacobianOplusXi(0, 1) = -(1 + (x * x * invz_2)) * fx;
        _jacobianOplusXi(0, 2) = y * invz * fx;
        _jacobianOplusXi(0, 3) = -invz * fx;
        _jacobianOplusXi(0, 4) = 0;
        _jacobianOplusXi(0, 5) = x * invz_2 * fx;
        _jacobianOplusXi(1, 0) = (1 + y * y * invz_2) * fy;
        _jacobianOplusXi(1, 1) = -x * y * invz_2 * fy;
        _jacobianOplusXi(1, 2) = -x * invz * fy;
        _jacobianOplusXi(1, 3) = 0;
        _jacobianOplusXi(1, 4) = -invz * fy;
        _jacobianOplusXi(1, 5) = y * invz_2 * fy;
    }
};

class StereoEdge : public g2o::BaseUnaryEdge<3, Eigen::Vector3d, PoseVertex> {   // EdgeStereoSE3ProjectXYZOnlyPose
   public:
    EIGEN_MAKE_ALIGNED_OPERATOR_NEW
    Eigen::Vector3d Xw;
    double fx = 1, fy = 1, cx = 0, cy = 0, bf = 0;
    bool read(std::istream&) override { return false; }
    bool write(std::ostream&) const override { return false; }
    Eigen::Vector3d cam_project(const Eigen::Vector3d& t) const {
        const float invz = 1.0f / t[2];   // a double division rounded to float
        Eigen::Vector3d res;
        res[0] = t[0] * invz * fx + cx;
        res[1] = t[1] * invz * fy + cy;
        res[2] = res[0] - bf * invz;
        return res;
    }
    void computeError() override {
        const Eigen::Vector3d obs(_measurement);
        _error = obs - cam_project(static_cast<const PoseVertex*>(_vertices[0])->estimate().map(Xw));
    }
    void linearizeOplus() override {
        const Eigen::Vector3d c = static_cast<const PoseVertex*>(_vertices[0])->estimate().map(Xw);
        const double x = c[0], y = c[1], invz = 1.0 / c[2], invz_2 = invz * invz;
        _jacobianOplusXi(0, 0) = x * y * invz_2 * fx;
        _jacobianOplusXi(0, 1) = -(1 + (x * x * invz_2)) * fx;
        _jacobianOplusXi(0, 2) = y * invz * fx;
        _jacobianOplusXi(0, 3) = -invz * fx;
        _jacobianOplusXi(0, 4) = 0;
        _jacobianOplusXi(0, 5) = x * invz_2 * fx;
        _jacobianOplusXi(1, 0) = (1 + y * y * invz_2) * fy;
        _jacobianOplusXi(1, 1) = -x * y * invz_2 * fy;
        _jacobianOplusXi(1, 2) = -x * invz * fy;
        _jacobianOplusXi(1, 3) = 0;
        _jacobianOplusXi(1, 4) = -invz * fy;
        _jacobianOplusXi(1, 5) = y * invz_2 * fy;
        _jacobianOplusXi(2, 0) = _jacobianOplusXi(0, 0) - bf * y * invz_2;
        _jacobianOplusXi(2, 1) = _jacobianOplusXi(0, 1) + bf * x * invz_2;
        _jacobianOplusXi(2, 2) = _jacobianOplusXi(0, 2);
        _jacobianOplusXi(2, 3) = _jacobianOplusXi(0, 3);
        _jacobianOplusXi(2, 4) = 0;
        _jacobianOplusXi(2, 5) = _jacobianOplusXi(0, 5) - bf * invz_2;
    }
};

class WeightedHuber : public g2o::RobustKernel {   // WeightedHubberRobustKernel: the weight scales rho only
   public:
    double W = 1, D = 1;
    void robustify(double e2, g2o::Vector3& rho) const override {
        const double dsqr = D * D;
        if (e2 <= dsqr) { rho[0] = W * e2; rho[1] = 1.; rho[2] = 0.; }
        else { const double sq = std::sqrt(e2); rho[0] = W * (2 * sq * D - dsqr); rho[1] = D / sq; rho[2] = -0.5 * rho[1] / e2; }
    }
};

// The Levenberg trials of every iteration, as g2o counts them itself (G2OBatchStatistics::levenbergIterations, incremented by
// OptimizationAlgorithmLevenberg::solve at the head of every trial through G2OBatchStatistics::globalStats()).  The optimiser's own
// setComputeBatchStatistics(true) would also recompute the active errors after every iteration, at the pose Levenberg RESTORED after a
// rejected last trial — the solver under test relabels with the errors of the last trial g2o evaluated (pnpsolver.cpp:358-371 reads
// e->chi2()), so that switch changes the outcome.  This action only points the global statistics at the iteration's own record.
class TrialCounter : public g2o::HyperGraphAction {
   public:
    g2o::G2OBatchStatistics stat[10];
    void reset() { for (auto& s : stat) s = g2o::G2OBatchStatistics(); g2o::G2OBatchStatistics::setGlobalStats(0); }
    g2o::HyperGraphAction* operator()(const g2o::HyperGraph*, Parameters* p = 0) override {
        auto* it = dynamic_cast<ParametersIteration*>(p);
        if (it && it->iteration >= 0 && it->iteration < 10) g2o::G2OBatchStatistics::setGlobalStats(&stat[it->iteration]);
        return this;
    }
};

// jitter > 0: a seeded relative perturbation of the map points in the graph's doubles, |rel| <= 1e-12 (the screen of
// tests/golden/make_pnp_hard_golden.py: a case whose outcome hangs on rounding noise cannot pin a solver)
struct Jitter {
    uint64_t s;
    explicit Jitter(int seed) : s(0x9E3779B97F4A7C15ull * (uint64_t)(seed + 1)) {}
    double next() {   // splitmix64 -> [-1, 1)
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
    }
};

// trials_out: NULL, or 4 x 10 ints (the Levenberg trials of every iteration of every round); jitter: 0 = none
int solve_impl(const float* pose_f2g, const float* intr4, int n, const float* p3d, const float* kp, const float* invsigma, const float* weight,
               const float* depth, float bl, float* pose_out, uint8_t* bad_out, int32_t* iters_out, double* state_out, int32_t* trials_out, int jitter);

}  // namespace

// depth: n floats (<= 0 = monocular match) or NULL; bl = the stereo baseline.  Returns the inlier count.
extern "C" int pnp_stereo_ref_solve(const float* pose_f2g, const float* intr4, int n, const float* p3d, const float* kp, const float* invsigma,
                                    const float* weight, const float* depth, float bl, float* pose_out, uint8_t* bad_out, int32_t* iters_out,
                                    double* state_out) {
    return solve_impl(pose_f2g, intr4, n, p3d, kp, invsigma, weight, depth, bl, pose_out, bad_out, iters_out, state_out, nullptr, 0);
}

// the same solve; trials_out [4][10]: Levenberg trials per round and iteration (0 where none ran); jitter: 0, or the seed of a relative
// 1e-12 perturbation of the map points
extern "C" int pnp_hard_ref_solve(const float* pose_f2g, const float* intr4, int n, const float* p3d, const float* kp, const float* invsigma,
                                  const float* weight, const float* depth, float bl, int jitter, float* pose_out, uint8_t* bad_out,
                                  int32_t* iters_out, double* state_out, int32_t* trials_out) {
    return solve_impl(pose_f2g, intr4, n, p3d, kp, invsigma, weight, depth, bl, pose_out, bad_out, iters_out, state_out, trials_out, jitter);
}

namespace {
int solve_impl(const float* pose_f2g, const float* intr4, int n, const float* p3d, const float* kp, const float* invsigma, const float* weight,
               const float* depth, float bl, float* pose_out, uint8_t* bad_out, int32_t* iters_out, double* state_out, int32_t* trials_out, int jitter) {
    g2o::SparseOptimizer opt;
    auto linearSolver = g2o::make_unique<g2o::LinearSolverEigen<g2o::BlockSolver_6_3::PoseMatrixType>>();
    auto* lm = new g2o::OptimizationAlgorithmLevenberg(g2o::make_unique<g2o::BlockSolver_6_3>(std::move(linearSolver)));
    lm->setWriteDebug(false);   // (a failed factorisation would leave a debug.txt in the working directory; the arithmetic is the same)
    opt.setAlgorithm(lm);
    auto toSE3 = [&]() {
        Eigen::Matrix3d R;
        R << pose_f2g[0], pose_f2g[1], pose_f2g[2], pose_f2g[4], pose_f2g[5], pose_f2g[6], pose_f2g[8], pose_f2g[9], pose_f2g[10];
        return g2o::SE3Quat(R, Eigen::Vector3d(pose_f2g[3], pose_f2g[7], pose_f2g[11]));
    };
    auto* cam = new PoseVertex();
    cam->setEstimate(toSE3());
    cam->setId(0);
    cam->setFixed(false);
    opt.addVertex(cam);
    TrialCounter counter;
    if (trials_out) {
        opt.addPreIterationAction(&counter);
        for (int i = 0; i < 40; i++) trials_out[i] = 0;
    }
    Jitter jit(jitter);
    auto point = [&](int i) {
        Eigen::Vector3d X(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
        if (jitter > 0)
            for (int a = 0; a < 3; a++) X[a] *= 1.0 + 1e-12 * jit.next();
        return X;
    };
    const float Chi2D = 5.99, Chi3D = 7.815;
    const float thHuber2D = std::sqrt(5.99), thHuber3D = std::sqrt(7.815);
    const float fx = intr4[0], fy = intr4[1], cx = intr4[2], cy = intr4[3];
    std::vector<g2o::OptimizableGraph::Edge*> ed(n);
    std::vector<float> maxChi(n);
    for (int i = 0; i < n; i++) {
        float edge_weight = weight[i];
        const float d = depth ? depth[i] : 0.f;
        auto* rk = new WeightedHuber();
        if (d <= 0) {
            auto* e = new MonoEdge();
            e->Xw = point(i);
            e->fx = fx; e->fy = fy; e->cx = cx; e->cy = cy;
            e->setVertex(0, cam);
            e->setMeasurement(Eigen::Vector2d(kp[2 * i], kp[2 * i + 1]));
            e->setInformation(Eigen::Matrix2d::Identity() * invsigma[i]);
            rk->D = thHuber2D; rk->W = edge_weight;
            e->setRobustKernel(rk);
            opt.addEdge(e);
            ed[i] = e; maxChi[i] = Chi2D;
        } else {
            const float mbf = bl * fx;
            const float kp_ur = kp[2 * i] - mbf / d;
            auto* e = new StereoEdge();
            e->setVertex(0, cam);
            e->setMeasurement(Eigen::Vector3d(kp[2 * i], kp[2 * i + 1], kp_ur));
            e->setInformation(Eigen::Matrix3d::Identity() * invsigma[i]);
            edge_weight *= 2;
            rk->D = thHuber3D; rk->W = edge_weight;
            e->setRobustKernel(rk);
            e->fx = fx; e->fy = fy; e->cx = cx; e->cy = cy; e->bf = mbf;
            e->Xw = point(i);
            opt.addEdge(e);
            ed[i] = e; maxChi[i] = Chi3D;
        }
    }
    std::vector<char> bad(n, 0);
    for (int it = 0; it < 4; it++) iters_out[it] = 0;
    if (n > 0)
        for (int it = 0; it < 4; it++) {
            cam->setEstimate(toSE3());
            opt.initializeOptimization(0);
            if (trials_out) counter.reset();
            iters_out[it] = opt.optimize(10);
            if (trials_out) {
                g2o::G2OBatchStatistics::setGlobalStats(0);
                for (int i = 0; i < iters_out[it] && i < 10; i++) trials_out[10 * it + i] = counter.stat[i].levenbergIterations;
            }
            int nGood = 0;
            for (int i = 0; i < n; i++) {
                if (bad[i]) ed[i]->computeError();
                bad[i] = ed[i]->chi2() > maxChi[i];
                ed[i]->setLevel(bad[i] ? 1 : 0);
                if (it >= 2) ed[i]->setRobustKernel(nullptr);
                if (!bad[i]) nGood++;
            }
            if (nGood < 10) break;
        }
    Eigen::Matrix<double, 4, 4> Hm = cam->estimate().to_homogeneous_matrix();
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) pose_out[i * 4 + j] = (float)Hm(i, j);
    int good = 0;
    for (int i = 0; i < n; i++) { bad_out[i] = bad[i]; good += !bad[i]; }
    const g2o::SE3Quat& T = cam->estimate();
    state_out[0] = T.rotation().x(); state_out[1] = T.rotation().y(); state_out[2] = T.rotation().z(); state_out[3] = T.rotation().w();
    state_out[4] = T.translation()[0]; state_out[5] = T.translation()[1]; state_out[6] = T.translation()[2];
    if (trials_out) opt.removePreIterationAction(&counter);
    return good;
}
}  // namespace
