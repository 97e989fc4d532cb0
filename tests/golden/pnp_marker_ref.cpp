// TEST INFRASTRUCTURE ONLY — the pose-only PnP with keypoint matches AND squared planar markers, on the REAL reference g2o (the core
// objects that `make -C oracle ref` leaves in oracle/_ref/obj/; built by tests/golden/make_pnp_marker_golden.py into oracle/_ref/, never
// into git).
//
// The reference's own graph types (src/optimization/typesg2o.h) cannot be compiled without OpenCV, so this driver restates them on g2o's
// base classes and runs the loop of PnPSolver::solvePnp (pnpsolver.cpp:116-409):
//   * the pose vertex and the two keypoint edges as tests/golden/pnp_stereo_ref.cpp states them (typesg2o.h:521-650);
//   * the marker edge (typesg2o.h:414-471) on g2o's BaseBinaryEdge<8, ...>: vertex 0 = the marker's pose g2m (fixed), vertex 1 = the
//     camera; error = measured corners - projection of the four corners (-+s/2, +-s/2, 0) through c2g * g2m, every projected coordinate
//     ROUNDED TO FLOAT; no linearizeOplus, so g2o's own numeric differentiation runs with _delta_der = 1e-4 (a float);
//   * pnpsolver.cpp:280-386: weight_marker in the reference's mixed float / double arithmetic (+inf without keypoint matches), one
//     WeightedHuber(sqrt(15.507), weight_marker) per marker, after every round computeError() and the kernel dropped for good when
//     chi2 > 15.507f or the round index is >= 2; the stop below 10 good matches only without markers.
// The solver stack (Levenberg, block solver, Eigen LDLT, SE3 exp, numeric Jacobian, robustification) is g2o's own code.
//
// jitter (test only): 0 = off; 1..8 multiply the camera-frame corner coordinates by 1 +- 1e-11 (x, y) and 1 +- 0.7e-11 (z) before the
// projection, bit 0 / 1 / 2 of (jitter - 1) choosing the sign for x / y / z.  The generator admits a case into the fixture only if all
// eight patterns leave the outcome where it is: the float rounding makes the reference itself discontinuous, and a case that sits on
// such a rounding edge would test a coin flip.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "g2o/core/base_binary_edge.h"
#include "g2o/core/base_unary_edge.h"
#include "g2o/core/base_vertex.h"
#include "g2o/core/block_solver.h"
#include "g2o/core/optimization_algorithm_levenberg.h"
#include "g2o/core/robust_kernel.h"
#include "g2o/core/sparse_optimizer.h"
#include "g2o/solvers/eigen/linear_solver_eigen.h"
#include "g2o/types/slam3d/se3quat.h"

namespace {

typedef Eigen::Matrix<double, 8, 1, Eigen::ColMajor> Vector8D;

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

// the 2x6 block both keypoint edges share (typesg2o.h:614-650)
template <class J>
void mono_rows(J& jac, const Eigen::Vector3d& c, double fx, double fy) {
    const double x = c[0], y = c[1], invz = 1.0 / c[2], invz_2 = invz * invz;
    jac(0, 0) = x * y * invz_2 * fx;
    jac(0, 1) = -(1 + (x * x * invz_2)) * fx;
    jac(0, 2) = y * invz * fx;
    jac(0, 3) = -invz * fx;
    jac(0, 4) = 0;
    jac(0, 5) = x * invz_2 * fx;
    jac(1, 0) = (1 + y * y * invz_2) * fy;
    jac(1, 1) = -x * y * invz_2 * fy;
    jac(1, 2) = -x * invz * fy;
    jac(1, 3) = 0;
    jac(1, 4) = -invz * fy;
    jac(1, 5) = y * invz_2 * fy;
}

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
    void linearizeOplus() override { mono_rows(_jacobianOplusXi, static_cast<const PoseVertex*>(_vertices[0])->estimate().map(Xw), fx, fy); }
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
        mono_rows(_jacobianOplusXi, c, fx, fy);
        const double x = c[0], y = c[1], invz = 1.0 / c[2], invz_2 = invz * invz;
        _jacobianOplusXi(2, 0) = _jacobianOplusXi(0, 0) - bf * y * invz_2;
        _jacobianOplusXi(2, 1) = _jacobianOplusXi(0, 1) + bf * x * invz_2;
        _jacobianOplusXi(2, 2) = _jacobianOplusXi(0, 2);
        _jacobianOplusXi(2, 3) = _jacobianOplusXi(0, 3);
        _jacobianOplusXi(2, 4) = 0;
        _jacobianOplusXi(2, 5) = _jacobianOplusXi(0, 5) - bf * invz_2;
    }
};

class MarkerProjEdge : public g2o::BaseBinaryEdge<8, Vector8D, PoseVertex, PoseVertex> {   // MarkerEdgeOnlyProject
   public:
    EIGEN_MAKE_ALIGNED_OPERATOR_NEW
    g2o::Vector3 corner[4];
    double fx = 1, fy = 1, cx = 0, cy = 0;
    double jx = 1, jy = 1, jz = 1;   // the test-only jitter factors
    explicit MarkerProjEdge(float size) {
        _delta_der = 1e-4;   // the step of g2o's numeric Jacobian
        // Marker::get3DPointsLocalRefSystem: float coordinates, the halves taken in double
        const float lo = -size / 2., hi = size / 2.;
        corner[0] = g2o::Vector3(lo, hi, 0);
        corner[1] = g2o::Vector3(hi, hi, 0);
        corner[2] = g2o::Vector3(hi, lo, 0);
        corner[3] = g2o::Vector3(lo, lo, 0);
    }
    bool read(std::istream&) override { return false; }
    bool write(std::ostream&) const override { return false; }
    void computeError() override {
        const PoseVertex* g2m = static_cast<const PoseVertex*>(_vertices[0]);
        const PoseVertex* c2g = static_cast<const PoseVertex*>(_vertices[1]);
        const g2o::SE3Quat c2m = c2g->estimate() * g2m->estimate();
        const Vector8D obs(_measurement);
        for (int i = 0; i < 4; i++) {
            g2o::Vector3 p = c2m.map(corner[i]);
            p[0] *= jx; p[1] *= jy; p[2] *= jz;
            const float projx = (p[0] / p[2]) * fx + cx;
            _error(2 * i) = obs(2 * i) - projx;
            const float projy = (p[1] / p[2]) * fy + cy;
            _error(2 * i + 1) = obs(2 * i + 1) - projy;
        }
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

g2o::SE3Quat to_se3(const float* M) {
    Eigen::Matrix3d R;
    R << M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10];
    return g2o::SE3Quat(R, Eigen::Vector3d(M[3], M[7], M[11]));
}

}  // namespace

// depth: n floats (<= 0 = monocular match) or NULL; bl = the stereo baseline.  nm markers: pose_g2m nm x 16, size nm, und_corners nm x 8.
// Returns the number of good keypoint matches.
extern "C" int pnp_marker_ref_solve(const float* pose_f2g, const float* intr4, int n, const float* p3d, const float* kp, const float* invsigma,
                                    const float* weight, const float* depth, float bl, int nm, const float* pose_g2m, const float* msize,
                                    const float* und_corners, int jitter, float* pose_out, uint8_t* bad_out, int32_t* iters_out, double* state_out) {
    for (int it = 0; it < 4; it++) iters_out[it] = 0;
    if (n == 0 && nm == 0) {   // :148-149: the pose comes back as it went in
        memcpy(pose_out, pose_f2g, 64);
        const g2o::SE3Quat T = to_se3(pose_f2g);
        state_out[0] = T.rotation().x(); state_out[1] = T.rotation().y(); state_out[2] = T.rotation().z(); state_out[3] = T.rotation().w();
        state_out[4] = T.translation()[0]; state_out[5] = T.translation()[1]; state_out[6] = T.translation()[2];
        return 0;
    }
    g2o::SparseOptimizer opt;
    auto linearSolver = g2o::make_unique<g2o::LinearSolverEigen<g2o::BlockSolver_6_3::PoseMatrixType>>();
    opt.setAlgorithm(new g2o::OptimizationAlgorithmLevenberg(g2o::make_unique<g2o::BlockSolver_6_3>(std::move(linearSolver))));
    auto* cam = new PoseVertex();
    cam->setEstimate(to_se3(pose_f2g));
    cam->setId(0);
    cam->setFixed(false);
    opt.addVertex(cam);
    const float Chi2D = 5.99, Chi3D = 7.815, Chi8D = 15.507;
    const float thHuber2D = std::sqrt(5.99), thHuber3D = std::sqrt(7.815), thHuber8D = std::sqrt(15.507);
    const float fx = intr4[0], fy = intr4[1], cx = intr4[2], cy = intr4[3];
    std::vector<g2o::OptimizableGraph::Edge*> ed(n);
    std::vector<float> maxChi(n);
    double KpWeightSum = 0;
    for (int i = 0; i < n; i++) {
        float edge_weight = weight[i];
        const float d = depth ? depth[i] : 0.f;
        auto* rk = new WeightedHuber();
        if (d <= 0) {
            auto* e = new MonoEdge();
            e->Xw = Eigen::Vector3d(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
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
            e->Xw[0] = p3d[3 * i]; e->Xw[1] = p3d[3 * i + 1]; e->Xw[2] = p3d[3 * i + 2];
            opt.addEdge(e);
            ed[i] = e; maxChi[i] = Chi3D;
        }
        KpWeightSum += edge_weight;
    }
    // :305-310: the markers' share of the total weight
    const float w_markers = 0.3;
    const int totalNEdges = n + nm;
    const double weight_marker = ((w_markers * totalNEdges) / (1. - w_markers)) / float(KpWeightSum);
    std::vector<MarkerProjEdge*> med;
    for (int m = 0; m < nm; m++) {
        auto* mv = new PoseVertex();
        mv->setEstimate(to_se3(pose_g2m + 16 * m));
        mv->setFixed(true);
        mv->setId(1 + m);
        opt.addVertex(mv);
        auto* e = new MarkerProjEdge(msize[m]);
        Vector8D obs;
        for (int i = 0; i < 8; i++) obs(i) = und_corners[8 * m + i];
        e->setMeasurement(obs);
        e->setVertex(0, mv);
        e->setVertex(1, cam);
        e->fx = fx; e->fy = fy; e->cx = cx; e->cy = cy;
        if (jitter > 0) {
            const int s = jitter - 1;
            e->jx = 1 + ((s & 1) ? -1e-11 : 1e-11);
            e->jy = 1 + ((s & 2) ? -1e-11 : 1e-11);
            e->jz = 1 + ((s & 4) ? -0.7e-11 : 0.7e-11);
        }
        e->setInformation(Eigen::Matrix<double, 8, 8>::Identity());
        auto* rk = new WeightedHuber();
        e->setRobustKernel(rk);
        rk->D = thHuber8D; rk->W = weight_marker;
        opt.addEdge(e);
        med.push_back(e);
    }
    std::vector<char> bad(n, 0);
    for (int it = 0; it < 4; it++) {
        cam->setEstimate(to_se3(pose_f2g));
        opt.initializeOptimization(0);
        iters_out[it] = opt.optimize(10);
        int nGood = 0;
        for (int i = 0; i < n; i++) {
            if (bad[i]) ed[i]->computeError();
            bad[i] = ed[i]->chi2() > maxChi[i];
            ed[i]->setLevel(bad[i] ? 1 : 0);
            if (it >= 2) ed[i]->setRobustKernel(nullptr);
            if (!bad[i]) nGood++;
        }
        for (auto* me : med) {
            me->computeError();
            if (me->chi2() > Chi8D || it >= 2) me->setRobustKernel(nullptr);
        }
        if (nGood < 10 && nm == 0) break;
    }
    Eigen::Matrix<double, 4, 4> Hm = cam->estimate().to_homogeneous_matrix();
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) pose_out[i * 4 + j] = (float)Hm(i, j);
    int good = 0;
    for (int i = 0; i < n; i++) { bad_out[i] = bad[i]; good += !bad[i]; }
    const g2o::SE3Quat& T = cam->estimate();
    state_out[0] = T.rotation().x(); state_out[1] = T.rotation().y(); state_out[2] = T.rotation().z(); state_out[3] = T.rotation().w();
    state_out[4] = T.translation()[0]; state_out[5] = T.translation()[1]; state_out[6] = T.translation()[2];
    return good;
}
