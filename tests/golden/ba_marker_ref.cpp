// TEST INFRASTRUCTURE ONLY — bundle adjustment with keypoint observations AND squared planar markers whose poses are free, on the REAL
// reference g2o (the core objects that `make -C oracle ref` leaves in oracle/_ref/obj/; built by tests/golden/make_ba_marker_golden.py
// into oracle/_ref/, never into git).
//
// The reference's own graph types (src/optimization/typesg2o.h) cannot be compiled without OpenCV, so this driver restates them on g2o's
// base classes: the pose vertex and the two keypoint edges as tests/golden/ba_stereo_ref.cpp states them, and the marker edge
// (typesg2o.h:108-167) on BaseBinaryEdge<8, ...>: vertex 0 = the marker's pose g2m, vertex 1 = the camera c2g, both VertexSE3Expmap;
// error = measured corners - projection of the four corners (-+s/2, +-s/2, 0) through c2g * g2m, every projected coordinate ROUNDED TO
// FLOAT; no linearizeOplus of its own, so g2o's numeric central differences run on both vertices (base_binary_edge.hpp:166-233) with
// _delta_der, a float member, set to 1e-4.  The graph is globaloptimizer_g2o.cpp's: every marker a free, non-marginalised vertex
// (:307-315), one edge per (marker, frame) with information w * I8 and NO robust kernel (:320-352); between the passes the marker
// edges stay at level 0 (:451-455 does nothing to them); getResults writes the marker poses back as float 4x4 (:526-527).  The solver
// stack (Levenberg, BlockSolver_6_3, Eigen LDLT, SE3 exp, numeric Jacobian, robustification) is g2o's own code.
//
// ur_shift / mono_limits_double: ba_stereo_ref.cpp's two conditioning probes.  jitter (test only): 0 = off; 1..8 multiply the
// camera-frame corner coordinates by 1 +- 1e-11 (x, y) and 1 +- 0.7e-11 (z) before the projection, bit 0 / 1 / 2 of (jitter - 1)
// choosing the sign for x / y / z — the float rounding makes the reference itself discontinuous.
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
#include "g2o/core/robust_kernel_impl.h"
#include "g2o/core/sparse_optimizer.h"
#include "g2o/solvers/eigen/linear_solver_eigen.h"
#include "g2o/types/slam3d/se3quat.h"

namespace {

typedef Eigen::Matrix<double, 8, 1, Eigen::ColMajor> Vector8D;

class PointVertex : public g2o::BaseVertex<3, g2o::Vector3> {   // VertexSBAPointXYZ
   public:
    EIGEN_MAKE_ALIGNED_OPERATOR_NEW
    bool read(std::istream&) override { return false; }
    bool write(std::ostream&) const override { return false; }
    void setToOriginImpl() override { _estimate.setZero(); }
    void oplusImpl(const number_t* u) override { _estimate += Eigen::Map<const g2o::Vector3>(u); }
};

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

// the pose rows both keypoint edges share
template <class J>
void pose_rows(J& jac, double x, double y, double z, double fx, double fy) {
    const double z_2 = z * z;
    jac(0, 0) = x * y / z_2 * fx;
    jac(0, 1) = -(1 + (x * x / z_2)) * fx;
    jac(0, 2) = y / z * fx;
    jac(0, 3) = -1. / z * fx;
    jac(0, 4) = 0;
    jac(0, 5) = x / z_2 * fx;
    jac(1, 0) = (1 + y * y / z_2) * fy;
    jac(1, 1) = -x * y / z_2 * fy;
    jac(1, 2) = -x / z * fy;
    jac(1, 3) = 0;
    jac(1, 4) = -1. / z * fy;
    jac(1, 5) = y / z_2 * fy;
}

class MonoEdge : public g2o::BaseBinaryEdge<2, Eigen::Vector2d, PointVertex, PoseVertex> {   // EdgeSE3ProjectXYZ
   public:
    EIGEN_MAKE_ALIGNED_OPERATOR_NEW
    double fx = 1, fy = 1, cx = 0, cy = 0;
    bool read(std::istream&) override { return false; }
    bool write(std::ostream&) const override { return false; }
    Eigen::Vector3d in_camera() const {
        return static_cast<const PoseVertex*>(_vertices[1])->estimate().map(static_cast<const PointVertex*>(_vertices[0])->estimate());
    }
    void computeError() override {
        const Eigen::Vector3d c = in_camera();
        _error = _measurement - Eigen::Vector2d((c[0] / c[2]) * fx + cx, (c[1] / c[2]) * fy + cy);
    }
    bool isDepthPositive() const { return in_camera()(2) > 0.0; }
    void linearizeOplus() override {
        const g2o::SE3Quat T(static_cast<const PoseVertex*>(_vertices[1])->estimate());
        const Eigen::Vector3d c = in_camera();
        const double x = c[0], y = c[1], z = c[2];
        Eigen::Matrix<double, 2, 3> tmp;
        tmp(0, 0) = fx; tmp(0, 1) = 0; tmp(0, 2) = -x / z * fx;
        tmp(1, 0) = 0; tmp(1, 1) = fy; tmp(1, 2) = -y / z * fy;
        _jacobianOplusXi = -1. / z * tmp * T.rotation().toRotationMatrix();
        pose_rows(_jacobianOplusXj, x, y, z, fx, fy);
    }
};

class StereoEdge : public g2o::BaseBinaryEdge<3, Eigen::Vector3d, PointVertex, PoseVertex> {   // EdgeStereoSE3ProjectXYZ
   public:
    EIGEN_MAKE_ALIGNED_OPERATOR_NEW
    double fx = 1, fy = 1, cx = 0, cy = 0, bf = 0;
    bool read(std::istream&) override { return false; }
    bool write(std::ostream&) const override { return false; }
    Eigen::Vector3d in_camera() const {
        return static_cast<const PoseVertex*>(_vertices[1])->estimate().map(static_cast<const PointVertex*>(_vertices[0])->estimate());
    }
    Eigen::Vector3d cam_project(const Eigen::Vector3d& trans_xyz, const float& bf) const {
        const float invz = 1.0f / trans_xyz[2];
        Eigen::Vector3d res;
        res[0] = trans_xyz[0] * invz * fx + cx;
        res[1] = trans_xyz[1] * invz * fy + cy;
        res[2] = res[0] - bf * invz;
        return res;
    }
    void computeError() override {
        Eigen::Vector3d obs(_measurement);
        _error = obs - cam_project(in_camera(), bf);
    }
    bool isDepthPositive() const { return in_camera()(2) > 0.0; }
    void linearizeOplus() override {
        const g2o::SE3Quat T(static_cast<const PoseVertex*>(_vertices[1])->estimate());
        const Eigen::Vector3d c = in_camera();
        const Eigen::Matrix3d R = T.rotation().toRotationMatrix();
        const double x = c[0], y = c[1], z = c[2], z_2 = z * z;
        for (int j = 0; j < 3; j++) {
            _jacobianOplusXi(0, j) = -fx * R(0, j) / z + fx * x * R(2, j) / z_2;
            _jacobianOplusXi(1, j) = -fy * R(1, j) / z + fy * y * R(2, j) / z_2;
            _jacobianOplusXi(2, j) = _jacobianOplusXi(0, j) - bf * R(2, j) / z_2;
        }
        pose_rows(_jacobianOplusXj, x, y, z, fx, fy);
        _jacobianOplusXj(2, 0) = _jacobianOplusXj(0, 0) - bf * y / z_2;
        _jacobianOplusXj(2, 1) = _jacobianOplusXj(0, 1) + bf * x / z_2;
        _jacobianOplusXj(2, 2) = _jacobianOplusXj(0, 2);
        _jacobianOplusXj(2, 3) = _jacobianOplusXj(0, 3);
        _jacobianOplusXj(2, 4) = 0;
        _jacobianOplusXj(2, 5) = _jacobianOplusXj(0, 5) - bf / z_2;
    }
};

class MarkerEdge : public g2o::BaseBinaryEdge<8, Vector8D, PoseVertex, PoseVertex> {
   public:
    EIGEN_MAKE_ALIGNED_OPERATOR_NEW
    g2o::Vector3 corner[4];
    double fx = 1, fy = 1, cx = 0, cy = 0;
    double jx = 1, jy = 1, jz = 1;   // the test-only jitter factors
    explicit MarkerEdge(float size) {
        _delta_der = 1e-4;   // a float member: the step of g2o's numeric Jacobian is (double)1e-4f
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

int count_trials(const g2o::SparseOptimizer& opt, int iters) {
    int n = 0;
    for (int i = 0; i < iters && i < (int)opt.batchStatistics().size(); i++) n += opt.batchStatistics()[i].levenbergIterations;
    return n;
}

g2o::RobustKernel* huber(double delta) {
    auto* rk = new g2o::RobustKernelHuber();
    rk->setDelta(delta);
    return rk;
}

g2o::SE3Quat to_se3(const float* M) {
    Eigen::Matrix3d R;
    R << M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10];
    return g2o::SE3Quat(R, Eigen::Vector3d(M[3], M[7], M[11]));
}

void put_pose(const g2o::SE3Quat& T, float* M, double* o) {
    Eigen::Matrix<double, 4, 4> H = T.to_homogeneous_matrix();
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) M[i * 4 + j] = (float)H(i, j);
    o[0] = T.rotation().x(); o[1] = T.rotation().y(); o[2] = T.rotation().z(); o[3] = T.rotation().w();
    o[4] = T.translation()[0]; o[5] = T.translation()[1]; o[6] = T.translation()[2];
}

}  // namespace

struct ba_marker_ref_in {
    int32_t K, P, E, M, EM, nIters;
    const float* poses_f2g; const uint8_t* fixed; const float* intr; const float* points;
    const int32_t* obs_pt; const int32_t* obs_kf; const float* obs_uv; const double* obs_invsigma; const float* obs_depth; const float* frame_bl;
    const float* mk_pose; const float* mk_size; const int32_t* me_marker; const int32_t* me_frame; const float* me_corners; const double* me_weight;
    double ur_shift; int32_t mono_limits_double, jitter;
};
struct ba_marker_ref_out {
    float* poses; float* points; double* chi2; uint8_t* bad; int32_t* iters; double* state;
    float* marker_poses; double* marker_state; double* marker_chi2;
    double* lin_err;   // EM x 8: every marker edge's error at the initial state
    double* lin_Ji;    // EM x 8 x 6 row-major: d error / d marker (every marker is free)
    double* lin_Jj;    // EM x 8 x 6: d error / d frame, zero where the frame is fixed (g2o skips it)
    double* chi2_mid; double* z_mid; double* z_fin; double* zf_fin; int32_t* active;
    int32_t* trials;   // 2: Levenberg trials per pass (= iterations when none was rejected)
};

extern "C" int ba_marker_ref_optimize(const ba_marker_ref_in* in, ba_marker_ref_out* out) {
    const int K = in->K, P = in->P, E = in->E, M = in->M, EM = in->EM;
    const float Chi2D = 5.99;
    const float Chi3D = 7.815;
    const float thHuber2D = std::sqrt(5.99);
    const float thHuber3D = std::sqrt(7.815);
    const double lim2D = in->mono_limits_double ? 5.99 : (double)Chi2D;
    const double hub2D = in->mono_limits_double ? std::sqrt(5.99) : (double)thHuber2D;
    g2o::SparseOptimizer opt;
    auto linearSolver = g2o::make_unique<g2o::LinearSolverEigen<g2o::BlockSolver_6_3::PoseMatrixType>>();
    opt.setAlgorithm(new g2o::OptimizationAlgorithmLevenberg(g2o::make_unique<g2o::BlockSolver_6_3>(std::move(linearSolver))));
    opt.setVerbose(false);
    opt.setComputeBatchStatistics(true);   // for the count of Levenberg trials only: it recomputes the active errors after an iteration, nothing else
    std::vector<PoseVertex*> vp(K);
    for (int k = 0; k < K; k++) {   // frames first (vertex ids 0..K-1), points after, markers last
        auto* v = new PoseVertex();
        v->setEstimate(to_se3(in->poses_f2g + 16 * k));
        v->setId(k);
        if (in->fixed[k]) v->setFixed(true);
        opt.addVertex(v);
        vp[k] = v;
    }
    std::vector<PointVertex*> vx(P);
    for (int p = 0; p < P; p++) {
        auto* v = new PointVertex();
        v->setEstimate(Eigen::Vector3d(in->points[3 * p], in->points[3 * p + 1], in->points[3 * p + 2]));
        v->setId(K + p);
        v->setMarginalized(true);
        opt.addVertex(v);
        vx[p] = v;
    }
    std::vector<MonoEdge*> em(E, nullptr);
    std::vector<StereoEdge*> es(E, nullptr);
    for (int e = 0; e < E; e++) {
        const int k = in->obs_kf[e];
        const float* I = in->intr + 4 * k;
        const float depth = in->obs_depth[e];
        if (depth <= 0) {
            auto* ee = new MonoEdge();
            ee->fx = I[0]; ee->fy = I[1]; ee->cx = I[2]; ee->cy = I[3];
            ee->setVertex(0, vx[in->obs_pt[e]]);
            ee->setVertex(1, vp[k]);
            ee->setMeasurement(Eigen::Vector2d(in->obs_uv[2 * e], in->obs_uv[2 * e + 1]));
            ee->setInformation(Eigen::Matrix2d::Identity() * in->obs_invsigma[e]);
            ee->setRobustKernel(huber(hub2D));
            opt.addEdge(ee);
            em[e] = ee;
        } else {
            const float mbf = in->frame_bl[k] * I[0];
            const float kp_ur = in->obs_uv[2 * e] - mbf / depth;
            auto* ee = new StereoEdge();
            ee->setVertex(0, vx[in->obs_pt[e]]);
            ee->setVertex(1, vp[k]);
            ee->setMeasurement(Eigen::Vector3d(in->obs_uv[2 * e], in->obs_uv[2 * e + 1], (double)kp_ur + ((e & 1) ? -in->ur_shift : in->ur_shift)));
            ee->setInformation(Eigen::Matrix3d::Identity() * in->obs_invsigma[e]);
            ee->setRobustKernel(huber(thHuber3D));
            ee->fx = I[0]; ee->fy = I[1]; ee->cx = I[2]; ee->cy = I[3];
            ee->bf = mbf;
            opt.addEdge(ee);
            es[e] = ee;
        }
    }
    std::vector<PoseVertex*> vm(M);
    for (int m = 0; m < M; m++) {
        auto* v = new PoseVertex();
        v->setEstimate(to_se3(in->mk_pose + 16 * m));
        v->setId(K + P + m);
        opt.addVertex(v);
        vm[m] = v;
    }
    std::vector<MarkerEdge*> me(EM);
    for (int e = 0; e < EM; e++) {
        const int k = in->me_frame[e];
        const float* I = in->intr + 4 * k;
        auto* ee = new MarkerEdge(in->mk_size[in->me_marker[e]]);
        Vector8D obs;
        for (int i = 0; i < 8; i++) obs(i) = in->me_corners[8 * e + i];
        ee->setMeasurement(obs);
        ee->setVertex(0, vm[in->me_marker[e]]);
        ee->setVertex(1, vp[k]);
        ee->fx = I[0]; ee->fy = I[1]; ee->cx = I[2]; ee->cy = I[3];
        if (in->jitter > 0) {
            const int s = in->jitter - 1;
            ee->jx = 1 + ((s & 1) ? -1e-11 : 1e-11);
            ee->jy = 1 + ((s & 2) ? -1e-11 : 1e-11);
            ee->jz = 1 + ((s & 4) ? -0.7e-11 : 0.7e-11);
        }
        ee->setInformation(Eigen::Matrix<double, 8, 8>::Identity() * in->me_weight[e]);
        opt.addEdge(ee);
        me[e] = ee;
    }
    out->active[0] = E;
    opt.initializeOptimization();
    // the first linearisation, read off the edges (the workspace of the Jacobians is shared, so each edge is read at once)
    opt.computeActiveErrors();
    for (int e = 0; e < EM; e++) {
        me[e]->linearizeOplus(opt.jacobianWorkspace());
        const bool frame_fixed = in->fixed[in->me_frame[e]] != 0;
        for (int r = 0; r < 8; r++) {
            out->lin_err[8 * e + r] = me[e]->error()(r);
            for (int c = 0; c < 6; c++) {
                out->lin_Ji[48 * e + 6 * r + c] = me[e]->jacobianOplusXi()(r, c);
                out->lin_Jj[48 * e + 6 * r + c] = frame_fixed ? 0.0 : me[e]->jacobianOplusXj()(r, c);
            }
        }
    }
    out->iters[0] = opt.optimize(in->nIters, 1);
    out->trials[0] = count_trials(opt, out->iters[0]);
    int act2 = 0;
    for (int e = 0; e < E; e++) {
        if (es[e]) {
            out->chi2_mid[e] = es[e]->chi2(); out->z_mid[e] = es[e]->in_camera()(2);
            if (es[e]->chi2() > Chi3D || !es[e]->isDepthPositive()) es[e]->setLevel(1);
            es[e]->setRobustKernel(0);
            act2 += es[e]->level() == 0;
        } else {
            out->chi2_mid[e] = em[e]->chi2(); out->z_mid[e] = em[e]->in_camera()(2);
            if (em[e]->chi2() > lim2D || !em[e]->isDepthPositive()) em[e]->setLevel(1);
            em[e]->setRobustKernel(0);
            act2 += em[e]->level() == 0;
        }
    }
    for (int e = 0; e < EM; e++) {   // :451-455: setLevel(0) is the level the edge has, and it has no kernel to remove
        me[e]->setLevel(0);
        me[e]->setRobustKernel(0);
    }
    out->active[1] = act2;
    opt.initializeOptimization();
    out->iters[1] = opt.optimize(in->nIters * 2, 1);
    out->trials[1] = count_trials(opt, out->iters[1]);

    for (int k = 0; k < K; k++) {
        put_pose(vp[k]->estimate(), out->poses + 16 * k, out->state + 7 * k);
        if (in->fixed[k]) std::memcpy(out->poses + 16 * k, in->poses_f2g + 16 * k, 64);
    }
    for (int m = 0; m < M; m++) put_pose(vm[m]->estimate(), out->marker_poses + 16 * m, out->marker_state + 7 * m);
    for (int p = 0; p < P; p++) for (int a = 0; a < 3; a++) out->points[3 * p + a] = (float)vx[p]->estimate()[a];
    for (int e = 0; e < E; e++) {
        bool bad = false;
        if (es[e]) {
            out->chi2[e] = es[e]->chi2(); out->z_fin[e] = es[e]->in_camera()(2);
            if (es[e]->chi2() > Chi3D || !es[e]->isDepthPositive()) bad = true;
        } else {
            out->chi2[e] = em[e]->chi2(); out->z_fin[e] = em[e]->in_camera()(2);
            if (em[e]->chi2() > lim2D) bad = true;
        }
        const float* Mx = out->poses + 16 * in->obs_kf[e];
        const float* X = out->points + 3 * in->obs_pt[e];
        const float zf = Mx[8] * X[0] + Mx[9] * X[1] + Mx[10] * X[2] + Mx[11];
        out->zf_fin[e] = zf;
        if (!bad && zf < 0) bad = true;
        out->bad[e] = bad;
    }
    for (int e = 0; e < EM; e++) out->marker_chi2[e] = me[e]->chi2();
    return 0;
}
