// TEST INFRASTRUCTURE ONLY — bundle adjustment with stereo / RGB-D observations, on the REAL reference g2o (the core objects that
// `make -C oracle ref` leaves in oracle/_ref/obj/; built by tests/golden/make_ba_stereo_golden.py into oracle/_ref/, never into git).
//
// The reference's own graph types (src/optimization/typesg2o.h) cannot be compiled without OpenCV, so this driver restates the two
// binary edges on g2o's BaseBinaryEdge: the two-row one with the expressions of typesg2o.h:249-323 and the three-row one with those of
// :327-409.  Of the latter note cam_project(:399-406): its parameter is `const float& bf`, so invz is a double quotient rounded to
// float AND bf * invz is a float product; the Jacobians (:352-397) use the double z.  The graph is built per observation by depth as
// globaloptimizer_g2o.cpp:229-272 does (mbf = bl * fx and kp_ur = u - mbf / depth in float, information I * inv_sigma, Huber widths
// thHuber2D / thHuber3D), the four limits are `const float` like globaloptimizer_g2o.h:112-117, and the schedule is :418-464:
// optimize(nIters, 1) -> edges over their own limit or with the point not in front of the camera to level 1, every robust kernel
// dropped -> optimize(2 nIters, 1); results as :466-522.  The solver stack (Levenberg, BlockSolver_6_3, Eigen LDLT, SE3 exp,
// robustification) is g2o's own code.
//
// ur_shift: every kp_ur is moved, in double, by +-ur_shift px (sign alternating with the edge index) — the generator's conditioning
// probe; 0 for the recorded run.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "g2o/core/base_binary_edge.h"
#include "g2o/core/base_vertex.h"
#include "g2o/core/block_solver.h"
#include "g2o/core/optimization_algorithm_levenberg.h"
#include "g2o/core/robust_kernel_impl.h"
#include "g2o/core/sparse_optimizer.h"
#include "g2o/solvers/eigen/linear_solver_eigen.h"
#include "g2o/types/slam3d/se3quat.h"

namespace {

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
        const double x = c[0], y = c[1], z = c[2], z_2 = z * z;
        Eigen::Matrix<double, 2, 3> tmp;
        tmp(0, 0) = fx; tmp(0, 1) = 0; tmp(0, 2) = -x / z * fx;
        tmp(1, 0) = 0; tmp(1, 1) = fy; tmp(1, 2) = -y / z * fy;
        _jacobianOplusXi = -1. / z * tmp * T.rotation().toRotationMatrix();
        _jacobianOplusXj(0, 0) = x * y / z_2 * fx;
        _jacobianOplusXj(0, 1) = -(1 + (x * x / z_2)) * fx;
        _jacobianOplusXj(0, 2) = y / z * fx;
        _jacobianOplusXj(0, 3) = -1. / z * fx;
        _jacobianOplusXj(0, 4) = 0;
        _jacobianOplusXj(0, 5) = x / z_2 * fx;
        _jacobianOplusXj(1, 0) = (1 + y * y / z_2) * fy;
        _jacobianOplusXj(1, 1) = -x * y / z_2 * fy;
        _jacobianOplusXj(1, 2) = -x / z * fy;
        _jacobianOplusXj(1, 3) = 0;
        _jacobianOplusXj(1, 4) = -1. / z * fy;
        _jacobianOplusXj(1, 5) = y / z_2 * fy;
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
        const Eigen::Vector3d xyz_trans = in_camera();
        const Eigen::Matrix3d R = T.rotation().toRotationMatrix();
        const double x = xyz_trans[0], y = xyz_trans[1], z = xyz_trans[2], z_2 = z * z;
        _jacobianOplusXi(0, 0) = -fx * R(0, 0) / z + fx * x * R(2, 0) / z_2;
        _jacobianOplusXi(0, 1) = -fx * R(0, 1) / z + fx * x * R(2, 1) / z_2;
        _jacobianOplusXi(0, 2) = -fx * R(0, 2) / z + fx * x * R(2, 2) / z_2;
        _jacobianOplusXi(1, 0) = -fy * R(1, 0) / z + fy * y * R(2, 0) / z_2;
        _jacobianOplusXi(1, 1) = -fy * R(1, 1) / z + fy * y * R(2, 1) / z_2;
        _jacobianOplusXi(1, 2) = -fy * R(1, 2) / z + fy * y * R(2, 2) / z_2;
        _jacobianOplusXi(2, 0) = _jacobianOplusXi(0, 0) - bf * R(2, 0) / z_2;
        _jacobianOplusXi(2, 1) = _jacobianOplusXi(0, 1) - bf * R(2, 1) / z_2;
        _jacobianOplusXi(2, 2) = _jacobianOplusXi(0, 2) - bf * R(2, 2) / z_2;
        _jacobianOplusXj(0, 0) = x * y / z_2 * fx;
        _jacobianOplusXj(0, 1) = -(1 + (x * x / z_2)) * fx;
        _jacobianOplusXj(0, 2) = y / z * fx;
        _jacobianOplusXj(0, 3) = -1. / z * fx;
        _jacobianOplusXj(0, 4) = 0;
        _jacobianOplusXj(0, 5) = x / z_2 * fx;
        _jacobianOplusXj(1, 0) = (1 + y * y / z_2) * fy;
        _jacobianOplusXj(1, 1) = -x * y / z_2 * fy;
        _jacobianOplusXj(1, 2) = -x / z * fy;
        _jacobianOplusXj(1, 3) = 0;
        _jacobianOplusXj(1, 4) = -1. / z * fy;
        _jacobianOplusXj(1, 5) = y / z_2 * fy;
        _jacobianOplusXj(2, 0) = _jacobianOplusXj(0, 0) - bf * y / z_2;
        _jacobianOplusXj(2, 1) = _jacobianOplusXj(0, 1) + bf * x / z_2;
        _jacobianOplusXj(2, 2) = _jacobianOplusXj(0, 2);
        _jacobianOplusXj(2, 3) = _jacobianOplusXj(0, 3);
        _jacobianOplusXj(2, 4) = 0;
        _jacobianOplusXj(2, 5) = _jacobianOplusXj(0, 5) - bf / z_2;
    }
};

g2o::RobustKernel* huber(double delta) {
    auto* rk = new g2o::RobustKernelHuber();
    rk->setDelta(delta);
    return rk;
}

}  // namespace

// chi2_mid / z_mid: every edge's chi2() and camera-frame z when the edges are relabelled between the passes; z_fin: the final double
// z (isDepthPositive of getResults), zf_fin: the float pose * float point z of the last test.  active_out[2]: level-0 edges per pass.
extern "C" int ba_stereo_ref_optimize(int K, int P, int E, const float* poses_f2g, const uint8_t* fixed, const float* intr, const float* points,
                                      const int32_t* obs_pt, const int32_t* obs_kf, const float* obs_uv, const double* obs_invsigma,
                                      const float* obs_depth, const float* frame_bl, int nIters, double ur_shift, int mono_limits_double, float* poses_out,
                                      float* points_out, double* chi2_out, uint8_t* bad_out, int32_t* iters_out, double* pose_state_out,
                                      double* chi2_mid, double* z_mid, double* z_fin, double* zf_fin, int32_t* active_out) {
    const float Chi2D = 5.99;
    const float Chi3D = 7.815;
    const float thHuber2D = std::sqrt(5.99);
    const float thHuber3D = std::sqrt(7.815);
    // mono_limits_double: the two-row edges' limit and width as the doubles the product's monocular defaults are (5.99, sqrt(5.99)) instead
    // of the reference's floats — the generator's second conditioning probe; 0 for the recorded run
    const double lim2D = mono_limits_double ? 5.99 : (double)Chi2D;
    const double hub2D = mono_limits_double ? std::sqrt(5.99) : (double)thHuber2D;
    g2o::SparseOptimizer opt;
    auto linearSolver = g2o::make_unique<g2o::LinearSolverEigen<g2o::BlockSolver_6_3::PoseMatrixType>>();
    opt.setAlgorithm(new g2o::OptimizationAlgorithmLevenberg(g2o::make_unique<g2o::BlockSolver_6_3>(std::move(linearSolver))));
    opt.setVerbose(false);
    std::vector<PoseVertex*> vp(K);
    for (int k = 0; k < K; k++) {   // frames first (vertex ids 0..K-1), points after
        const float* M = poses_f2g + 16 * k;
        Eigen::Matrix3d R;
        R << M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10];
        auto* v = new PoseVertex();
        v->setEstimate(g2o::SE3Quat(R, Eigen::Vector3d(M[3], M[7], M[11])));
        v->setId(k);
        if (fixed[k]) v->setFixed(true);
        opt.addVertex(v);
        vp[k] = v;
    }
    std::vector<PointVertex*> vx(P);
    for (int p = 0; p < P; p++) {
        auto* v = new PointVertex();
        v->setEstimate(Eigen::Vector3d(points[3 * p], points[3 * p + 1], points[3 * p + 2]));
        v->setId(K + p);
        v->setMarginalized(true);
        opt.addVertex(v);
        vx[p] = v;
    }
    std::vector<MonoEdge*> em(E, nullptr);
    std::vector<StereoEdge*> es(E, nullptr);
    for (int e = 0; e < E; e++) {
        const int k = obs_kf[e];
        const float depth = obs_depth[e];
        if (depth <= 0) {
            auto* ee = new MonoEdge();
            ee->fx = intr[4 * k]; ee->fy = intr[4 * k + 1]; ee->cx = intr[4 * k + 2]; ee->cy = intr[4 * k + 3];
            ee->setVertex(0, vx[obs_pt[e]]);
            ee->setVertex(1, vp[k]);
            ee->setMeasurement(Eigen::Vector2d(obs_uv[2 * e], obs_uv[2 * e + 1]));
            ee->setInformation(Eigen::Matrix2d::Identity() * obs_invsigma[e]);
            ee->setRobustKernel(huber(hub2D));
            opt.addEdge(ee);
            em[e] = ee;
        } else {
            const float mbf = frame_bl[k] * intr[4 * k];
            const float kp_ur = obs_uv[2 * e] - mbf / depth;
            auto* ee = new StereoEdge();
            ee->setVertex(0, vx[obs_pt[e]]);
            ee->setVertex(1, vp[k]);
            ee->setMeasurement(Eigen::Vector3d(obs_uv[2 * e], obs_uv[2 * e + 1], (double)kp_ur + ((e & 1) ? -ur_shift : ur_shift)));
            ee->setInformation(Eigen::Matrix3d::Identity() * obs_invsigma[e]);
            ee->setRobustKernel(huber(thHuber3D));
            ee->fx = intr[4 * k]; ee->fy = intr[4 * k + 1]; ee->cx = intr[4 * k + 2]; ee->cy = intr[4 * k + 3];
            ee->bf = mbf;
            opt.addEdge(ee);
            es[e] = ee;
        }
    }
    active_out[0] = E;
    opt.initializeOptimization();
    iters_out[0] = opt.optimize(nIters, 1);
    int act2 = 0;
    for (int e = 0; e < E; e++) {
        if (es[e]) {
            chi2_mid[e] = es[e]->chi2(); z_mid[e] = es[e]->in_camera()(2);
            if (es[e]->chi2() > Chi3D || !es[e]->isDepthPositive()) es[e]->setLevel(1);
            es[e]->setRobustKernel(0);
            act2 += es[e]->level() == 0;
        } else {
            chi2_mid[e] = em[e]->chi2(); z_mid[e] = em[e]->in_camera()(2);
            if (em[e]->chi2() > lim2D || !em[e]->isDepthPositive()) em[e]->setLevel(1);
            em[e]->setRobustKernel(0);
            act2 += em[e]->level() == 0;
        }
    }
    active_out[1] = act2;
    opt.initializeOptimization();
    iters_out[1] = opt.optimize(nIters * 2, 1);

    for (int k = 0; k < K; k++) {
        float* M = poses_out + 16 * k;
        if (fixed[k]) std::memcpy(M, poses_f2g + 16 * k, 64);
        else {
            Eigen::Matrix<double, 4, 4> H = vp[k]->estimate().to_homogeneous_matrix();
            for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) M[i * 4 + j] = (float)H(i, j);
        }
        const g2o::SE3Quat& T = vp[k]->estimate();
        double* o = pose_state_out + 7 * k;
        o[0] = T.rotation().x(); o[1] = T.rotation().y(); o[2] = T.rotation().z(); o[3] = T.rotation().w();
        o[4] = T.translation()[0]; o[5] = T.translation()[1]; o[6] = T.translation()[2];
    }
    for (int p = 0; p < P; p++) for (int a = 0; a < 3; a++) points_out[3 * p + a] = (float)vx[p]->estimate()[a];
    for (int e = 0; e < E; e++) {
        bool bad = false;
        if (es[e]) {
            chi2_out[e] = es[e]->chi2(); z_fin[e] = es[e]->in_camera()(2);
            if (es[e]->chi2() > Chi3D || !es[e]->isDepthPositive()) bad = true;
        } else {
            chi2_out[e] = em[e]->chi2(); z_fin[e] = em[e]->in_camera()(2);
            if (em[e]->chi2() > lim2D) bad = true;
        }
        const float* M = poses_out + 16 * obs_kf[e];
        const float* X = points_out + 3 * obs_pt[e];
        const float zf = M[8] * X[0] + M[9] * X[1] + M[10] * X[2] + M[11];
        zf_fin[e] = zf;
        if (!bad && zf < 0) bad = true;
        bad_out[e] = bad;
    }
    return 0;
}
