// The body of pnp_solve_kernel<CACHED, STEREO, MARKERS> and of pnp_solve_batch_kernel<CACHED> (pnp.hip), included inside both: in scope
// are A (PnpArgs) and the three flags.  No include guard: the text is included once per kernel.
    extern __shared__ __attribute__((aligned(16))) unsigned char s_cache[];
    __shared__ __attribute__((aligned(16))) double s_part[kPnpWaves * 32];
    __shared__ __attribute__((aligned(16))) double s_tot[32];
    __shared__ __attribute__((aligned(16))) double s_pose[4][12];   // [0] pose to evaluate + accumulate, [1] pose of the excluded matches' fresh chi2 (end of the last
                                                                    // round), [2] pose the kept chi2 belong to (the last one evaluated), [3] the input pose
    __shared__ __attribute__((aligned(16))) double s_H[28];         // the normal equations of the current pose (21 + 6): wave 0's, parked here between solves
    __shared__ __attribute__((aligned(16))) double s_T[12], s_x[8]; // wave 0's: the current (last accepted) pose and the last solved step
    __shared__ int s_ctl[4];                                        // mode, classify, drop_robust, ladder length
    __shared__ __attribute__((aligned(16))) double s_lad[2];        // ladder request: lambda and ni of its first candidate
    __shared__ __attribute__((aligned(16))) double s_cand[kLadderMax][20];   // per candidate: trial pose (12), step (6), factorisation ok (1)
    const int tid = threadIdx.x, lane = tid & 63;
    int n = A.n;
    if (A.n_dev) {   // (uh_track_pose: the matches were chosen on the device)
        const int nd = __builtin_amdgcn_readfirstlane(*A.n_dev);
        n = nd < n ? nd : n;
        // pnpsolver.cpp:149-150: without matches the pose comes back as it went in.  The tracker's first solve (dec.dyn17) runs only with
        // MORE than min_inliers matches (system.cpp:6595); otherwise the reference tries its FrameMatcher fallback, which is the caller's:
        // taken to find nothing, nInliers = 0 and no solve is reported (pose in, no iterations, no outlier flags)
        // (with markers a solve without matches runs, pnpsolver.cpp:148-158; the tracker's rule for its first solve stays)
        if ((!MARKERS && n <= 0) || (A.dec.dyn17 && n <= A.dec.min_inliers)) {
            if (tid < 16) A.pose_out[tid] = A.pose_in[tid];
            if (tid < 5) A.result[tid] = 0;
            for (int e = tid; e < n; e += kPnpThreads) A.bad_out[e] = 0;
            if (A.dec.dyn17 && tid == 0) pnp_decide(A, 0, A.pose_in);
            return;
        }
    }
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);        // wave index as a scalar: the role split below is an s_cbranch
    if (A.clk && tid == 0) A.clk[0] = __builtin_readcyclecounter();
    const double fx = A.intr[0], fy = A.intr[1], cx = A.intr[2], cy = A.intr[3];
    const double delta = (double)sqrtf(5.99f), dsqr = delta * delta;
    // stereo edges (pnpsolver.cpp:175-181, 248-274): thHuber3D = (float)sqrt(7.815), relabelled above Chi3D = 7.815f, bf = mbf as a double
    double delta3 = 0, dsqr3 = 0, bf = 0;
    if constexpr (STEREO) { delta3 = (double)(float)sqrt(7.815); dsqr3 = delta3 * delta3; bf = (double)(A.bl * A.intr[0]); }
    // one name for both instantiations; in each the pointer has a single provenance (LDS or HBM): ds_* or global_* accesses, never flat
    MatchRec* rec;
    if constexpr (CACHED) rec = reinterpret_cast<MatchRec*>(s_cache);
    else rec = reinterpret_cast<MatchRec*>(A.work);
    float* urs = nullptr;   // STEREO: kp_ur per match, behind the n records
    if constexpr (STEREO) urs = reinterpret_cast<float*>(rec + n);
    for (int e = tid; e < n; e += kPnpThreads) {
        MatchRec r;
        r.X = A.p3d[3 * e]; r.Y = A.p3d[3 * e + 1]; r.Z = A.p3d[3 * e + 2]; r.u = A.kp[2 * e]; r.v = A.kp[2 * e + 1];
        r.invsig = A.invsig[e]; r.weight = A.weight[e]; r.flags = kActive | kRobust;
        if constexpr (STEREO) {
            // pnpsolver.cpp:239-246: depth <= 0 keeps the monocular edge; else mbf = bl * fx and kp_ur = x - mbf / depth, all float
            // (a correctly rounded float division: the build does not use fast math)
            const float depth = A.depth[e];
            float ur = 0.f;
            if (!(depth <= 0.f)) {
                const float mbf = A.bl * A.intr[0];
                ur = r.u - mbf / depth;
                r.flags |= kStereo;
            }
            urs[e] = ur;
        }
        rec[e] = r;
    }
    {
        double Rt0[12];
        rt_from_pose16(A.pose_in, Rt0);
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < 12; i++) { s_pose[3][i] = Rt0[i]; s_pose[1][i] = Rt0[i]; s_pose[2][i] = Rt0[i]; }
        }
    }
    // markers: the records, and weight_marker of pnpsolver.cpp:305-310 in its mixed float / double arithmetic — KpWeightSum is the
    // double sum of the per-match kernel weights after the stereo doubling (block_sum's fixed pairing instead of the reference's
    // match order: the same bits whenever the partial sums are exact, as they are for the weights 0.5 / 1 / 2); +inf without matches
    // (in the dynamic LDS behind the A.n match records the launch sized it for — nothing is added to the marker-free instantiations)
    const int nmk = MARKERS ? A.n_mk : 0;
    MarkerRec* s_mk = reinterpret_cast<MarkerRec*>(s_cache + (CACHED ? pnp_marker_offset(A.n, STEREO) : 0));
    double* s_mkw = reinterpret_cast<double*>(s_mk + kPnpMaxMarkers);
    double* s_mkpart = s_mkw + 1;
    // marker i belongs to wave 7 - i % 8: wave 0, whose serial steps every pass waits for, is the last to get one
    const int mk_first = kPnpWaves - 1 - wv;
    if constexpr (MARKERS) {
        double ws = 0;
        for (int e = tid; e < n; e += kPnpThreads) {   // (this thread's own records: no second trip to the caller's arrays)
            float w = rec[e].weight;
            if constexpr (STEREO) { if (rec[e].flags & kStereo) w *= 2.f; }
            ws += (double)w;
        }
        ws = block_sum<kPnpWaves>(ws, s_part);
        if (tid == 0) *s_mkw = ((double)(0.3f * (float)(n + nmk)) / (1. - (double)0.3f)) / (double)(float)ws;
        if (tid < nmk) {
            double G[12];   // Marker::pose_g2m
            rt_from_pose16(A.mk_pose + 16 * tid, G);
            const float sz = A.mk_size[tid];
            const double hi = (double)(float)((double)sz / 2.), lo = (double)(float)(-(double)sz / 2.);   // Marker::get3DPointsLocalRefSystem: cv::Point3f
            const double px[4] = {lo, hi, hi, lo}, py[4] = {hi, hi, lo, lo};
            MarkerRec& r = s_mk[tid];
#pragma unroll
            for (int c = 0; c < 4; c++)
#pragma unroll
                for (int a = 0; a < 3; a++) r.P[c][a] = fma(G[3 * a + 1], py[c], fma(G[3 * a], px[c], G[9 + a]));
#pragma unroll
            for (int i = 0; i < 8; i++) r.uv[i] = A.mk_corners[8 * tid + i];
            r.robust = 1; r.pad = 0;
        }
    }
    __syncthreads();
    if (A.clk && tid == 0) A.clk[1] = __builtin_readcyclecounter();
    // the marker edge's kernel: thHuber8D = (float)sqrt(15.507), relabelled against Chi8D = 15.507f
    constexpr double delta8 = 0x1.f80cep+1, dsqr8 = delta8 * delta8;      // (double)(float)sqrt(15.507) = 3.9378929138183594
    constexpr double mk_delta = (double)1e-4f, mk_scalar = 1 / (2 * mk_delta);
    // SE3Quat::exp for omega = delta e_d (theta = delta >= 1e-5): R = I + sin(theta)/theta Omega + (1 - cos(theta))/theta^2 Omega^2, i.e. the
    // entries (sin(delta) / delta) * delta and 1 - ((1 - cos(delta)) / delta^2) * delta^2 in double, as constants (wave-uniform values
    // computed at run time would sit in vector registers for the whole solve)
    constexpr double mk_sin = 0x1.a36e2df44599cp-14, mk_cos = 0x1.ffffffd50ce26p-1;
    // the error of corner c of a marker at the pose Rt perturbed by pattern k: 0 = not, 1..6 = +delta along dimension k - 1, 7..12 =
    // -delta along dimension k - 7.  Projections rounded to float (typesg2o.h:461-465)
    auto marker_err = [&](const MarkerRec& m, int c, int k, const double* Rt, double& ex, double& ey) {
        double p0, p1, p2;
        to_camera(Rt, m.P[c][0], m.P[c][1], m.P[c][2], p0, p1, p2);
        if (k > 0) {
            const double sg = k > 6 ? -1.0 : 1.0;
            const int d = k > 6 ? k - 7 : k - 1;
            if (d < 3) {   // rotation about axis d: (u, v, w) = the components (d, d + 1, d + 2) cyclically
                const double v = d == 0 ? p1 : d == 1 ? p2 : p0, w = d == 0 ? p2 : d == 1 ? p0 : p1;
                const double s = sg * mk_sin;
                const double v2 = mk_cos * v - s * w, w2 = s * v + mk_cos * w;
                if (d == 0) { p1 = v2; p2 = w2; } else if (d == 1) { p2 = v2; p0 = w2; } else { p0 = v2; p1 = w2; }
            } else {
                const double t = sg * mk_delta;
                if (d == 3) p0 += t; else if (d == 4) p1 += t; else p2 += t;
            }
        }
        const double projx = (double)(float)((p0 / p2) * fx + cx), projy = (double)(float)((p1 / p2) * fy + cy);
        ex = (double)m.uv[2 * c] - projx;
        ey = (double)m.uv[2 * c + 1] - projy;
    };
    // chi2 of a marker at Rt (no perturbation), valid in every lane: lane l evaluates corner l & 3, the quad adds up
    auto marker_chi2 = [&](const MarkerRec& m, const double* Rt) -> double {
        double ex, ey;
        marker_err(m, lane & 3, 0, Rt, ex, ey);
        double c = fma(ex, ex, ey * ey);
        c += __shfl_xor(c, 1);
        c += __shfl_xor(c, 2);
        return c;
    };
    auto marker_rho0 = [&](double c) -> double {   // WeightedHubberRobustKernel's rho[0]
        const double wt = *s_mkw;
        return c <= dsqr8 ? wt * c : wt * (2 * sqrt(c) * delta8 - dsqr8);
    };

    // chi2 of a match at the pose Rt; xz, yz, invz for the Jacobian
    auto project = [&](const MatchRec& m, const double* Rt, double& ex, double& ey, double& xz, double& yz, double& invz) -> double {
        double p0, p1, p2;
        to_camera(Rt, m.X, m.Y, m.Z, p0, p1, p2);
        invz = rcp_nr(p2);
        xz = p0 * invz; yz = p1 * invz;
        ex = (double)m.u - fma(xz, fx, cx);
        ey = (double)m.v - fma(yz, fy, cy);
        return (double)m.invsig * fma(ex, ex, ey * ey);
    };
    // EdgeStereoSE3ProjectXYZOnlyPose (typesg2o.h:521-590): cam_project divides in double and ROUNDS 1/z TO FLOAT before it uses it in
    // double, un-fused; the Jacobian uses the double 1/z (invz, as the monocular edge's).  er = kp_ur - (u_proj - bf / z).
    auto project_st = [&](const MatchRec& m, float ur, const double* Rt, double& ex, double& ey, double& er, double& xz, double& yz,
                          double& invz) -> double {
        double p0, p1, p2;
        to_camera(Rt, m.X, m.Y, m.Z, p0, p1, p2);
        invz = rcp_nr(p2);
        xz = p0 * invz; yz = p1 * invz;
        const double izf = (double)(float)(1.0 / p2);
        const double r0 = p0 * izf * fx + cx, r1 = p1 * izf * fy + cy;
        const double r2 = r0 - bf * izf;
        ex = (double)m.u - r0;
        ey = (double)m.v - r1;
        er = (double)ur - r2;
        return (double)m.invsig * fma(er, er, fma(ex, ex, ey * ey));
    };
    // ---- the one edge evaluation of classify, accumulate and the ladder.  st: the match has the three-row edge (STEREO instantiations only;
    // in the others it is the constant false and everything stereo folds away)
    auto edge = [&](const MatchRec& m, bool st, float ur, const double* Rt, double& ex, double& ey, double& er, double& xz, double& yz, double& invz) -> double {
        if constexpr (STEREO) { if (st) return project_st(m, ur, Rt, ex, ey, er, xz, yz, invz); }
        return project(m, Rt, ex, ey, xz, yz, invz);
    };
    // WeightedHubberRobustKernel: returns rho[0] and leaves rho[1] in rho1 above the threshold (the caller's 1 stays below it)
    auto huber = [&](double c, double wt, double dl, double ds, double& rho1) -> double {
        if (c <= ds) return wt * c;
        const double rs = rsq_nr(c);
        const double rc = wt * fma(2 * (c * rs), dl, -ds);   // (rho[0] before rho[1]: the other order renames the monocular kernels' registers)
        rho1 = dl * rs;
        return rc;
    };
    // the kernel of a match: the stereo edge's weight is doubled in float (pnpsolver.cpp:258) and its threshold is thHuber3D
    auto robust = [&](const MatchRec& m, bool st, double c, double& rho1) -> double {
        double wt = m.weight, dl = delta, ds = dsqr;
        if constexpr (STEREO) { if (st) { wt = (double)(m.weight * 2.f); dl = delta3; ds = dsqr3; } }
        return huber(c, wt, dl, ds, rho1);
    };

    // One pass over this thread's matches (every wave).  classify: first the reclassification that ends a round
    // (pnpsolver.cpp:358-371): a match that was excluded gets a fresh chi2 at RtC, the others the chi2 of the LAST pose the optimiser
    // evaluated them at (RtK: g2o keeps the edge errors of its last trial, accepted or not) — recomputed here instead of stored, same
    // bits; chi2 > 5.99 -> outlier; drop_robust as the reference from its third round on.  Then (RtA != nullptr) every active match:
    // error, chi2, robust weight and Jacobian at RtA, accumulated into the 29 sums; the wave's totals go to s_part.
    auto pass = [&](bool accumulate, const double* RtA, bool classify, bool drop_robust) {
        double acc[kNS];
#pragma unroll
        for (int i = 0; i < kNS; i++) acc[i] = 0;
        for (int e = tid; e < n; e += kPnpThreads) {
            const MatchRec m = rec[e];
            unsigned f = m.flags;
            double ex, ey, er = 0, xz, yz, invz;
            bool st = false;
            float ur = 0.f;
            if constexpr (STEREO) { st = (f & kStereo) != 0; ur = urs[e]; }
            if (classify) {
                double Rs[12];
#pragma unroll
                for (int i = 0; i < 12; i++) Rs[i] = s_pose[(f & kBad) ? 1 : 2][i];   // (read per match: four classifying passes per solve)
                const double c = edge(m, st, ur, Rs, ex, ey, er, xz, yz, invz);
                const bool b = c > (double)(st ? 7.815f : 5.99f);   // Chi3D, Chi2D
                f = (b ? kBad : kActive) | (drop_robust ? 0u : (f & kRobust));
                if constexpr (STEREO) f |= m.flags & kStereo;
                rec[e].flags = f;
                acc[28] += b ? 0.0 : 1.0;
            }
            if (!(f & kActive) || !accumulate) continue;
            const double c = edge(m, st, ur, RtA, ex, ey, er, xz, yz, invz);
            const double w = m.invsig;
            double rho1 = 1.0, rc = c;
            if (f & kRobust) rc = robust(m, st, c, rho1);
            acc[27] += rc;
            // 2x6 Jacobian rows (typesg2o.h:614-650): j = d ex / d xi, k = d ey / d xi; j[4] = k[3] = 0
            const double zf = invz * fx, zg = invz * fy, xf = xz * fx, yg = yz * fy;
            const double j0 = xf * yz, j1 = -fma(xf, xz, fx), j2 = yz * fx, j3 = -zf, j5 = xz * zf;
            const double k0 = fma(yg, yz, fy), k1 = -(xz * yg), k2 = -(xz * fy), k4 = -zg, k5 = yz * zg;
            const double s = rho1 * w;
            const double J[6] = {j0, j1, j2, j3, 0.0, j5}, K[6] = {k0, k1, k2, 0.0, k4, k5};
            const double sJ[6] = {s * j0, s * j1, s * j2, s * j3, 0.0, s * j5}, sK[6] = {s * k0, s * k1, s * k2, 0.0, s * k4, s * k5};
#pragma unroll
            for (int a = 0; a < 6; a++)
#pragma unroll
                for (int cc = a; cc < 6; cc++) {   // (the structural zeros are compile-time: their products are never formed)
                    double v = acc[tri(a, cc)];
                    if (a != 4 && cc != 4) v = fma(sJ[a], J[cc], v);
                    if (a != 3 && cc != 3) v = fma(sK[a], K[cc], v);
                    acc[tri(a, cc)] = v;
                }
#pragma unroll
            for (int a = 0; a < 6; a++) {
                double v = acc[21 + a];
                if (a != 4) v = fma(-sJ[a], ex, v);
                if (a != 3) v = fma(-sK[a], ey, v);
                acc[21 + a] = v;
            }
            if constexpr (STEREO) {
                if (st) {
                    // third Jacobian row (typesg2o.h:563-568): row 0 with the bf terms; l[2], l[3] = j[2], j[3]; l[4] = 0
                    const double bi = bf * invz;
                    const double L[6] = {j0 - bi * yz, j1 + bi * xz, j2, j3, 0.0, j5 - bi * invz};
                    const double sL[6] = {s * L[0], s * L[1], s * L[2], s * L[3], 0.0, s * L[5]};
#pragma unroll
                    for (int a = 0; a < 6; a++)
#pragma unroll
                        for (int cc = a; cc < 6; cc++)
                            if (a != 4 && cc != 4) acc[tri(a, cc)] = fma(sL[a], L[cc], acc[tri(a, cc)]);
#pragma unroll
                    for (int a = 0; a < 6; a++)
                        if (a != 4) acc[21 + a] = fma(-sL[a], er, acc[21 + a]);
                }
            }
        }
        int off = 0, real = kNS;
        WaveTransposeValu<kNS, 32>::run(acc, lane, off, real);   // lane l ends with the wave total of one value index
        if (real >= 1) s_part[wv * 32 + off] = acc[0];
    };
    // The markers of a pass, taken before its matches (no sum is live yet; the poses are read from LDS): a wave linearises its markers (mk_first,
    // mk_first + 8, ...); lane = 4 * pattern + corner (52 of the 64 lanes), the twelve perturbed errors of a corner are gathered into its lane
    // 0..3, which parks the two Jacobian rows in the marker's record; lane l < 28 then forms the marker's share of sum l — J^T rho1 J (21),
    // -J^T rho1 e (6), rho[0] (the information is the identity) — and the wave leaves its markers' shares in s_mkpart, where wave 0 adds
    // them to the totals of the pass.
    auto marker_linearise = [&](bool classify, bool drop_robust) __attribute__((noinline)) {
        if (mk_first >= nmk) return;
        int ja = 0, jc = lane;
        while (jc >= 6 - ja && ja < 6) { jc -= 6 - ja; ja++; }   // lane < 21: entry (ja, ja + jc) of the upper triangle; 21..26: b[lane - 21]
        jc += ja;
        double share = 0;
        for (int mi = mk_first; mi < nmk; mi += kPnpWaves) {
            MarkerRec& m = s_mk[mi];
            int robust = m.robust;
            if (classify) {
                // pnpsolver.cpp:376-380: computeError() at the pose the round ended with (the vertex's estimate), the kernel
                // dropped for good above Chi8D or from the third round on; never excluded, never counted
                const double c = marker_chi2(m, s_pose[1]);
                if (c > (double)15.507f || drop_robust) robust = 0;
                if (lane == 0) m.robust = robust;
            }
            const int k = lane < 52 ? lane >> 2 : 0, cn = lane & 3;
            double ex, ey;
            marker_err(m, cn, k, s_pose[0], ex, ey);
#pragma unroll
            for (int d = 0; d < 6; d++) {
                const int lp = (1 + d) * 4 + cn, lm = (7 + d) * 4 + cn;
                const double jx = mk_scalar * (__shfl(ex, lp) - __shfl(ex, lm)), jy = mk_scalar * (__shfl(ey, lp) - __shfl(ey, lm));
                if (lane < 4) { m.J[2 * cn][d] = jx; m.J[2 * cn + 1][d] = jy; }
            }
            double c = fma(ex, ex, ey * ey);   // (lanes 0..3: the unperturbed errors)
            c += __shfl_xor(c, 1);
            c += __shfl_xor(c, 2);
            if (lane < 4) { m.e[2 * cn] = ex; m.e[2 * cn + 1] = ey; }
            if (lane == 0) {
                double rho1 = 1.0, rc = c;
                if (robust) {
                    rc = marker_rho0(c);
                    if (!(c <= dsqr8)) rho1 = delta8 / sqrt(c);
                }
                m.rho1 = rho1; m.rc = rc;
            }
            // (written by this wave: its LDS operations complete in order)
            double v = 0;
            if (lane < 21) {
#pragma unroll
                for (int r = 0; r < 8; r++) v = fma(m.J[r][ja], m.J[r][jc], v);
                v *= m.rho1;
            } else if (lane < 27) {
#pragma unroll
                for (int r = 0; r < 8; r++) v = fma(m.J[r][lane - 21], m.e[r], v);
                v *= -m.rho1;
            } else if (lane == 27) v = m.rc;
            share += v;
        }
        if (lane < 32) s_mkpart[wv * 32 + lane] = share;
    };
    // what a pass does is published by wave 0 through s_ctl / s_pose before barrier A
    auto run_published_pass = [&]() -> int {
        const int mode = s_ctl[0];
        if (mode == kModeExit) return mode;
        if constexpr (MARKERS) { if (mode != kModeClassify) marker_linearise(s_ctl[1] != 0, s_ctl[2] != 0); }
        double RtA[12];
#pragma unroll
        for (int i = 0; i < 12; i++) RtA[i] = s_pose[0][i];
        pass(mode != kModeClassify, RtA, s_ctl[1] != 0, s_ctl[2] != 0);
        return mode;
    };

    // ---- the damping ladder.  When a trial is rejected, Levenberg multiplies lambda by ni, doubles ni and tries again from the SAME
    // pose and normal equations, up to ten times — at convergence (rho < 0 by rounding noise) it walks the whole ladder, which as
    // dependent passes is most of a solve.  The candidates do not depend on each other's outcome, only the DECISION is sequential:
    // wave w solves and applies candidates w, w + 8 (every wave the same bits as the sequential loop would produce), one pass
    // evaluates the robust chi2 of all of them, wave 0 then walks the decisions in order and stops where the loop would have.
    auto solve_candidates = [&]() {
        const int K = s_ctl[3];
        for (int k = wv; k < K; k += kPnpWaves) {
            double lam = s_lad[0], nn = s_lad[1];
            for (int j = 0; j < k; j++) { lam *= nn; nn *= 2; }
            double Hu[21], b[6], Tt[12], xs[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 21; i++) Hu[i] = s_H[i];
#pragma unroll
            for (int i = 0; i < 6; i++) b[i] = s_H[21 + i];
#pragma unroll
            for (int i = 0; i < 12; i++) Tt[i] = s_pose[0][i];
            const bool ok = p_solve6(Hu, b, lam, xs);
            if (ok) p_oplus_rt(Tt, xs);
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 12; i++) s_cand[k][i] = Tt[i];
#pragma unroll
                for (int i = 0; i < 6; i++) s_cand[k][12 + i] = xs[i];
                s_cand[k][18] = ok ? 1.0 : 0.0;
            }
        }
    };
    auto ladder_pass = [&]() {
        const int K = s_ctl[3];
        double chi[kLadderMax];
#pragma unroll
        for (int k = 0; k < kLadderMax; k++) {
            chi[k] = 0;
            if (k < K) {
                double Rt[12];
#pragma unroll
                for (int i = 0; i < 12; i++) Rt[i] = s_cand[k][i];
                for (int e = tid; e < n; e += kPnpThreads) {
                    const MatchRec m = rec[e];
                    if (!(m.flags & kActive)) continue;
                    double ex, ey, er, xz, yz, invz, rho1;
                    bool st = false;
                    if constexpr (STEREO) st = (m.flags & kStereo) != 0;
                    const double c = edge(m, st, st ? urs[e] : 0.f, Rt, ex, ey, er, xz, yz, invz);   // (kp_ur read only for a stereo match: read for every match, a stereo pass costs 1-2 % more clocks)
                    double rc = c;
                    if (m.flags & kRobust) rc = robust(m, st, c, rho1);
                    chi[k] += rc;
                }
            }
        }
        if constexpr (MARKERS) {
            // the wave's markers at ALL candidates at once: lane = 4 * candidate + corner (32 lanes), the candidate's pose read from LDS
            const int kk = lane >> 2;
            for (int mi = mk_first; mi < nmk; mi += kPnpWaves) {
                const MarkerRec& m = s_mk[mi];
                const double c = marker_chi2(m, s_cand[kk < K ? kk : 0]);
                const double rc = m.robust ? marker_rho0(c) : c;
#pragma unroll
                for (int k = 0; k < kLadderMax; k++)
                    if (k < K && lane == 4 * k) chi[k] += rc;
            }
        }
        int off = 0, real = kLadderMax;
        WaveTransposeValu<kLadderMax, 32>::run(chi, lane, off, real);
        if (real >= 1) s_part[wv * 32 + off] = chi[0];
    };

    if (wv != 0) {
        // ---- the seven worker waves: evaluate what wave 0 publishes until it says stop
        for (;;) {
            __syncthreads();                    // A: the request is in LDS
            if (s_ctl[0] == kModeLadder) {
                solve_candidates();
                __syncthreads();                // A2: the candidates' poses are in LDS
                ladder_pass();
            } else {
                const int mode = run_published_pass();
                if (mode == kModeExit) break;
            }
            __syncthreads();                    // B: the partial sums are in LDS
        }
    } else {
        // ---- wave 0: g2o's SparseOptimizer::optimize + OptimizationAlgorithmLevenberg::solve as a state machine whose every
        // transition is ONE pass (or one damping-ladder pass) over the matches: a single call site for the pass keeps the code and
        // the register allocation of this wave small.  The control flow is the reference's, statement for statement:
        //   for round < 4 { T = T0; [classify previous round]; linearise;                         -> ST_INIT
        //     for it < 10 { swap(prev, cur); qmax = 0;
        //        do { solve; oplus; chi2 of the trial; accept / reject; } while (rho < 0 && ++qmax < 10)   -> ST_TRIAL, then ST_LADDER
        //        (a pose accepted inside a ladder pass is linearised by ST_RELIN before the next solve)
        //        stop on terminate or when the float chi2 no longer decreases }
        //   } classify the last round                                                               -> ST_FINAL
        enum : int { ST_INIT, ST_RELIN, ST_TRIAL, ST_LADDER, ST_FINAL, ST_DONE };
        int st = (MARKERS || n > 0) ? ST_INIT : ST_DONE;
        // measurement (A.clk != NULL only): cycles of wave 0 by section of a plain pass — [16] request prepared (solve + update), [17] barrier A,
        // [18] its share of the matches + butterfly, [19] barrier B, [20] totals + decision; [21] ladder passes as a whole
        long long ph[6] = {0, 0, 0, 0, 0, 0}, tp = A.clk ? (long long)__builtin_readcyclecounter() : 0;
        auto stamp = [&](int i) { if (A.clk) { const long long t = (long long)__builtin_readcyclecounter(); ph[i] += t - tp; tp = t; } };
        int n_pass = 0, round = 0, it = 0, qmax = 0, done = 0, last_round = -1, good = n;
        bool stale_H = false, lam_finite = true, ok2 = false;
        double lambda = 0, ni = 2, currentChi = 0, lastChiRaw = 0, rho = 0, scale = 1;
        float prevChi = FLT_MAX, curChi = FLT_MAX;
        // (the pose and the last solved step live in LDS, s_T / s_x: nothing but scalars stays in registers across a pass.  A failed
        // factorisation leaves the step as it was — g2o's solution vector does the same)
        if (lane < 8) s_x[lane] = 0;

        auto iter_begin = [&]() {
            const float t = prevChi; prevChi = curChi; curChi = t;   // swap(prevChi2, curChi2) at loop entry
            qmax = 0; rho = 0; lam_finite = true;
            st = stale_H ? ST_RELIN : ST_TRIAL;
        };
        auto round_end = [&]() {
            if (lane < 12) s_pose[1][lane] = s_T[lane];
            if (lane == 0) A.result[1 + round] = done;
            last_round = round;
            ++round;
            st = round < 4 ? ST_INIT : ST_FINAL;
        };
        auto after_trials = [&]() {          // the do-while of Levenberg's solve() has just evaluated a trial
            if (lam_finite && rho < 0 && qmax < 10) { st = ST_LADDER; return; }
            done++;
            const bool terminate = (qmax == 10 || rho == 0 || !isfinite(lambda));
            curChi = (float)lastChiRaw;
            const float diff = prevChi - curChi;
            if (terminate || !(diff > 0.f) || it + 1 >= 10) round_end();
            else { ++it; iter_begin(); }
        };
        auto decide = [&](bool ok, double chi, const double* pose_lds) -> bool {   // one accept / reject decision (lambda, ni, currentChi, T)
            lastChiRaw = chi;
            const double tempChi = ok ? chi : DBL_MAX;
            const double r = (currentChi - tempChi) / scale;
            const bool acc = r > 0 && isfinite(tempChi);
            if (acc) {
                const double t3 = 2 * r - 1;
                double alpha = 1. - t3 * t3 * t3;
                alpha = fmin(alpha, 2. / 3.);
                lambda *= fmax(1. / 3., alpha);
                ni = 2;
                currentChi = tempChi;
                if (lane < 12) s_T[lane] = pose_lds[lane];
            } else {
                lambda *= ni; ni *= 2;                          // T and the normal equations stay those of the last accepted pose
                if (!isfinite(lambda)) lam_finite = false;
            }
            rho = r;
            return acc;
        };

        while (st != ST_DONE) {
            if (st == ST_LADDER) {
                // ---- rejected: the rest of the damping ladder in one pass
                const int K = 10 - qmax < kLadderMax ? 10 - qmax : kLadderMax;
                if (lane < 12) s_pose[0][lane] = s_T[lane];
                if (lane == 0) {
                    s_ctl[0] = kModeLadder; s_ctl[3] = K;
                    s_lad[0] = lambda; s_lad[1] = ni;
                }
                __syncthreads();                // A
                solve_candidates();
                __syncthreads();                // A2
                ladder_pass();
                __syncthreads();                // B
                ++n_pass;
                if (lane < kLadderMax) {
                    double mine = s_part[lane];
#pragma unroll
                    for (int w2 = 1; w2 < kPnpWaves; w2++) mine += s_part[w2 * 32 + lane];   // wave order
                    s_tot[lane] = mine;
                }
                double bb[6], x[6];
#pragma unroll
                for (int i = 0; i < 6; i++) { bb[i] = s_H[21 + i]; x[i] = s_x[i]; }
                int k_last = 0;
                for (int k = 0; k < K; k++) {   // the decisions, in the order the sequential loop takes them
                    const bool okk = s_cand[k][18] != 0.0;
                    if (okk) {
#pragma unroll
                        for (int i = 0; i < 6; i++) x[i] = s_cand[k][12 + i];
                    }
                    double sc = 0;
#pragma unroll
                    for (int i = 0; i < 6; i++) sc += x[i] * (lambda * x[i] + bb[i]);
                    scale = 1e-3 + sc;
                    k_last = k;
                    if (decide(okk, s_tot[k], s_cand[k])) stale_H = true;   // (a ladder pass does not linearise)
                    if (!lam_finite) break;   // the reference leaves its loop before the increment when lambda overflows
                    qmax++;
                    if (!(rho < 0 && qmax < 10)) break;
                }
                if (lane < 12) s_pose[2][lane] = s_cand[k_last][lane];   // the edges keep the errors of the last trial the loop evaluated
                if (lane == 0) {
#pragma unroll
                    for (int i = 0; i < 6; i++) s_x[i] = x[i];
                }
                after_trials();
                stamp(5);
                continue;
            }
            // ---- the request of this state
            int mode = kModeEval;
            bool classify = false, drop = false;
            if (st == ST_INIT) {
                if (lane < 12) { s_T[lane] = s_pose[3][lane]; s_pose[0][lane] = s_pose[3][lane]; }   // every round restarts from the input pose (:354)
                classify = round > 0; drop = round - 1 >= 2;
            } else if (st == ST_RELIN) {
                if (lane < 12) s_pose[0][lane] = s_T[lane];
            } else if (st == ST_TRIAL) {
                double Tt[12], x[6], Hu[21], b[6];
#pragma unroll
                for (int i = 0; i < 12; i++) Tt[i] = s_T[i];
#pragma unroll
                for (int i = 0; i < 6; i++) x[i] = s_x[i];
#pragma unroll
                for (int i = 0; i < 21; i++) Hu[i] = s_H[i];
#pragma unroll
                for (int i = 0; i < 6; i++) b[i] = s_H[21 + i];
                ok2 = p_solve6(Hu, b, lambda, x);
                if (ok2) p_oplus_rt(Tt, x);
                double sc = 0;
#pragma unroll
                for (int i = 0; i < 6; i++) sc += x[i] * (lambda * x[i] + b[i]);
                scale = 1e-3 + sc;
                if (lane == 0) {
#pragma unroll
                    for (int i = 0; i < 12; i++) s_pose[0][i] = Tt[i];
#pragma unroll
                    for (int i = 0; i < 6; i++) s_x[i] = x[i];
                }
            } else if (st == ST_FINAL) {
                mode = kModeClassify; classify = true; drop = last_round >= 2;
            }
            if (lane == 0) { s_ctl[0] = mode; s_ctl[1] = classify ? 1 : 0; s_ctl[2] = drop ? 1 : 0; }
            stamp(0);
            __syncthreads();                    // A
            stamp(1);
            run_published_pass();
            stamp(2);
            __syncthreads();                    // B
            stamp(3);
            ++n_pass;
            if (lane < kNS) {
                double mine = s_part[lane];
#pragma unroll
                for (int w2 = 1; w2 < kPnpWaves; w2++) mine += s_part[w2 * 32 + lane];   // wave order
                if constexpr (MARKERS) {
                    if (mode == kModeEval)
                        for (int j = 0; j < nmk && j < kPnpWaves; j++) mine += s_mkpart[(kPnpWaves - 1 - j) * 32 + lane];   // marker order
                }
                s_tot[lane] = mine;
            }
            if (mode == kModeEval && lane < 12) s_pose[2][lane] = s_pose[0][lane];   // the pose the edges' errors now belong to
            // (the same wave wrote s_tot: LDS operations of one wave complete in order)
            const double chi_sum = s_tot[27], good_sum = s_tot[28];
            if (st == ST_INIT) {
                if (round > 0) {
                    good = (int)good_sum;
                    if constexpr (!MARKERS) {   // pnpsolver.cpp:383: the stop below ten good matches applies only without markers
                        if (good < 10) { st = ST_DONE; continue; }
                    }
                }
                if (lane < 27) s_H[lane] = s_tot[lane];          // the totals of the pass are the normal equations of the pose it evaluated
                currentChi = chi_sum; lastChiRaw = chi_sum; ni = 2;
                {
                    double m = 0;
#pragma unroll
                    for (int j = 0; j < 6; j++) {   // computeLambdaInit's std::max(fabs(h), m): a NaN diagonal entry is kept unless a number follows it
                        const double h = fabs(s_H[tri(j, j)]);
                        m = h < m ? m : h;
                    }
                    lambda = 1e-5 * m;
                }
                prevChi = FLT_MAX; curChi = FLT_MAX; done = 0; stale_H = false; it = 0;
                iter_begin();
            } else if (st == ST_RELIN) {
                if (lane < 27) s_H[lane] = s_tot[lane];
                stale_H = false;
                st = ST_TRIAL;
            } else if (st == ST_TRIAL) {
                if (decide(ok2, chi_sum, s_pose[0])) { if (lane < 27) s_H[lane] = s_tot[lane]; }   // the pass has linearised at the accepted pose already
                if (lam_finite) qmax++;   // (the reference leaves its loop before the increment when lambda overflows)
                after_trials();
            } else {   // ST_FINAL: the classification that ends the last round
                good = (int)good_sum;
                st = ST_DONE;
            }
            stamp(4);
        }
        if (A.clk && lane == 0) { for (int i = 0; i < 6; i++) A.clk[16 + i] = ph[i]; }
        if (A.clk && lane == 0) A.clk[2] = __builtin_readcyclecounter();
        if (lane == 0) {
            s_ctl[0] = kModeExit;
            for (int r = last_round + 1; r < 4; r++) A.result[1 + r] = 0;
            A.result[0] = n > 0 ? good : 0;
            double Tend[12];
#pragma unroll
            for (int i = 0; i < 12; i++) Tend[i] = s_pose[1][i];
            float M[16];   // the pose this solve returns: pose_out, and what the tracker's decision reads
            for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) M[r * 4 + c] = (float)Tend[r * 3 + c]; M[r * 4 + 3] = (float)Tend[9 + r]; }
            M[12] = M[13] = M[14] = 0.f; M[15] = 1.f;
            for (int i = 0; i < 16; i++) A.pose_out[i] = M[i];
            if (A.dec.dyn17) pnp_decide(A, n > 0 ? good : 0, M);
            if (A.state_out) {
                double q[4];
                quat_from_R(Tend, q);
                quat_norm_pos(q);
                for (int i = 0; i < 4; i++) A.state_out[i] = q[i];
                for (int i = 0; i < 3; i++) A.state_out[4 + i] = Tend[9 + i];
            }
            if (A.clk) A.clk[4] = n_pass;
        }
        __syncthreads();                        // A of the exit request
    }
    for (int e = tid; e < n; e += kPnpThreads) A.bad_out[e] = (rec[e].flags & kBad) ? 1 : 0;
    if (A.host_done) {   // results went to pinned host memory: make them visible, then post the completion word
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        __syncthreads();
        if (tid == 0) __hip_atomic_store(A.host_done, A.done_word, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (A.clk && tid == 0) A.clk[3] = __builtin_readcyclecounter();
