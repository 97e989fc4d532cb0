// Host code of ba.hip under a sanitizer, without a GPU (nothing is launched; arrays behind the arena's pinned prefix are not copied):
//   plan_ba() for 0 .. 70 free keyframes, with and without three-row edges, against the table tests/het_ba_synth.py restates
//   (planned_form, dense_wide_nown), one line per window;
//   the SSE and AVX-512 observation packers against the scalar records: odd E, E < 8, an inexact inv_sigma, an index out of range;
//   quat_from_R / quat_norm_pos / quat_to_R on the host, one rotation per branch;
//   carve_arena() against the take sequence the arena had before it existed: every pointer, the prefix length, the arena size and
//   the bytes of the pinned prefix, on twelve problems (chain with each Schur kernel, stereo, wide, no free keyframe, no landmark).
//   This last part (carve() below) is a MIGRATION check: it holds the arena order a second time, as it stood before carve_arena, to
//   show the move changed nothing.  It is to be deleted with the first intended layout change, not kept in step with it.
// Not run by the test suite (it compiles ba.hip: most of a minute); run it by hand when plan_ba, the packers or the table in
// tests/het_ba_synth.py change.
// Build and run from the repository root (exit status 0 and "ALL OK"):
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -ffp-contract=off -fno-fast-math -Wno-unused-variable -x hip \
//         -Xarch_host -fsanitize=address,undefined scripts/ba_host_check.cpp -o /tmp/ba_host_check && /tmp/ba_host_check
#include "../ucoslam-cv3_amd/csrc/ba.hip"
#include <cstdio>
#include <random>
namespace uh { void set_error(const char*, ...) {} }
extern "C" const char* uh_last_error(void) { return ""; }
static const char* form_name(const BAPlan& p) { return p.form == kFormWide ? "wide" : p.form == kFormChain ? "chain" : (p.ps.NF == 8 ? "persist8" : "persist16"); }
static const char* planned_form(int nfree, bool stereo) { if (nfree > 64) return "wide"; if (stereo || nfree > 16) return "chain"; return nfree <= 8 ? "persist8" : "persist16"; }
static int dense_wide_nown(int nfree) { int ntt = (6 * nfree + 15) / 16, T = ntt * (ntt + 1) / 2, SP = (T + 79) / 80, need = (((T + SP - 1) / SP) + 3) / 4; return need <= 12 ? 12 : need <= 16 ? 16 : 20; }
static int plan_and_packers() {
    BAKnobs kn; BALimits lim{256, 160 * 1024, 4384};
    int bad = 0;
    for (int stereo = 0; stereo < 2; stereo++)
        for (int nfree = 0; nfree <= 70; nfree++) {
            BAPlanIn in{nfree + 2, 200, 1500, nfree, stereo != 0, true};
            const BAPlan p = plan_ba(in, kn, lim);
            const char* want = nfree == 0 ? "chain" : planned_form(nfree, stereo);
            if (std::string(want) != form_name(p)) { printf("MISMATCH nfree %d stereo %d: %s vs %s\n", nfree, stereo, form_name(p), want); bad++; }
            if (p.form == kFormChain && nfree > 32 && p.sd.nown != dense_wide_nown(nfree)) { printf("nown mismatch %d\n", nfree); bad++; }
            if (!stereo) printf("nfree %2d %-9s schur %d nsplit %2d solve %d pre %d asm %d ns %d/%d lds %zu/%zu G %d SP %d nown %d\n", nfree, form_name(p), p.schur, p.nsplit, p.solve, p.pre_mode, (int)p.assemble_pairs, p.ns_backsub, p.ns_solve, p.lds_schur, p.lds_solve, p.sd.G, p.sd.SP, p.sd.nown);
        }
    // packers
    std::mt19937 rng(1);
    for (int E : {0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 1001}) for (int inexact = 0; inexact < 2; inexact++) {
        const int P = 500, K = 20;
        std::vector<int32_t> pt(E), kf(E); std::vector<float> uv(2 * E); std::vector<double> w(E);
        for (int e = 0; e < E; e++) { pt[e] = rng() % P; kf[e] = rng() % K; uv[2 * e] = (rng() % 10000) / 7.f; uv[2 * e + 1] = (rng() % 10000) / 3.f; w[e] = (double)(float)(1.0 / (1 + rng() % 8)); }
        if (inexact && E) w[E - 1] = 1.0 / 3.0;
        uh_ba_problem pr{}; pr.n_frames = K; pr.n_points = P; pr.n_obs = E; pr.obs_point = pt.data(); pr.obs_frame = kf.data(); pr.obs_uv = uv.data(); pr.obs_inv_sigma = w.data();
        for (int avx = 0; avx < 2; avx++) {
            if (avx && !host_has_avx512()) continue;
            std::vector<uh_ba_obs> o16(E + 1), o24(E + 1);
            bool exact = true; unsigned oob = 0;
            pack_obs(&pr, 0, E, true, avx, o16.data(), exact, oob);
            bool e2 = true; pack_obs(&pr, 0, E, false, avx, o24.data(), e2, oob);
            if (oob) { printf("oob set\n"); bad++; }
            if (exact != !(inexact && E)) { printf("exact flag wrong E %d inexact %d avx %d\n", E, inexact, avx); bad++; }
            const unsigned char* r = reinterpret_cast<const unsigned char*>(o16.data());
            for (int e = 0; e < E; e++) {
                unsigned pk; float f[3]; memcpy(&pk, r + 16 * e, 4); memcpy(f, r + 16 * e + 4, 12);
                if ((int)(pk & 0xFFFFFF) != pt[e] || (int)(pk >> 24) != kf[e] || f[0] != uv[2 * e] || f[1] != uv[2 * e + 1] || f[2] != (float)w[e]) { printf("rec16 %d bad\n", e); bad++; break; }
                if (o24[e].point != pt[e] || o24[e].frame != kf[e] || o24[e].u != uv[2 * e] || o24[e].v != uv[2 * e + 1] || o24[e].inv_sigma != w[e]) { printf("rec24 %d bad\n", e); bad++; break; }
            }
        }
        if (E) { pt[E / 2] = P; std::vector<uh_ba_obs> o(E + 1); bool ex = true; unsigned oob = 0; pack_obs(&pr, 0, E, true, false, o.data(), ex, oob); unsigned oob2 = 0; pack_obs(&pr, 0, E, false, false, o.data(), ex, oob2); if (!oob || !oob2) { printf("oob missed E %d\n", E); bad++; } }
    }
    // snapshot: quaternion of a rotation in each of the four branches, back to R
    const double qs[4][4] = {{0.1, 0.2, 0.3, 0.9}, {0.9, 0.1, 0.2, 0.05}, {0.1, 0.9, 0.2, 0.05}, {0.1, 0.2, 0.9, 0.05}};
    for (auto& q0 : qs) {
        double q[4] = {q0[0], q0[1], q0[2], q0[3]}, R[9], q2[4], R2[9];
        quat_norm_pos(q); quat_to_R(q, R); quat_from_R(R, q2); quat_norm_pos(q2); quat_to_R(q2, R2);
        for (int i = 0; i < 9; i++) if (std::fabs(R[i] - R2[i]) > 1e-14) { printf("quat round trip\n"); bad++; break; }
    }
    return bad;
}
static int bad = 0;
#define CHECK(ptr, off) do { if ((const char*)(ptr) - base != (long long)(off)) { printf("  MISMATCH %s: %lld vs %zu\n", #ptr, (long long)((const char*)(ptr) - base), (size_t)(off)); bad++; } } while (0)
static void one(int K, int nfixed, int P, int per_pt, bool stereo, bool force_wide, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<float> poses(16 * K, 0.f), intr(4 * K, 500.f), pts(3 * P, 1.f);
    for (int k = 0; k < K; k++) { float* M = &poses[16 * k]; M[0] = M[5] = M[10] = M[15] = 1; M[3] = 0.1f * k; }
    std::vector<unsigned char> fixed(K, 0); for (int k = 0; k < nfixed; k++) fixed[k] = 1;
    std::vector<int32_t> op, of; std::vector<float> uv; std::vector<double> w;
    for (int p = 0; p < P; p++) { std::vector<int> ks(K); for (int k = 0; k < K; k++) ks[k] = k; std::shuffle(ks.begin(), ks.end(), rng);
        for (int j = 0; j < std::min(per_pt, K); j++) { op.push_back(p); of.push_back(ks[j]); uv.push_back(1.f); uv.push_back(2.f); w.push_back(1.0); } }
    const int E = (int)op.size(), nfree = K - nfixed;
    uh_ba_problem pr{}; pr.n_frames = K; pr.n_points = P; pr.n_obs = E; pr.poses_f2g = poses.data(); pr.fixed = fixed.data(); pr.intr = intr.data(); pr.points = pts.data();
    pr.obs_point = op.data(); pr.obs_frame = of.data(); pr.obs_uv = uv.data(); pr.obs_inv_sigma = w.data();
    uh_ba* b = new uh_ba();
    b->knobs.wide = force_wide;
    b->lim = BALimits{256, 160 * 1024, 1552};
    b->plan = plan_ba(BAPlanIn{K, P, E, nfree, stereo, false}, b->knobs, b->lim);
    const bool wide = b->plan.form == kFormWide;
    StereoIn sinv; sinv.ur.assign(E, 0.0); sinv.bf.assign(E, 0.0); sinv.st.assign(E, 1);
    const StereoIn* sin = stereo ? &sinv : nullptr;
    BAGraph g; WideLists wl; BASnapshot s;
    if (build_graph(&pr, wide, g)) { printf("graph failed\n"); bad++; return; }
    if (wide && build_wide_lists(&pr, g, wl)) { printf("wide failed\n"); bad++; return; }
    build_snapshot(&pr, s);
    fill_dims(b, K, P, E, nfree);
    ArenaCarver sizes; ArenaTables t; carve_arena(sizes, t, b->dims, b->plan, &pr, g, wl, s, sin);
    std::vector<char> arena(sizes.A.off + 256), pin(sizes.prefix + 256, 0x55);
    ArenaCarver c; c.dry = false; c.base = arena.data(); c.pin = pin.data(); c.prefix = sizes.prefix;
    carve_arena(c, t, b->dims, b->plan, &pr, g, wl, s, sin);   // (arrays behind the prefix: hipMemcpyAsync fails without a device — c.rc, not looked at)
    const char* base = arena.data();
    // ---- the layout as set_problem_tables spelled it before carve_arena (commit 88a8c31): one take per array, in this order
    const BADims& d = b->dims;
    const std::vector<int>&cam_edges = g.cam_edges, &edge_of = g.edge_of, &w_pair_s1 = wl.pair_s1, &w_item_pair = wl.item_pair, &w_tri_pt = wl.tri_pt;
    const bool dense = b->plan.schur != kSchurPair; const SchurDense& sd = b->plan.sd; const int nsplit = b->plan.nsplit;
    uh::Layout A;
    const size_t o_pt_ptr = A.take<int>(P + 1), o_pt_edges = A.take<int>(E), o_cam_ptr = A.take<int>(nfree + 1), o_cam_edges = A.take<int>(cam_edges.size());
    const size_t o_e_pt = A.take<int>(E), o_e_kf = A.take<int>(E), o_uv = A.take<double>(2 * (size_t)E), o_w = A.take<double>(E);
    const size_t o_slot = A.take<int>(K), o_free = A.take<int>(std::max(nfree, 1)), o_intr = A.take<double>(4 * (size_t)K), o_edge_of = A.take<int>(edge_of.size());
    const size_t o_ur = sin ? A.take<double>(E) : 0, o_bf = sin ? A.take<double>(E) : 0, o_est = sin ? A.take<unsigned char>(E) : 0;   // (inside the pinned prefix)
    const size_t o_pose0 = A.take<double>(7 * (size_t)K), o_pts0 = A.take<double>(3 * (size_t)P);
    size_t o_pose[2], o_poseR[2], o_pts[2];
    for (int i = 0; i < 2; i++) { o_pose[i] = A.take<double>(7 * (size_t)K); o_poseR[i] = A.take<double>(12 * (size_t)K); o_pts[i] = A.take<double>(3 * (size_t)P); }
    const size_t o_act = A.take<unsigned char>(E), o_rob = A.take<unsigned char>(E), o_err = A.take<double>(2 * (size_t)E), o_chi2 = A.take<double>(E);
    size_t o_Hll[2], o_bl[2], o_Hpl[2];
    for (int i = 0; i < 2; i++) { o_Hll[i] = A.take<double>(9 * (size_t)P); o_bl[i] = A.take<double>(3 * (size_t)P); o_Hpl[i] = A.take<double>(18 * (size_t)E); }
    const size_t o_Hpp = A.take<double>(27 * (size_t)kCamChunks * std::max(nfree, 1)), o_bp = A.take<double>(std::max(d.n, 1));
    const int npairs_h = nfree * (nfree + 1) / 2;
    const size_t o_dpart = A.take<double>(dense ? (size_t)sd.G * sd.T * 256 : 1), o_dbpart = A.take<double>(dense ? (size_t)sd.G * 16 * sd.ntt : 1);
    const size_t o_S = A.take<double>((size_t)(d.n + 1) * (d.n + 1)), o_Sp = A.take<double>(wide ? 42 : (size_t)nsplit * std::max(npairs_h, 1) * 42), o_xp = A.take<double>(std::max(d.n, 1));
    const size_t wn_pairs = w_pair_s1.size(), wn_items = w_item_pair.size(), wn_tri = w_tri_pt.size();
    const size_t o_wps1 = A.take<int>(wn_pairs + 1), o_wps2 = A.take<int>(wn_pairs + 1), o_wpip = A.take<int>(wn_pairs + 2);
    const size_t o_wip = A.take<int>(wn_items + 1), o_wib = A.take<int>(wn_items + 1), o_wic = A.take<int>(wn_items + 1);
    const size_t o_wtp = A.take<int>(wn_tri + 1), o_wt1 = A.take<int>(wn_tri + 1), o_wt2 = A.take<int>(wn_tri + 1);
    const size_t o_wpart = A.take<double>((wn_items + 1) * 42), o_wY = A.take<double>(wide ? (size_t)(d.n + 1) * kWNB : 1), o_wfail = A.take<int>(4);
    const size_t o_plc = A.take<double>(d.nPointBlocks), o_pmd = A.take<double>(d.nPointBlocks), o_pc = A.take<double>(d.nPointBlocks), o_ps = A.take<double>(d.nPointBlocks);
    const size_t o_st = A.take<BAState>(2), o_clk = A.take<long long>(64);
    const size_t prefix_bytes = o_pts0 + 3 * (size_t)P * sizeof(double);
    // ---- compare
    const int before = bad;
    if (A.off != sizes.A.off || A.off != c.A.off) { printf("  total %zu vs %zu\n", sizes.A.off, A.off); bad++; }
    if (prefix_bytes != sizes.prefix) { printf("  prefix %zu vs %zu\n", sizes.prefix, prefix_bytes); bad++; }
    const BAPtrs& p = t.p; const BAWide& W = t.W;
    CHECK(p.pt_ptr, o_pt_ptr); CHECK(p.pt_edges, o_pt_edges); CHECK(p.cam_ptr, o_cam_ptr); CHECK(p.cam_edges, o_cam_edges);
    CHECK(p.e_pt, o_e_pt); CHECK(p.e_kf, o_e_kf); CHECK(p.e_uv, o_uv); CHECK(p.e_w, o_w);
    CHECK(p.slot, o_slot); CHECK(p.free_kf, o_free); CHECK(p.intr, o_intr); CHECK(p.edge_of, o_edge_of);
    for (int i = 0; i < 2; i++) { CHECK(p.pose[i], o_pose[i]); CHECK(p.poseR[i], o_poseR[i]); CHECK(p.pts[i], o_pts[i]); CHECK(p.Hll[i], o_Hll[i]); CHECK(p.bl[i], o_bl[i]); CHECK(p.Hpl[i], o_Hpl[i]); }
    CHECK(p.e_active, o_act); CHECK(p.e_robust, o_rob); CHECK(p.e_err, o_err); CHECK(p.e_chi2, o_chi2);
    CHECK(p.HppPart, o_Hpp); CHECK(p.bp, o_bp); CHECK(p.S, o_S); CHECK(p.Spart, o_Sp); CHECK(p.xp, o_xp); CHECK(p.dpart, o_dpart); CHECK(p.dbpart, o_dbpart);
    CHECK(W.pair_s1, o_wps1); CHECK(W.pair_s2, o_wps2); CHECK(W.pair_item_ptr, o_wpip); CHECK(W.item_pair, o_wip); CHECK(W.item_begin, o_wib); CHECK(W.item_count, o_wic);
    CHECK(W.tri_pt, o_wtp); CHECK(W.tri_e1, o_wt1); CHECK(W.tri_e2, o_wt2); CHECK(W.Wpart, o_wpart); CHECK(W.S, o_S); CHECK(W.Y, o_wY); CHECK(W.fail, o_wfail);
    CHECK(p.part_lin_chi, o_plc); CHECK(p.part_maxdiag, o_pmd); CHECK(p.part_chi, o_pc); CHECK(p.part_scale, o_ps); CHECK(p.st, o_st); CHECK(p.clk, o_clk);
    CHECK(t.pose0, o_pose0); CHECK(t.pts0, o_pts0);
    if (sin) { CHECK(t.sx.e_ur, o_ur); CHECK(t.sx.e_bf, o_bf); CHECK(t.sx.e_st, o_est); }
    if (W.n_pairs != (int)wn_pairs || W.n_items != (int)wn_items || W.ld != d.n + 1) { printf("  wide counts\n"); bad++; }
    // the pinned prefix holds what the parent's up() calls put there
    auto same = [&](size_t off, const void* src, size_t bytes, const char* what) { if (bytes && memcmp(pin.data() + off, src, bytes)) { printf("  prefix content %s\n", what); bad++; } };
    same(o_pt_ptr, g.pt_ptr.data(), g.pt_ptr.size() * 4, "pt_ptr"); same(o_pt_edges, g.pt_edges.data(), g.pt_edges.size() * 4, "pt_edges"); same(o_cam_ptr, g.cam_ptr.data(), g.cam_ptr.size() * 4, "cam_ptr");
    same(o_cam_edges, g.cam_edges.data(), g.cam_edges.size() * 4, "cam_edges"); same(o_e_pt, pr.obs_point, (size_t)E * 4, "e_pt"); same(o_e_kf, pr.obs_frame, (size_t)E * 4, "e_kf");
    same(o_uv, s.uv.data(), s.uv.size() * 8, "uv"); same(o_w, s.w.data(), s.w.size() * 8, "w"); same(o_slot, g.slot.data(), g.slot.size() * 4, "slot"); same(o_free, g.free_kf.data(), g.free_kf.size() * 4, "free");
    same(o_intr, s.intr.data(), s.intr.size() * 8, "intr"); same(o_edge_of, g.edge_of.data(), g.edge_of.size() * 4, "edge_of"); same(o_pose0, s.pose0.data(), s.pose0.size() * 8, "pose0"); same(o_pts0, s.pts0.data(), s.pts0.size() * 8, "pts0");
    if (sin) { same(o_ur, sinv.ur.data(), (size_t)E * 8, "ur"); same(o_bf, sinv.bf.data(), (size_t)E * 8, "bf"); same(o_est, sinv.st.data(), (size_t)E, "est"); }
    printf("K %d nfree %d P %d E %d stereo %d form %d schur %d: arena %zu prefix %zu pairs %zu items %zu tri %zu %s\n", K, nfree, P, E, (int)stereo, b->plan.form, b->plan.schur, A.off, prefix_bytes, wn_pairs, wn_items, wn_tri, bad == before ? "EQUAL" : "DIFFERENT");
    delete b;
}
static int carve() {
    one(3, 2, 50, 3, false, false, 1); one(10, 2, 300, 5, false, false, 2); one(12, 2, 333, 6, true, false, 3); one(22, 2, 200, 7, false, false, 4); one(26, 2, 1000, 9, true, false, 5);
    one(42, 2, 777, 11, false, false, 6); one(66, 2, 129, 13, true, false, 7); one(67, 2, 500, 20, false, false, 8); one(70, 2, 2000, 40, true, false, 9); one(8, 2, 100, 4, false, true, 10);
    one(4, 4, 20, 2, false, false, 11); one(5, 1, 0, 0, false, false, 12);
    return bad;
}
int main() {
    const int n = plan_and_packers() + carve();
    printf("%s (%d)\n", n ? "FAILED" : "ALL OK", n);
    return n != 0;
}
