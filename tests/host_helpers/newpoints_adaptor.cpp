// The new-map-point adaptors (include/ucoslam_hip/adaptors.hpp: Triangulate, NewPointCreator) on toy frames: one new keyframe, three
// neighbours.  Without arguments: the host-side helpers (Se3Transform::inv, getCameraCenter) on a known pose; prints "newpoints host
// ok".  With a file name: runs NewPointCreator::create and Triangulate on the device and dumps the inputs the adaptor derived and its
// results for the Python side to repeat through the mirror (tests/test_newpoints_adaptor.py); prints "no device" and succeeds where
// there is none.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../include/ucoslam_hip/adaptors.hpp"
#include "toy_frames.hpp"

using namespace ucoslam_hip;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static std::array<float, 16> pose_of(double yaw, double cx, double cy, double cz) {   // global -> camera of a camera at (cx, cy, cz) turned about y
    const double c = std::cos(yaw), s = std::sin(yaw);
    const double R[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
    std::array<float, 16> M{};
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) M[4 * r + k] = (float)R[3 * r + k];
        M[4 * r + 3] = (float)-(R[3 * r] * cx + R[3 * r + 1] * cy + R[3 * r + 2] * cz);
    }
    M[15] = 1;
    return M;
}

static ToyPoint2f project(const ToyViewFrame& f, const double X[3]) {
    double c[3];
    for (int r = 0; r < 3; r++) c[r] = f.pose_f2g[4 * r] * X[0] + f.pose_f2g[4 * r + 1] * X[1] + f.pose_f2g[4 * r + 2] * X[2] + f.pose_f2g[4 * r + 3];
    return ToyPoint2f{(float)(f.imageParams.fx() * c[0] / c[2] + f.imageParams.cx()), (float)(f.imageParams.fy() * c[1] / c[2] + f.imageParams.cy())};
}

int main(int argc, char** argv) {
    {   // a quarter turn about y and a translation: the inverse and the centre by hand
        const float M[16] = {0, 0, 1, 1, 0, 1, 0, 2, -1, 0, 0, 3, 0, 0, 0, 1};
        float inv[16], c[3];
        se3_inverse(M, inv);
        camera_center(M, c);
        const float want[16] = {0, 0, -1, 3, 0, 1, 0, -2, 1, 0, 0, -1, 0, 0, 0, 1};
        for (int k = 0; k < 16; k++) REQUIRE(inv[k] == want[k]);
        REQUIRE(c[0] == 3.f && c[1] == -2.f && c[2] == -1.f);
        float P[16];
        mat44_product(M, inv, P);
        for (int k = 0; k < 16; k++) REQUIRE(P[k] == (k % 5 == 0 ? 1.f : 0.f));
    }
    std::printf("newpoints host ok\n");
    if (argc < 2) return 0;

    const int n_pts = 45, n_levels = 8;
    std::vector<float> sf(n_levels);
    for (int l = 0; l < n_levels; l++) sf[l] = l ? sf[l - 1] * 1.2f : 1.f;
    ToyViewFrame kf;
    kf.idx = 17; kf.pose_f2g = pose_of(0.03, 0.1, -0.05, 0.2); kf.scaleFactors = sf;
    std::vector<ToyViewFrame> nb(3);
    const double centres[3][3] = {{1.1, -0.05, 0.2}, {-0.8, 0.2, 0.1}, {0.1, 0.9, 0.35}};
    const uint32_t ids[3] = {4, 9, 2};
    for (int j = 0; j < 3; j++) { nb[j].idx = ids[j]; nb[j].pose_f2g = pose_of(0.03 - 0.02 * (j + 1), centres[j][0], centres[j][1], centres[j][2]); nb[j].scaleFactors = sf; }
    std::vector<std::vector<uh_dmatch>> matches(3);
    uint32_t lcg = 12345;
    auto rnd = [&]() { lcg = lcg * 1664525u + 1013904223u; return (double)(lcg >> 8) / (double)(1u << 24); };
    for (int i = 0; i < n_pts; i++) {
        const double X[3] = {-1.5 + 3.0 * rnd(), -1.0 + 2.0 * rnd(), 4.0 + 4.0 * rnd()};
        const int oct = i % 4;
        ToyPoint2f p = project(kf, X);
        if (i % 11 == 5) p.y += 25.f;   // some refused
        kf.und_kpts.push_back(ToyKeyPoint{p, oct});
        for (int j = 0; j < 3; j++) nb[j].und_kpts.push_back(ToyKeyPoint{project(nb[j], X), (oct + (i + j) % 3) % 5});
    }
    for (int j = 0; j < 3; j++) {   // the neighbour's keypoints in reverse order, so that queryIdx != trainIdx
        std::vector<ToyKeyPoint> rev(nb[j].und_kpts.rbegin(), nb[j].und_kpts.rend());
        nb[j].und_kpts = rev;
        for (int i = 0; i < n_pts; i++)
            if ((i + j) % 4 != 0) matches[j].push_back(uh_dmatch{n_pts - 1 - i, i, 0, 20.f + (float)(3 * i + j)});
    }

    std::unique_ptr<Context> ctx;
    try { ctx.reset(new Context(0)); } catch (const std::exception& e) { std::printf("no device: %s\n", e.what()); return 0; }
    NewPointCreator creator(*ctx);
    const std::vector<const ToyViewFrame*> nbp = {&nb[0], &nb[1], &nb[2]};
    const std::vector<NewPointInfo> pts = creator.create(kf, nbp, matches, 1.2f);
    REQUIRE(!pts.empty());
    float inv[16], RT0[16];
    se3_inverse(kf.pose_f2g.data(), inv);
    mat44_product(nb[0].pose_f2g.data(), inv, RT0);
    const std::vector<std::array<float, 3>> tri = Triangulate(*ctx, kf, nb[0], RT0, matches[0]);
    REQUIRE(tri.size() == matches[0].size());

    FILE* fp = std::fopen(argv[1], "wb");
    REQUIRE(fp);
    auto put_i = [&](int32_t v) { std::fwrite(&v, 4, 1, fp); };
    auto put_frame = [&](const ToyViewFrame& f) {
        put_i((int32_t)f.idx); put_i((int32_t)f.und_kpts.size());
        std::fwrite(f.pose_f2g.data(), 4, 16, fp);
        for (const auto& k : f.und_kpts) { std::fwrite(&k.pt.x, 4, 1, fp); std::fwrite(&k.pt.y, 4, 1, fp); }
        for (const auto& k : f.und_kpts) put_i(k.octave);
    };
    put_i(n_levels); std::fwrite(sf.data(), 4, n_levels, fp);
    put_frame(kf);
    for (int j = 0; j < 3; j++) {
        put_frame(nb[j]);
        float RT[16];
        mat44_product(nb[j].pose_f2g.data(), inv, RT);
        std::fwrite(RT, 4, 16, fp);
        put_i((int32_t)matches[j].size());
        std::fwrite(matches[j].data(), sizeof(uh_dmatch), matches[j].size(), fp);
    }
    put_i((int32_t)pts.size());
    for (const auto& p : pts) {
        put_i((int32_t)p.kp_idx); std::fwrite(p.xyz, 4, 3, fp); std::fwrite(&p.dist, 4, 1, fp);
        put_i((int32_t)p.frame_kpt.size());
        for (const auto& fk : p.frame_kpt) { put_i((int32_t)fk.first); put_i((int32_t)fk.second); }
    }
    for (const auto& t : tri) std::fwrite(t.data(), 4, 3, fp);
    std::fclose(fp);
    std::printf("newpoints adaptor ok\n");
    return 0;
}
