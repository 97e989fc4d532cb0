// The stereo / RGB-D adaptors (include/ucoslam_hip/adaptors.hpp: FrameExtractor::processStereo / process_rgbd) on a toy Frame.
//   stereo_adaptor            host only: uh_stereo_depth_host through the C ABI on a scene whose depth is known in closed form
//   stereo_adaptor dump.bin   GPU: both adaptors on a procedural image pair; images and frames are written out for tests/test_stereo_adaptor.py
#include <cstdio>
#include <cstring>
#include <random>

#include "../../include/ucoslam_hip/adaptors.hpp"

struct ToyPoint2f { float x, y; };
struct ToyKeyPoint { ToyPoint2f pt; float size, angle, response; int octave, class_id; };
struct ToyFrame {   // ucoslam::Frame as far as the adaptors write it
    std::vector<ToyPoint2f> kpts;
    std::vector<ToyKeyPoint> und_kpts;
    std::vector<uint8_t> desc;
    std::vector<float> depth;
    uint32_t fseq_idx = 0;
};

static constexpr int W = 320, H = 200, DISP = 9;

static void make_pair(std::vector<uint8_t>& left, std::vector<uint8_t>& right) {
    const int bw = W + 64;
    std::vector<float> img((size_t)bw * H, 110.f);
    std::mt19937 scene(77);
    for (int i = 0; i < 700; i++) {
        const int cx = scene() % bw, cy = scene() % H, sx = 3 + scene() % 14, sy = 3 + scene() % 14;
        const float c = (30.f + scene() % 91) * ((scene() & 1) ? 1.f : -1.f);
        for (int y = std::max(cy - sy, 0); y < std::min(cy + sy, H); y++) for (int x = std::max(cx - sx, 0); x < std::min(cx + sx, bw); x++) img[(size_t)y * bw + x] += c;
    }
    std::mt19937 noise(5);
    left.resize((size_t)W * H); right.resize((size_t)W * H);
    for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
        left[(size_t)y * W + x] = (uint8_t)std::min(255.f, std::max(0.f, img[(size_t)y * bw + x] + (float)(noise() % 5)));
        right[(size_t)y * W + x] = (uint8_t)std::min(255.f, std::max(0.f, img[(size_t)y * bw + x + DISP] + (float)(noise() % 5)));
    }
}

template <typename T> static void put(FILE* f, const T* p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }
static void put_frame(FILE* f, const ToyFrame& fr) {
    const int32_t n = (int32_t)fr.und_kpts.size();
    put(f, &n, 1);
    put(f, fr.kpts.data(), fr.kpts.size());
    put(f, fr.und_kpts.data(), fr.und_kpts.size());
    put(f, fr.desc.data(), fr.desc.size());
    put(f, fr.depth.data(), fr.depth.size());
    put(f, &fr.fseq_idx, 1);
}

static int host_only() {
    // constant left image, right image a V of slope 2 around column 24.5: the SAD minimum of a keypoint at x = 20 is at offset +5 with equal
    // neighbours, so xr = 25 exactly and depth = bl * fx / (und.x - 25)
    const int cols = 64, rows = 48;
    std::vector<uint8_t> L((size_t)cols * rows, 100), R((size_t)cols * rows);
    for (int y = 0; y < rows; y++) for (int x = 0; x < cols; x++) R[(size_t)y * cols + x] = (uint8_t)(100 + std::abs(2 * x - 49));
    uh_keypoint lk[2] = {{27.f, 20.f, 31.f, 0.f, 20.f, 0, -1}, {29.f, 30.f, 31.f, 0.f, 20.f, 0, -1}}, rk[1] = {{20.f, 20.f, 31.f, 0.f, 20.f, 1, -1}};
    uint8_t ld[64] = {0}, rd[32] = {0};
    rd[3] = 0x11;
    uh_stereo_args a{};
    a.left = L.data(); a.left_stride = cols; a.right = R.data(); a.right_stride = cols; a.cols = a.right_cols = cols; a.rows = a.right_rows = rows;
    a.n_left = 2; a.left_und_kpts = lk; a.left_desc = ld; a.n_right = 1; a.right_kpts = rk; a.right_desc = rd;
    a.bl = 0.5f; a.fx = 400.f; a.max_desc_dist = 50.f;
    float depth[2] = {-1.f, -1.f};
    int32_t match[2] = {7, 7};
    ucoslam_hip::check(uh_stereo_depth_host(&a, depth, match));
    if (match[0] != 0 || match[1] != -1 || depth[0] != 100.f || depth[1] != 0.f) { std::printf("unexpected: %d %d %g %g\n", match[0], match[1], depth[0], depth[1]); return 1; }
    a.right_rows = rows - 1;
    if (uh_stereo_depth_host(&a, depth, match) != UH_EINVAL || !std::strstr(uh_last_error(), "right image")) { std::printf("unequal sizes accepted\n"); return 1; }
    std::printf("stereo host ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return host_only();
    using namespace ucoslam_hip;
    std::vector<uint8_t> left, right;
    make_pair(left, right);
    std::vector<uint16_t> D((size_t)W * H);
    std::mt19937 dr(9);
    for (auto& v : D) v = (dr() % 4 == 0) ? 0 : (uint16_t)(dr() & 0xffff);
    auto ctx = std::make_shared<Context>(0);
    FrameExtractor fe(ctx, FeatParams(800, 5, 1.2f, -1), 50.f);
    StereoImageParams ip{517.3f, 516.5f, 158.6f, 99.3f, {}, 0.11f, 1.f / 5000.f};
    ToyFrame fs, fd;
    fe.processStereo(ImageView{left.data(), W, H, (size_t)W, 1}, ImageView{right.data(), W, H, (size_t)W, 1}, ip, fs, 41);
    fe.process_rgbd(ImageView{left.data(), W, H, (size_t)W, 1}, ImageView{D.data(), W, H, (size_t)W * 2, 1}, ip, fd, 42);
    bool threw = false;
    try { fe.processStereo(ImageView{left.data(), W, H, (size_t)W, 1}, ImageView{right.data(), W, H - 1, (size_t)W, 1}, ip, fs, 43); } catch (const std::runtime_error&) { threw = true; }
    if (!threw || fs.fseq_idx != 41) { std::printf("unequal sizes accepted\n"); return 1; }
    FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 2;
    const int32_t hd[2] = {W, H};
    put(f, hd, 2);
    put(f, left.data(), left.size()); put(f, right.data(), right.size()); put(f, D.data(), D.size());
    put_frame(f, fs); put_frame(f, fd);
    std::fclose(f);
    std::printf("stereo adaptor ok\n");
    return 0;
}
