"""Constructed scenes for the stereo / RGB-D depth stage, shared by tests/test_stereo_host.py (CPU) and tests/test_stereo.py (GPU).
A scene is dict(L, R, lk, ld, rk, rd, bl, fx, mdd): gray images, left undistorted keypoints + descriptors, right keypoints + descriptors,
ImageParams::bl / fx(), Params::maxDescDistance.  CASES maps a name to a function returning a LIST of scenes (64 x 48 unless stated)."""
import numpy as np

from stereo_oracle import FLT_MAX, KEYPOINT_DTYPE

COLS, ROWS = 64, 48
BL, FX = 0.12, 458.654


def kps(rows):
    """rows: (x, y, octave) tuples -> KEYPOINT_DTYPE array"""
    a = np.zeros(len(rows), KEYPOINT_DTYPE)
    for i, (x, y, o) in enumerate(rows):
        a[i] = (x, y, 31.0, 0.0, 20.0, o, -1)
    return a


def base_desc(seed):
    return np.random.default_rng(seed).integers(0, 256, 32, dtype=np.uint8)


def flip(desc, bits):
    """a copy of `desc` with the listed bit positions (0..255) flipped: Hamming distance len(bits) from it"""
    d = desc.copy()
    for b in bits:
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def texture(seed, rows=ROWS, cols=COLS):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8)


def scene(L, R, left, right, ld, rd, mdd=50.0, bl=BL, fx=FX):
    return dict(L=np.ascontiguousarray(L), R=np.ascontiguousarray(R), lk=kps(left), rk=kps(right), ld=np.array(ld, np.uint8).reshape(-1, 32),
                rd=np.array(rd, np.uint8).reshape(-1, 32), bl=bl, fx=fx, mdd=mdd)


def shifted(seed, s):
    """L random, R(y, x) = L(y, x + s) (wrapping): the window of L around lx equals the window of R around lx - s"""
    L = texture(seed)
    return L, np.roll(L, -s, axis=1)


def equal_hamming():
    B = base_desc(1)
    L, R = shifted(11, 4)
    # row 20: j = 0 and j = 1 both at distance 5 (0 wins), j = 2 at 7; row 30: the lowest j is NOT the nearest
    right = [(25.0, 20.0, 0), (24.0, 20.2, 0), (26.0, 19.8, 0), (22.0, 30.0, 0), (21.0, 30.0, 0), (20.0, 30.0, 0)]
    rd = [flip(B, range(5)), flip(B, range(5, 10)), flip(B, range(7)), flip(B, range(9)), flip(B, range(3)), flip(B, range(10, 13))]
    return [scene(L, R, [(30.0, 20.0, 0), (28.0, 30.0, 0)], right, [B, B], rd)]


def x_filter():
    B = base_desc(2)
    L, R = shifted(12, 3)
    above = float(np.nextafter(np.float32(30.0), np.float32(100.0)))
    # the keypoint just right of the left one is nearer in descriptor space but skipped; equality is kept
    return [scene(L, R, [(30.0, 20.0, 0)], [(above, 20.0, 0), (30.0, 20.0, 0), (31.0, 20.0, 0)], [B], [flip(B, [0]), flip(B, range(6)), B])]


def octave_filter():
    B = base_desc(3)
    L, R = shifted(13, 5)
    right = [(20.0, 20.0, 4), (21.0, 20.0, 0), (22.0, 20.0, 3), (23.0, 20.0, 1)]
    rd = [flip(B, [0]), flip(B, range(2)), flip(B, range(10)), flip(B, range(12))]
    return [scene(L, R, [(30.0, 20.0, 2)], right, [B], rd)]


def distance_bound():
    B = base_desc(4)
    L, R = shifted(14, 6)
    left = [(30.0, 20.0, 0), (30.0, 30.0, 0)]
    right = [(20.0, 20.0, 0), (20.0, 30.0, 0)]
    rd = [flip(B, range(50)), flip(B, range(49))]   # d == maxDescDistance is rejected, 49 accepted
    far = [~B, ~B]                                    # distance 256: only FLT_MAX admits it
    return [scene(L, R, left, right, [B, B], rd, mdd=50.0), scene(L, R, left, right, [B, B], far, mdd=50.0), scene(L, R, left, right, [B, B], far, mdd=FLT_MAX)]


def half_rows():
    B = base_desc(5)
    L, R = shifted(15, 2)
    # left y: 20.5 -> row 21; -0.5 -> row -1 (no candidates); 47.5 -> row 48 (none); -0.4 -> row 0; 0.5 -> row 1; 46.5 -> row 47
    left = [(30.0, 20.5, 0), (30.0, -0.5, 0), (30.0, 47.5, 0), (30.0, -0.4, 0), (30.0, 0.5, 0), (30.0, 46.5, 0), (30.0, 20.49, 0)]
    # right y: 20.5 -> 21; 21.4 -> 21; -0.5 -> -1 and 47.5 -> 48: in no bucket; -0.49 -> 0; 0.5 -> 1; 46.5 -> 47; 19.5 -> 20
    right = [(20.0, 20.5, 0), (19.0, 21.4, 0), (20.0, -0.5, 0), (20.0, 47.5, 0), (20.0, -0.49, 0), (20.0, 0.5, 0), (20.0, 46.5, 0), (20.0, 19.5, 0)]
    rd = [flip(B, range(3)), flip(B, range(4)), B, B, flip(B, [1]), flip(B, [2]), flip(B, [3]), flip(B, [4])]
    return [scene(L, R, left, right, [B] * len(left), rd)]


def window_centres():
    """left and right centres at 2, 3, cols-4, cols-3 (and the same in y): the four skips and their neighbours"""
    B = base_desc(6)
    out = []
    edge_x, edge_y = (2, 3, COLS - 4, COLS - 3), (2, 3, ROWS - 4, ROWS - 3)

    def one(lx, ly, rx, ry):   # the true offset one step inside the (clamped) range, so that only the window tests decide
        o = 1 if rx < COLS // 2 else -1
        L, R = shifted(16, lx - rx - o)
        return scene(L, R, [(float(lx), float(ly), 0)], [(float(rx), float(ry), 0)], [B], [B])

    for cx in edge_x:   # left x on the edge (the right keypoint inside, or as far right as the x filter allows)
        out.append(one(cx, 20, min(cx, 20), 20))
    for cx in edge_x:   # right x on the edge
        out.append(one(max(cx, 30), 20, cx, 20))
    for cy in edge_y:   # both y on the edge (one row)
        out.append(one(30, cy, 24, cy))
    # rounding moves a centre across the bound: 2.5 -> 3 (kept), 2.49 -> 2 (skipped), cols - 3.5 -> cols - 3 (skipped)
    L, R = shifted(16, 30 - 3 - 1)
    out.append(scene(L, R, [(30.0, 20.0, 0), (30.0, 21.0, 0), (COLS - 3.5, 22.0, 0)], [(2.5, 20.0, 0), (2.49, 21.0, 0), (30.0, 22.0, 0)], [B] * 3, [B] * 3))
    return out


def rx_edges():
    """rx at 3..10 and cols-10..cols-4: clamped offset ranges.  One scene per (rx, true offset): the minimum on the lower edge of the range
    (depth 0), one inside it, on the upper edge (depth 0), one below the upper edge."""
    B = base_desc(7)
    out = []
    for rx in list(range(3, 11)) + list(range(COLS - 10, COLS - 3)):
        lo, hi = max(-7, 3 - rx), min(7, COLS - 3 - rx)
        lx = max(rx, 30) if rx < 32 else COLS - 4
        for o in (lo, lo + 1, hi, hi - 1):
            L, R = shifted(100 + rx, lx - rx - o)
            out.append(scene(L, R, [(float(lx), 20.0, 0)], [(float(rx), 20.0, 0)], [B], [B]))
    return out


def equal_sad():
    """columns with period 4: the cost is 0 at four offsets, the first wins"""
    B = base_desc(8)
    T = np.random.default_rng(17).integers(0, 256, (ROWS, 4), dtype=np.uint8)
    L = np.tile(T, (1, COLS // 4))
    const = np.full((ROWS, COLS), 77, np.uint8)   # every cost equal: the first offset of the range wins, which is its edge
    return [scene(L, L.copy(), [(30.0, 20.0, 0)], [(20.0, 20.0, 0)], [B], [B]), scene(const, const.copy(), [(30.0, 20.0, 0)], [(20.0, 20.0, 0)], [B], [B])]


def inf_and_negative():
    """L constant, R a V of slope 2 around the half-integer column c* - 0.5: the cost is symmetric about the window centre c*, so delta is the
    integer offset exactly and xr = right.x + o*.  left.und.x == xr gives +inf, left.und.x < xr a negative depth; both are stored."""
    B = base_desc(9)
    L = np.full((ROWS, COLS), 100, np.uint8)
    cstar = 25
    R = np.tile((100 + np.abs(2 * np.arange(COLS) - 2 * cstar + 1)).clip(0, 255).astype(np.uint8), (ROWS, 1))
    left = [(25.0, 20.0, 0), (24.5, 21.0, 0), (26.0, 22.0, 0)]
    right = [(20.0, 20.0, 0), (20.0, 21.0, 0), (20.0, 22.0, 0)]
    return [scene(L, R, left, right, [B] * 3, [B] * 3)]


def identical_images():
    B = base_desc(10)
    L = texture(18)
    pts = [(10.0, 8.0, 0), (30.3, 20.0, 1), (50.7, 40.2, 2), (20.0, 30.5, 0)]
    return [scene(L, L.copy(), pts, pts, [flip(B, [k]) for k in range(4)], [flip(B, [k]) for k in range(4)])]


def empty_sides():
    B = base_desc(11)
    L, R = shifted(19, 3)
    return [scene(L, R, [], [(20.0, 20.0, 0)], [], [B]), scene(L, R, [(30.0, 20.0, 0)], [], [B], []), scene(L, R, [], [], [], [])]


def crowded_row():
    """one row holding 200 right keypoints (more than any lane group's width), equal distances among them"""
    rng = np.random.default_rng(12)
    B = base_desc(12)
    L, R = shifted(20, 5)
    right = [(float(np.float32(3.0 + 50.0 * rng.random())), float(np.float32(19.5 + 0.99 * rng.random())), int(rng.integers(0, 3))) for _ in range(200)]
    rd = [flip(B, rng.choice(256, int(rng.integers(4, 40)), replace=False)) for _ in range(200)]
    left = [(float(np.float32(20.0 + 40.0 * rng.random())), 20.0, int(rng.integers(0, 3))) for _ in range(24)]
    ld = [flip(B, rng.choice(256, int(rng.integers(0, 6)), replace=False)) for _ in range(24)]
    return [scene(L, R, left, right, ld, rd, mdd=60.0)]


def random_scene(n=3000, cols=1241, rows=376, seed=21):
    """A textured image shifted by a block-wise disparity map; n keypoints a side whose right partners sit at the shifted position (up to 2 px
    off, so the SAD minimum is interior), in shuffled order, plus mismatched octaves and unrelated descriptors."""
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    bw = 64
    disp = rng.integers(8, 40, (rows // 47 + 1, cols // bw + 2))
    R = np.zeros_like(L)
    for by in range(disp.shape[0]):
        for bx in range(disp.shape[1] - 1):
            y0, y1, x0, x1 = by * 47, min((by + 1) * 47, rows), bx * bw, min((bx + 1) * bw, cols)
            if y0 >= rows or x0 >= cols:
                continue
            src = np.clip(np.arange(x0, x1) + disp[by, bx], 0, cols - 1)
            R[y0:y1, x0:x1] = L[y0:y1][:, src]
    lx = rng.uniform(60, cols - 20, n).astype(np.float32)
    ly = rng.uniform(16, rows - 16, n).astype(np.float32)
    lo = rng.integers(0, 8, n)
    lk = np.zeros(n, KEYPOINT_DTYPE)
    lk["x"], lk["y"], lk["octave"], lk["size"], lk["class_id"] = lx, ly, lo, 31.0, -1
    ld = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d = disp[(ly.astype(int)) // 47, (lx.astype(int)) // bw]
    perm = rng.permutation(n)
    rk = np.zeros(n, KEYPOINT_DTYPE)
    rk["x"] = (lx - d + rng.uniform(-2, 2, n)).astype(np.float32)
    rk["y"] = ly
    rk["octave"] = lo + rng.integers(-2, 3, n) * (rng.random(n) < 0.15)
    rk["size"], rk["class_id"] = 31.0, -1
    rd = ld.copy()
    for i in range(n):
        if rng.random() < 0.1:
            rd[i] = rng.integers(0, 256, 32, dtype=np.uint8)
        else:
            rd[i] = flip(rd[i], rng.choice(256, int(rng.integers(0, 30)), replace=False))
    rk, rd = rk[perm], rd[perm]
    return [dict(L=L, R=R, lk=lk, rk=rk, ld=ld, rd=rd, bl=BL, fx=FX, mdd=50.0)]


CASES = dict(equal_hamming=equal_hamming, x_filter=x_filter, octave_filter=octave_filter, distance_bound=distance_bound, half_rows=half_rows,
             window_centres=window_centres, rx_edges=rx_edges, equal_sad=equal_sad, inf_and_negative=inf_and_negative,
             identical_images=identical_images, empty_sides=empty_sides, crowded_row=crowded_row, random_scene=random_scene)


def rgbd_scene():
    """pixel 0, pixel 65535, keypoints at k + 0.5 with k even and odd (cvRound: to even), scale 1 / 5000"""
    rng = np.random.default_rng(31)
    D = rng.integers(1, 65535, (ROWS, COLS)).astype(np.uint16)
    D[10, 10], D[11, 12], D[20, 20], D[20, 22] = 0, 65535, 0, 65535
    # the last one rounds to column COLS: outside the image (0 by the library's documented choice; the reference reads unchecked)
    pts = [(10.0, 10.0, 0), (12.0, 11.0, 0), (10.5, 10.5, 0), (11.5, 11.0, 0), (12.5, 10.5, 0), (21.5, 20.0, 0), (20.5, 20.49, 0), (22.5, 19.5, 0),
           (0.0, 0.0, 0), (COLS - 1.0, ROWS - 1.0, 0), (0.5, 0.5, 0), (1.5, 2.5, 0), (33.3, 7.7, 1), (COLS - 0.51, ROWS - 0.51, 0), (COLS - 0.5, 10.0, 0)]
    return kps(pts), D, np.float32(1.0 / 5000.0)
