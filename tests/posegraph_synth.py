"""Synthetic loop closures for the pose-graph tests: a ring trajectory (radius 5) whose estimated poses carry accumulated drift, one
closing edge between the last and the first keyframe of the ring, and the essential graph's other edges.  Shared by
tests/golden/make_posegraph_golden.py (the real g2o) and tests/test_posegraph*.py, so both sides see bit-identical inputs."""
import numpy as np

INPUT_KEYS = ("poses", "edge_i", "edge_j", "edge_w", "expected", "idx")


def _rot(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _T(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def posegraph_problem(n, seed, fix_scale, rot_noise=0.002, trans_noise=0.01, scale_jump=0.0, close_rot=0.0, skip2=0, reverse_every=0,
                      duplicate_every=0, weights=False, isolated=False, old_fan=0, zero=False):
    """n poses in all.  The ring visits them in the order seq = n//2, n//2 + 1, .., n - 1, 0, .., n//2 - 1 (an isolated pose left out), so
    that idx_old = seq[0] lies in the middle of the index range and idx_new = seq[-1] is not the last index.
      scale_jump   the drifted trajectory's steps are longer by this fraction in all (what a monocular map does)
      close_rot    extra rotation (rad) between the drifted and the expected pose of the new keyframe
      skip2        every skip2-th ring position also gets an edge to the position two ahead
      reverse_every / duplicate_every   every k-th edge is given as (j, i) / is given twice, the copy reversed
      weights      edge weights drawn from {0.2, 0.4, 0.8, 1.6, 3.2}, else NULL (= 1)
      isolated     index n//4 has no edge at all
      old_fan      the old keyframe gets edges to this many further ring positions
      zero         every pose the identity rotation at one position, expected == current: chi2 is exactly 0"""
    rng = np.random.RandomState(seed)
    seq = [(n // 2 + k) % n for k in range(n)]
    iso = n // 4 if isolated else -1
    if isolated:
        seq.remove(iso)
    m = len(seq)
    true, est = [], []
    for k in range(m):
        a = 2 * np.pi * k / (m + 1)   # the ring is not closed by a step of its own: the closing edge spans the gap
        c = np.array([5 * np.cos(a), 0.3 * np.sin(3 * a), 5 * np.sin(a)])
        R = _rot(rng.uniform(-0.05, 0.05, 3)) @ _rot(np.array([0, -a, 0]))
        true.append(_T(R, -R @ c))
    if zero:
        true = [_T(np.eye(3), np.array([1.0, 2.0, 3.0])) for _ in range(m)]
    step_scale = (1 + scale_jump) ** (1.0 / max(m - 1, 1))
    est.append(true[0].copy())
    for k in range(1, m):
        rel = true[k] @ np.linalg.inv(true[k - 1])
        rel[:3, 3] *= step_scale
        d = np.eye(4) if zero else _T(_rot(rng.normal(0, rot_noise, 3)), rng.normal(0, trans_noise, 3))
        est.append(d @ rel @ est[k - 1])
    # where the loop detector says the new keyframe is: the true relative pose to the old keyframe applied to the old estimate
    expected = _T(_rot(np.array([0.0, close_rot, 0.0])), np.zeros(3)) @ true[m - 1] @ np.linalg.inv(true[0]) @ est[0]
    poses = np.zeros((n, 16), np.float32)
    for k, idx in enumerate(seq):
        poses[idx] = est[k].astype(np.float32).reshape(16)
    if isolated:
        poses[iso] = _T(_rot(np.array([0.3, -2.5, 0.2])), np.array([0.5, -0.25, 2.0])).astype(np.float32).reshape(16)   # w < 0 out of the conversion
    pairs = [(seq[k], seq[k + 1]) for k in range(m - 1)] if m > 2 else []   # two poses: the closing edge only
    if skip2:
        pairs += [(seq[k], seq[k + 2]) for k in range(0, m - 2, skip2)]
    for f in range(old_fan):
        pairs.append((seq[0], seq[2 + 2 * f]))
    pairs.append((seq[-1], seq[0]))   # the closing edge (new, old)
    ei, ej = [], []
    for q, (a, b) in enumerate(pairs):
        if reverse_every and q % reverse_every == reverse_every - 1:
            a, b = b, a
        ei.append(a); ej.append(b)
        if duplicate_every and q % duplicate_every == duplicate_every - 1:
            ei.append(b); ej.append(a)
    E = len(ei)
    w = np.float32(0.2) * (2.0 ** rng.randint(0, 5, E)).astype(np.float32) if weights else np.zeros(0, np.float32)
    return dict(n=n, E=E, poses=poses, edge_i=np.array(ei, np.int32), edge_j=np.array(ej, np.int32), edge_w=w.astype(np.float32),
                expected=expected.astype(np.float32).reshape(16), idx=np.array([seq[-1], seq[0]], np.int32), idx_new=int(seq[-1]), idx_old=int(seq[0]),
                fix_scale=int(fix_scale), isolated=iso)


# the fixture's cases: name -> keyword arguments of posegraph_problem.  A seed is replaced when tests/golden/make_posegraph_golden.py
# says that the case does not pass its admission conditions; FIRST_CHOICE keeps the seeds the cases were first written with.
CASES = {
    "pg2_zero": dict(n=2, seed=301, fix_scale=False, zero=True),
    "pg3": dict(n=3, seed=302, fix_scale=False),
    "pg4": dict(n=4, seed=303, fix_scale=True),
    "pg5": dict(n=5, seed=304, fix_scale=False),
    "pg8_mixed": dict(n=8, seed=305, fix_scale=False, reverse_every=2, duplicate_every=3, weights=True),
    "pg12_mixed": dict(n=12, seed=306, fix_scale=True, reverse_every=3, duplicate_every=4, weights=True, isolated=True, old_fan=3, skip2=2),
    "pg12_big": dict(n=12, seed=307, fix_scale=False, rot_noise=0.02, scale_jump=0.10, close_rot=0.15),
    "pg10": dict(n=10, seed=308, fix_scale=False, skip2=3),
    "pg11": dict(n=11, seed=309, fix_scale=True, skip2=3),
    "pg20": dict(n=20, seed=314, fix_scale=False, skip2=4),
    "pg64_free": dict(n=64, seed=311, fix_scale=False, skip2=8),
    "pg64_fixed": dict(n=64, seed=312, fix_scale=True, skip2=8),
    "pg150_fixed": dict(n=150, seed=313, fix_scale=True),
}
FIRST_CHOICE = {"pg2_zero": 301, "pg3": 302, "pg4": 303, "pg5": 304, "pg8_mixed": 305, "pg12_mixed": 306, "pg12_big": 307, "pg10": 308,
                "pg11": 309, "pg20": 310, "pg64_free": 311, "pg64_fixed": 312, "pg150_fixed": 313}
