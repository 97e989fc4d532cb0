"""Deterministic single hypotheses for the three-point solver (csrc/p3p_math.hpp) and quartics for its roots(): the inputs of
tests/golden/p3p_golden.npz.  A case is float32 `P (4, 3)`, `px (4, 2)` with pnp_ransac_synth.INTR; everything is a function of the
seeds below, numpy only.

Families (what each must contain is asserted on the fixture alone, tests/test_p3p_branches_host.py):
  overhead  a triangle of radius 0.5-1.5 in a plane, the camera 0.5-2 above it within 0.3 of the axis and turned by about pi about x,
            the fourth point off the plane: the geometry in which the three-point problem has 1, 2, 3 and 4 solutions
  far       the scenes of pnp_ransac_synth (a far camera and a random cloud): both forms of the resolvent cubic
  a4        the camera centre is P1 turned about the line P2 P3 by 0.5-2.5 rad and then moved radially by a relative offset, looking at
            the centroid: at offset 0 the quartic's leading coefficient vanishes up to the float32 rounding of the inputs
  rot       noise-free matches of planted poses whose rotation is I, tiny, pi about an axis, or just short of pi: the branches of rodrigues()
The seeds of `overhead` and `far` were taken, in ascending order from the first, so that each count of solutions / each form of the cubic
occurs 16 / 20 times (the counts and forms themselves are asserted on the fixture); a seed of `a4` or `rot` that the admission of
tests/golden/make_p3p_golden.py rejected is replaced in SEEDS and stays in FIRST_CHOICE."""
from __future__ import annotations

import numpy as np

import pnp_ransac_synth as S

f32, f64 = np.float32, np.float64
INTR = S.INTR
FAMILIES = ("overhead", "far", "a4", "rot")
A4_OFFSETS = (0.0, 1e-6, 1e-5, 1e-4, 1e-2)
A4_PER_OFFSET = 8
ROT_KINDS = ("identity", "1e-9", "1e-6", "3e-5", "pi_x", "pi_y", "pi_z", "pi_skew", "pi-1e-9", "pi-3e-6")
ROT_PER_KIND = 3
SKEW_AXIS = np.array([0.48, -0.6, 0.64])   # a unit vector with no zero component

OVERHEAD_SEEDS = (1000, 1001, 1002, 1003, 1004, 1005, 1006, 1007, 1008, 1009, 1010, 1011, 1012, 1013, 1014, 1015, 1016, 1017, 1018, 1019, 1020, 1021,
                  1022, 1023, 1024, 1025, 1028, 1034, 1036, 1037, 1042, 1045, 1049, 1054, 1055, 1056, 1059, 1060, 1063, 1064, 1066, 1072, 1073, 1080,
                  1089, 1098, 1103, 1107, 1114, 1121, 1122, 1131, 1132, 1135, 1139, 1141, 1145, 1149, 1158, 1167, 1176, 1183, 1185, 1187)
FAR_SEEDS = (2000, 2001, 2002, 2003, 2004, 2005, 2006, 2007, 2008, 2009, 2010, 2011, 2012, 2013, 2014, 2015, 2016, 2017, 2018, 2019, 2020, 2021,
             2033, 2083, 2100, 2125, 2131, 2135, 2139, 2162, 2182, 2189, 2192, 2201, 2230, 2235, 2237, 2243, 2251, 2279)
FIRST_CHOICE = {"a4": tuple(range(7000, 7000 + len(A4_OFFSETS) * A4_PER_OFFSET)), "rot": tuple(range(8000, 8000 + len(ROT_KINDS) * ROT_PER_KIND))}
# replaced: a4 seed 7039 (offset 1e-2) gives a scaled |A4| of 8.8e-4, below the 1e-3 the family must show at that offset; 7040 (6.7e-4) likewise
SEEDS = {"overhead": OVERHEAD_SEEDS, "far": FAR_SEEDS, "a4": FIRST_CHOICE["a4"][:-1] + (7041,), "rot": FIRST_CHOICE["rot"]}


def _case(R, t, X):
    """float32 world points and the float32 pixels of their exact projection"""
    X = np.asarray(X, f64).astype(f32)
    px = S.project(R, t, INTR, X.astype(f64)).astype(f32)
    return np.ascontiguousarray(X), np.ascontiguousarray(px)


def overhead(seed):
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0, 2 * np.pi, 3))
    rad = rng.uniform(0.5, 1.5, 3)
    X = np.zeros((4, 3))
    X[:3, 0], X[:3, 1] = rad * np.cos(ang), rad * np.sin(ang)
    X[3] = [rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0.2, 0.6) * rng.choice([-1.0, 1.0])]
    centre = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(0.5, 2.0)])
    centre[:2] *= 0.3 / max(0.3, np.hypot(*centre[:2]))
    R = S.rodrigues(np.array([np.pi, 0, 0]) + rng.normal(0, 0.05, 3))   # looking down
    return _case(R, -R @ centre, X)


def far(seed):
    pr = S.scene(seed, 8, 1, outliers=0.0)
    idx = pr["samples"][0]
    return np.ascontiguousarray(pr["p3d"][idx]), np.ascontiguousarray(pr["kp"][idx])


def _look_at(centre, target, up):
    z = target - centre
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


def a4(seed, offset):
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0, 2 * np.pi, 3)) + np.array([0.0, 0.4, 0.8])
    rad = rng.uniform(0.5, 1.5, 3)
    X = np.zeros((4, 3))
    X[:3, 0], X[:3, 1] = rad * np.cos(ang), rad * np.sin(ang)
    X[:3] = X[:3] @ S.rodrigues(rng.normal(0, 0.5, 3)).T + rng.normal(0, 0.3, 3)
    X = X.astype(f32).astype(f64)              # the surface is that of the points the solver sees
    axis = X[2] - X[1]
    axis /= np.linalg.norm(axis)
    phi = rng.uniform(0.5, 2.5) * rng.choice([-1.0, 1.0])
    rel = X[0] - X[1]
    along = (rel @ axis) * axis
    centre = X[1] + along + (1 + offset) * (S.rodrigues(axis * phi) @ (rel - along))
    cen = X[:3].mean(0)
    X[3] = cen + rng.normal(0, 0.4, 3) + 0.5 * np.cross(X[1] - X[0], X[2] - X[0])
    R = _look_at(centre, cen, np.cross(axis, cen - centre))
    return _case(R, -R @ centre, X)


def rot_planted(kind):
    if kind == "identity":
        return np.zeros(3)
    if kind in ("1e-9", "1e-6", "3e-5"):
        return None   # a random axis times the angle, drawn in rot()
    if kind.startswith("pi_"):
        ax = {"x": [1.0, 0, 0], "y": [0, 1.0, 0], "z": [0, 0, 1.0], "skew": SKEW_AXIS}[kind[3:]]
        return np.pi * np.asarray(ax, f64)
    return None


def rot(seed, kind):
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    rv = rot_planted(kind)
    if rv is None:
        rv = ax * (float(kind) if not kind.startswith("pi-") else np.pi - float(kind[3:]))
    R = np.eye(3) if kind == "identity" else S.rodrigues(rv)
    t = rng.normal(0, 0.5, 3)
    fx, fy, cx, cy = [float(v) for v in INTR]
    px = np.stack([rng.uniform(20, S.W - 20, 4), rng.uniform(20, S.H - 20, 4)], 1)
    depth = rng.uniform(2, 10, 4)
    Xc = np.stack([(px[:, 0] - cx) / fx * depth, (px[:, 1] - cy) / fy * depth, depth], 1)
    return _case(R, t, (Xc - t) @ R)


def family(name, seeds=None):
    """dict(P (m, 4, 3) f32, px (m, 4, 2) f32, seed (m), tag (m) str) of one family"""
    seeds = SEEDS[name] if seeds is None else seeds
    P, px, tag = [], [], []
    for k, seed in enumerate(seeds):
        if name == "overhead":
            c, tg = overhead(seed), ""
        elif name == "far":
            c, tg = far(seed), ""
        elif name == "a4":
            off = A4_OFFSETS[k // A4_PER_OFFSET]
            c, tg = a4(seed, off), repr(off)
        else:
            tg = ROT_KINDS[k // ROT_PER_KIND]
            c = rot(seed, tg)
        P.append(c[0]); px.append(c[1]); tag.append(tg)
    return dict(P=np.stack(P).astype(f32), px=np.stack(px).astype(f32), seed=np.asarray(seeds, np.int64), tag=np.asarray(tag))


def problem(fam):
    """One family as ONE uh_pnp_ransac problem: n = 4 x cases, hypothesis i samples the matches 4 i .. 4 i + 3."""
    m = len(fam["P"])
    p3d = np.ascontiguousarray(fam["P"].reshape(4 * m, 3))
    nrm = np.zeros_like(p3d)
    nrm[:, 2] = 1
    return dict(n=4 * m, p3d=p3d, normal=nrm, kp=np.ascontiguousarray(fam["px"].reshape(4 * m, 2)), iters=m,
                samples=np.arange(4 * m, dtype=np.int32).reshape(m, 4), rt6_in=np.zeros(6, f32), intr=INTR)


# ---- quartics for roots(): (name, coefficients A0..A4 in float64, asserted against mpmath.polyroots on the same float64 numbers)

def _poly(roots, lead=1.0):
    """coefficients A0..A4 of lead * prod (v - r) over real roots r and complex pairs given as (re, im) tuples, in float64 arithmetic"""
    c = np.array([1.0])
    for r in roots:
        c = np.polymul(c, [1.0, -2 * r[0], r[0] * r[0] + r[1] * r[1]] if isinstance(r, tuple) else [1.0, -r])
    return (lead * c)[::-1].copy()


def _biquadratic(shift, z1, z2):
    """((v - shift)^2 - z1) ((v - shift)^2 - z2)"""
    y = np.polymul([1.0, 0.0, -z1], [1.0, 0.0, -z2])
    s = np.array([1.0, -shift])
    c = np.zeros(5)
    for k, a in enumerate(y[::-1]):
        c = np.polyadd(c, a * (np.poly1d(s) ** k).coeffs)
    return c[::-1].copy()


def quartics():
    q = [("simple", _poly([0.5, 1.25, 2.0, 3.5])),
         ("biquadratic4", _biquadratic(1.5, 0.25, 1.0)), ("biquadratic2", _biquadratic(1.5, 0.25, -1.0)), ("biquadratic0", _biquadratic(1.5, -0.25, -1.0))]
    for d in (4e-9, 4e-7, 4e-5):
        q.append((f"almost_biquadratic_{d:g}", _poly([1.0, 2.0 + d, (1.5, 1.0)])))   # biquadratic2 with one root moved
    q += [("double_two_simple", _poly([1.0, 1.0, 2.0, 3.5])), ("double_complex", _poly([1.5, 1.5, (0.5, 0.75)])),
          ("pair_1e-6", _poly([1.0, 1.0 + 1e-6, 2.5, 4.0])), ("pair_1e-9", _poly([1.0, 1.0 + 1e-9, 2.5, 4.0])),
          ("triple", _poly([1.5, 1.5, 1.5, 3.0])), ("complex_1e-6", _poly([0.75, 3.0, (1.5, 1e-6)])),
          ("scaled_1e8", 1e8 * _poly([0.5, 1.25, 2.0, 3.5])), ("scaled_1e-8", 1e-8 * _poly([0.5, 1.25, 2.0, 3.5])),
          ("negative_lead", _poly([0.5, 1.25, 2.0, 3.5], -2.0)), ("spread", _poly([1e-3, 0.1, 10.0, 1e3]))]
    cubic = np.array([-6.0, 11.0, -6.0, 1.0])           # (v - 1)(v - 2)(v - 3)
    for a4 in (1e-2, 1e-4, 1e-5, 1e-6, 1e-8, 1e-10, -1e-4, -1e-6, 0.0):
        q.append((f"lead_{a4:g}", np.concatenate([-cubic, [a4]])))          # A4 v^4 - v^3 + 6 v^2 - 11 v + 6
    for a0 in (1e-2, 1e-5, 1e-8, 1e-10, -1e-6, 0.0):
        q.append((f"tail_{a0:g}", np.concatenate([[a0], cubic])))            # v (v - 1)(v - 2)(v - 3) + A0: a root at v -> 0
    return [(n, np.asarray(c, f64)) for n, c in q]
