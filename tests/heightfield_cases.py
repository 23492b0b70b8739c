"""The cases the height-field tests share (tests/test_heightfield_host.py, test_heightfield_sanitizers.py, test_gpu_heightfield.py): the fields, the edge points of the
sampling rule and the random walkers, each computed once and never changed."""
import itertools

import numpy as np

import heightfield_ref as HR
import walk_ref as WR

NMAX = 257
_SHARED = {}


def fields(pkg):
    """name -> heightfield_ref.Field: the smallest fields at which indexing can go wrong, every node a value of its own (a transposed nx / ny reads another one), and a
    64 x 48 rough field.  The grids cover about [-1, 1] x [-1, 1], so the random robots (positions of unit variance) stand inside and beyond every side; the heights lie
    around the feet's, so that feet are on both sides of the ground.  All spacings but the 5 x 3 field's are dyadic, so that a node's coordinates x0 + i dx come back
    as the grid coordinate i exactly (edge_points); the 5 x 3 field's reciprocals 1 / 0.55 and 1 / 0.9 are rounded ones"""
    if "fields" not in _SHARED:
        distinct = lambda nx, ny: -0.05 + 0.013 * np.arange(nx * ny, dtype=np.float64).reshape(ny, nx) * (8.0 / (nx * ny))
        F = {"1x1/0": HR.Field(np.array([[0.03]]), 0.2, -0.1, 0.5, 0.25, 0), "2x2/1": HR.Field(distinct(2, 2), -1.0, -1.0, 2.0, 2.0, 1)}
        for interp in (0, 1):
            F[f"3x2/{interp}"] = HR.Field(distinct(3, 2), -1.0, -0.75, 1.0, 1.5, interp)
            F[f"5x3/{interp}"] = HR.Field(distinct(5, 3), -1.1, -0.9, 0.55, 0.9, interp)
            F[f"64x48/{interp}"] = HR.Field(pkg.heightfields.rough(64, 48, 77, 0.05), -1.5, -1.25, 0.046875, 0.0546875, interp)
        _SHARED["fields"] = F
    return _SHARED["fields"]


def point_fields(pkg):
    """fields() and a 4 x 3 field, both interp, whose node (0, 0) IS the world's origin (x0 = y0 = 0.0): only there do X = -1e-300 and X = -0.0 reach the rule as a tiny
    negative ux and as ux = -0.0 (with any other x0 the subtraction X - x0 rounds them away and gives +0.0)"""
    if "point_fields" not in _SHARED:
        F = dict(fields(pkg))
        for interp in (0, 1):
            F[f"4x3@0/{interp}"] = HR.Field(-0.05 + 0.009 * np.arange(12, dtype=np.float64).reshape(3, 4), 0.0, 0.0, 0.5, 0.25, interp)
        _SHARED["point_fields"] = F
    return _SHARED["point_fields"]


TINY = slice(-13, -10)   # the rows of edge_points (and of edge_points_few) that hold the three points a hair below node 0 / at -0.0


def edge_points(f):
    """the points of the sampling rule's edge cases for the field f, in WORLD coordinates without an origin: every node; the last node of each axis (ux == nx - 1
    exactly, as (nx - 1) * dx / dx is); cell interiors; outside each of the four sides and each corner; x0 - 1e-300 and x0 - 0.0 (rows TINY: on a field of point_fields
    with x0 = y0 = 0.0 these are X = -1e-300 and X = -0.0 and reach the rule as such, tiny_points_reach_the_rule; elsewhere they round to node 0); +-inf; NaN in X
    only, in Y only"""
    xs = [f.x0 + i * f.dx for i in range(f.nx)]; ys = [f.y0 + j * f.dy for j in range(f.ny)]
    pts = [(x, y) for x in xs for y in ys]
    pts += [(x + 0.37 * f.dx, y + 0.61 * f.dy) for x in xs for y in ys]
    lo_x, hi_x, lo_y, hi_y = xs[0] - 2.5 * f.dx, xs[-1] + 2.5 * f.dx, ys[0] - 1.5 * f.dy, ys[-1] + 1.5 * f.dy
    mid_x, mid_y = 0.5 * (xs[0] + xs[-1]) + 0.1 * f.dx, 0.5 * (ys[0] + ys[-1]) + 0.1 * f.dy
    pts += [(lo_x, mid_y), (hi_x, mid_y), (mid_x, lo_y), (mid_x, hi_y), (lo_x, lo_y), (lo_x, hi_y), (hi_x, lo_y), (hi_x, hi_y)]
    zx, zy = (-0.0 if f.x0 == 0.0 else f.x0 - 0.0), (-0.0 if f.y0 == 0.0 else f.y0 - 0.0)   # (0.0 - 0.0 is +0.0: the negative zero is written down as such)
    pts += [(f.x0 - 1e-300, mid_y), (mid_x, f.y0 - 1e-300), (zx, zy)]
    inf, nan = np.inf, np.nan
    pts += [(inf, mid_y), (-inf, mid_y), (mid_x, inf), (mid_x, -inf), (inf, -inf), (-inf, inf), (nan, mid_y), (mid_x, nan), (nan, nan), (nan, inf)]
    return np.array(pts, dtype=np.float64)


def walkers(scen):
    """257 random walkers (all 16 contact patterns), ten extra words per row, bodies at standing height, an origin row each: computed once, never changed"""
    if "walk" not in _SHARED:
        rng = np.random.default_rng(9600)
        sc = WR.random_walkers(scen, rng, NMAX)
        sc["state"][:, 5] = rng.uniform(0.25, 0.45, NMAX)
        sc["wide"] = np.concatenate([sc["state"], rng.normal(0, 1, (NMAX, 10))], 1)
        sc["origin"] = np.concatenate([rng.uniform(-0.5, 0.5, (NMAX, 2)), rng.uniform(-0.02, 0.02, (NMAX, 1))], 1)
        for v in sc.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _SHARED["walk"] = sc
    return _SHARED["walk"]


CONFIGS = list(itertools.product((1, 3), (0.0, 0.5, 1.0), ("1x1/0", "2x2/1", "3x2/0", "3x2/1", "5x3/0", "5x3/1", "64x48/0", "64x48/1")))   # sub-steps (3: a wrench), track, field


def flags(k):
    """configuration k -> (origin given, ground_out given, in place): the eight combinations, walked so that every field, sub-step count and swing_track meets each
    value of each flag (48 configurations; k and k // 8 differ in how they run through the fields)"""
    m = (k + k // 8) % 8
    return bool(m & 1), bool(m & 2), bool(m & 4)


def ref(pkg, scen, k):
    """the restatement of configuration k on all 257 robots (a robot's outputs do not depend on the batch: the first n rows are the reference of the first n robots)"""
    if ("ref", k) not in _SHARED:
        sc = walkers(scen)
        sub, track, name = CONFIGS[k]
        with_origin = flags(k)[0]
        r = HR.step(sc["params"], sc["wide"], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["Rz"], sc["target"], fields(pkg)[name], sc["origin"] if with_origin else None,
                    sc["ext"] if sub == 3 else None, 0.0025, sub, swing_track=track)
        for a in r:
            a.setflags(write=False)
        _SHARED[("ref", k)] = r
    return _SHARED[("ref", k)]


def edge_points_few(f):
    """edge_points(f), thinned on a field of more than 64 nodes to its first and last column of nodes, the points outside and the special ones: what a test that pays
    per point (a process per call, a batch of at most max_batch) takes"""
    pts = edge_points(f)
    k = f.nx * f.ny
    return pts if k <= 64 else pts[np.r_[0:f.ny, k - f.ny:k, 2 * k:len(pts)]]


def point_origins(rng, pts):
    """a random origin row per point and the points moved by it -> (origin (n, 3), moved points): dyadic shifts in x and y, exact to undo, and a lift; rows TINY keep
    a shift of +0.0 and their coordinates as they are (adding even +0.0 to -0.0 gives +0.0), so that (X - ox) - x0 is still X there"""
    n = len(pts)
    origin = np.concatenate([rng.integers(-4, 5, (n, 2)) * 0.25, rng.uniform(-0.02, 0.02, (n, 1))], 1)
    origin[TINY, :2] = 0.0
    moved = pts + origin[:, :2]
    moved[TINY] = pts[TINY]
    return origin, moved


def tiny_points_reach_the_rule(f, pts, origin=None):
    """on a field with x0 = y0 = 0.0: asserts that the grid coordinates the rule forms of rows TINY are ux = -1e-300 / dx (negative, tiny), uy = -1e-300 / dy, and
    (ux, uy) = (-0.0, -0.0) with the sign bit set -> True; on any other field -> False (nothing to assert: there they are node 0)"""
    if f.x0 != 0.0 or f.y0 != 0.0:
        return False
    X, Y = pts[TINY, 0], pts[TINY, 1]
    if origin is not None:
        X, Y = X - origin[TINY, 0], Y - origin[TINY, 1]
    ux, uy = (X - f.x0) * (1.0 / f.dx), (Y - f.y0) * (1.0 / f.dy)
    assert ux[0] == -1e-300 * (1.0 / f.dx) and -1e-299 < ux[0] < 0.0 and uy[1] == -1e-300 * (1.0 / f.dy) and -1e-299 < uy[1] < 0.0
    assert ux[2] == 0.0 and uy[2] == 0.0 and np.signbit(ux[2]) and np.signbit(uy[2])
    return True
