"""Height-field terrain on the CPU: the product's kernel text compiled for the host (tests/emu/heightfield_host.py: 64 host threads in lock step are one wavefront)
against the elementwise numpy restatement of tests/heightfield_ref.py -- the sampling rule on its edge cases, the step on the smallest fields at which indexing can go
wrong, the reductions to the ground step and to a robot alone, and ground_out as the episode record's ground row."""
import numpy as np
import pytest

import episode_ref as ER
import heightfield_cases as HC
import heightfield_host as host
import heightfield_ref as HR
import plant_ref as PR
import walk_step_ground_host as ground_host

SIZES = (1, 15, 16, 17, 65, 257)
NMAX = HC.NMAX
_SHARED = {}


# ---- the sampling rule
def test_the_kernel_text_and_the_restatement_on_points_whose_height_is_known():
    """heights worked out by hand, held against the restatement AND the sample kernel's text: nodes give their own height under both rules; cell-constant cells are
    half-open and the last node owns only its line; the bilinear rule is exact on a field whose values are dyadic; outside the grid the edge values; inf is clamped, a
    NaN gives a NaN; an origin row moves and lifts the field"""
    H = np.array([[1.0, 2.0, 4.0], [8.0, 16.0, 32.0]])

    def both(f, X, Y, origin=None):
        X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
        r, k = HR.sample(f, X, Y, origin), host.sample(f, np.stack([X, Y], 1), origin)
        assert HR.same_heights(r, k)
        return k
    for interp in (0, 1):
        f = HR.Field(H, 10.0, -3.0, 0.5, 2.0, interp)
        X, Y = np.meshgrid(10.0 + 0.5 * np.arange(3), -3.0 + 2.0 * np.arange(2))
        assert np.array_equal(both(f, X.ravel(), Y.ravel()), H.ravel())
        assert np.array_equal(both(f, [-np.inf, np.inf, 9.0, 99.0], [-np.inf, np.inf, 99.0, -99.0]), [1.0, 32.0, 8.0, 4.0])
        assert np.isnan(both(f, [np.nan, 10.0, np.nan], [-3.0, np.nan, np.nan])).all()
        assert np.array_equal(both(f, [110.5], [197.0], np.array([[100.0, 200.0, 0.25]])), [2.25])
    f0, f1 = HR.Field(H, 10.0, -3.0, 0.5, 2.0, 0), HR.Field(H, 10.0, -3.0, 0.5, 2.0, 1)
    assert np.array_equal(both(f0, [10.49, 10.5, 10.99, 11.0, 10.99], [-3.0, -1.01, -1.0, -1.01, -1.0]), [1.0, 2.0, 16.0, 4.0, 16.0])
    assert np.array_equal(both(f1, [10.25, 10.75, 10.25], [-3.0, -3.0, -2.0]), [1.5, 3.0, 0.5 * (1.5 + 12.0)])
    # X = -1e-300 and X = -0.0 on a field whose node (0, 0) is the world's origin: ux is a tiny negative / -0.0, clamped to node 0, never an index of -1
    for interp in (0, 1):
        z = HR.Field(H, 0.0, 0.0, 0.5, 2.0, interp)
        assert np.array_equal(both(z, [-1e-300, -0.0, 0.5, -1e-300], [0.0, -0.0, -1e-300, -1e-300]), [1.0, 1.0, 2.0, 1.0])
        assert np.array_equal(both(z, [-1e-300, -0.0], [-0.0, -1e-300], np.array([[0.0, 0.0, 0.5], [0.0, 0.0, 0.5]])), [1.5, 1.5])


@pytest.mark.parametrize("with_origin", [False, True])
def test_sample_kernel_text_on_the_host_equals_the_restatement_on_the_edge_cases(pkg, with_origin):
    """every field, and two at the world's origin on which X = -1e-300 and X = -0.0 reach the rule as ux = -1e-300 / dx and ux = -0.0 (asserted); the edge points
    (through a random origin row per point as well: the points are moved by it, so the same grid coordinates come out up to rounding); heights bit for bit, NaN where X or Y is one and nowhere else; +-inf give a finite height; points exactly on nodes give the node's height; the tail stays poisoned"""
    rng = np.random.default_rng(9500)
    tiny = 0
    for name, f in HC.point_fields(pkg).items():
        pts = HC.edge_points(f)
        n = len(pts)
        origin = None
        if with_origin:
            origin, pts = HC.point_origins(rng, pts)
        tiny += HC.tiny_points_reach_the_rule(f, pts, origin)   # (asserts ux = -1e-300 / dx and ux = -0.0 where the field lets them through)
        out = host.sample(f, pts, origin, rows=n + 5)
        ref = HR.sample(f, pts[:, 0], pts[:, 1], origin)
        assert (out[n:] == -1e300).all() and HR.same_heights(out[:n], ref), name
        at0 = pts[HC.TINY].copy(); at0[0, 0] = f.x0 if origin is None else f.x0 + origin[n - 13, 0]; at0[1, 1] = f.y0 if origin is None else f.y0 + origin[n - 12, 1]
        at0[2] = [f.x0, f.y0] if origin is None else [f.x0 + origin[n - 11, 0], f.y0 + origin[n - 11, 1]]
        assert HR.same_heights(out[:n][HC.TINY], HR.sample(f, at0[:, 0], at0[:, 1], None if origin is None else origin[HC.TINY])), name   # a hair below node 0 IS node 0
        nan = np.isnan(pts).any(axis=1)
        assert nan.sum() == 4 and np.array_equal(np.isnan(out[:n]), nan) and np.isinf(pts[~nan]).any(axis=1).sum() == 6
        if not with_origin:
            nodes = out[:f.nx * f.ny].reshape(f.nx, f.ny).T   # (edge_points walks x outermost)
            # (bilinear on the LAST node of an axis is h00 + 1 * (h10 - h00): the node's height up to one rounding, exact everywhere else)
            # on the 5 x 3 field a node's own coordinates x0 + i dx need not come back as i exactly: the claim is held where they do (node 0 of each axis always does)
            k = f.nx * f.ny
            ux, uy = ((pts[:k, 0] - f.x0) * (1.0 / f.dx)).reshape(f.nx, f.ny).T, ((pts[:k, 1] - f.y0) * (1.0 / f.dy)).reshape(f.nx, f.ny).T
            on = (ux == np.arange(f.nx)[None, :]) & (uy == np.arange(f.ny)[:, None])
            assert on[0, 0] and (on.all() or name.startswith("5x3")), (name, on.sum())   # (so ux == nx - 1 and uy == ny - 1 exactly are among the points)
            inner = on.copy()
            if f.interp == 1:
                inner[-1, :] = False; inner[:, -1] = False
            assert np.array_equal(nodes[inner], f.H[inner]) and np.abs(nodes - f.H)[on].max() <= 2e-17, name
            corners = np.array([out[n - 11] - f.H[0, 0], out[n - 6] - f.H[0, f.nx - 1], out[n - 5] - f.H[f.ny - 1, 0]])   # (-0.0, -0.0); (inf, -inf); (-inf, inf)
            assert corners[0] == 0.0 and np.abs(corners).max() <= (0.0 if f.interp == 0 else 2e-17), (name, corners)
    assert tiny == 2   # the two fields at the world's origin
    print("edge cases:", n, "points on the last field,", len(HC.point_fields(pkg)), "fields")


# ---- the step
def _same_step(out, ref, n, stride, in_place, wide):
    so, Ro, fo, vo, to, go = out
    assert not np.isnan(so[:n, :12]).any() and not np.isnan(Ro[:n]).any() and not np.isnan(fo[:n]).any() and not np.isnan(vo[:n]).any()
    assert np.isnan(vo[n:]).all() and (to[n:] == 0xFF).all()
    if in_place:
        assert np.array_equal(so[:, 12:], wide[:n, 12:stride])   # (the command half of a tick record survives)
    else:
        assert np.isnan(so[n:]).all() and np.isnan(Ro[n:]).all() and np.isnan(fo[n:]).all() and np.isnan(so[:n, 12:]).all()
    assert PR.bits_equal(so[:n, 3:12], ref[0][:n, 3:12]) and PR.bits_equal(Ro[:n], ref[1][:n]) and PR.bits_equal(fo[:n], ref[2][:n]) and PR.bits_equal(vo[:n], ref[3][:n])
    assert np.array_equal(to[:n], ref[4][:n])
    if go is not None:
        assert np.isnan(go[n:]).all() and PR.bits_equal(go[:n], ref[5][:n])   # (the two zeros are +0)
    worst = float(np.abs(so[:n, :3] - ref[0][:n, :3]).max())
    assert worst <= PR.ANGLE_BAR, worst
    return worst


@pytest.mark.parametrize("stride", [12, 13, 22])
@pytest.mark.parametrize("n", SIZES)
def test_step_kernel_text_on_the_host_equals_the_restatement_bit_for_bit(pkg, scen, n, stride):
    """a lone robot, either side of a wavefront edge, several workgroups with a partly filled last one; the three row widths; sub-steps 1 (no wrench) and 3 (with one);
    swing_track 0 / 0.5 / 1; the eight fields; with and without origin and ground_out, in place and out of place.  pos, R, v, omega, the feet, foot_vel_body, touch and
    ground_out bit for bit, the angles within the walk tests' bar; poisoned rows beyond n and words [12:stride) stay poisoned"""
    sc = HC.walkers(scen)
    worst = 0.0
    seen = set()
    for k, (sub, track, name) in enumerate(HC.CONFIGS):
        with_origin, with_out, in_place = HC.flags(k)
        seen.add((name, with_origin, with_out, in_place))
        out = host.run(sc["params"], sc["wide"][:n, :stride], sc["R"][:n], sc["foot"][:n], sc["grf"][:n], sc["contacts"][:n], sc["Rz"][:n], sc["target"][:n], HC.fields(pkg)[name],
                       sc["origin"][:n] if with_origin else None, sc["ext"][:n] if sub == 3 else None, 0.0025, sub, swing_track=track, rows=n if in_place else n + 5,
                       in_place=in_place, ground_out=with_out)
        assert (out[5] is None) == (not with_out)
        worst = max(worst, _same_step(out, HC.ref(pkg, scen, k), n, stride, in_place, sc["wide"]))
    for name in HC.fields(pkg):
        for flag in range(3):
            assert {s[1 + flag] for s in seen if s[0] == name} == {False, True}, (name, flag)
    print(f"n {n} stride {stride}: {len(HC.CONFIGS)} configurations bit for bit; angles within {worst:.1e}")


def test_the_inputs_reach_both_sides_of_the_fields_and_every_node(pkg, scen):
    """on every field there are swing feet below the ground (lifted, touch 1) and above it (left alone, touch 0); feet land on every node of the small fields and beyond
    every side of them; the bodies too"""
    sc = HC.walkers(scen)
    swing = sc["contacts"] == 0
    for k, (sub, track, name) in enumerate(HC.CONFIGS):
        if sub != 1 or track != 1.0:
            continue
        so, _, fo, _, touch, go = HC.ref(pkg, scen, k)
        assert touch[swing].sum() >= 10 and (touch[swing] == 0).sum() >= 10, name
        f = HC.fields(pkg)[name]
        if f.nx * f.ny > 16:
            continue
        o = sc["origin"] if HC.flags(k)[0] else np.zeros((NMAX, 3))
        ux = ((so[:, 3:4] + fo.reshape(NMAX, 4, 3)[:, :, 0]) - o[:, 0:1] - f.x0) / f.dx; uy = ((so[:, 4:5] + fo.reshape(NMAX, 4, 3)[:, :, 1]) - o[:, 1:2] - f.y0) / f.dy
        assert (ux < 0).any() and (ux > f.nx - 1).any() and (uy < 0).any() and (uy > f.ny - 1).any(), name
        cells = {(int(a), int(b)) for a, b in zip(np.clip(ux, 0, f.nx - 1).ravel(), np.clip(uy, 0, f.ny - 1).ravel())}
        assert len(cells) == f.nx * f.ny or f.interp == 1, (name, cells)


@pytest.mark.parametrize("interp", [0, 1])
def test_a_constant_field_reduces_to_the_ground_step(scen, interp):
    """a constant field of the value c, origin NULL: every other output is the ground step's kernel text's with ground = (c, 0, 0), bit for bit; ground_out is (c, 0, 0)"""
    sc = HC.walkers(scen)
    c = 0.0375
    a = (sc["params"], sc["wide"][:, :13], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["Rz"], sc["target"])
    level = np.tile([c, 0.0, 0.0], (NMAX, 1))
    shape = (2, 3) if interp else (1, 1)
    f = HR.Field(np.full(shape, c), -0.3, 0.2, 0.4, 0.7, interp)
    for sub, track in ((1, 1.0), (3, 0.5), (2, 0.0)):
        g = ground_host.run(*a, level, sc["ext"], dt=0.0025, substeps=sub, swing_track=track)
        h = host.run(*a, f, None, sc["ext"], dt=0.0025, substeps=sub, swing_track=track)
        assert all(PR.bits_equal(x, y) for x, y in zip(h[:4], g[:4])) and np.array_equal(h[4], g[4]) and PR.bits_equal(h[5], level), (sub, track)
        assert (g[4][sc["contacts"] == 0] == 1).any() and (g[4][sc["contacts"] == 0] == 0).any()


def test_a_robot_alone_is_the_robot_in_the_batch(pkg, scen):
    """robot i alone == robot i of the 257, in whichever wavefront and lane it sat; in place == out of place"""
    sc = HC.walkers(scen)
    f = HC.fields(pkg)["64x48/1"]
    kw = dict(dt=0.0025, substeps=2, swing_track=1.0)
    args = lambda sl: (sc["params"], sc["wide"][sl, :22], sc["R"][sl], sc["foot"][sl], sc["grf"][sl], sc["contacts"][sl], sc["Rz"][sl], sc["target"][sl], f, sc["origin"][sl],
                       sc["ext"][sl])
    base = host.run(*args(slice(0, NMAX)), **kw)
    for i in (0, 15, 16, 36, 255, 256):
        one = host.run(*args(slice(i, i + 1)), **kw)
        assert all(PR.bits_equal(x[:, :12], y[i:i + 1, :12]) for x, y in zip(one[:4], base[:4])) and np.array_equal(one[4], base[4][i:i + 1]), i
        assert PR.bits_equal(one[5], base[5][i:i + 1])
    part = host.run(*args(slice(100, 137)), **kw)
    assert all(PR.bits_equal(x[:, :12], y[100:137, :12]) for x, y in zip(part[:4], base[:4])) and PR.bits_equal(part[5], base[5][100:137])


def test_ground_out_is_the_episode_records_ground_row(pkg, scen):
    """the episode update fed ground_out has the height pos_z - hf(pos_x, pos_y), bit for bit: its record equals the record of an update without a ground on a state
    whose pos_z IS that difference (computed here from the restatement of the rule), and the height ends the episodes of the robots that stand too low on the field"""
    sc = HC.walkers(scen)
    f = HC.fields(pkg)["64x48/1"]
    so, Ro, fo, vo, touch, go = host.run(sc["params"], sc["wide"][:, :12], sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["Rz"], sc["target"], f, sc["origin"], None, 0.0025, 1)
    want = so[:, 5] - HR.sample(f, so[:, 3], so[:, 4], sc["origin"])
    above = so.copy(); above[:, 5] = want
    zero = np.zeros((NMAX, ER.WORDS))
    d_z = np.full(NMAX, 0.3)
    cfg = dict(ER.DEFAULT, min_up=-2.0, min_height=0.3)
    a = ER.update(zero, 0, so, Ro, root_pos_d_z=d_z, ground=go, cfg=cfg)
    b = ER.update(zero, 0, above, Ro, root_pos_d_z=d_z, cfg=cfg)
    assert ER.bits_equal(a, b)
    ended = a[:, ER.W["end_code"]] == 3.0
    assert np.array_equal(ended, want < 0.3) and ended.sum() >= 10 and (~ended).sum() >= 10
    assert ER.bits_equal(a[~ended, ER.W["height_err_sum"]], (want[~ended] - 0.3) * (want[~ended] - 0.3))
