"""The plant-step kernel on the CPU: the product's kernel text compiled for the host (tests/emu/plant_host.py: 64 host threads in lock step are one wavefront) against the
elementwise numpy restatement of tests/plant_ref.py -- pos, R, v, omega and the feet bit for bit, the angles within 1e-12 -- and the physics checks of
tests/test_gpu_plant.py (which runs the same comparisons on the GPU) on the restatement, whose bits the kernel text has."""
import os, sys
import numpy as np
import pytest
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import plant_host as host
import plant_ref as PR


def _same(out, ref, n, stride):
    so, Ro, fo = out
    assert not np.isnan(so[:n, :12]).any() and not np.isnan(Ro[:n]).any() and not np.isnan(fo[:n]).any()
    assert np.isnan(so[n:]).all() and np.isnan(Ro[n:]).all() and np.isnan(fo[n:]).all() and np.isnan(so[:n, 12:]).all()   # the tail rows, and words [12:stride)
    assert PR.bits_equal(so[:n, 3:12], ref[0][:, 3:12]) and PR.bits_equal(Ro[:n], ref[1]) and PR.bits_equal(fo[:n], ref[2])
    worst = float(np.abs(so[:n, :3] - ref[0][:, :3]).max())
    assert worst <= PR.ANGLE_BAR, worst
    return worst


@pytest.mark.parametrize("with_ext", [False, True])
@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("n,stride", [(1, 12), (17, 13), (67, 22)])
def test_kernel_text_on_the_host_equals_the_restatement_bit_for_bit(scen, n, stride, substeps, with_ext):
    """a lone robot, a partly filled second wavefront, several workgroups with a partly filled last one; the three row widths; all 16 contact patterns (robot i has pattern
    i mod 16) from 17 robots on; one and four sub-steps; the wrench null and given.  NaN-poisoned rows beyond n and words [12:stride) stay NaN"""
    rng = np.random.default_rng(1000 * n + 10 * substeps + with_ext)
    sc = PR.random_robots(scen, rng, n)
    if n >= 16:
        assert len({tuple(c) for c in sc["contacts"]}) == 16
    state = np.concatenate([sc["state"], rng.normal(0, 1, (n, stride - 12))], 1)
    ext = sc["ext"] if with_ext else None
    ref = PR.step(sc["params"], state, sc["R"], sc["foot"], sc["grf"], sc["contacts"], ext, 0.0025, substeps)
    out = host.run(sc["params"], state, sc["R"], sc["foot"], sc["grf"], sc["contacts"], ext, 0.0025, substeps, rows=n + 5)
    worst = _same(out, ref, n, stride)
    moved = np.abs(ref[1] - sc["R"]).max(axis=1)
    print(f"n {n} stride {stride} substeps {substeps} ext {with_ext}: bits equal; angles within {worst:.1e}; the attitude moved by {moved.min():.1e} .. {moved.max():.1e}")
    assert (moved > 1e-6).all()   # (a kernel that returns its input would not pass)
    if with_ext:
        assert not PR.bits_equal(PR.step(sc["params"], state, sc["R"], sc["foot"], sc["grf"], sc["contacts"], None, 0.0025, substeps)[0][:, 3:12], ref[0][:, 3:12])


def test_kernel_text_structural_bit_equalities(scen):
    """in place == out of place, at a stride whose extra words must survive; robot i alone == robot i of the batch; a NaN force on a swing leg leaves the robot finite; a NaN
    pos poisons pos of that robot alone; the input angles are not read; other dt / gravity reach the result"""
    n = 37
    rng = np.random.default_rng(77)
    sc = PR.random_robots(scen, rng, n)
    P = sc["params"]
    state = np.concatenate([sc["state"], rng.normal(0, 1, (n, 10))], 1)
    args = (sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["ext"], 0.0025, 2)
    so, Ro, fo = host.run(P, state, *args)
    si, Ri, fi = host.run(P, state, *args, in_place=True)
    assert PR.bits_equal(si[:, :12], so[:, :12]) and PR.bits_equal(Ri, Ro) and PR.bits_equal(fi, fo) and np.array_equal(si[:, 12:], state[:, 12:])
    for i in (0, 15, 16, 36):
        one = host.run(P, state[i:i + 1], sc["R"][i:i + 1], sc["foot"][i:i + 1], sc["grf"][i:i + 1], sc["contacts"][i:i + 1], sc["ext"][i:i + 1], 0.0025, 2)
        assert PR.bits_equal(one[0][:, :12], so[i:i + 1, :12]) and PR.bits_equal(one[1], Ro[i:i + 1]) and PR.bits_equal(one[2], fo[i:i + 1])
    grf = sc["grf"].copy(); swing = np.argwhere(sc["contacts"] == 0)
    for i, l in swing:
        grf[i, 3 * l + (i + l) % 3] = np.nan
    sn = host.run(P, state, sc["R"], sc["foot"], grf, sc["contacts"], sc["ext"], 0.0025, 2)
    assert len(swing) > n and PR.bits_equal(sn[0][:, :12], so[:, :12]) and PR.bits_equal(sn[1], Ro) and PR.bits_equal(sn[2], fo)
    bad = state.copy(); bad[20, 4] = np.nan
    sb, Rb, fb = host.run(P, bad, *args)
    keep = np.arange(n) != 20
    assert PR.bits_equal(sb[keep, :12], so[keep, :12]) and PR.bits_equal(Rb, Ro) and np.isnan(sb[20, 4]) and np.isfinite(np.delete(sb[20, :12], 4)).all()
    other = state.copy(); other[:, :3] = rng.normal(0, 5, (n, 3))
    assert PR.bits_equal(host.run(P, other, *args)[0][:, :12], so[:, :12])
    for kw in (dict(dt=0.005), dict(gravity=-1.6)):
        a = host.run(P, state, sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["ext"], **dict(dict(dt=0.0025, substeps=2), **kw))
        b = PR.step(P, state, sc["R"], sc["foot"], sc["grf"], sc["contacts"], sc["ext"], **dict(dict(dt=0.0025, substeps=2), **kw))
        assert PR.bits_equal(a[0][:, 3:12], b[0][:, 3:12]) and not PR.bits_equal(a[0][:, 3:12], so[:, 3:12])


def test_step_0_brings_R_back_to_orthogonal_to_first_order(scen):
    """an R off by 1e-8 comes out orthogonal to that squared (the Newton step leaves 3/4 E^2) plus rounding; one that is orthogonal to rounding moves by an ulp at most; both in the kernel text's bits"""
    n = 16
    rng = np.random.default_rng(79)
    sc = PR.random_robots(scen, rng, n)
    off = sc["R"] + rng.normal(0, 1e-8, (n, 9))
    orth = lambda R: float(np.abs(np.einsum("bji,bjk->bik", R.reshape(-1, 3, 3), R.reshape(-1, 3, 3)) - np.eye(3)).max())
    P = np.stack(PR.polish([off[:, k] for k in range(9)]), 1)
    assert orth(off) > 1e-9 and orth(P) <= orth(off) ** 2 + 1e-15 and np.abs(P - off).max() < 1e-7
    assert np.abs(np.stack(PR.polish([sc["R"][:, k] for k in range(9)]), 1) - sc["R"]).max() <= 2.3e-16
    st = sc["state"].copy(); st[:, 6:9] = 0.0   # (omega = 0: the Cayley factor is the identity, R_out is step 0's R)
    out = host.run(sc["params"], st, off, sc["foot"], sc["grf"], np.zeros((n, 4), np.uint8))
    assert PR.bits_equal(out[1], P)


def test_cofactor_inverse_is_the_inverse(scen):
    for ps in scen.PARAM_SETS.values():
        I = np.asarray(ps["inertia"], float).reshape(3, 3) + np.array([[0, -3.66e-5, -6.11e-5], [-3.66e-5, 0, -2.75e-5], [-6.11e-5, -2.75e-5, 0]])
        Ii = np.array(PR.inverse_by_cofactors(list(I.reshape(9)))).reshape(3, 3)
        assert np.abs(Ii @ I - np.eye(3)).max() <= 1e-14


def test_kernel_text_chained_in_place_follows_the_restatement(scen):
    """30 calls in place on tick records, R and feet (what the closed loop does): bit for bit the restatement's chain; the command half of the records survives"""
    n = 19
    rng = np.random.default_rng(78)
    sc = PR.random_robots(scen, rng, n)
    tick = np.concatenate([sc["state"], rng.normal(0, 1, (n, 10))], 1)
    a, b = (tick, sc["R"], sc["foot"]), (tick, sc["R"], sc["foot"])
    for _ in range(30):
        a = host.run(sc["params"], a[0], a[1], a[2], sc["grf"], sc["contacts"], None, 0.0025, 1, in_place=True)
        b = PR.step(sc["params"], b[0], b[1], b[2], sc["grf"], sc["contacts"], None, 0.0025, 1)
    assert PR.bits_equal(a[0][:, 3:12], b[0][:, 3:12]) and PR.bits_equal(a[1], b[1]) and PR.bits_equal(a[2], b[2]) and np.array_equal(a[0][:, 12:], tick[:, 12:])
    assert np.abs(a[0][:, :3] - b[0][:, :3]).max() <= PR.ANGLE_BAR


# ---- the physics checks of tests/test_gpu_plant.py, here on the restatement (the kernel text has its bits: above), 64 robots
def _stepper(scen):
    return PR.ref_stepper(dict(scen.PARAM_SETS["gazebo"], **scen.MPC_CONSTANTS)), 64


def test_torque_free_flight_keeps_orthogonality_and_the_swing_feet(scen):
    step, n = _stepper(scen)
    dL, orth, feet = PR.torque_free_flight(step, scen, n=n)
    print(f"400 calls without contacts: |R R' - I| {orth:.1e}, swing feet in the body frame {feet:.1e} (|dL| / |L| {dL:.1e})")
    assert orth <= 1e-12 and feet <= 1e-10


def test_torque_free_flight_keeps_world_angular_momentum(scen):
    """R I_b R' omega after 400 CALLS against before, relative, the worst of the robots; bar 1e-12.  L is carried inside a call only: the next call rebuilds it from omega
    through R, and R'R - I enters that rebuild times the inertia's condition number 3.  Step 0 of the scheme (R <- R - R (R'R - I) / 2 at the start of a call) keeps the
    rounding of earlier Cayley products from piling up in R'R: 7e-14 with it (six seeds: 6.8e-14 .. 7.7e-14), 1.8e-12 .. 4.1e-12 without."""
    step, n = _stepper(scen)
    dL, _, _ = PR.torque_free_flight(step, scen, n=n)
    print(f"400 calls without contacts: |dL| / |L| {dL:.2e}")
    assert dL <= 1e-12


def test_free_fall_follows_the_closed_forms(scen):
    step, n = _stepper(scen)
    dv, dz = PR.free_fall(step, scen, n=n)
    print(f"400 calls of free fall: v_z off by {dv:.1e}, pos_z by {dz:.1e}")
    assert dv <= 1e-10 and dz <= 1e-10


def test_a_standing_robot_does_not_move(scen):
    step, n = _stepper(scen)
    moved = PR.standing(step, scen, n=n)
    print(f"400 calls standing on m g / 4 per leg: largest move {moved:.1e}")
    assert moved <= 1e-12


def test_the_scheme_is_first_order_in_h(scen):
    step, n = _stepper(scen)
    r1, r2 = PR.rotation_order(step, scen, n=n)
    print(f"rotation error against 4096 sub-steps shrinks by {r1:.3f} (40 -> 80 steps) and {r2:.3f} (80 -> 160)")
    assert 1.7 <= r1 <= 2.4 and 1.7 <= r2 <= 2.4
