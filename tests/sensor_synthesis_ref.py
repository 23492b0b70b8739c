"""a1mpc_sensor_synthesis_batch restated in numpy, ELEMENTWISE: every value is a vector over the robots and every operation one IEEE add, subtract, multiply, divide or
sqrt in the order include/a1mpc.h states (three-term sums left to right, the legs as (0 + 1) + (2 + 3)) -- no `@`, no einsum, no sum(), so neither BLAS nor a fused
multiply-add can enter.  The outputs that pass through + - * / alone (gyro, accelerometer, foot force, foot_pos_rel, foot_vel_rel) equal the kernel's bit for bit; the
others pass through sqrt / atan2 / acos / sin / cos and are held by the tolerance rule of `noise_floor`: the restatement is evaluated in float64 and in the 80-bit
numpy.longdouble on the test's own inputs, E = the largest difference per output array is this computation's float64 noise floor, and the gate is |kernel - 80-bit| <= 4 E
(a second libm at 1-2 ulp and the device sqrt fit in the factor; a formula error shows at 1e-3 or more).  Test infrastructure only."""
import numpy as np

BITS = ("imu_gyro_raw", "imu_acc_raw", "foot_force", "foot_pos_rel", "foot_vel_rel")   # + - * / alone: bit for bit
NOISY = ("quat", "joint_pos", "joint_vel")                                            # through sqrt / atan2 / acos / sin / cos: within 4 E of the 80-bit evaluation
OUTPUTS = ("quat", "imu_acc_raw", "imu_gyro_raw", "joint_pos", "joint_vel", "foot_force", "reach", "foot_pos_rel", "foot_vel_rel")
FACTOR = 4.0
A1_RHO_FIX = np.array([[0.1805, 0.047, 0.0838, 0.21, 0.21], [0.1805, -0.047, -0.0838, 0.21, 0.21], [-0.1805, 0.047, 0.0838, 0.21, 0.21],
                       [-0.1805, -0.047, -0.0838, 0.21, 0.21]])


def _mv(M, x):
    return [(M[3 * i] * x[0] + M[3 * i + 1] * x[1]) + M[3 * i + 2] * x[2] for i in range(3)]


def _mtv(M, x):
    return [(M[i] * x[0] + M[3 + i] * x[1]) + M[6 + i] * x[2] for i in range(3)]


def _pick(i, a0, a1, a2):
    return np.where(i == 0, a0, np.where(i == 1, a1, a2))


def quaternion_of(R, dtype=np.float64):
    """Eigen's matrix-to-quaternion (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl for a 3 x 3): R a list of 9 vectors, row-major -> [w, x, y, z]"""
    one, half = dtype(1.0), dtype(0.5)
    tr = (R[0] + R[4]) + R[8]
    pos = tr > 0
    i = np.where(R[4] > R[0], np.where(R[8] > R[4], 2, 1), np.where(R[8] > R[0], 2, 0))
    dii, djj, dkk = _pick(i, R[0], R[4], R[8]), _pick(i, R[4], R[8], R[0]), _pick(i, R[8], R[0], R[4])
    kj, jk = _pick(i, R[7], R[2], R[3]), _pick(i, R[5], R[6], R[1])
    ji, ij = _pick(i, R[3], R[7], R[2]), _pick(i, R[1], R[5], R[6])
    ki, ik = _pick(i, R[6], R[1], R[5]), _pick(i, R[2], R[3], R[7])
    t = np.sqrt(np.where(pos, tr + one, ((dii - djj) - dkk) + one))
    hq, u = half * t, half / t
    qi, qw, qj, qk = hq, (kj - jk) * u, (ji + ij) * u, (ki + ik) * u
    return [np.where(pos, hq, qw), np.where(pos, (R[7] - R[5]) * u, _pick(i, qi, qk, qj)), np.where(pos, (R[2] - R[6]) * u, _pick(i, qj, qi, qk)),
            np.where(pos, (R[3] - R[1]) * u, _pick(i, qk, qj, qi))]


def quaternion_branch(R):
    """(n, 9) -> which of Eigen's four branches a row takes: 3 = positive trace, else the largest diagonal"""
    R = np.asarray(R, np.float64).reshape(-1, 9)
    i = np.where(R[:, 4] > R[:, 0], np.where(R[:, 8] > R[:, 4], 2, 1), np.where(R[:, 8] > R[:, 0], 2, 0))
    return np.where((R[:, 0] + R[:, 4]) + R[:, 8] > 0, 3, i)


def leg_geometry(fix, opt, l, dtype=np.float64):
    f, o = [dtype(x) for x in np.asarray(fix, np.float64).reshape(4, 5)[l]], [dtype(x) for x in np.asarray(opt, np.float64).reshape(4, 3)[l]]
    return dict(ox=f[0], oy=f[1], L=f[2] + o[1], lt=f[3], al=f[4] - o[2], r0=o[0])


def forward_leg(g, q):
    """a1mpc_leg_kernel's forward map and Jacobian for one leg: q a list of 3 vectors -> (p (3), J (9, the kernel's J[3 c + row]))"""
    s0, c0, s1, c1, s12, c12 = np.sin(q[0]), np.cos(q[0]), np.sin(q[1]), np.cos(q[1]), np.sin(q[1] + q[2]), np.cos(q[1] + q[2])
    Xq = g["r0"] * c12 - g["al"] * s12; Zq = -(g["al"] * c12) - g["r0"] * s12
    Xr = Xq - g["lt"] * s1; Zp = Zq - g["lt"] * c1
    p = [g["ox"] + Xr, g["oy"] + (g["L"] * c0 - Zp * s0), g["L"] * s0 + Zp * c0]
    zero = p[0] * 0
    J = [zero, -p[2], p[1] - g["oy"], Zp, s0 * Xr, -(c0 * Xr), Zq, s0 * Xq, -(c0 * Xq)]
    return p, J


def inverse_leg(g, p, dtype=np.float64):
    """the closed-form inverse: p a list of 3 vectors -> (q (3), flags)"""
    zero, one, two = dtype(0.0), dtype(1.0), dtype(2.0)
    dx, dy = p[0] - g["ox"], p[1] - g["oy"]
    yz, LL = dy * dy + p[2] * p[2], g["L"] * g["L"]
    clamp0 = yz < LL
    Zp = -np.sqrt(np.where(clamp0, zero, yz - LL))
    q0 = np.arctan2(p[2], dy) - np.arctan2(Zp, g["L"])
    ell, phi = np.sqrt(g["al"] * g["al"] + g["r0"] * g["r0"]), np.arctan2(g["r0"], g["al"])
    c = (((dx * dx + Zp * Zp) - g["lt"] * g["lt"]) - ell * ell) / ((two * g["lt"]) * ell)
    clamp1 = (c < -one) | (c > one)
    k = -np.arccos(np.where(c > one, one, np.where(c < -one, -one, c)))
    q1 = np.arctan2(-dx, -Zp) - np.arctan2(ell * np.sin(k), g["lt"] + ell * np.cos(k))
    return [q0, q1, k + phi], clamp0.astype(np.uint8) | (clamp1.astype(np.uint8) << 1)


def inverse_by_cofactors(I):
    c00 = I[4] * I[8] - I[5] * I[7]; c01 = I[5] * I[6] - I[3] * I[8]; c02 = I[3] * I[7] - I[4] * I[6]
    d = 1.0 / ((I[0] * c00 + I[1] * c01) + I[2] * c02)
    return [c00 * d, (I[2] * I[7] - I[1] * I[8]) * d, (I[1] * I[5] - I[2] * I[4]) * d,
            c01 * d, (I[0] * I[8] - I[2] * I[6]) * d, (I[2] * I[3] - I[0] * I[5]) * d,
            c02 * d, (I[1] * I[6] - I[0] * I[7]) * d, (I[0] * I[4] - I[1] * I[3]) * d]


def synthesise(mass, state, R, foot, grf, contacts, ext=None, rho_fix=A1_RHO_FIX, rho_opt=None, dtype=np.float64):
    """state (n, >= 12) rows of [euler, pos, omega, v] of which omega and v are read, R (n, 9), foot (n, 12), grf (n, 12) body frame, contacts (n, 4), ext None or (n, 6)
    -> dict of OUTPUTS in `dtype` (reach uint8)"""
    with np.errstate(all="ignore"):
        fx = lambda a: np.ascontiguousarray(a, dtype=np.float64).astype(dtype)
        state, R, foot, grf = fx(state), fx(R).reshape(-1, 9), fx(foot).reshape(-1, 12), fx(grf).reshape(-1, 12)
        n = R.shape[0]
        ct = np.asarray(contacts).reshape(n, 4) != 0
        opt = np.zeros((4, 3)) if rho_opt is None else rho_opt
        m, zero = dtype(mass), np.zeros(n, dtype)
        w = [state[:, 6 + k] for k in range(3)]; v = [state[:, 9 + k] for k in range(3)]
        Rm = [R[:, k] for k in range(9)]
        r = [[foot[:, 3 * l + k] for k in range(3)] for l in range(4)]
        f = [[np.where(ct[:, l], grf[:, 3 * l + k], zero) for k in range(3)] for l in range(4)]
        gyro = _mtv(Rm, w)
        acc = [((f[0][k] + f[1][k]) + (f[2][k] + f[3][k])) / m for k in range(3)]
        if ext is not None:
            e = fx(ext).reshape(n, 6)
            feb = _mtv(Rm, [e[:, k] for k in range(3)])
            acc = [acc[k] + feb[k] / m for k in range(3)]
        quat = quaternion_of(Rm, dtype)
        ff, jp, jv, pr, vr, reach = [], [], [], [], [], []
        for l in range(4):
            g = leg_geometry(rho_fix, opt, l, dtype)
            ff.append(np.where(ct[:, l], (Rm[6] * grf[:, 3 * l] + Rm[7] * grf[:, 3 * l + 1]) + Rm[8] * grf[:, 3 * l + 2], zero))
            p = _mtv(Rm, r[l])
            q, flags = inverse_leg(g, p, dtype)
            u = [v[0] + (w[1] * r[l][2] - w[2] * r[l][1]), v[1] + (w[2] * r[l][0] - w[0] * r[l][2]), v[2] + (w[0] * r[l][1] - w[1] * r[l][0])]
            ub = _mtv(Rm, u)
            fv = [np.where(ct[:, l], -ub[k], zero) for k in range(3)]
            _, J = forward_leg(g, q)
            Ji = inverse_by_cofactors([J[0], J[3], J[6], J[1], J[4], J[7], J[2], J[5], J[8]])
            qd = [np.where(flags != 0, zero, x) for x in _mv(Ji, fv)]
            jp += q; jv += qd; pr += p; vr += fv; reach.append(flags)
        S = lambda cols: np.stack(cols, 1)
        return dict(quat=S(quat), imu_acc_raw=S(acc), imu_gyro_raw=S(gyro), joint_pos=S(jp), joint_vel=S(jv), foot_force=S(ff), reach=S(reach), foot_pos_rel=S(pr),
                    foot_vel_rel=S(vr))


def bits_equal(a, b):
    """the same doubles bit for bit, except that any NaN equals any NaN"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def noise_floor(ref64, ref80, keys=NOISY):
    """E per output array: the largest |float64 evaluation - 80-bit evaluation| on these inputs"""
    return {k: float(np.abs(ref64[k].astype(np.longdouble) - ref80[k]).max()) for k in keys}


def assert_is_ref(out, ref64, ref80, n, label=""):
    """out: dict of OUTPUTS (float64; foot_pos_rel / foot_vel_rel may be None) whose first n rows are the first n robots of the references.  BITS bit for bit, reach
    equal, NOISY within FACTOR * E of the 80-bit evaluation, E taken over ALL rows of the references (the test's own inputs: a suite computes them once and checks every
    batch size against their head) -> {key: (error against the 80-bit evaluation, E)}"""
    for k in BITS:
        if out.get(k) is not None:
            assert bits_equal(out[k][:n], ref64[k][:n]), (label, k)
    assert np.array_equal(out["reach"][:n], ref64["reach"][:n]), (label, "reach")
    E = noise_floor(ref64, ref80)
    figs = {}
    for k in NOISY:
        err = float(np.abs(out[k][:n].astype(np.longdouble) - ref80[k][:n]).max())
        figs[k] = (err, E[k])
        assert err <= FACTOR * E[k], (label, k, err, E[k])
    return figs


# ---- the round trips through the stages the synthesis inverts (a1mpc_leg_state_batch, a1mpc_sensor_frontend_batch), restated in `dtype`
ROUND_TRIPS = ("foot_abs", "v_stance", "R_world", "omega")


def rotation_of(q, dtype=np.float64):
    """Eigen::Quaternion::toRotationMatrix as the sensor front end spells it: q = [w, x, y, z] vectors -> 9 vectors, row-major"""
    one, two = dtype(1.0), dtype(2.0)
    w, x, y, z = q
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return [one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx, txz - twy, tyz + twx, one - (txx + tyy)]


def stance_velocity(R, vrel, gyro, p):
    """-R (v_rel + gyro x p) per leg: what the EKF takes for the body's velocity from a stance leg (A1BasicEKF.cpp:122); (n, 9), (n, 12), (n, 3), (n, 12) -> (n, 12)"""
    Rm = [R[:, k] for k in range(9)]; g = [gyro[:, k] for k in range(3)]; out = []
    for l in range(4):
        pl = [p[:, 3 * l + k] for k in range(3)]; vl = [vrel[:, 3 * l + k] for k in range(3)]
        t = [vl[0] + (g[1] * pl[2] - g[2] * pl[1]), vl[1] + (g[2] * pl[0] - g[0] * pl[2]), vl[2] + (g[0] * pl[1] - g[1] * pl[0])]
        out += [-x for x in _mv(Rm, t)]
    return np.stack(out, 1)


def round_trips(syn, R, rho_fix=A1_RHO_FIX, rho_opt=None, dtype=np.float64):
    """syn: synthesise(..., dtype=dtype) of robots with attitude R -> dict of ROUND_TRIPS: foot_abs = R p(joint_pos) and v_stance = -R (J(joint_pos) joint_vel + gyro x
    p(joint_pos)), the leg stage's forward map and Jacobian; R_world = the front end's matrix of the quaternion and omega = R_world gyro"""
    fx = lambda a: np.ascontiguousarray(a, dtype=np.float64).astype(dtype)
    R = fx(R).reshape(-1, 9)
    Rm = [R[:, k] for k in range(9)]
    opt = np.zeros((4, 3)) if rho_opt is None else rho_opt
    fa, pr, vr = [], [], []
    for l in range(4):
        q = [syn["joint_pos"][:, 3 * l + k] for k in range(3)]; qd = [syn["joint_vel"][:, 3 * l + k] for k in range(3)]
        p, J = forward_leg(leg_geometry(rho_fix, opt, l, dtype), q)
        pr += p; fa += _mv(Rm, p)
        vr += [(J[r] * qd[0] + J[3 + r] * qd[1]) + J[6 + r] * qd[2] for r in range(3)]
    Rq = rotation_of([syn["quat"][:, k] for k in range(4)], dtype)
    return dict(foot_abs=np.stack(fa, 1), v_stance=stance_velocity(R, np.stack(vr, 1), syn["imu_gyro_raw"], np.stack(pr, 1)), R_world=np.stack(Rq, 1),
                omega=np.stack(_mv(Rq, [syn["imu_gyro_raw"][:, k] for k in range(3)]), 1))


# ---- the inputs both suites feed
def rotation_about(axis, angle):
    """(n,) angles about a unit axis (3,) -> (n, 9) row-major, Rodrigues"""
    a = np.asarray(axis, float); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    ang = np.asarray(angle, float).reshape(-1, 1, 1)
    return (np.eye(3)[None] + np.sin(ang) * K[None] + (1 - np.cos(ang)) * (K @ K)[None]).reshape(-1, 9)


def forward_feet(rho_fix, rho_opt, q):
    """(n, 12) joint angles -> (n, 12) body-frame feet through the forward map"""
    q = np.asarray(q, np.float64).reshape(-1, 12); out = []
    for l in range(4):
        p, _ = forward_leg(leg_geometry(rho_fix, rho_opt, l), [q[:, 3 * l + k] for k in range(3)])
        out += p
    return np.stack(out, 1)


def random_robots(scen, rng, n, rho_opt=None):
    """n robots: attitudes |roll|, |pitch| <= 0.5 at any yaw, except that rows 1, 2, 3 (mod 16, as far as n reaches) are turned by nearly pi about x, y, z, so that all four
    quaternion branches occur from n = 4 on; feet from joint angles (hip +-0.6, thigh 0.2 .. 1.4, calf -2.4 .. -0.9) through the forward map, so reach == 0 by construction;
    the 16 contact patterns in turn; random forces, rates and wrench -> dict"""
    P = scen.PARAM_SETS["gazebo"]
    opt = np.zeros((4, 3)) if rho_opt is None else np.asarray(rho_opt, float).reshape(4, 3)
    eul = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-3.0, 3.0, n)], 1)
    R = scen.rot_zyx(eul[:, 0], eul[:, 1], eul[:, 2]).reshape(n, 9)
    for b in range(n):
        if b % 16 in (1, 2, 3):
            axis = np.eye(3)[b % 16 - 1] + rng.normal(0, 0.02, 3)
            R[b] = rotation_about(axis, np.pi - rng.uniform(0.001, 0.1))[0]
    q = np.stack([rng.uniform(-0.6, 0.6, (n, 4)), rng.uniform(0.2, 1.4, (n, 4)), rng.uniform(-2.4, -0.9, (n, 4))], 2).reshape(n, 12)
    pb = forward_feet(A1_RHO_FIX, opt, q)
    foot = np.einsum("bij,blj->bli", R.reshape(n, 3, 3), pb.reshape(n, 4, 3)).reshape(n, 12)
    state = np.concatenate([rng.normal(0, 9.0, (n, 3)), rng.normal(0, 1.0, (n, 3)), rng.normal(0, 0.5, (n, 3)), rng.normal(0, 0.5, (n, 3))], 1)
    grf = rng.normal(0, 15.0, (n, 12)) + np.tile([0.0, 0.0, 30.0], 4)
    contacts = ((np.arange(n)[:, None] >> np.arange(4)[None, :]) & 1).astype(np.uint8)
    ext = np.concatenate([rng.normal(0, 20.0, (n, 3)), rng.normal(0, 3.0, (n, 3))], 1)
    return dict(mass=float(P["mass"]), q=q, state=np.ascontiguousarray(state), R=np.ascontiguousarray(R), foot=np.ascontiguousarray(foot), grf=grf,
                contacts=np.ascontiguousarray(contacts), ext=ext, rho_opt=opt)


UNREACHABLE_OPT = np.array([[0.0, 0.0, 0.05], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])   # leg 0: al = ell = 0.16 < lt = 0.21, so a folded leg cannot reach its own hip


def unreachable_feet():
    """body-frame feet of leg 0 under UNREACHABLE_OPT (reach: 0.05 <= distance in the leg plane <= 0.37) that the leg cannot reach, and the flag bits each must raise.
    Bit 0: inside the hip cylinder, dy^2 + p2^2 < L^2 (the leg then hangs from Zp = 0); bit 1: c outside [-1, 1], beyond full extension or closer than the folded leg"""
    ox, oy, L = A1_RHO_FIX[0, :3]
    return [((ox + 0.3, oy + 0.03, -0.04), 1),      # inside the cylinder, dx within reach: c = 0.30
            ((ox + 0.45, oy + 0.05, 0.02), 3),      # inside the cylinder and dx beyond full extension
            ((ox + 0.01, oy - 0.02, 0.03), 3),      # inside the cylinder and closer than the folded leg
            ((ox + 0.0, oy + L, -0.5), 2),          # straight below, 0.5 > 0.37
            ((ox + 0.3, oy + L, -0.4), 2),          # 0.5 away, forward and down
            ((ox + 0.001, oy + L, -0.01), 2)]       # 0.01 from the hip: closer than lt - ell = 0.05
