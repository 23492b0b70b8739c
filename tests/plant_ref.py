"""The single-rigid-body plant step of a1mpc_plant_step_batch restated in numpy, ELEMENTWISE: every value is a vector over the robots and every operation one IEEE add,
subtract, multiply or divide in the order include/a1mpc.h states (three-term sums left to right, the legs as (0 + 1) + (2 + 3)) -- no `@`, no einsum, no sum(), so neither
BLAS nor a fused multiply-add can enter.  pos, R, v, omega and the feet of the kernel equal this bit for bit; the angles (library atan2 / asin on bit-identical arguments)
within ANGLE_BAR.  Test infrastructure only."""
import numpy as np

ANGLE_BAR = 1e-12   # library atan2 / asin against numpy's on the same arguments (the bar of the sensor front end's test)
GRAVITY = -9.8


def _mv(M, x):
    """M x, M a list of 9 vectors (row-major), x a list of 3"""
    return [(M[3 * i] * x[0] + M[3 * i + 1] * x[1]) + M[3 * i + 2] * x[2] for i in range(3)]


def _mtv(M, x):
    return [(M[i] * x[0] + M[3 + i] * x[1]) + M[6 + i] * x[2] for i in range(3)]


def inverse_by_cofactors(I):
    """the 3 x 3 inverse as the kernel spells it (I: 9 scalars or vectors, row-major)"""
    c00 = I[4] * I[8] - I[5] * I[7]; c01 = I[5] * I[6] - I[3] * I[8]; c02 = I[3] * I[7] - I[4] * I[6]
    d = 1.0 / ((I[0] * c00 + I[1] * c01) + I[2] * c02)
    return [c00 * d, (I[2] * I[7] - I[1] * I[8]) * d, (I[1] * I[5] - I[2] * I[4]) * d,
            c01 * d, (I[0] * I[8] - I[2] * I[6]) * d, (I[2] * I[3] - I[0] * I[5]) * d,
            c02 * d, (I[1] * I[6] - I[0] * I[7]) * d, (I[0] * I[4] - I[1] * I[3]) * d]


def polish(R):
    """R - R (R'R - I) / 2: the first-order step towards the nearest orthogonal matrix, as the kernel spells it (R: 9 vectors, row-major)"""
    E = [(R[i] * R[j] + R[3 + i] * R[3 + j]) + R[6 + i] * R[6 + j] for i in range(3) for j in range(3)]
    for i in range(3):
        E[4 * i] = E[4 * i] - 1.0
    return [R[3 * i + j] - 0.5 * ((R[3 * i] * E[j] + R[3 * i + 1] * E[3 + j]) + R[3 * i + 2] * E[6 + j]) for i in range(3) for j in range(3)]


def euler_of(R):
    """(n, 9) -> (n, 3): the rot_zyx angles"""
    R = np.asarray(R, np.float64).reshape(-1, 9)
    sp = -R[:, 6]; sp = np.where(sp > 1.0, 1.0, np.where(sp < -1.0, -1.0, sp))
    return np.stack([np.arctan2(R[:, 7], R[:, 8]), np.arcsin(sp), np.arctan2(R[:, 3], R[:, 0])], 1)


def step(params, state, R, foot, grf, contacts, ext=None, dt=0.0025, substeps=1, gravity=GRAVITY):
    """one call: state (n, >= 12) rows of [euler (not read), pos, omega, v], R (n, 9), foot (n, 12), grf (n, 12) body frame, contacts (n, 4), ext None or (n, 6)
    -> (state (n, 12), R (n, 9), foot (n, 12))"""
    with np.errstate(all="ignore"):
        f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        state, R, foot, grf = f8(state), f8(R).reshape(-1, 9), f8(foot).reshape(-1, 12), f8(grf).reshape(-1, 12)
        n = R.shape[0]
        ct = np.asarray(contacts).reshape(n, 4) != 0
        pos = [state[:, 3 + k].copy() for k in range(3)]; w = [state[:, 6 + k].copy() for k in range(3)]; v = [state[:, 9 + k].copy() for k in range(3)]
        Rm = [R[:, k].copy() for k in range(9)]
        r = [[foot[:, 3 * l + k].copy() for k in range(3)] for l in range(4)]
        f = [[grf[:, 3 * l + k] for k in range(3)] for l in range(4)]
        Rm = polish(Rm)
        Ib = [np.float64(x) for x in np.asarray(params["inertia"], np.float64).reshape(9)]
        Ii = inverse_by_cofactors(Ib)
        m = np.float64(params["mass"]); g = np.float64(gravity)
        L = _mv(Rm, _mv(Ib, _mtv(Rm, w)))
        h = np.float64(dt) / np.float64(substeps); half = h / np.float64(2.0)
        zero = np.zeros(n)
        for _ in range(int(substeps)):
            fw, tq = [], []
            for l in range(4):
                x = _mv(Rm, f[l])
                x = [np.where(ct[:, l], x[k], zero) for k in range(3)]
                fw.append(x)
                tq.append([r[l][1] * x[2] - r[l][2] * x[1], r[l][2] * x[0] - r[l][0] * x[2], r[l][0] * x[1] - r[l][1] * x[0]])
            F = [(fw[0][k] + fw[1][k]) + (fw[2][k] + fw[3][k]) for k in range(3)]
            T = [(tq[0][k] + tq[1][k]) + (tq[2][k] + tq[3][k]) for k in range(3)]
            if ext is not None:
                e = f8(ext).reshape(n, 6)
                F = [F[k] + e[:, k] for k in range(3)]; T = [T[k] + e[:, 3 + k] for k in range(3)]
            v = [v[0] + h * (F[0] / m), v[1] + h * (F[1] / m), v[2] + h * (F[2] / m + g)]
            dp = [h * v[k] for k in range(3)]
            pos = [pos[k] + dp[k] for k in range(3)]
            a0, a1, a2 = half * w[0], half * w[1], half * w[2]
            s = 2.0 / (1.0 + ((a0 * a0 + a1 * a1) + a2 * a2))
            Cm = [1.0 - s * (a1 * a1 + a2 * a2), s * (a0 * a1 - a2), s * (a0 * a2 + a1),
                  s * (a0 * a1 + a2), 1.0 - s * (a0 * a0 + a2 * a2), s * (a1 * a2 - a0),
                  s * (a0 * a2 - a1), s * (a1 * a2 + a0), 1.0 - s * (a0 * a0 + a1 * a1)]
            Rn = [(Cm[3 * i] * Rm[j] + Cm[3 * i + 1] * Rm[3 + j]) + Cm[3 * i + 2] * Rm[6 + j] for i in range(3) for j in range(3)]
            L = [L[k] + h * T[k] for k in range(3)]
            w = _mv(Rn, _mv(Ii, _mtv(Rn, L)))
            for l in range(4):
                rs = _mv(Rn, _mtv(Rm, r[l]))
                r[l] = [np.where(ct[:, l], r[l][k] - dp[k], rs[k]) for k in range(3)]
            Rm = Rn
        R_out = np.stack(Rm, 1)
        out = np.concatenate([euler_of(R_out), np.stack(pos, 1), np.stack(w, 1), np.stack(v, 1)], 1)
        return out, R_out, np.stack([r[l][k] for l in range(4) for k in range(3)], 1)


def bits_equal(a, b):
    """the same doubles bit for bit, except that any NaN equals any NaN (a NaN's payload is not part of the contract)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def random_robots(scen, rng, n, w_sig=0.5, all_patterns=True):
    """n robots at random attitudes (|roll|, |pitch| <= 0.5, any yaw) with random feet, forces and wrench; the 16 contact patterns in turn -> dict"""
    P = scen.PARAM_SETS["gazebo"]
    eul = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-3.0, 3.0, n)], 1)
    R = scen.rot_zyx(eul[:, 0], eul[:, 1], eul[:, 2]).reshape(n, 9)
    state = np.concatenate([rng.normal(0, 9.0, (n, 3)), rng.normal(0, 1.0, (n, 3)), rng.normal(0, w_sig, (n, 3)), rng.normal(0, 0.5, (n, 3))], 1)   # (euler: not read)
    foot = (np.array(P["foot"], float).reshape(1, 12) + rng.uniform(-0.05, 0.05, (n, 12)))
    grf = rng.normal(0, 15.0, (n, 12)) + np.tile([0.0, 0.0, 30.0], 4)
    pat = (np.arange(n) % 16) if all_patterns else rng.integers(0, 16, n)
    contacts = ((pat[:, None] >> np.arange(4)[None, :]) & 1).astype(np.uint8)
    ext = np.concatenate([rng.normal(0, 20.0, (n, 3)), rng.normal(0, 3.0, (n, 3))], 1)
    return dict(params=dict(P, **scen.MPC_CONSTANTS), state=np.ascontiguousarray(state), R=np.ascontiguousarray(R), foot=np.ascontiguousarray(foot), grf=grf,
                contacts=np.ascontiguousarray(contacts), ext=ext)


# ---- the physics checks, on any `stepper(state12, R, foot, grf, contacts, ext, dt, substeps) -> (state12, R, foot)`: the restatement, the host-compiled kernel text, the GPU
def _m3(R):
    return np.asarray(R, np.float64).reshape(-1, 3, 3)


def world_momentum(params, R, w):
    Ib = np.asarray(params["inertia"], np.float64).reshape(3, 3); Rm = _m3(R)
    return np.einsum("bij,jk,blk,bl->bi", Rm, Ib, Rm, w)


def torque_free_flight(stepper, scen, n=64, calls=400, seed=11):
    """no contacts, omega != 0 -> (relative move of R I_b R' omega, |R R' - I|, move of the swing feet in the body frame), the worst robot each"""
    rng = np.random.default_rng(seed); sc = random_robots(scen, rng, n, w_sig=2.0)
    ct = np.zeros((n, 4), np.uint8)
    st, R, foot = sc["state"], sc["R"], sc["foot"]
    assert (np.linalg.norm(st[:, 6:9], axis=1) > 0.1).all()
    L0 = world_momentum(sc["params"], R, st[:, 6:9]); fb0 = np.einsum("bji,blj->bli", _m3(R), foot.reshape(n, 4, 3))
    for _ in range(calls):
        st, R, foot = stepper(st, R, foot, sc["grf"], ct, None, 0.0025, 1)
    L1 = world_momentum(sc["params"], R, st[:, 6:9]); fb1 = np.einsum("bji,blj->bli", _m3(R), foot.reshape(n, 4, 3))
    Rm = _m3(R)
    return (float((np.linalg.norm(L1 - L0, axis=1) / np.linalg.norm(L0, axis=1)).max()), float(np.abs(np.einsum("bij,bkj->bik", Rm, Rm) - np.eye(3)).max()),
            float(np.abs(fb1 - fb0).max()))


def free_fall(stepper, scen, n=64, calls=400, seed=12, dt=0.0025):
    """no contacts -> the worst |v_z - (v0 + g N h)| and |pos_z - (p0 + N h v0 + g h^2 N (N + 1) / 2)|"""
    rng = np.random.default_rng(seed); sc = random_robots(scen, rng, n)
    ct = np.zeros((n, 4), np.uint8)
    st, R, foot = sc["state"], sc["R"], sc["foot"]
    v0, p0, N = st[:, 11].copy(), st[:, 5].copy(), calls
    for _ in range(calls):
        st, R, foot = stepper(st, R, foot, sc["grf"], ct, None, dt, 1)
    return float(np.abs(st[:, 11] - (v0 + GRAVITY * N * dt)).max()), float(np.abs(st[:, 5] - (p0 + N * dt * v0 + GRAVITY * dt * dt * N * (N + 1) / 2)).max())


def standing(stepper, scen, n=64, calls=400, seed=13):
    """four legs carry m g / 4 each on symmetric feet, level body at any yaw and place -> the largest move of pos, R, v, omega, feet"""
    rng = np.random.default_rng(seed)
    P = dict(scen.PARAM_SETS["gazebo"], **scen.MPC_CONSTANTS)
    yaw = rng.uniform(-3.0, 3.0, n); yaw[0] = 0.0
    R0 = scen.rot_zyx(0 * yaw, 0 * yaw, yaw).reshape(n, 9)
    fb = np.array(P["foot"], float) * rng.uniform(0.8, 1.2, (n, 1, 3))   # symmetric about the COM, another size for every robot
    foot0 = np.einsum("bij,blj->bli", _m3(R0), fb).reshape(n, 12)
    st0 = np.concatenate([np.zeros((n, 3)), rng.normal(0, 1.0, (n, 2)), np.full((n, 1), 0.3), np.zeros((n, 6))], 1)
    grf = np.tile([0.0, 0.0, P["mass"] * 9.8 / 4.0], (n, 4)); ct = np.ones((n, 4), np.uint8)
    st, R, foot = st0, R0, foot0
    for _ in range(calls):
        st, R, foot = stepper(st, R, foot, grf, ct, None, 0.0025, 1)
    return float(max(np.abs(st[:, 3:12] - st0[:, 3:12]).max(), np.abs(R - R0).max(), np.abs(foot - foot0).max()))


def rotation_order(stepper, scen, n=64, seed=14, T=0.1):
    """constant forces over T = 0.1 s: the rotation error against 4096 sub-steps (64 calls of 64) at 40 / 80 / 160 steps, the worst entry of R over the batch -> the two
    ratios err(N) / err(2N)"""
    rng = np.random.default_rng(seed); sc = random_robots(scen, rng, n, w_sig=2.0)

    def run(calls, substeps):
        st, R, foot = sc["state"], sc["R"], sc["foot"]
        for _ in range(calls):
            st, R, foot = stepper(st, R, foot, sc["grf"], sc["contacts"], sc["ext"], T / calls, substeps)
        return R
    fine = run(64, 64)
    err = [float(np.abs(run(N, 1) - fine).max()) for N in (40, 80, 160)]
    return err[0] / err[1], err[1] / err[2]


def ref_stepper(params):
    return lambda st, R, foot, grf, ct, ext, dt, substeps: step(params, st, R, foot, grf, ct, ext, dt, substeps)
