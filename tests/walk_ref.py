"""a1mpc_walk_step_batch and a1mpc_walk_sensors_batch restated in numpy, ELEMENTWISE, in the manner of tests/plant_ref.py and tests/sensor_synthesis_ref.py (whose
helpers they use): every value is a vector over the robots and every operation one IEEE add, subtract, multiply, divide or sqrt in the order include/a1mpc.h states -- no
`@`, no einsum, no sum().  Of the step, pos, R, v, omega, the feet and foot_vel_body equal the kernel's bit for bit and the angles lie within plant_ref.ANGLE_BAR; the
sensors follow the rule of sensor_synthesis_ref (BITS bit for bit, NOISY within 4 E of the 80-bit evaluation).  Test infrastructure only."""
import numpy as np

import plant_ref as PR
import sensor_synthesis_ref as SR
from plant_ref import _mv, _mtv


def step(params, state, R, foot, grf, contacts, Rz=None, target=None, ext=None, dt=0.0025, substeps=1, gravity=PR.GRAVITY, swing_track=1.0, flat_ground=0, ground_z=0.0):
    """one call: the arguments of plant_ref.step, Rz (n, 9) and target (n, 12) (not read with swing_track == 0) -> (state (n, 12), R (n, 9), foot (n, 12),
    foot_vel_body (n, 12))"""
    with np.errstate(all="ignore"):
        f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        state, R, foot, grf = f8(state), f8(R).reshape(-1, 9), f8(foot).reshape(-1, 12), f8(grf).reshape(-1, 12)
        n = R.shape[0]
        ct = np.asarray(contacts).reshape(n, 4) != 0
        pos = [state[:, 3 + k].copy() for k in range(3)]; w = [state[:, 6 + k].copy() for k in range(3)]; v = [state[:, 9 + k].copy() for k in range(3)]
        Rm = [R[:, k].copy() for k in range(9)]
        r = [[foot[:, 3 * l + k].copy() for k in range(3)] for l in range(4)]
        f = [[grf[:, 3 * l + k] for k in range(3)] for l in range(4)]
        Rm = PR.polish(Rm)
        Ib = [np.float64(x) for x in np.asarray(params["inertia"], np.float64).reshape(9)]
        Ii = PR.inverse_by_cofactors(Ib)
        m = np.float64(params["mass"]); g = np.float64(gravity)
        L = _mv(Rm, _mv(Ib, _mtv(Rm, w)))
        zero = np.zeros(n)
        track = np.float64(swing_track); tracking = track != 0.0
        d = [[zero] * 3 for _ in range(4)]; vel = [[zero] * 3 for _ in range(4)]
        if tracking:
            Rz, target = f8(Rz).reshape(n, 9), f8(target).reshape(n, 12)
            Z = [Rz[:, k] for k in range(9)]
            for l in range(4):
                p0 = _mtv(Rm, r[l]); pt = _mtv(Rm, _mv(Z, [target[:, 3 * l + k] for k in range(3)]))
                dl = [track * (pt[k] - p0[k]) for k in range(3)]
                d[l] = [dl[k] / np.float64(substeps) for k in range(3)]; vel[l] = [dl[k] / np.float64(dt) for k in range(3)]
        h = np.float64(dt) / np.float64(substeps); half = h / np.float64(2.0)
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
                pb = _mtv(Rm, r[l])
                if tracking:
                    pb = [pb[k] + d[l][k] for k in range(3)]
                rs = _mv(Rn, pb)
                r[l] = [np.where(ct[:, l], r[l][k] - dp[k], rs[k]) for k in range(3)]
            Rm = Rn
        if flat_ground:
            gz = np.float64(ground_z) - pos[2]
            for l in range(4):
                r[l][2] = np.where(ct[:, l], gz, np.where(r[l][2] < gz, gz, r[l][2]))
        R_out = np.stack(Rm, 1)
        out = np.concatenate([PR.euler_of(R_out), np.stack(pos, 1), np.stack(w, 1), np.stack(v, 1)], 1)
        vel_out = np.stack([np.where(ct[:, l], zero, vel[l][k]) for l in range(4) for k in range(3)], 1)
        return out, R_out, np.stack([r[l][k] for l in range(4) for k in range(3)], 1), vel_out


def sensors(mass, state, R, foot, grf, contacts, foot_vel_body=None, ext=None, rho_fix=SR.A1_RHO_FIX, rho_opt=None, dtype=np.float64):
    """sensor_synthesis_ref.synthesise with the swing legs' foot_vel_rel taken from foot_vel_body (n, 12; None: +0) -> its dict of outputs in `dtype`"""
    with np.errstate(all="ignore"):
        fx = lambda a: np.ascontiguousarray(a, dtype=np.float64).astype(dtype)
        state, R, foot, grf = fx(state), fx(R).reshape(-1, 9), fx(foot).reshape(-1, 12), fx(grf).reshape(-1, 12)
        n = R.shape[0]
        ct = np.asarray(contacts).reshape(n, 4) != 0
        opt = np.zeros((4, 3)) if rho_opt is None else rho_opt
        m, zero = dtype(mass), np.zeros(n, dtype)
        fb = None if foot_vel_body is None else fx(foot_vel_body).reshape(n, 12)
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
        quat = SR.quaternion_of(Rm, dtype)
        ff, jp, jv, pr, vr, reach = [], [], [], [], [], []
        for l in range(4):
            g = SR.leg_geometry(rho_fix, opt, l, dtype)
            ff.append(np.where(ct[:, l], (Rm[6] * grf[:, 3 * l] + Rm[7] * grf[:, 3 * l + 1]) + Rm[8] * grf[:, 3 * l + 2], zero))
            p = _mtv(Rm, r[l])
            q, flags = SR.inverse_leg(g, p, dtype)
            u = [v[0] + (w[1] * r[l][2] - w[2] * r[l][1]), v[1] + (w[2] * r[l][0] - w[0] * r[l][2]), v[2] + (w[0] * r[l][1] - w[1] * r[l][0])]
            ub = _mtv(Rm, u)
            fv = [np.where(ct[:, l], -ub[k], zero if fb is None else fb[:, 3 * l + k]) for k in range(3)]
            _, J = SR.forward_leg(g, q)
            Ji = SR.inverse_by_cofactors([J[0], J[3], J[6], J[1], J[4], J[7], J[2], J[5], J[8]])
            qd = [np.where(flags != 0, zero, x) for x in _mv(Ji, fv)]
            jp += q; jv += qd; pr += p; vr += fv; reach.append(flags)
        S = lambda cols: np.stack(cols, 1)
        return dict(quat=S(quat), imu_acc_raw=S(acc), imu_gyro_raw=S(gyro), joint_pos=S(jp), joint_vel=S(jv), foot_force=S(ff), reach=S(reach), foot_pos_rel=S(pr),
                    foot_vel_rel=S(vr))


def random_walkers(scen, rng, n):
    """plant_ref.random_robots and, per robot, a yaw rotation R_z near the robot's own yaw and swing targets within 0.1 m of the feet's present place in the R_z frame"""
    sc = PR.random_robots(scen, rng, n)
    yaw = np.arctan2(sc["R"][:, 3], sc["R"][:, 0]) + rng.uniform(-0.05, 0.05, n)
    Rz = scen.rot_zyx(0 * yaw, 0 * yaw, yaw).reshape(n, 9)
    cur = np.einsum("bji,blj->bli", Rz.reshape(n, 3, 3), sc["foot"].reshape(n, 4, 3)).reshape(n, 12)   # foot_pos_cur = R_z^T foot_pos_abs
    sc.update(Rz=np.ascontiguousarray(Rz), target=np.ascontiguousarray(cur + rng.uniform(-0.1, 0.1, (n, 12))))
    return sc
