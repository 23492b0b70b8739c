"""a1mpc_ground_step_batch and a1mpc_touch_sensors_batch restated in numpy, ELEMENTWISE, from the text of include/a1mpc.h: the restatements of tests/walk_ref.py
(every value a vector over the robots, every operation one IEEE operation in the header's order) with the ground rule applied behind the step and the touch rule in
front of the foot-force output.  Of the step, pos, R, v, omega, the feet, foot_vel_body and touch equal the kernel's bit for bit and the angles lie within
plant_ref.ANGLE_BAR; the sensors follow sensor_synthesis_ref's rule.  Test infrastructure only."""
import numpy as np

import plant_ref as PR
import sensor_synthesis_ref as SR
import walk_ref as WR


def plane(ground, X, Y):
    """hz(X, Y) = (z0 + sx X) + sy Y, in that order; ground (n, 3), X and Y (n,) or (n, k)"""
    g = np.asarray(ground, np.float64)
    z0, sx, sy = (g[:, k].reshape((-1,) + (1,) * (np.ndim(X) - 1)) for k in range(3))
    with np.errstate(all="ignore"):
        return (z0 + sx * X) + sy * Y


def step(params, state, R, foot, grf, contacts, Rz=None, target=None, ground=None, ext=None, dt=0.0025, substeps=1, gravity=PR.GRAVITY, swing_track=1.0, flat_ground=0,
         ground_z=0.0):
    """walk_ref.step's arguments and ground (n, 3) or None -> (state (n, 12), R (n, 9), foot (n, 12), foot_vel_body (n, 12), touch (n, 4) uint8)"""
    with np.errstate(all="ignore"):
        # the sub-steps are the walk step's; the ground comes after the last of them, so the walk step WITHOUT a ground gives pos', R' and r' of the rule
        so, Ro, fo, vo = WR.step(params, state, R, foot, grf, contacts, Rz, target, ext, dt, substeps, gravity, swing_track, 0, 0.0)
        n = Ro.shape[0]
        ct = np.asarray(contacts).reshape(n, 4) != 0
        fo = fo.copy()
        touch = ct.copy()
        if ground is not None or flat_ground:
            for l in range(4):
                if ground is not None:
                    X = so[:, 3] + fo[:, 3 * l]; Y = so[:, 4] + fo[:, 3 * l + 1]
                    gz = plane(ground, X, Y) - so[:, 5]
                else:
                    gz = np.float64(ground_z) - so[:, 5]
                rz = fo[:, 3 * l + 2]
                lifted = rz < gz
                fo[:, 3 * l + 2] = np.where(ct[:, l], gz, np.where(lifted, gz, rz))
                touch[:, l] = ct[:, l] | lifted
        return so, Ro, fo, vo, touch.astype(np.uint8)


def sensors(mass, state, R, foot, grf, contacts, foot_vel_body=None, touch=None, touch_force=0.0, ext=None, rho_fix=SR.A1_RHO_FIX, rho_opt=None, dtype=np.float64):
    """walk_ref.sensors with foot_force = touch_force (selected) on a swing leg whose touch byte is non-zero"""
    out = WR.sensors(mass, state, R, foot, grf, contacts, foot_vel_body, ext, rho_fix, rho_opt, dtype)
    if touch is not None:
        n = out["foot_force"].shape[0]
        ct = np.asarray(contacts).reshape(n, 4) != 0
        hit = ~ct & (np.asarray(touch).reshape(n, 4) != 0)
        out["foot_force"] = np.where(hit, dtype(touch_force), out["foot_force"])
    return out


def random_planes(sc, rng, n):
    """(n, 3) planes with |sx|, |sy| <= 0.3 whose z0 puts the plane through the middle of each robot's feet, so that feet lie on both sides of it"""
    sx, sy = rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)
    pos, foot = sc["state"][:n, 3:6], sc["foot"][:n].reshape(n, 4, 3)
    X, Y, Z = pos[:, 0:1] + foot[:, :, 0], pos[:, 1:2] + foot[:, :, 1], pos[:, 2:3] + foot[:, :, 2]
    z0 = (Z - sx[:, None] * X - sy[:, None] * Y).mean(axis=1) + rng.uniform(-0.02, 0.02, n)
    return np.ascontiguousarray(np.stack([z0, sx, sy], 1))
