"""The closed loop  walk sensors -> tick -> walk step -> walk sensors  on the CPU: tests/sensor_loop.py's OracleLoop with the plant and the sensors of tests/walk_ref.py,
a stick command and the mode toggle.  Shared by tests/test_walk_host.py (which holds it to the trot's conditions) and tests/test_gpu_walk.py (which runs the same
schedule on the device and compares the end state).

The schedule: PRIME priming ticks on the unstepped plant, STAND closed ticks standing (the robots settle: toggled on the first closed tick the tilt peaks at 0.33), then
WALK ticks with the mode toggle on the first and a forward stick command of SPEED -- three gait cycles of the default gait (240 counts at speed 2: 120 ticks a cycle, a
diagonal pair swings for 59 ticks, and on the tick between two swings all four legs are in stance: the reference's `gait_counter <= counter_per_swing`).

The swing target z of the default gait is -0.35 under a body that stands at 0.30: the plane stops every swing foot 5 cm above its target, on every step."""
import numpy as np

import frontend_ref as FR
import sensor_loop as SL
import walk_ref as WR

PRIME, STAND, WALK, SPEED = SL.PRIME, 100, 360, 0.2
COUNTERS, COUNTER_SPEED, PER_GAIT, PER_SWING = np.array([0.0, 120.0, 120.0, 0.0]), 2.0, 240.0, 120.0
HEIGHT_ESTIMATE = 1e-2   # |estimated - true height| on every tick
SWING_RISE = 0.10        # every swing lifts the foot at least this far off the plane
HEADING_SPEED = (0.15, 0.25)   # the plant's velocity along its heading, mean of the last 120 ticks


def expected_contacts(k):
    """the plan of walk tick k (0 = the tick of the toggle): update_plan advances the counters before it reads them"""
    return (np.fmod(COUNTERS + COUNTER_SPEED * (k + 1), PER_GAIT) <= PER_SWING).astype(np.uint8)


class WalkLoop(SL.OracleLoop):
    """n robots of sensor_loop.perturbed_standing_robots under a1mpc_walk_step_batch's restatement"""

    def __init__(self, oracle, scen, sc, n, swing_track=1.0, flat_ground=1, ground_z=0.0):
        super().__init__(oracle, scen, sc, n)
        self.walk = dict(swing_track=swing_track, flat_ground=flat_ground, ground_z=ground_z)
        self.fvb = np.zeros((n, 12))

    def tick(self, step_plant=True, cmd=None, toggle=None):
        """OracleLoop.tick with the stick command (n, 6) and the toggle (n,) of this tick, the walk sensors in front and the walk step behind"""
        o, n, P, H = self.o, self.n, self.P, SL.H
        s = WR.sensors(P["mass"], self.x, self.R, self.foot, self.grf, self.ct, self.fvb)
        self.sensors = s
        Rw = FR.quat_to_rotation(s["quat"]); eul = SL.euler_of_quat(s["quat"]); Rz = FR.yaw_rotation(eul[:, 2])
        f = self.filt(np.concatenate([s["imu_acc_raw"], s["imu_gyro_raw"]], 1))
        acc, gyro = f[:, :3], f[:, 3:]
        w = FR.rotate(Rw, gyro)
        c = FR.command_step(self.cmd, np.zeros((n, 6)) if cmd is None else cmd, np.zeros(n, np.uint8) if toggle is None else toggle, self.pos, SL.CONTROL_DT)
        xref = np.zeros((n, 13 * H)); fa = np.zeros((n, 12)); ct = np.zeros((n, 4), np.uint8)
        for b in range(n):
            leg = o.leg_state(s["joint_pos"][b], s["joint_vel"][b], Rw[b], self.pos[b], self.vel[b])
            self.pos[b], self.vel[b], _ = o.ekf_step(self.ekf[b], SL.CONTROL_DT, c["movement_mode"][b], s["foot_force"][b], Rw[b], acc[b], gyro[b], leg["foot_pos_rel"],
                                                     leg["foot_vel_rel"], device=True)
            self.gc[b], pc, rel, _, _ = o.update_plan(self.gp, c["movement_mode"][b], self.gc[b], np.full(4, COUNTER_SPEED), self.vel[b], Rz[b], Rw[b], self.pos[b],
                                                      c["root_lin_vel_d"][b])
            o.swing_legs(Rz[b], leg["foot_pos_abs"], self.gc[b], rel, self.swing[0][b], self.swing[1][b], self.swing[2][b])
            ct[b], _, _, self.cmd["root_euler_d"][b, 1] = o.contact_terrain_step(self.cst[b], self.gc[b], pc, s["foot_force"][b], leg["foot_pos_abs"], self.pos[b, 2],
                                                                                 self.cmd["root_euler_d"][b, 1])
            fa[b] = leg["foot_pos_abs"]
            xref[b] = o.mpc_reference(H, P["dt"], eul[b], self.pos[b], Rw[b], self.cmd["root_euler_d"][b], c["root_lin_vel_d"][b], c["root_ang_vel_d"][b], c["root_pos_d_z"][b])
        x0 = self.scen.pack_x0(eul, self.pos, w, self.vel)
        sol = o.mpc_solve_batch(self.pr, self.st, x0, xref, Rw, fa, ct)
        self.status = sol["status"]
        if step_plant:
            self.grf, self.ct = sol["grf"], ct
            self.x, self.R, self.foot, self.fvb = WR.step(P, self.x, self.R, self.foot, self.grf, self.ct, Rz, self.swing[2], None, SL.CONTROL_DT, 1, **self.walk)
        return sol


def schedule(n):
    """(step_plant, cmd, toggle) of every tick of the run"""
    out = []
    for t in range(PRIME + STAND + WALK):
        walking = t >= PRIME + STAND
        cmd = np.zeros((n, 6)); cmd[:, 0] = SPEED if walking else 0.0
        out.append((t >= PRIME, cmd, np.full(n, 1 if t == PRIME + STAND else 0, np.uint8)))
    return out


def heading_speed(x, R):
    """the plant's velocity along its heading (the body's x axis laid flat): x (n, >= 12), R (n, 9) -> (n,)"""
    hx, hy = R[:, 0], R[:, 3]
    nrm = np.sqrt(hx * hx + hy * hy)
    return (x[:, 9] * hx + x[:, 10] * hy) / nrm


def walk_conditions(hist, n):
    """the whole-walk conditions on a history: dict of arrays over the WALK ticks -- contacts (T, n, 4), foot (T, n, 12) and state (T, n, 12) AFTER each tick's step, R
    (T, n, 9) likewise; ground: whether the plane was on -> (list of what failed, dict of figures)"""
    bad, figs = [], {}
    ct, foot, st = hist["contacts"], hist["foot"].reshape(WALK, n, 4, 3), hist["state"]
    want = np.stack([expected_contacts(k) for k in range(WALK)])
    if not (ct == want[:, None, :]).all():
        bad.append("contacts are not the planned diagonal pairs")
    pairs = {(1, 0, 0, 1), (0, 1, 1, 0), (1, 1, 1, 1)}
    if not {tuple(r) for r in want.tolist()} == pairs:
        bad.append("the plan is not two diagonal pairs")
    hz = foot[:, :, :, 2] + st[:, :, None, 5]        # the feet's height in the world
    edge = (ct[1:] == 1) & (ct[:-1] == 0)
    figs["touchdowns"] = int(edge.sum())
    td = hz[1:][edge]
    figs["touchdown_z"] = (float(td.min()), float(td.max()))
    figs["swing_rise"] = float(np.where(ct == 0, hz, -np.inf).max(axis=0).min())   # the lowest, over robots and legs, of the highest point of a leg's swings
    figs["below_plane"] = float(hz.min())
    figs["heading_speed"] = heading_speed(st[-120:].reshape(-1, 12), hist["R"][-120:].reshape(-1, 9)).reshape(120, n).mean(axis=0)
    return bad, figs
