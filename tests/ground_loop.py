"""The closed loop  touch sensors -> tick -> ground step -> touch sensors  on the CPU: tests/walk_loop.py's WalkLoop with the plant and the sensors of
tests/ground_ref.py -- a ground plane per robot and a touch force on the swing feet the ground stops.  Shared by tests/test_ground_host.py (which holds it to the
conditions below) and tests/test_gpu_ground.py (which runs the same schedule on the device and compares).

The schedule and the per-tick conditions are walk_loop's; the height condition is taken above the robot's OWN plane, pos_z - hz(pos_x, pos_y), and every z0 is chosen
so that hz is 0 under the robot's starting position.  Figures measured on this loop are in profiles/ground_walk.md."""
import numpy as np

import frontend_ref as FR
import ground_ref as GR
import sensor_loop as SL
import walk_loop as WL

SLOPES = (0.15, 0.10, 0.05)   # tried in this order: the largest at which the ramp loop keeps conditions_hold empty on every tick is RAMP_SLOPE
RAMP_SLOPE = 0.15
TOUCH_FORCE = 60.0            # above foot_force_low = 30 and above the EKF's 50 N contact mark
TOUCHDOWN = 1e-12             # |foot height above its plane| on every touchdown
TERRAIN_TICKS = 120           # the terrain angle is looked at over the last 120 ticks (one gait cycle; the reference averages it over 100)
# |terrain_angle - atan(RAMP_SLOPE)| on the two pitch ramps over those ticks: twice the worst deviation measured on this CPU loop (profiles/ground_walk.md)
TERRAIN_BAR = 1.75e-4   # (measured: 8.72e-5; atan(0.15) / 2 = 7.4e-2: the estimate tracks the slope)


def ramp_planes(sc, s, n=4):
    """(n, 3): robots 0 .. 3 on (sx, sy) = (+s, 0), (-s, 0), (0, +s), (0, 0), any further robot flat; hz = 0 under every starting position"""
    g = np.zeros((n, 3))
    g[:4, 1:] = np.array([[s, 0.0], [-s, 0.0], [0.0, s], [0.0, 0.0]])[:min(n, 4)]
    pos = sc["state"][:n, 3:5]
    g[:, 0] = -(g[:, 1] * pos[:, 0] + g[:, 2] * pos[:, 1])
    g[3:, 0] = 0.0   # (the flat robots: exactly the plane z = 0)
    return g


def above_plane(ground, x):
    """the state with pos_z replaced by the height above the robot's own plane: what conditions_hold is given"""
    y = np.array(x[:, :12], dtype=np.float64)
    y[:, 5] = x[:, 5] - GR.plane(ground, x[:, 3], x[:, 4])
    return y


class GroundLoop(WL.WalkLoop):
    """n robots of sensor_loop.perturbed_standing_robots under a1mpc_ground_step_batch's and a1mpc_touch_sensors_batch's restatements"""

    def __init__(self, oracle, scen, sc, n, ground=None, touch_force=0.0, use_terrain_adapt=1):
        super().__init__(oracle, scen, sc, n)
        self.ground = np.zeros((n, 3)) if ground is None else np.ascontiguousarray(ground, dtype=np.float64)
        self.touch_force, self.adapt = float(touch_force), int(use_terrain_adapt)
        self.touch = np.ones((n, 4), np.uint8)   # (the unstepped plant stands on all four feet)
        self.plan = np.ones((n, 4), np.uint8); self.terrain_angle = np.zeros(n); self.recent = np.zeros((n, 12)); self.touch_read = self.touch.copy()

    def tick(self, step_plant=True, cmd=None, toggle=None):
        """WalkLoop.tick with the touch sensors in front and the ground step behind; keeps the tick's plan, terrain angle, recent contact points and the touch bytes its
        sensors read"""
        o, n, P, H = self.o, self.n, self.P, SL.H
        self.touch_read = self.touch.copy()
        s = GR.sensors(P["mass"], self.x, self.R, self.foot, self.grf, self.ct, self.fvb, self.touch, self.touch_force)
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
            self.gc[b], pc, rel, _, _ = o.update_plan(self.gp, c["movement_mode"][b], self.gc[b], np.full(4, WL.COUNTER_SPEED), self.vel[b], Rz[b], Rw[b], self.pos[b],
                                                      c["root_lin_vel_d"][b])
            o.swing_legs(Rz[b], leg["foot_pos_abs"], self.gc[b], rel, self.swing[0][b], self.swing[1][b], self.swing[2][b])
            ct[b], self.recent[b], self.terrain_angle[b], self.cmd["root_euler_d"][b, 1] = o.contact_terrain_step(
                self.cst[b], self.gc[b], pc, s["foot_force"][b], leg["foot_pos_abs"], self.pos[b, 2], self.cmd["root_euler_d"][b, 1], use_terrain_adapt=self.adapt)
            self.plan[b] = pc
            fa[b] = leg["foot_pos_abs"]
            xref[b] = o.mpc_reference(H, P["dt"], eul[b], self.pos[b], Rw[b], self.cmd["root_euler_d"][b], c["root_lin_vel_d"][b], c["root_ang_vel_d"][b], c["root_pos_d_z"][b])
        x0 = self.scen.pack_x0(eul, self.pos, w, self.vel)
        sol = o.mpc_solve_batch(self.pr, self.st, x0, xref, Rw, fa, ct)
        self.status = sol["status"]
        if step_plant:
            self.grf, self.ct = sol["grf"], ct
            self.x, self.R, self.foot, self.fvb, self.touch = GR.step(P, self.x, self.R, self.foot, self.grf, self.ct, Rz, self.swing[2], self.ground, None, SL.CONTROL_DT, 1,
                                                                      swing_track=1.0)
        return sol


KEYS = ("contacts", "plan", "touch_read", "foot", "state", "R", "gc", "terrain_angle", "pitch_d", "recent", "root_pos", "foot_force")


def run(loop, n):
    """walk_loop.schedule on `loop` -> (history over the WALK ticks: contacts, plan, touch_read (the bytes the tick's sensors read), gc (the gait counters after the
    tick's update), terrain_angle, pitch_d (root_euler_d[1]), recent, root_pos (the estimate), foot_force, and foot, state, R AFTER the tick's step; list of (tick, what
    conditions_hold reported) over the closed ticks)"""
    hist = {k: [] for k in KEYS}
    failed = []
    for t, (stepped, cmd, toggle) in enumerate(WL.schedule(n)):
        loop.tick(step_plant=stepped, cmd=cmd, toggle=toggle)
        if not stepped:
            continue
        finite = all(np.isfinite(np.asarray(v, float)).all() for v in loop.sensors.values()) and np.isfinite(loop.grf).all() and np.isfinite(loop.x).all()
        bad = SL.conditions_hold(above_plane(loop.ground, loop.x), loop.sensors["reach"], loop.status, finite)
        if bad:
            failed.append((t, bad))
        if t >= WL.PRIME + WL.STAND:
            for k, v in (("contacts", loop.ct), ("plan", loop.plan), ("touch_read", loop.touch_read), ("foot", loop.foot), ("state", loop.x), ("R", loop.R), ("gc", loop.gc),
                         ("terrain_angle", loop.terrain_angle), ("pitch_d", loop.cmd["root_euler_d"][:, 1]), ("recent", loop.recent), ("root_pos", loop.pos),
                         ("foot_force", loop.sensors["foot_force"])):
                hist[k].append(np.array(v, copy=True))
    return {k: np.stack(v) for k, v in hist.items()}, failed


def touchdown_heights(hist, ground):
    """the height above its robot's plane of every foot on the tick its contact goes 0 -> 1 (the plant's feet, after that tick's step)"""
    T, n = hist["contacts"].shape[:2]
    foot, st = hist["foot"].reshape(T, n, 4, 3), hist["state"]
    X, Y, Z = st[:, :, None, 3] + foot[:, :, :, 0], st[:, :, None, 4] + foot[:, :, :, 1], st[:, :, None, 5] + foot[:, :, :, 2]
    g = np.asarray(ground)
    h = Z - ((g[None, :, None, 0] + g[None, :, None, 1] * X) + g[None, :, None, 2] * Y)
    edge = (hist["contacts"][1:] == 1) & (hist["contacts"][:-1] == 0)
    return h[1:][edge], h


def early_contacts(hist):
    """[(tick, robot, leg)] where the tick's contacts differ from its plan"""
    return [tuple(int(i) for i in idx) for idx in np.argwhere(hist["contacts"] != hist["plan"])]


def latch_by_the_reference_rule(hist, per_swing=120.0, force_low=30.0):
    """the early-contact latch recomputed from the history by S/A1RobotControl.cpp:259-271 (cleared while gait_counter <= 1.5 counter_per_swing, set by a swing leg past
    it whose foot force exceeds force_low, kept otherwise) -> contacts (T, n, 4) it implies, from a cleared latch at the first walk tick"""
    T, n = hist["contacts"].shape[:2]
    latch = np.zeros((n, 4), bool); out = np.zeros((T, n, 4), np.uint8)
    for t in range(T):
        late = hist["gc"][t] > per_swing * 1.5
        latch &= late
        latch |= (hist["plan"][t] == 0) & late & (hist["foot_force"][t] > force_low)
        out[t] = (hist["plan"][t] != 0) | latch
    return out
