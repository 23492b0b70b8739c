"""The closed loop  sensors -> tick -> plant -> sensors  on the CPU, shared by tests/test_sensor_synthesis_host.py (which holds it to the loop's conditions) and
tests/test_gpu_sensor_synthesis.py (which compares the device loop's end state with it): every stage of a1mpc_control_tick_sensors_device from the oracle's stage
functions, chained the way tests/test_gpu_gait_cycle.py chains them (leg state -> EKF, device variant -> update_plan -> swing legs -> contacts / terrain -> cold MPC
solve), the sensor and command front end from tests/frontend_ref.py, the plant from tests/plant_ref.py and the sensors from tests/sensor_synthesis_ref.py.

The robots stand (no mode toggle, zero stick command).  Their stance feet lie on the plane z = 0 of the world, so that the height the EKF estimates from the feet
(assume_flat_ground) has a truth to be compared with: the plant's pos_z.

PRIME = 10: the EKF starts every robot at height 0.09 (A1BasicEKF.cpp:54-68) and is primed with sensors synthesised from the UNSTEPPED plant under the equilibrium forces
(m g / 4 per leg, all legs in stance).  Measured on the CPU loop, the worst height error of the four robots: 0.24 m after the first priming tick (which only initialises
the filter), 1.2e-4 m after the second, 1.3e-5 m after the tenth (test_closed_loop_on_the_cpu prints and asserts it): two ticks bring it within 1 mm, ten are taken.

The perturbation: roll / pitch / yaw, the height, the horizontal place, omega and the feet's scatter have the magnitudes of tests/test_gpu_plant.py's
_perturbed_standing_robots; v starts at ZERO where that test draws it from N(0, 0.1): the plant is not stepped while the EKF is primed, and a robot that reports a
velocity while its feet stay where they are contradicts itself -- with v from N(0, 0.1) the height estimate runs AWAY from the truth during the priming (1.4 mm after 10
ticks, 6 mm after 60) and no P meets the 1 mm.  (omega != 0 on an unstepped plant is no such contradiction to the EKF: the foot velocities carry omega x r and the
filter takes it out again.)

IMU_WINDOW = 1: the tick's sensor stage averages the IMU over a window (5 in the reference, against sensor noise).  The synthesised sensors carry no noise, and in this
loop -- massless legs, forces applied without any actuator dynamics, the reference's MPC weights -- the two ticks of delay of a 5-sample mean of the gyro turn the roll
axis into a growing oscillation (period 10 ticks, |omega_x| 0.5 -> 4.8 rad/s over 100 ticks, measured on this CPU loop; the tilt and height conditions still hold there,
but an end state on a growing oscillation is no yardstick).  Windows 1 and 2 settle monotonically."""
import numpy as np

import frontend_ref as FR
import plant_ref as PR
import sensor_synthesis_ref as SR

PRIME, TICKS, H = 10, 100, 10
CONTROL_DT = 0.0025
IMU_WINDOW = 1
DEFAULT_FOOT_POS = np.array([0.17, 0.15, -0.35, 0.17, -0.15, -0.35, -0.17, 0.15, -0.35, -0.17, -0.15, -0.35])
CONDITIONS = dict(tilt=0.2, height=0.05)   # |roll|, |pitch| <= 0.2; |pos_z - 0.3| <= 0.05, on every tick


def perturbed_standing_robots(scen, nb=17, seed=5):
    rng = np.random.default_rng(seed)
    P = scen.PARAM_SETS["gazebo"]
    roll = rng.uniform(-.1, .1, nb); pit = rng.uniform(-.1, .1, nb); yaw = rng.uniform(-.5, .5, nb)
    R = scen.rot_zyx(roll, pit, yaw)
    pos = np.stack([rng.normal(0, 1, nb), rng.normal(0, 1, nb), 0.3 + rng.uniform(-.03, .03, nb)], 1)
    footb = np.array(P["foot"], float).reshape(1, 4, 3) + rng.uniform(-.02, .02, (nb, 4, 3))
    foot = np.einsum("bij,blj->bli", R, footb); foot[:, :, 2] = -pos[:, 2:3]   # the feet on the plane z = 0
    w = rng.normal(0, .2, (nb, 3))
    state = np.concatenate([PR.euler_of(R.reshape(nb, 9)), pos, w, np.zeros((nb, 3))], 1)
    params = dict(P, **scen.MPC_CONSTANTS)
    feq = np.einsum("bji,j->bi", R, np.array([0.0, 0.0, params["mass"] * 9.8 / 4.0]))   # R^T (0, 0, m g / 4): the equilibrium force of a leg in the body frame
    return dict(params=params, horizon=H, state=np.ascontiguousarray(state), R=np.ascontiguousarray(R.reshape(nb, 9)), foot=np.ascontiguousarray(foot.reshape(nb, 12)),
                grf_eq=np.ascontiguousarray(np.tile(feq, (1, 4))), contact=np.ones((nb, 4), np.uint8))


def euler_of_quat(q):
    """Utils::quat_to_euler, S/utils/Utils.cpp:7-33, in numpy; (n, 4) as w, x, y, z -> (n, 3)"""
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    ysq = y * y
    t2 = np.clip(2.0 * (w * y - z * x), -1.0, 1.0)
    return np.stack([np.arctan2(2.0 * (w * x + y * z), 1.0 - 2.0 * (x * x + ysq)), np.arcsin(t2), np.arctan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (ysq + z * z))], 1)


class WindowFilter:
    """MovingWindowFilter, S/utils/filter.hpp:26-62, on (n, 6) samples: Neumaier sums, divided by the window length from the first sample on"""

    def __init__(self, n, window=IMU_WINDOW):
        self.window, self.q, self.sum, self.corr = window, [], np.zeros((n, 6)), np.zeros((n, 6))

    def _add(self, val):
        ns = self.sum + val
        self.corr = self.corr + np.where(np.abs(self.sum) >= np.abs(val), (self.sum - ns) + val, (val - ns) + self.sum)
        self.sum = ns

    def __call__(self, x):
        if len(self.q) >= self.window:
            self._add(-self.q.pop(0))
        self._add(x); self.q.append(x.copy())
        return (self.sum + self.corr) / float(self.window)


class OracleLoop:
    """n robots of perturbed_standing_robots on the CPU"""

    def __init__(self, oracle, scen, sc, n):
        self.o, self.scen, self.n, self.P = oracle, scen, n, sc["params"]
        P = self.P
        self.pr = oracle.mpc_params(H, P["dt"], P["mu"], P["fz_min"], P["fz_max"], P["q"], P["r"], P["mass"], P["inertia"])
        self.st = oracle.default_settings()
        self.gp = oracle.gait_params(DEFAULT_FOOT_POS)
        self.x, self.R, self.foot = sc["state"][:n].copy(), sc["R"][:n].copy(), sc["foot"][:n].copy()
        self.grf, self.ct = sc["grf_eq"][:n].copy(), sc["contact"][:n].copy()
        self.filt = WindowFilter(n)
        self.cmd = FR.initial_state(n)
        self.ekf = [oracle.ekf_state() for _ in range(n)]; self.cst = [oracle.contact_state() for _ in range(n)]
        self.pos, self.vel = np.tile([0.0, 0.0, 0.3], (n, 1)), np.zeros((n, 3))   # (the estimate a tick world starts from: gpu_common.tick_world)
        self.gc = np.tile([0.0, 120.0, 120.0, 0.0], (n, 1))
        self.swing = [np.zeros((n, 12)), np.zeros((n, 12)), np.zeros((n, 12))]
        self.sensors = self.status = None

    def tick(self, step_plant=True):
        """one tick: sensors from the plant's state and the forces applied last, the control tick, and (step_plant) the plant under the tick's forces"""
        o, n, P = self.o, self.n, self.P
        s = SR.synthesise(P["mass"], self.x, self.R, self.foot, self.grf, self.ct)
        self.sensors = s
        Rw = FR.quat_to_rotation(s["quat"]); eul = euler_of_quat(s["quat"]); Rz = FR.yaw_rotation(eul[:, 2])
        f = self.filt(np.concatenate([s["imu_acc_raw"], s["imu_gyro_raw"]], 1))
        acc, gyro = f[:, :3], f[:, 3:]
        w = FR.rotate(Rw, gyro)
        c = FR.command_step(self.cmd, np.zeros((n, 6)), np.zeros(n, np.uint8), self.pos, CONTROL_DT)
        x0 = np.zeros((n, 13)); xref = np.zeros((n, 13 * H)); fa = np.zeros((n, 12)); ct = np.zeros((n, 4), np.uint8)
        for b in range(n):
            leg = o.leg_state(s["joint_pos"][b], s["joint_vel"][b], Rw[b], self.pos[b], self.vel[b])
            self.pos[b], self.vel[b], _ = o.ekf_step(self.ekf[b], CONTROL_DT, c["movement_mode"][b], s["foot_force"][b], Rw[b], acc[b], gyro[b], leg["foot_pos_rel"],
                                                     leg["foot_vel_rel"], device=True)
            self.gc[b], pc, rel, _, _ = o.update_plan(self.gp, c["movement_mode"][b], self.gc[b], np.full(4, 2.0), self.vel[b], Rz[b], Rw[b], self.pos[b], c["root_lin_vel_d"][b])
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
            self.x, self.R, self.foot = PR.step(P, self.x, self.R, self.foot, self.grf, self.ct, None, CONTROL_DT, 1)
        return sol


def conditions_hold(x, reach, status, finite):
    """the loop's conditions on one tick: x (n, >= 12) the plant's state -> list of what failed"""
    bad = []
    if not finite: bad.append("a non-finite output")
    if not (np.asarray(status) == 1).all(): bad.append(f"status {np.unique(status)}")
    if np.asarray(reach).any(): bad.append("a reach flag")
    if np.abs(x[:, 0:2]).max() > CONDITIONS["tilt"]: bad.append(f"tilt {np.abs(x[:, 0:2]).max():.3f}")
    if np.abs(x[:, 5] - 0.3).max() > CONDITIONS["height"]: bad.append(f"height {x[:, 5].min():.3f} .. {x[:, 5].max():.3f}")
    return bad
