"""The pushed trot of tests/episode_loop.py with the respawn of tests/respawn_ref.py behind every tick, on the CPU: what the device loop of tests/test_gpu_respawn.py does
with a1mpc_respawn_batch_device and a1mpc_respawn_rows_device.  Every tick steps the plant; there is no `first` special case: every robot starts held for PRIME ticks
(life[:, 0] = PRIME), a held robot's plant rows are put back behind its step, and the mode toggle is each robot's own, when its record's clock reaches STAND.  A
respawned robot gets a new EKF, new contact / terrain filters, a new IMU window of its own (the loops' shared WindowFilter keeps one queue for the batch, which cannot
forget one robot: here every robot has a filter of one row) and the spawn values of everything the caller carries.  The push belongs to the episode it fells: the
wrench reaches a robot only while its episodes_done is 0."""
import numpy as np

import episode_loop as EL
import noise_ref as NR
import respawn_ref as RR
import sensor_loop as SL
import walk_loop as WL


class RobotFilters:
    """one sensor_loop.WindowFilter per robot behind the batch filter's call: the same elementwise arithmetic, and reset(b) forgets robot b alone"""

    def __init__(self, n, window):
        self.window, self.f = window, [SL.WindowFilter(1, window) for _ in range(n)]

    def __call__(self, x):
        return np.concatenate([f(x[b:b + 1]) for b, f in enumerate(self.f)], 0)

    def reset(self, b):
        self.f[b] = SL.WindowFilter(1, self.window)


class RespawnLoop(EL.PushedLoop):
    def __init__(self, oracle, scen, sc, n, cfg, noise=NR.NOMINAL):
        super().__init__(oracle, scen, sc, n, noise=noise)
        self.cfg = cfg
        self.filt = RobotFilters(n, SL.IMU_WINDOW)
        self.spawn = dict(x=self.x.copy(), R=self.R.copy(), foot=self.foot.copy(), grf=self.grf.copy(), ct=self.ct.copy(), pos=self.pos.copy(), vel=self.vel.copy(),
                          gc=self.gc.copy(), cmd={k: v.copy() for k, v in self.cmd.items()})
        self.life = np.zeros((n, 2), np.int32); self.life[:, 0] = cfg["hold_ticks"]
        self.finished = np.zeros((n, RR.WORDS))
        self.mask = np.zeros(n, np.uint8)

    def tick(self):
        n, clock = self.n, self.episode[:, 0]
        cmd = np.zeros((n, 6)); cmd[:, 0] = np.where(clock >= WL.STAND, WL.SPEED, 0.0)
        toggle = (clock == WL.STAND).astype(np.uint8)
        wrench, first = EL.wrench, (self.life[:, 1] == 0).astype(np.float64)[:, None]
        EL.wrench = lambda n_, t: wrench(n_, t) * first
        try:
            sol = super().tick(True, cmd, toggle)
        finally:
            EL.wrench = wrench
        self.episode, self.life, self.finished, self.mask = RR.decide(self.episode, self.life, self.cfg, self.finished)
        s = self.spawn
        for b in np.flatnonzero(self.mask):   # the plant's rows: on respawn and on every held tick
            self.x[b], self.R[b], self.foot[b], self.fvb[b], self.grf[b], self.ct[b] = s["x"][b], s["R"][b], s["foot"][b], 0.0, s["grf"][b], s["ct"][b]
        for b in np.flatnonzero(self.mask == 1):   # the handle's state of the robot (what = 15) and the rows the caller carries
            self.ekf[b], self.cst[b] = self.o.ekf_state(), self.o.contact_state()
            self.filt.reset(b)
            self.pos[b], self.vel[b], self.gc[b], self.bias[b] = s["pos"][b], s["vel"][b], s["gc"][b], 0.0
            for a in self.swing:
                a[b] = 0.0
            for k, v in self.cmd.items():
                v[b] = s["cmd"][k][b]
        return sol
