"""The noisy trot of tests/noise_loop.py with one robot pushed over and an episode record kept beside it: NoisyWalkLoop with an external wrench on one robot during
a window of ticks (it reaches the plant step and, as on the device, the accelerometer), and tests/episode_ref.py's update after every closed tick.  Shared by
tests/test_episode_loop.py (the restatement alone: the push does tip the robot over, the others never notice) and tests/test_gpu_episode.py (the same push in the device
loop, the records kept by a1mpc_episode_update_batch_device).

The push: a roll torque of 150 N m on robot 5 for 60 ticks from walk tick 100.  The legs cannot answer it -- two legs at fz_max = 180 N and a lever of 0.13 m give 47 N m
-- so the body rolls past 60 degrees within the window whatever the controller does: a physical fall, nothing else."""
import numpy as np

import episode_ref as ER
import noise_loop as NL
import noise_ref as NR
import walk_loop as WL
import walk_ref as WR

ROBOT, TORQUE, PUSH_TICKS = 5, 150.0, 60
PUSH_FIRST = WL.PRIME + WL.STAND + 100          # the loop's tick index of the first pushed tick
CLOSED = WL.STAND + WL.WALK                     # closed ticks of the run: what `ticks` of a robot that stays up must read


def wrench(n, t):
    """the external wrench (n, 6: force, torque, world frame) of the loop's tick t"""
    w = np.zeros((n, 6))
    if PUSH_FIRST <= t < PUSH_FIRST + PUSH_TICKS:
        w[ROBOT, 3] = TORQUE
    return w


class PushedLoop(NL.NoisyWalkLoop):
    """NoisyWalkLoop under wrench(); self.episode holds the records of the restatement, updated after every closed tick with the truth, the estimate, the forces, the
    solver's status and the reach flags"""

    def __init__(self, oracle, scen, sc, n, noise=NR.NOMINAL):
        super().__init__(oracle, scen, sc, n, noise=noise)
        self.episode = np.zeros((n, ER.WORDS))

    def tick(self, step_plant=True, cmd=None, toggle=None):
        ext = wrench(self.n, self.t)
        step, sensors, t = WR.step, WR.sensors, self.t
        WR.step = lambda *a, **kw: step(*a[:8], ext, *a[9:], **kw)
        WR.sensors = lambda *a, **kw: sensors(*a, ext=ext, **kw)
        try:
            with np.errstate(all="ignore"):
                sol = super().tick(step_plant, cmd, toggle)
        finally:
            WR.step, WR.sensors = step, sensors
        if step_plant:
            self.episode = ER.update(self.episode, t, self.x, self.R, root_pos=self.pos, root_lin_vel=self.vel, grf_body=self.grf, contacts=self.ct, status=self.status,
                                     reach=self.sensors["reach"])
        return sol
