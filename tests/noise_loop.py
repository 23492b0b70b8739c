"""The trot of tests/walk_loop.py with sensor noise: WalkLoop with tests/noise_ref.py applied to the walk sensors before the tick reads them -- robot b is row b, the
noise's tick is the loop's tick index from 0 (the priming ticks count), the IMU bias starts at zero and is carried by the loop.  Shared by tests/test_noise_host.py
(which holds it to the clean trot's conditions) and tests/test_gpu_noise.py (which runs the same schedule on the device and compares the end state).

The levels are noise_ref.NOMINAL.  Measured on this loop with 4 and 17 robots (seed 5, IMU window 1, 10 + 100 + 360 ticks): every condition of the clean trot holds; the
height estimate is off by 3.8e-3 / 6.5e-3 at most (clean: 3.9e-3; the bar is 1e-2), the heading speed is 0.188 .. 0.203 (clean 0.194 .. 0.195).  Findings, not asserted:
at twice NOMINAL the contacts stop being the planned pairs (10 N of force noise reaches the early-contact latch), and with an IMU window of 5 this loop's known delay
oscillation (tests/sensor_loop.py) takes the height to 0.25 with or without noise -- `findings()` prints both."""
import numpy as np

import noise_ref as NR
import sensor_loop as SL
import walk_loop as WL
import walk_ref as WR


class NoisyWalkLoop(WL.WalkLoop):
    """WalkLoop whose sensors pass through noise_ref.apply (noise None: the clean loop, bit for bit)"""

    def __init__(self, oracle, scen, sc, n, noise=None, window=SL.IMU_WINDOW, **walk):
        super().__init__(oracle, scen, sc, n, **walk)
        self.noise, self.t, self.bias, self.z = noise, 0, np.zeros((n, 6)), None
        self.filt = SL.WindowFilter(n, window)
        self.vel_error = 0.0   # the worst |estimated - true velocity| over the closed ticks

    def _sensors(self, clean):
        def sensors(*a, **kw):
            s = clean(*a, **kw)
            if self.noise is not None:
                out, self.bias, self.z = NR.apply(self.noise, 0, self.t, {k: s[k] for k in NR.SENSORS}, self.bias)
                s = dict(s, **out)
            return s
        return sensors

    def tick(self, step_plant=True, cmd=None, toggle=None):
        clean = WR.sensors
        WR.sensors = self._sensors(clean)   # (WalkLoop.tick synthesises its sensors itself: the noise goes between that call and everything that reads them)
        try:
            sol = super().tick(step_plant, cmd, toggle)
        finally:
            WR.sensors = clean
        if step_plant:
            self.vel_error = max(self.vel_error, float(np.abs(self.vel - self.x[:, 9:12]).max()))
        self.t += 1
        return sol


def scaled(cfg, factor):
    return dict(cfg, **{k: factor * cfg[k] for k in NR.LEVELS})


def findings(oracle, scen, n=4):
    """the two findings of the module's docstring, measured: dict of what each run did (no assertion)"""
    sc = SL.perturbed_standing_robots(scen)
    out = {}
    for name, noise, window in (("twice NOMINAL", scaled(NR.NOMINAL, 2.0), 1), ("window 5, NOMINAL", NR.NOMINAL, 5), ("window 5, clean", None, 5)):
        loop = NoisyWalkLoop(oracle, scen, sc, n, noise=noise, window=window)
        hist = dict(contacts=[], foot=[], state=[], R=[])
        lo, hi, failed = np.inf, -np.inf, None
        for t, (stepped, cmd, toggle) in enumerate(WL.schedule(n)):
            loop.tick(step_plant=stepped, cmd=cmd, toggle=toggle)
            if not stepped:
                continue
            bad = SL.conditions_hold(loop.x, loop.sensors["reach"], loop.status, bool(np.isfinite(loop.x).all()))
            failed = (t, bad) if bad and failed is None else failed
            lo, hi = min(lo, float(loop.x[:, 5].min())), max(hi, float(loop.x[:, 5].max()))
            if t >= WL.PRIME + WL.STAND:
                for k, v in (("contacts", loop.ct), ("foot", loop.foot), ("state", loop.x), ("R", loop.R)):
                    hist[k].append(v.copy())
        bad, walk = WL.walk_conditions({k: np.stack(v) for k, v in hist.items()}, n)
        out[name] = dict(first_failed_tick=failed, height=(lo, hi), walk=bad, heading_speed=(float(walk["heading_speed"].min()), float(walk["heading_speed"].max())))
    return out
