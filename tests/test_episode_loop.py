"""CPU: the pushed trot of tests/episode_loop.py under the restatement alone (tests/episode_ref.py) -- the yardstick of the device loop of tests/test_gpu_episode.py.  The
push tips robot 5 over inside its window and nothing else: the other 16 stay alive through all 460 closed ticks, and their records are what numpy makes of the per-tick
history."""
import numpy as np

import episode_loop as EL
import episode_ref as ER
import sensor_loop as SL
import walk_loop as WL


def test_the_push_fells_one_robot_and_the_restatement_sees_it(oracle, scen):
    sc = SL.perturbed_standing_robots(scen)
    n = 17
    loop = EL.PushedLoop(oracle, scen, sc, n)
    tilt, verr, start, end = np.zeros(n), np.zeros(n), None, None
    for t, (stepped, cmd, toggle) in enumerate(WL.schedule(n)):
        loop.tick(step_plant=stepped, cmd=cmd, toggle=toggle)
        if stepped:
            start = loop.x[:, 3:5].copy() if start is None else start
            d = loop.vel - loop.x[:, 9:12]
            tilt = np.maximum(tilt, 1.0 - loop.R[:, 8]); verr = np.maximum(verr, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            end = loop.x[:, 3:5].copy()
    ep = loop.episode
    others = np.arange(n) != EL.ROBOT
    print("the pushed robot:", dict(zip(ER.FIELDS, ep[EL.ROBOT])))
    print("the others: tilt_max", ep[others, 5].max(), "est_vel_err_max", ep[others, 8].max(), "dist2", ep[others, 15].min(), "..", ep[others, 15].max())
    assert ep[EL.ROBOT, 2] in (2, 3) and EL.PUSH_FIRST <= ep[EL.ROBOT, 1] - 1 < EL.PUSH_FIRST + EL.PUSH_TICKS
    assert (ep[others, 2] == 0).all() and (ep[others, 1] == 0).all() and (ep[others, 0] == EL.CLOSED).all()
    assert ep[EL.ROBOT, 0] == ep[EL.ROBOT, 1] - 1 - WL.PRIME   # every closed tick before the fall was accumulated
    assert ER.bits_equal(ep[others, 5], tilt[others]) and ER.bits_equal(ep[others, 8], verr[others])
    dx, dy = end[:, 0] - start[:, 0], end[:, 1] - start[:, 1]
    assert ER.bits_equal(ep[others, 15], (dx * dx + dy * dy)[others]) and ER.bits_equal(ep[others, 13:15], start[others])
    s = ER.summary(ep)
    assert list(s[:5]) == [n, n - 1, 0, ep[EL.ROBOT, 2] == 2, ep[EL.ROBOT, 2] == 3] and s[5] == ep[EL.ROBOT, 1] - 1 and s[6] == ep[:, 0].sum()
