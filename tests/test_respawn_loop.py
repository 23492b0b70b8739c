"""CPU: the pushed trot with respawn under the restatements alone (tests/respawn_loop.py) -- the yardstick of the device loop of tests/test_gpu_respawn.py.  The pushed
robot falls inside the push window, is respawned, held for PRIME ticks and stands up again; nobody else notices: their records are, bit for bit, those of the
PushedLoop run without respawn."""
import numpy as np

import episode_loop as EL
import episode_ref as ER
import respawn_loop as RL
import respawn_ref as RR
import sensor_loop as SL
import walk_loop as WL


def test_the_pushed_robot_is_respawned_held_and_stands_up_again(oracle, scen):
    sc = SL.perturbed_standing_robots(scen)
    n, g = 7, EL.ROBOT
    assert n >= 6 and g < n
    T = WL.PRIME + WL.STAND + WL.WALK
    plain = EL.PushedLoop(oracle, scen, sc, n)
    for stepped, cmd, toggle in WL.schedule(n):
        plain.tick(step_plant=stepped, cmd=cmd, toggle=toggle)
    loop = RL.RespawnLoop(oracle, scen, sc, n, dict(RR.DEFAULT, hold_ticks=WL.PRIME))
    masks, bad = [], []
    for t in range(T):
        sol = loop.tick()
        masks.append(loop.mask[g])
        if loop.life[g, 1] == 1 and loop.mask[g] == 0:   # a free tick of its second episode
            finite = all(np.isfinite(v[g]).all() for v in (loop.x, loop.R, loop.foot, loop.pos, loop.vel, sol["grf"]))
            bad += [(t, what) for what in SL.conditions_hold(loop.x[g:g + 1], loop.sensors["reach"][g], loop.status[g:g + 1], finite)]
    first, second = loop.finished[g], loop.episode[g]
    others = np.arange(n) != g
    print("first episode:", dict(zip(ER.FIELDS, first)))
    print("second episode:", dict(zip(ER.FIELDS, second)), "life", loop.life[g])
    assert first[2] in (2, 3) and EL.PUSH_FIRST <= first[1] - 1 < EL.PUSH_FIRST + EL.PUSH_TICKS
    assert ER.bits_equal(first, plain.episode[g])
    t_fall = int(first[1]) - 1
    assert masks[:WL.PRIME] == [2] * WL.PRIME and masks[t_fall] == 1 and masks[t_fall + 1:t_fall + 1 + WL.PRIME] == [2] * WL.PRIME
    assert not any(masks[WL.PRIME:t_fall]) and not any(masks[t_fall + 1 + WL.PRIME:])
    assert list(loop.life[g]) == [0, 1] and not loop.life[others].any() and not loop.finished[others].any()
    assert second[2] == 0 and second[0] == T - (t_fall + 1 + WL.PRIME) and second[11] == 0 and second[12] == 0
    assert bad == [], bad[:5]
    assert ER.bits_equal(loop.episode[others], plain.episode[others])
