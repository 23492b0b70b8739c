"""The closed loops over a height field on the CPU (tests/heightfield_loop.py): four robots on ramp tiles of one bilinear field, and on cell-constant stairs with the
touch sensor -- the yardsticks of the GPU loops of tests/test_gpu_heightfield.py.  Each loop runs once."""
import numpy as np

import ground_loop as GL
import heightfield_loop as HL
import sensor_loop as SL
import walk_loop as WL

_SHARED = {}


def loops(oracle, scen, pkg):
    """the CPU loops, each run once: the ramp tiles at GL.RAMP_SLOPE (touch_force 0) and the stairs at HL.STAIR_RISE (touch_force GL.TOUCH_FORCE)"""
    if "loops" not in _SHARED:
        n = 4
        sc = SL.perturbed_standing_robots(scen)
        out = {}
        field, origin = HL.ramp_tiles(pkg.heightfields, sc, GL.ramp_planes(sc, GL.RAMP_SLOPE))
        out["ramp"] = (field, origin) + HL.run(HL.HeightfieldLoop(oracle, scen, sc, n, field, origin), n)
        field, origin = HL.stairs_field(pkg.heightfields, sc, HL.STAIR_RISE)
        out["stairs"] = (field, origin) + HL.run(HL.HeightfieldLoop(oracle, scen, sc, n, field, origin, touch_force=GL.TOUCH_FORCE), n)
        _SHARED["loops"] = out
    return _SHARED["loops"]


def test_loop_ramp_tiles(oracle, scen, pkg):
    """the four robots of ground_loop.ramp_planes (slopes (+s, 0), (-s, 0), (0, +s), flat; s = 0.15), each on a 33 x 33 tile of ONE bilinear field sampled from its plane,
    dx = dy = 0.05, origin rows that put hf = 0 under each start: no foot leaves its tile; conditions_hold (height above ground_out) stays empty on every closed tick; the
    terrain angle on the two pitch tiles over the last 120 ticks is atan(s) within ground_loop's bar (measured on this loop: 8.72e-5, the plane loop's own figure);
    ground_out is the field under the body; every touchdown is on the field"""
    field, origin, hist, failed = loops(oracle, scen, pkg)["ramp"]
    assert WL.WALK * WL.SPEED * SL.CONTROL_DT + 0.3 < (HL.TILE_NODES - 1) * HL.SPACING / 2.0   # a walk's length and a leg's reach fit half a tile
    assert field.interp == 1 and field.dx == field.dy == 0.05 and field.nx == 4 * HL.TILE_NODES
    assert not failed, failed[:3]
    ux, uy = HL.feet_in_field_coordinates(hist, field, origin)
    for k in range(4):
        lo = k * HL.TILE_NODES
        assert ux[:, k].min() >= lo + 1 and ux[:, k].max() <= lo + HL.TILE_NODES - 2 and uy[:, k].min() >= 1 and uy[:, k].max() <= HL.TILE_NODES - 2, k
    s = GL.RAMP_SLOPE
    ta = hist["terrain_angle"][-GL.TERRAIN_TICKS:]
    dev = float(np.abs(ta[:, :2] - np.arctan(s)).max())
    td, h = HL.heights_above_the_field(hist, field, origin)
    under = HL.HR.sample(field, hist["state"][-1][:, 3], hist["state"][-1][:, 4], origin)
    print(f"ramp tiles s = {s}: terrain angle on the pitch tiles off atan(s) by {dev:.3e} at most (bar {HL.TERRAIN_BAR:.2e}); {len(td)} touchdowns off the field by "
          f"{np.abs(td).max():.1e} at most; hf under the bodies at the end {under}")
    assert HL.TERRAIN_BAR == GL.TERRAIN_BAR and dev <= HL.TERRAIN_BAR, dev
    assert len(td) == 12 * 4 and np.abs(td).max() <= GL.TOUCHDOWN and h.min() >= -GL.TOUCHDOWN
    assert HL.HR.same_heights(hist["ground"][-1][:, 0], under) and not hist["ground"][:, :, 1:].any()
    assert under[0] > 0.01 and under[1] < -0.01 and under[3] == 0.0   # (uphill, downhill, flat)
    assert not GL.early_contacts(hist)


def test_loop_stairs(oracle, scen, pkg):
    """cell-constant stairs along x, run 0.30 m, rise HL.STAIR_RISE (the largest of 0.08 / 0.05 / 0.03 / 0.02 at which the loop holds its conditions), touch_force 60:
    conditions_hold stays empty on every tick; every 0 -> 1 contact edge leaves the foot on the field under it; every robot's body gains a rise in ground_out over the
    schedule; the contacts are those of the reference's latch rule; the touch sensor fires (early contacts on every robot)"""
    field, origin, hist, failed = loops(oracle, scen, pkg)["stairs"]
    assert field.interp == 0 and HL.STAIR_RUN == 0.30 and HL.STAIR_RISE == max(r for r in HL.RISES if r <= HL.STAIR_RISE)
    assert not failed, failed[:3]
    td, h = HL.heights_above_the_field(hist, field, origin)
    gain = hist["ground"][-1][:, 0] - hist["ground"][0][:, 0]
    ec = GL.early_contacts(hist)
    print(f"stairs rise {HL.STAIR_RISE}: {len(td)} touchdowns off the field by {np.abs(td).max():.1e} at most, lowest foot {h.min():.1e}; ground_out gained {gain}; "
          f"{len(ec)} early-contact ticks; tilt {np.abs(hist['state'][:, :, :2]).max():.3f}")
    assert len(td) >= 12 * 4 and np.abs(td).max() <= GL.TOUCHDOWN and h.min() >= -GL.TOUCHDOWN
    assert gain.max() >= HL.STAIR_RISE - 1e-12
    assert np.array_equal(GL.latch_by_the_reference_rule(hist), hist["contacts"])
    assert min(sum(1 for e in ec if e[1] == b) for b in range(4)) >= 1
    ux, uy = HL.feet_in_field_coordinates(hist, field, origin)
    assert ux.min() >= 1 and ux.max() <= field.nx - 2 and uy.min() >= 1 and uy.max() <= field.ny - 2
    treads = {int(v) for v in np.floor(ux * HL.SPACING / HL.STAIR_RUN + 1e-9).ravel()}
    assert len(treads) >= 2   # (the feet stand on more than one tread)
