"""The closed loop  touch sensors -> tick -> height-field step -> touch sensors  on the CPU: tests/ground_loop.py's GroundLoop with the plant step of
tests/heightfield_ref.py -- one gridded field under all robots, each on a tile of its own through its origin row.  Shared by tests/test_heightfield_loop.py (which holds
it to the conditions below) and tests/test_gpu_heightfield.py (which runs the same schedules on the device and compares).

The schedule and the per-tick conditions are walk_loop's; the height condition is taken above the step's ground_out, pos_z - hf(pos_x, pos_y), and every origin is chosen
so that hf is 0 under the robot's starting position.  Figures measured on these loops are in profiles/heightfield.md."""
import numpy as np

import frontend_ref as FR
import ground_loop as GL
import heightfield_ref as HR
import sensor_loop as SL

SPACING = 0.05           # dx = dy of both schedules' fields
TILE_NODES = 33          # a ramp tile is 1.6 m x 1.6 m with the robot at its middle: a walk of WALK ticks at SPEED covers 0.18 m and a foot is within 0.3 m of the body
RISES = (0.08, 0.05, 0.03, 0.02)   # tried in this order: the largest at which the stairs loop keeps conditions_hold empty on every tick is STAIR_RISE
STAIR_RUN = 0.30
STAIR_RISE = 0.03        # 0.08 tilts past the bar while standing (0.234), 0.05 drops the height above the field to 0.243 as the body crosses the riser: profiles/heightfield.md
STAIR_NODES = 41         # 2.0 m x 2.0 m of stairs along x
STAIR_START = (0.85, 1.0)   # where a robot's body starts on the stairs, in the field's frame: 0.05 m in front of the riser at x = 0.90, on the tread 0.60 .. 0.90
# |terrain_angle - atan(RAMP_SLOPE)| on the two pitch tiles over the last GL.TERRAIN_TICKS ticks: ground_loop's bar, measured there on the plane loop
TERRAIN_BAR = GL.TERRAIN_BAR


def loop_planes(sc, n):
    """the planes of the device loops: robots 0 .. 3 are the CPU loop's ((+s, 0), (-s, 0), (0, +s), flat); robot b >= 4 stands on the pattern of robot b % 4 with a
    slope between 0.2 s and 0.5 s; hz = 0 under every start.  A COPY of _loop_planes(sc, n, True) of tests/test_gpu_ground.py, seed 8600 included (that file is a
    yardstick and is not imported from): the two must stay equal, so that the height-field loops stand on the slopes the plane loops were chosen on"""
    g = np.zeros((n, 3))
    g[:4] = GL.ramp_planes(sc, GL.RAMP_SLOPE)
    scale = np.random.default_rng(8600).uniform(0.2, 0.5, n)
    for b in range(4, n):
        g[b, 1:] = g[b % 4, 1:] * scale[b]
    pos = sc["state"][:n, 3:5]
    g[4:, 0] = -(g[4:, 1] * pos[4:, 0] + g[4:, 2] * pos[4:, 1])
    return g


def ramp_tiles(heightfields, sc, planes):
    """the n planes (z0, sx, sy) -- ground_loop.ramp_planes(sc, s) on the CPU -- as n bilinear tiles of ONE field, side by side along x -> (heightfield_ref.Field,
    origin (n, 3)).  Tile k is its robot's plane sampled at the nodes; the robot starts at the tile's middle and its origin row lifts the tile so that hf is 0 there"""
    n = len(planes)
    tiles = [heightfields.ramp(TILE_NODES, TILE_NODES, SPACING, SPACING, planes[k, 1], planes[k, 2]) for k in range(n)]
    H, origin = heightfields.tiles(tiles, dx=SPACING)
    mid = (TILE_NODES - 1) * SPACING / 2.0
    pos = sc["state"][:n, 3:5]
    origin[:, 0] += pos[:, 0] - mid
    origin[:, 1] = pos[:, 1] - mid
    field = HR.Field(H, 0.0, 0.0, SPACING, SPACING, 1)
    origin[:, 2] = -HR.sample(field, pos[:, 0], pos[:, 1], np.ascontiguousarray(origin))
    return field, np.ascontiguousarray(origin)


def stairs_field(heightfields, sc, rise, n=4):
    """cell-constant stairs along x with run STAIR_RUN, one field under every robot -> (Field, origin (n, 3)): each robot's origin row puts its start at STAIR_START of the
    field's frame and hf = 0 under it.  A robot's feet span more than one run, so its front feet start one tread up"""
    H = heightfields.stairs(STAIR_NODES, STAIR_NODES, SPACING, SPACING, rise, STAIR_RUN, 0)
    field = HR.Field(H, 0.0, 0.0, SPACING, SPACING, 0)
    pos = sc["state"][:n, 3:5]
    origin = np.zeros((n, 3))
    origin[:, 0] = pos[:, 0] - STAIR_START[0]; origin[:, 1] = pos[:, 1] - STAIR_START[1]
    origin[:, 2] = -HR.sample(field, pos[:, 0], pos[:, 1], origin)
    return field, origin


class HeightfieldLoop(GL.GroundLoop):
    """GroundLoop with a1mpc_heightfield_step_batch's restatement as the plant step; nothing else of the tick changes.  self.ground is the step's ground_out -- the row
    the height condition of ground_loop.run and the episode record take"""

    def __init__(self, oracle, scen, sc, n, field, origin=None, touch_force=0.0, use_terrain_adapt=1):
        super().__init__(oracle, scen, sc, n, ground=None, touch_force=touch_force, use_terrain_adapt=use_terrain_adapt)
        self.field, self.origin = field, None if origin is None else np.ascontiguousarray(origin, dtype=np.float64)
        self.ground[:, 0] = HR.sample(field, self.x[:, 3], self.x[:, 4], self.origin)   # (under the unstepped plant)

    def tick(self, step_plant=True, cmd=None, toggle=None):
        """GroundLoop.tick; its plane step (over the previous ground_out, a level plane) is thrown away and the height-field step taken from the same inputs instead:
        the state before the step, the tick's forces, contacts and swing targets, and R_z as the tick made it of the sensors' quaternion"""
        x, R, foot = self.x.copy(), self.R.copy(), self.foot.copy()
        sol = super().tick(step_plant=step_plant, cmd=cmd, toggle=toggle)
        if step_plant:
            # GroundLoop.tick's own step overwrites self.x, self.R, self.foot, self.fvb and self.touch -- all five are assigned again below -- and nothing else: the
            # forces and contacts it was fed are the tick's, and the swing targets are the swing-leg stage's, made before the step
            assert self.grf is sol["grf"] and self.ct.shape == (self.n, 4) and (self.ct >= self.plan).all()   # (this tick's solution; its contacts: the plan and the latch)
            Rz = FR.yaw_rotation(SL.euler_of_quat(self.sensors["quat"])[:, 2])
            self.x, self.R, self.foot, self.fvb, self.touch, self.ground = HR.step(self.P, x, R, foot, self.grf, self.ct, Rz, self.swing[2], self.field, self.origin, None,
                                                                                   SL.CONTROL_DT, 1, swing_track=1.0)
        return sol


def run(loop, n):
    """ground_loop.run (its height condition reads loop.ground: here the step's ground_out) with the ground_out rows of the WALK ticks in the history"""
    kept = []
    tick = loop.tick

    def keeping(step_plant=True, cmd=None, toggle=None):
        sol = tick(step_plant=step_plant, cmd=cmd, toggle=toggle)
        kept.append(loop.ground.copy())
        return sol
    loop.tick = keeping
    try:
        hist, failed = GL.run(loop, n)
    finally:
        del loop.tick
    hist["ground"] = np.stack(kept[-hist["state"].shape[0]:])
    return hist, failed


def heights_above_the_field(hist, field, origin):
    """the height above the field of every foot after every WALK tick's step (T, n, 4), and those on the ticks where the leg's contact goes 0 -> 1"""
    T, n = hist["contacts"].shape[:2]
    foot, st = hist["foot"].reshape(T, n, 4, 3), hist["state"]
    h = np.zeros((T, n, 4))
    for t in range(T):
        X, Y, Z = st[t, :, None, 3] + foot[t, :, :, 0], st[t, :, None, 4] + foot[t, :, :, 1], st[t, :, None, 5] + foot[t, :, :, 2]
        h[t] = Z - HR.sample(field, X, Y, origin)
    edge = (hist["contacts"][1:] == 1) & (hist["contacts"][:-1] == 0)
    return h[1:][edge], h


def feet_in_field_coordinates(hist, field, origin):
    """(ux, uy) of every foot over the WALK ticks, in nodes: inside the grid between 0 and nx - 1 / ny - 1"""
    T, n = hist["contacts"].shape[:2]
    foot, st = hist["foot"].reshape(T, n, 4, 3), hist["state"]
    o = np.zeros((n, 3)) if origin is None else origin
    ux = (st[:, :, None, 3] + foot[:, :, :, 0] - o[None, :, None, 0] - field.x0) / field.dx
    uy = (st[:, :, None, 4] + foot[:, :, :, 1] - o[None, :, None, 1] - field.y0) / field.dy
    return ux, uy
