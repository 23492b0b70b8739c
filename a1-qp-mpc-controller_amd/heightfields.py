"""Small generators of height fields for a1mpc_heightfield_step_batch (numpy only).  Every field is heights (ny, nx), row-major with x fastest: heights[j, i] is the
height of node (i, j) at (x0 + i dx, y0 + j dy), the layout of a1mpc_heightfield.height.  Pass one to Engine.heightfield with the same dx, dy."""
import numpy as np


def ramp(nx, ny, dx, dy, sx, sy):
    """the plane sx x + sy y sampled at the nodes (x = i dx, y = j dy): with interp 1 the field IS that plane inside the grid, up to rounding"""
    x, y = np.arange(nx, dtype=np.float64) * dx, np.arange(ny, dtype=np.float64) * dy
    return np.ascontiguousarray(sx * x[None, :] + sy * y[:, None])


def stairs(nx, ny, dx, dy, rise, run, axis=0):
    """treads of depth `run` that climb by `rise` along x (axis 0) or y (axis 1), for interp 0: the node at distance s from node 0 along the axis is on tread
    floor(s / run).  run should be a multiple of the spacing along the axis, so that every riser stands on a node line"""
    n, d = (nx, dx) if axis == 0 else (ny, dy)
    tread = np.floor(np.arange(n, dtype=np.float64) * d / run + 1e-9)   # (the guard keeps k * d / run from landing just under an integer)
    h = rise * tread
    return np.ascontiguousarray(np.broadcast_to(h[None, :] if axis == 0 else h[:, None], (ny, nx)), dtype=np.float64)


def rough(nx, ny, seed, amplitude):
    """independent heights, uniform in [-amplitude, amplitude), reproducible from the seed"""
    return np.random.default_rng(seed).uniform(-amplitude, amplitude, (ny, nx))


def tiles(fields, dx=1.0):
    """lays fields side by side along x -> (heights (max ny, sum nx), origins (k, 3)).  A shorter tile is continued along y with its last row, as the sampling rule
    continues a field past its edge.  Row k of origins is the (ox, oy, oz) that puts node (0, 0) of tile k at the world position (x0, y0) of the whole field for a robot
    that is given it: ox = -(first column of tile k) dx, oy = oz = 0; add a robot's own offset to it.  Tiles touch: a robot that leaves its tile along x walks onto its
    neighbour's, so make a tile as wide as its robot's schedule needs"""
    fields = [np.asarray(f, dtype=np.float64) for f in fields]
    ny = max(f.shape[0] for f in fields)
    padded = [np.concatenate([f, np.repeat(f[-1:, :], ny - f.shape[0], axis=0)], axis=0) for f in fields]
    first = np.concatenate([[0], np.cumsum([f.shape[1] for f in fields])[:-1]])
    origins = np.zeros((len(fields), 3))
    origins[:, 0] = -first.astype(np.float64) * dx
    return np.ascontiguousarray(np.concatenate(padded, axis=1)), origins
