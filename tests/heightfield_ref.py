"""a1mpc_heightfield_sample_batch and a1mpc_heightfield_step_batch restated in numpy, ELEMENTWISE, from the text of include/a1mpc.h: the sampling rule hf(X, Y) one IEEE
operation per step in the header's order (every value a vector over the robots), and the step as tests/ground_ref.py does it -- tests/walk_ref.py's step without a
ground, then the rule.  pos, R, v, omega, the feet, foot_vel_body, touch and ground_out equal the kernel's bit for bit and the angles lie within plant_ref.ANGLE_BAR.
Test infrastructure only."""
import numpy as np

import plant_ref as PR
import walk_ref as WR


class Field:
    """a1mpc_heightfield on the host: heights (ny, nx), H[j, i] at (x0 + i dx, y0 + j dy)"""

    def __init__(self, heights, x0=0.0, y0=0.0, dx=1.0, dy=1.0, interp=0):
        self.H = np.ascontiguousarray(heights, dtype=np.float64)
        assert self.H.ndim == 2
        self.ny, self.nx = self.H.shape
        self.x0, self.y0, self.dx, self.dy, self.interp = np.float64(x0), np.float64(y0), np.float64(dx), np.float64(dy), int(interp)
        self.H.setflags(write=False)


def sample(field, X, Y, origin=None):
    """hf(X, Y); X, Y (n,) or (n, k), origin (n, 3) or None (then the subtraction is skipped, not done with 0)"""
    f = field
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    with np.errstate(all="ignore"):
        inv_dx, inv_dy = np.float64(1.0) / f.dx, np.float64(1.0) / f.dy
        if origin is not None:
            o = np.asarray(origin, np.float64)
            ox, oy, oz = (o[:, k].reshape((-1,) + (1,) * (X.ndim - 1)) for k in range(3))
            ux = ((X - ox) - f.x0) * inv_dx; uy = ((Y - oy) - f.y0) * inv_dy
        else:
            ux = (X - f.x0) * inv_dx; uy = (Y - f.y0) * inv_dy
        valid = (ux == ux) & (uy == uy)
        mx, my = np.float64(f.nx - 1), np.float64(f.ny - 1)
        cx = np.where(ux > 0.0, ux, 0.0); cx = np.where(cx < mx, cx, mx)
        cy = np.where(uy > 0.0, uy, 0.0); cy = np.where(cy < my, cy, my)
        assert np.isfinite(cx).all() and np.isfinite(cy).all() and cx.min(initial=0.0) >= 0.0 and cy.min(initial=0.0) >= 0.0   # only these are converted
        i, j = cx.astype(np.int64), cy.astype(np.int64)   # (truncation, as a C cast of a value that is not negative)
        flat = f.H.reshape(-1)
        nx = np.int64(f.nx)
        if f.interp == 0:
            h = flat[j * nx + i]
        else:
            i = np.where(i < f.nx - 1, i, f.nx - 2); j = np.where(j < f.ny - 1, j, f.ny - 2)
            tx = cx - i.astype(np.float64); ty = cy - j.astype(np.float64)
            h00, h10, h01, h11 = flat[j * nx + i], flat[j * nx + i + 1], flat[(j + 1) * nx + i], flat[(j + 1) * nx + i + 1]
            a = h00 + tx * (h10 - h00)
            b = h01 + tx * (h11 - h01)
            h = a + ty * (b - a)
        top = np.where(valid, h, np.nan)
        if origin is not None:
            top = top + oz
        return top


def step(params, state, R, foot, grf, contacts, Rz=None, target=None, field=None, origin=None, ext=None, dt=0.0025, substeps=1, gravity=PR.GRAVITY, swing_track=1.0):
    """ground_ref.step's arguments with (field, origin) where ground is -> (state (n, 12), R (n, 9), foot (n, 12), foot_vel_body (n, 12), touch (n, 4) uint8,
    ground_out (n, 3))"""
    with np.errstate(all="ignore"):
        # the sub-steps are the walk step's; the field comes after the last of them, so the walk step WITHOUT a ground gives pos', R' and r' of the rule
        so, Ro, fo, vo = WR.step(params, state, R, foot, grf, contacts, Rz, target, ext, dt, substeps, gravity, swing_track, 0, 0.0)
        n = Ro.shape[0]
        ct = np.asarray(contacts).reshape(n, 4) != 0
        fo = fo.copy()
        touch = ct.copy()
        for l in range(4):
            X = so[:, 3] + fo[:, 3 * l]; Y = so[:, 4] + fo[:, 3 * l + 1]
            gz = sample(field, X, Y, origin) - so[:, 5]
            rz = fo[:, 3 * l + 2]
            lifted = rz < gz
            fo[:, 3 * l + 2] = np.where(ct[:, l], gz, np.where(lifted, gz, rz))
            touch[:, l] = ct[:, l] | lifted
        ground_out = np.zeros((n, 3))
        ground_out[:, 0] = sample(field, so[:, 3], so[:, 4], origin)
        return so, Ro, fo, vo, touch.astype(np.uint8), ground_out


def same_heights(a, b):
    """bit for bit, with every NaN equal to every NaN (the payload of a NaN + oz is the adder's business)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))
