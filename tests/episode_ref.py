"""a1mpc_episode_update_batch and a1mpc_episode_summary_batch restated in numpy, elementwise, in the header's operation order: IEEE + - * and comparisons only, so every
word is compared bit for bit.  Shared by tests/test_episode_host.py (the kernel text on the host), tests/test_episode_abi.py and tests/test_gpu_episode.py (the device).

update(episode, tick, state, R, ...) returns the new records and never changes its arguments; summary(episode) returns the 20 words.  The sum of a column is the balanced
tree of the header: the column padded to the next power of two with +0, then `while len(x) > 1: x = x[0::2] + x[1::2]`."""
import numpy as np

WORDS, SUMMARY = 16, 20
FIELDS = ("ticks", "end_tick_p1", "end_code", "vel_err_sum", "height_err_sum", "tilt_max", "est_pos_err_sum", "est_vel_err_sum", "est_vel_err_max", "effort_sum", "fz_max",
          "solver_bad", "reach_bad", "x0", "y0", "dist2")
W = {k: i for i, k in enumerate(FIELDS)}
SUMMARY_FIELDS = ("n", "alive", "ended_nonfinite", "ended_tilt", "ended_height", "first_end_tick", "ticks", "vel_err_sum", "height_err_sum", "tilt_max", "tilt_max_row",
                  "est_pos_err_sum", "est_vel_err_sum", "est_vel_err_max", "effort_sum", "fz_max", "solver_bad", "reach_bad", "dist2_sum", "dist2_max")
S = {k: i for i, k in enumerate(SUMMARY_FIELDS)}
OPTIONAL = ("estimate", "root_lin_vel_d", "root_pos_d_z", "ground", "forces", "status", "reach")   # the inputs that may be NULL (two of them pairs)
WORDS_OF = dict(estimate=(6, 7, 8), root_lin_vel_d=(3,), root_pos_d_z=(4,), forces=(9, 10), status=(11,), reach=(12,), ground=())   # the words each one feeds alone
DEFAULT = dict(min_up=0.5, min_height=0.12)
TICK_END = 2 ** 53 - 1


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def update(episode, tick, state, R, root_pos=None, root_lin_vel=None, root_lin_vel_d=None, root_pos_d_z=None, ground=None, grf_body=None, contacts=None, status=None,
           reach=None, cfg=DEFAULT):
    """one update of the n records, robot by robot -> the new (n, 16) array"""
    ep = np.array(episode, dtype=np.float64)
    n = ep.shape[0]
    assert 0 <= tick < TICK_END and (root_pos is None) == (root_lin_vel is None) and (grf_body is None) == (contacts is None)
    state, R = np.asarray(state, dtype=np.float64), np.asarray(R, dtype=np.float64).reshape(n, 9)
    fin = np.isfinite
    with np.errstate(all="ignore"):
        for b in range(n):
            w = ep[b]
            if w[2] != 0.0:   # 1: frozen (a NaN is not 0)
                continue
            pos, v, Rb = state[b, 3:6], state[b, 9:12], R[b]
            ok = fin(pos).all() and fin(v).all() and fin(Rb).all()   # 2
            if root_pos is not None:
                ok = ok and fin(root_pos[b]).all() and fin(root_lin_vel[b]).all()
            if root_lin_vel_d is not None:
                ok = ok and fin(root_lin_vel_d[b][:2]).all()
            if root_pos_d_z is not None:
                ok = ok and fin(root_pos_d_z[b])
            if ground is not None:
                ok = ok and fin(ground[b]).all()
            if grf_body is not None:
                for l in range(4):
                    if contacts[b][l] != 0:
                        ok = ok and fin(grf_body[b][3 * l:3 * l + 3]).all()
            hz = np.float64(0.0) if ground is None else (ground[b][0] + ground[b][1] * pos[0]) + ground[b][2] * pos[1]
            height = pos[2] - hz
            code = 1 if not ok else (2 if Rb[8] < cfg["min_up"] else (3 if height < cfg["min_height"] else 0))
            if code:
                w[1], w[2] = float(tick + 1), float(code)
                continue
            first = w[0] == 0.0   # 5
            w[0] = w[0] + 1.0
            if root_lin_vel_d is not None:
                ex = ((Rb[0] * v[0] + Rb[3] * v[1]) + Rb[6] * v[2]) - root_lin_vel_d[b][0]
                ey = ((Rb[1] * v[0] + Rb[4] * v[1]) + Rb[7] * v[2]) - root_lin_vel_d[b][1]
                w[3] = w[3] + (ex * ex + ey * ey)
            if root_pos_d_z is not None:
                ez = height - root_pos_d_z[b]
                w[4] = w[4] + ez * ez
            t = 1.0 - Rb[8]
            w[5] = t if t > w[5] else w[5]
            if root_pos is not None:
                d, u = root_pos[b] - pos, root_lin_vel[b] - v
                tp, tv = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]
                w[6] = w[6] + tp; w[7] = w[7] + tv
                w[8] = tv if tv > w[8] else w[8]
            if grf_body is not None:
                s = []
                for l in range(4):
                    f = grf_body[b][3 * l:3 * l + 3]
                    stance = contacts[b][l] != 0
                    s.append((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2] if stance else np.float64(0.0))
                    if stance:
                        w[10] = f[2] if f[2] > w[10] else w[10]
                w[9] = w[9] + ((s[0] + s[1]) + (s[2] + s[3]))
            if status is not None and status[b] != 1:
                w[11] = w[11] + 1.0
            if reach is not None:
                w[12] = w[12] + float(sum(1 for l in range(4) if reach[b][l] != 0))
            if first:
                w[13], w[14] = pos[0], pos[1]
            dx, dy = pos[0] - w[13], pos[1] - w[14]
            w[15] = dx * dx + dy * dy
    return ep


def tree_sum(x):
    x = np.asarray(x, dtype=np.float64)
    p = 1
    while p < len(x):
        p *= 2
    x = np.concatenate([x, np.zeros(p - len(x))])
    while len(x) > 1:
        x = x[0::2] + x[1::2]
    return x[0]


def summary(episode):
    ep = np.asarray(episode, dtype=np.float64)
    n = ep.shape[0]
    assert n >= 1
    code = ep[:, 2]
    ended = code != 0.0
    out = np.zeros(SUMMARY)
    out[0] = n
    for c in range(4):
        out[1 + c] = float((code == c).sum())
    out[5] = (ep[ended, 1].min() - 1.0) if ended.any() else -1.0
    for word, col in ((6, 0), (7, 3), (8, 4), (11, 6), (12, 7), (14, 9), (16, 11), (17, 12), (18, 15)):
        out[word] = tree_sum(ep[:, col])
    out[9] = ep[:, 5].max(); out[10] = float(np.argmax(ep[:, 5] == out[9]))   # (argmax of booleans: the first True, the LOWEST row)
    out[13] = ep[:, 8].max(); out[15] = ep[:, 10].max(); out[19] = ep[:, 15].max()
    return out


def random_inputs(n, seed=9100, stride=12, ticks=1):
    """`ticks` consecutive sets of finite inputs for n robots, near an upright walking robot (every robot stays alive under DEFAULT), each array read-only: computed by the
    caller once, never changed.  -> list of dicts with the keyword names of update()"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(ticks):
        state = rng.normal(0, 0.3, (n, stride)); state[:, 5] = rng.uniform(0.2, 0.4, n)
        a = rng.normal(0, 0.15, (n, 3))   # a rotation of some tenths of a radian, by Rodrigues
        th = np.sqrt((a * a).sum(1)); k = a / th[:, None]
        K = np.zeros((n, 3, 3)); K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
        R = np.eye(3)[None] + np.sin(th)[:, None, None] * K + (1 - np.cos(th))[:, None, None] * (K @ K)
        ct = (rng.uniform(0, 1, (n, 4)) > 0.4).astype(np.uint8)
        d = dict(state=state, R=R.reshape(n, 9), root_pos=state[:, 3:6] + rng.normal(0, 0.01, (n, 3)), root_lin_vel=state[:, 9:12] + rng.normal(0, 0.05, (n, 3)),
                 root_lin_vel_d=rng.normal(0, 0.3, (n, 3)), root_pos_d_z=rng.uniform(0.25, 0.35, n), ground=rng.normal(0, 0.02, (n, 3)),
                 grf_body=rng.normal(0, 30, (n, 12)), contacts=ct, status=rng.choice(np.array([1, 1, 1, 2, -3], dtype=np.int32), n),
                 reach=(rng.uniform(0, 1, (n, 4)) > 0.8).astype(np.uint8) * rng.integers(1, 4, (n, 4)).astype(np.uint8))
        for v in d.values():
            v.setflags(write=False)
        out.append(d)
    return out


def without(inputs, key):
    """the inputs with one optional input (of OPTIONAL) NULL"""
    drop = dict(estimate=("root_pos", "root_lin_vel"), forces=("grf_body", "contacts")).get(key, (key,))
    return {k: (None if k in drop else v) for k, v in inputs.items()}


def random_records(n, seed=9200):
    """n plausible records, some of them ended, every summed word at least +0: what a summary is checked on"""
    rng = np.random.default_rng(seed)
    ep = np.abs(rng.normal(0, 3, (n, WORDS)))
    ep[:, 0] = rng.integers(0, 500, n); ep[:, 11] = rng.integers(0, 9, n); ep[:, 12] = rng.integers(0, 30, n)
    code = rng.choice([0, 0, 0, 1, 2, 3], n)
    ep[:, 2] = code; ep[:, 1] = np.where(code != 0, rng.integers(1, 470, n), 0)
    ep[:, 5] = rng.uniform(0, 0.5, n)
    return ep
