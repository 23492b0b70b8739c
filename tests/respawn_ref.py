"""The a1mpc_respawn_* family restated in numpy: the three rules of a1mpc_respawn_batch, the copy of a1mpc_respawn_rows_device, and which bytes of which state block of a
handle belong to robot b (the layouts are the ones the comments of csrc/a1mpc_hip.hip give for the whole-handle resets' blocks, not the kernel's table).  Copies,
comparisons and integer arithmetic only, so everything is compared bit for bit.  Shared by tests/test_respawn_host.py (the kernel text on the host),
tests/test_respawn_abi.py, tests/respawn_loop.py and tests/test_gpu_respawn.py (the device).  No function changes its arguments."""
import numpy as np

WORDS = 16
EKF, CONTACT, SENSOR, WARM = 1, 2, 4, 8
ALL = 15
DEFAULT = dict(codes=0xE, max_ticks=0, hold_ticks=10, what=ALL)
FIELDS = (("uint32_t", "codes"), ("uint64_t", "max_ticks"), ("int32_t", "hold_ticks"), ("uint32_t", "what"))
ROWS_FIELDS = (("void*", "dst"), ("const void*", "src"), ("int32_t", "row_bytes"), ("int32_t", "src_rows"), ("uint32_t", "when"))
ROWS_MAX = 16
EKF_STATE = 18 + 18 * 18 + 1            # x, P, the flag word (0 = new)
CT_RECORD, LEG_WINDOW, TERRAIN_WINDOW = 384, 60, 100
IMU_FILTERS = 6


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def decide(episode, life, cfg=DEFAULT, finished=None):
    """rules 1 - 3 on n records -> (episode, life, finished or None, mask): new arrays"""
    ep = np.array(episode, dtype=np.float64); lf = np.array(life, dtype=np.int32)
    fin = None if finished is None else np.array(finished, dtype=np.float64)
    n = ep.shape[0]
    mask = np.zeros(n, dtype=np.uint8)
    for b in range(n):
        if lf[b, 0] > 0:                                   # 1: held; the record is not consulted
            ep[b] = 0.0; lf[b, 0] -= 1; mask[b] = 2
            continue
        ticks, code = ep[b, 0], ep[b, 2]
        ended = any(code == float(c) and (cfg["codes"] >> c) & 1 for c in (1, 2, 3))
        timed = code == 0.0 and cfg["max_ticks"] > 0 and ticks >= float(cfg["max_ticks"])
        if ended or timed:                                  # 2: respawned
            if fin is not None:
                fin[b] = ep[b]
            ep[b] = 0.0; lf[b, 0] = cfg["hold_ticks"]; lf[b, 1] += 1; mask[b] = 1
    return ep, lf, fin, mask


def rows(mask, table, n=None):
    """table: [(dst, src, when)], dst with a row per robot, src with one row or a row per robot -> the new dst arrays"""
    mask = np.asarray(mask, dtype=np.uint8)
    n = mask.shape[0] if n is None else n
    out = []
    for dst, src, when in table:
        d = np.array(dst)
        for b in range(n):
            if (mask[b] == 1 and when & 1) or (mask[b] == 2 and when & 2):
                d[b] = src[0] if src.shape[0] == 1 else src[b]
        out.append(d)
    return out


def carry_stride(horizon):
    return 0 if horizon == 1 else 72 * horizon + 14      # c, D, E0, E1, g, Z0, Z1 (12 H each), the pattern words, one pad


def block_bytes(geom):
    """bytes of every state block of a handle: dict(max_batch, horizon, window)"""
    M, H, w = geom["max_batch"], geom["horizon"], geom["window"]
    size = dict(ekf=M * EKF_STATE * 8, contact=M * (CT_RECORD + (4 * LEG_WINDOW * 4 + TERRAIN_WINDOW) * 8), sensor_filt=IMU_FILTERS * (w + 2) * M * 8,
                sensor_cursor=2 * M * 4, wx=M * 12 * H * 8, wy=M * 20 * H * 8, rho=M * 8)
    if carry_stride(H):
        size["carry"] = M * carry_stride(H) * 8
    return size


BLOCKS_OF = {EKF: ("ekf",), CONTACT: ("contact",), SENSOR: ("sensor_filt", "sensor_cursor"), WARM: ("wx", "wy", "rho", "carry")}


def robot_bytes(block, b, geom):
    """the byte offsets inside `block` that are robot b's"""
    M, H, w = geom["max_batch"], geom["horizon"], geom["window"]
    span = lambda start, count: np.arange(start, start + count, dtype=np.int64)
    if block == "ekf":
        return span(b * EKF_STATE * 8, EKF_STATE * 8)                       # [robot][343]
    if block == "contact":                                                   # records [robot], leg rings [robot][4][60][4], terrain ring [100][max_batch]
        leg = 4 * LEG_WINDOW * 4 * 8
        parts = [span(b * CT_RECORD, CT_RECORD), span(M * CT_RECORD + b * leg, leg)]
        parts += [span(M * (CT_RECORD + leg) + (slot * M + b) * 8, 8) for slot in range(TERRAIN_WINDOW)]
        return np.concatenate(parts)
    if block == "sensor_filt":                                               # [filter][slot | sum | corr][max_batch]
        return np.concatenate([span((j * M + b) * 8, 8) for j in range(IMU_FILTERS * (w + 2))])
    if block == "sensor_cursor":                                             # [count | cursor][max_batch] int32
        return np.concatenate([span((j * M + b) * 4, 4) for j in range(2)])
    per = dict(wx=12 * H * 8, wy=20 * H * 8, rho=8, carry=carry_stride(H) * 8)[block]
    return span(b * per, per)


def reset(images, mask, what, geom, n=None):
    """images: dict block -> uint8 array (a missing block is one that is not allocated) -> the new images"""
    mask = np.asarray(mask, dtype=np.uint8)
    n = mask.shape[0] if n is None else n
    out = {k: np.array(v) for k, v in images.items()}
    for bit, blocks in BLOCKS_OF.items():
        if not what & bit:
            continue
        if bit == SENSOR and not ("sensor_filt" in out and "sensor_cursor" in out):   # (the IMU windows and their cursors are allocated, and reset, together)
            continue
        for block in blocks:
            if block not in out:
                continue
            for b in range(n):
                if mask[b] & 1:
                    out[block][robot_bytes(block, b, geom)] = 0
    return out


def pattern_images(geom, seed):
    """every block filled with bytes that are never zero"""
    rng = np.random.default_rng(seed)
    return {k: rng.integers(1, 256, size=v, dtype=np.uint8) for k, v in block_bytes(geom).items()}


MASKS = ("none", "all", "first", "15, 16", "63, 64", "half")


def make_mask(kind, n, seed=0):
    m = np.zeros(n, dtype=np.uint8)
    if kind == "all": m[:] = 1
    elif kind == "first": m[0] = 1
    elif kind == "15, 16": m[[i for i in (15, 16) if i < n]] = 1
    elif kind == "63, 64": m[[i for i in (63, 64) if i < n]] = 1
    elif kind == "half": m[np.random.default_rng(7700 + n + seed).random(n) < 0.5] = 1
    else: assert kind == "none"
    return m


def decision_cases(n, seed, max_ticks=50):
    """records with every end code, -0, NaN payloads, ticks either side of max_ticks, holds 0 / 1 / 7 -> (episode, life)"""
    rng = np.random.default_rng(seed)
    ep = rng.normal(size=(n, WORDS))
    ep[:, 0] = rng.choice([0.0, 3.0, max_ticks - 1.0, float(max_ticks), max_ticks + 5.0], size=n)
    ep[:, 2] = rng.choice([0.0, -0.0, 1.0, 2.0, 3.0, 4.0, np.nan], size=n)
    ep[:, 1] = np.where(ep[:, 2] != 0, 17.0, 0.0)
    pay = rng.random(n) < 0.3
    ep.view(np.uint64)[pay, 7] = 0x7FF8DEADBEEF0001
    nan_clock = rng.random(n) < 0.1
    ep[nan_clock, 0] = np.nan
    life = np.stack([rng.choice([0, 0, 1, 7], size=n), rng.integers(0, 5, size=n)], axis=1).astype(np.int32)
    return ep, life
