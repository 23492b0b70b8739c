"""Respawn on the CPU: the product's kernel text compiled for the host (tests/emu/respawn_host.py: 64 host threads in lock step are one wavefront) against the numpy
restatement of tests/respawn_ref.py, bit for bit -- both kernels only copy, compare and count, so there is no bar anywhere in this file.  The masked reset on images
of all four state blocks (exactly the restatement's bytes become zero, every other byte keeps its bits), the decision with its hold, the rows with canaries."""
import numpy as np
import pytest

import respawn_host as host
import respawn_ref as RR

SIZES = (1, 63, 64, 65, 130)
GEOMS = [dict(max_batch=70, horizon=10, window=w) for w in (1, 5, 64)] + [dict(max_batch=70, horizon=1, window=5)]
POISON = 0x7FF8DEADBEEF0001
_SHARED = {}


def _geom(g, n):
    """max_batch = 70 != n where the batch fits; the two sizes beyond it get 140: every stride still differs from n"""
    return dict(g, max_batch=g["max_batch"] if n <= g["max_batch"] else 2 * g["max_batch"])


def _images(geom):
    key = tuple(sorted(geom.items()))
    if key not in _SHARED:
        im = RR.pattern_images(geom, seed=8100 + geom["window"] + geom["horizon"])
        for v in im.values():
            v.setflags(write=False)
        _SHARED[key] = im
    return _SHARED[key]


def _same(a, b):
    return a.keys() == b.keys() and all(RR.bits_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("kind", RR.MASKS)
@pytest.mark.parametrize("n", SIZES)
def test_masked_reset_on_the_host_zeroes_the_restatements_bytes_and_no_others(n, kind):
    """every geometry (IMU windows 1, 5, 64 at horizon 10; horizon 1, which has no carry), all four blocks together: the images after the kernel text are the
    restatement's -- the masked robots' bytes zero, every other byte, rows >= n included, unchanged"""
    mask = np.concatenate([RR.make_mask(kind, n), np.ones(5, dtype=np.uint8)])   # (rows beyond n are masked too: nobody may look at them)
    for g in GEOMS:
        geom = _geom(g, n)
        im = _images(geom)
        assert ("carry" in im) == (geom["horizon"] > 1)
        out = host.reset(im, mask, RR.ALL, geom, n=n)
        ref = RR.reset(im, mask, RR.ALL, geom, n=n)
        assert _same(out, ref), [k for k in out if not RR.bits_equal(out[k], ref[k])]
        zeroed = sum(int((out[k] == 0).sum()) for k in out)
        assert zeroed == int((mask[:n] & 1).sum()) * sum(len(RR.robot_bytes(k, 0, geom)) for k in im)   # (the pattern has no zero byte of its own)


@pytest.mark.parametrize("what", [RR.EKF, RR.CONTACT, RR.SENSOR, RR.WARM, RR.EKF | RR.WARM, 0])
def test_each_block_alone(what):
    """every single bit: its blocks and no others; a block that is not allocated is skipped, and so is its partner (the IMU windows without their cursors)"""
    n, geom = 65, GEOMS[1]
    im = _images(geom)
    mask = RR.make_mask("half", n)
    out = host.reset(im, mask, what, geom)
    assert _same(out, RR.reset(im, mask, what, geom))
    touched = {k for k in im if not RR.bits_equal(out[k], im[k])}
    assert touched == {k for bit, blocks in RR.BLOCKS_OF.items() if what & bit for k in blocks}
    for missing in (("ekf",), ("contact",), ("sensor_cursor",), ("carry",), ("ekf", "contact", "sensor_filt", "sensor_cursor", "carry")):
        less = {k: v for k, v in im.items() if k not in missing}
        got = host.reset(less, mask, RR.ALL, geom)
        assert _same(got, RR.reset(less, mask, RR.ALL, geom)), missing
        assert "sensor_filt" not in less or "sensor_cursor" in less or RR.bits_equal(got["sensor_filt"], im["sensor_filt"])


def test_bit_zero_of_a_given_mask_selects():
    n, geom = 10, GEOMS[1]
    im = _images(geom)
    mask = np.array([0, 1, 2, 3, 254, 255, 0, 0, 1, 0], dtype=np.uint8)
    out = host.reset(im, mask, RR.ALL, geom)
    assert _same(out, RR.reset(im, mask, RR.ALL, geom))
    hit = [b for b in range(n) if not out["ekf"][RR.robot_bytes("ekf", b, geom)].any()]
    assert hit == [1, 3, 5, 8]


@pytest.mark.parametrize("with_finished", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_decision_on_the_host_is_the_restatement(n, with_finished):
    """every end code, -0, a code of 4 and a NaN code, NaN payloads, a NaN clock, ticks at max_ticks - 1 / max_ticks, hold 0 / 1 / 7, finished_out given and NULL;
    several configurations; every output bit for bit, three poisoned rows behind n untouched, and the state of exactly the respawned robots cleared"""
    geom = _geom(GEOMS[1], n)
    im = _images(geom)
    ep, life = RR.decision_cases(n + 3, seed=8200 + n)
    fin = np.zeros((n + 3, RR.WORDS)); fin.view(np.uint64)[:] = POISON
    for cfg in (RR.DEFAULT, dict(RR.DEFAULT, max_ticks=50), dict(codes=0x4, max_ticks=50, hold_ticks=0, what=RR.EKF | RR.SENSOR), dict(codes=0, max_ticks=0, hold_ticks=3, what=RR.ALL),
                dict(codes=0xA, max_ticks=2 ** 53 - 1, hold_ticks=2 ** 31 - 1, what=0)):
        f_in = fin if with_finished else None
        e, l, f, m, out = host.decide(ep, life, cfg, f_in, n=n, images=im, geom=geom)
        re, rl, rf, rm = RR.decide(ep[:n], life[:n], cfg, None if f_in is None else f_in[:n])
        assert RR.bits_equal(e[:n], re) and RR.bits_equal(l[:n], rl) and RR.bits_equal(m[:n], rm), cfg
        assert RR.bits_equal(e[n:], ep[n:]) and RR.bits_equal(l[n:], life[n:]) and (m[n:] == 0xEE).all()
        if with_finished:
            assert RR.bits_equal(f[:n], rf) and RR.bits_equal(f[n:], fin[n:])
        else:
            assert f is None
        assert _same(out, RR.reset(im, (rm == 1).astype(np.uint8), cfg["what"], geom)), cfg
        held = life[:n, 0] > 0
        assert (rm[held] == 2).all() and not e[:n][rm != 0].view(np.uint64).any() and RR.bits_equal(e[:n][rm == 0], ep[:n][rm == 0])
        if cfg is RR.DEFAULT:
            assert set(rm) == {0, 1, 2} or n == 1


def test_the_hold_counts_down_and_a_held_record_ends_nothing():
    """a robot that ended by tilt: respawned, held hold_ticks ticks whatever its record says in between (NaNs, another end code), free afterwards; the clock of the
    time limit restarts; episodes_done counts"""
    cfg = dict(RR.DEFAULT, hold_ticks=3, max_ticks=4)
    ep = np.zeros((2, RR.WORDS)); life = np.zeros((2, 2), dtype=np.int32)
    ep[0, :3] = (9, 31, 2); ep[1, 0] = 3
    fin = np.full((2, RR.WORDS), -1.0)
    seen = []
    for t in range(12):
        e, l, f, m = host.decide(ep, life, cfg, fin)
        re, rl, rf, rm = RR.decide(ep, life, cfg, fin)
        assert RR.bits_equal(e, re) and RR.bits_equal(l, rl) and RR.bits_equal(f, rf) and RR.bits_equal(m, rm)
        seen.append(tuple(m))
        ep, life, fin = e, l, f
        if life[0, 0] > 0:                       # (what a step and the episode update make of a robot that is held on the next tick)
            ep[0, 3:] = np.nan; ep[0, 2] = 1.0
        free = m == 0
        ep[free, 0] += 1.0                       # (the episode update of a free robot)
    assert [s[0] for s in seen] == [1, 2, 2, 2, 0, 0, 0, 0, 1, 2, 2, 2]
    assert [s[1] for s in seen] == [0, 1, 2, 2, 2, 0, 0, 0, 0, 1, 2, 2]
    assert list(life[:, 1]) == [2, 2] and fin[0, 0] == 4 and fin[0, 2] == 0 and fin[1, 0] == 4


ROW_BYTES = (1, 4, 8, 96, 4096, 13)


@pytest.mark.parametrize("when", [1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_rows_on_the_host_are_the_restatement(n, when):
    """rows of 1, 4, 8, 96, 4096 and 13 bytes, the last two tables on pointers that are no multiple of 8 (a 96-byte row there too: the byte path on a wide size);
    broadcast and per-robot sources; canaries in front of and behind every dst, and behind row n - 1 inside it"""
    rng = np.random.default_rng(8300 + n)
    mask = rng.integers(0, 4, size=n + 2, dtype=np.uint8)   # (3 selects nothing; two rows beyond n)
    table, keep, want = [], [], []
    for k, (rb, off) in enumerate([(rb, 0) for rb in ROW_BYTES] + [(96, 3), (13, 5), (8, 4)]):
        for per_robot in (False, True):
            store = np.full(64 + (n + 2) * rb + 64 + 8, 0xA5, dtype=np.uint8)
            dst = store[64 + off:64 + off + (n + 2) * rb].reshape(n + 2, rb)
            dst[:] = rng.integers(0, 256, size=dst.shape, dtype=np.uint8)
            src_store = rng.integers(0, 256, size=((n if per_robot else 1) * rb + 8), dtype=np.uint8)
            src = src_store[off:off + (n if per_robot else 1) * rb].reshape(-1, rb)
            assert dst.ctypes.data % 8 == (store.ctypes.data + off) % 8
            table.append((dst, src, when)); keep.append((store, store.copy(), off, rb))
    want = RR.rows(mask[:n], [(d.copy(), s, w) for d, s, w in table], n=n)
    for i in range(0, len(table), RR.ROWS_MAX):
        host.rows(mask, table[i:i + RR.ROWS_MAX], n=n)
    for (dst, src, _), ref, (store, before, off, rb) in zip(table, want, keep):
        assert RR.bits_equal(dst[:n], ref[:n]), (rb, off)
        assert RR.bits_equal(dst[n:], before[64 + off + n * rb:64 + off + (n + 2) * rb].reshape(2, rb))
        assert (store[:64 + off] == 0xA5).all() and (store[64 + off + (n + 2) * rb:] == 0xA5).all()
    sel = ((mask[:n] == 1) & bool(when & 1)) | ((mask[:n] == 2) & bool(when & 2))
    d0, s0, _ = table[1]
    assert RR.bits_equal(d0[:n][sel], s0[:n][sel]) and (n < 60 or sel.any())
