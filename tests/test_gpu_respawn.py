"""GPU: the respawn family -- a1mpc_respawn_batch(_device), a1mpc_respawn_reset_batch(_device), a1mpc_respawn_rows_device.  Yardsticks: the numpy restatement of
tests/respawn_ref.py bit for bit (the kernels copy, compare and count: there is no bar in this file), and for the masked reset the CONTRACT of the header: three
handles driven alike, one with the masked reset, one with nothing, one with the whole-handle resets -- from the reset on, a masked robot of the first is a robot of the
third and every other robot of the first is a robot of the second, in every output of the control tick, on every tick.  Then every refusal with poisoned arrays, and the
closed loop of tests/test_gpu_episode.py rebuilt with the two respawn stages."""
import ctypes as C

import numpy as np
import pytest

import episode_loop as EL
import episode_ref as ER
import noise_ref as NR
import respawn_ref as RR
import sensor_loop as SL
import walk_loop as WL
from gpu_common import FORCE_TICK, _engine, gait_cycle_fleet, stand_timetable, tick_buffers, tick_inputs_timetable, tick_world

pytestmark = pytest.mark.gpu
SIZES = [1, 17, 64, 65, 130]
POISON = 0x7FF8DEADBEEF0001
OK, INVALID, TOO_LARGE = 0, 1, 5
_SHARED = {}


def _dev():
    import torch
    return torch.device("cuda:0")


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(_dev())


@pytest.fixture(scope="module")
def eng(pkg, scen):
    e = _engine(pkg, scen.scenario_stand(), 4224, warm_start=0)
    yield e
    e.close()
    _SHARED.clear()


# ---- a. the decision
@pytest.mark.parametrize("n", SIZES)
def test_decision_entries_equal_the_restatement(eng, n):
    """the cases of the CPU test (every end code, -0, NaN payloads and clocks, ticks either side of max_ticks, holds 0 / 1 / 7) through the device entry and the host
    entry, finished_out given and NULL, several configurations: every output bit for bit, and the three rows behind n keep their bits"""
    import torch
    ep, life = RR.decision_cases(n + 3, seed=8200 + n)
    fin = np.zeros((n + 3, RR.WORDS)); fin.view(np.uint64)[:] = POISON
    for cfg in (RR.DEFAULT, dict(RR.DEFAULT, max_ticks=50), dict(codes=0x4, max_ticks=50, hold_ticks=0, what=RR.EKF | RR.SENSOR), dict(codes=0, max_ticks=0, hold_ticks=3, what=RR.ALL),
                dict(codes=0xA, max_ticks=2 ** 53 - 1, hold_ticks=2 ** 31 - 1, what=0)):
        rc = eng.respawn_config(**cfg)
        for with_finished in (True, False):
            re, rl, rf, rm = RR.decide(ep[:n], life[:n], cfg, fin[:n] if with_finished else None)
            e, l, f, m = _t(ep), _t(life), _t(fin), torch.full((n + 3,), 0xEE, dtype=torch.uint8, device=_dev())
            torch.cuda.synchronize()
            eng.respawn_device(n, e, l, m, d_finished=f if with_finished else None, config=rc)
            torch.cuda.synchronize()
            e, l, f, m = e.cpu().numpy(), l.cpu().numpy(), f.cpu().numpy(), m.cpu().numpy()
            assert RR.bits_equal(e[:n], re) and RR.bits_equal(l[:n], rl) and RR.bits_equal(m[:n], rm), (cfg, with_finished)
            assert RR.bits_equal(e[n:], ep[n:]) and RR.bits_equal(l[n:], life[n:]) and (m[n:] == 0xEE).all() and RR.bits_equal(f[n:], fin[n:])
            assert RR.bits_equal(f[:n], rf if with_finished else fin[:n])
            he, hl, hf = np.array(ep[:n]), np.array(life[:n]), np.array(fin[:n])
            hm = eng.respawn(he, hl, hf if with_finished else None, config=rc)
            assert RR.bits_equal(he, re) and RR.bits_equal(hl, rl) and RR.bits_equal(hm, rm) and RR.bits_equal(hf, rf if with_finished else fin[:n])


# ---- b. the contract of the masked reset
B_MAX, B_N, B_WINDOW, B_BEFORE, B_AFTER = 70, 65, 5, 101, 30
FRONT = (("R_world", 9), ("R_z", 9), ("root_euler", 3), ("imu_acc", 3), ("imu_ang_vel", 3), ("root_ang_vel", 3))
RAW = ("joint_pos", "joint_vel", "foot_force", "movement_mode", "mpc_active", "root_lin_vel_d", "root_ang_vel_d", "root_pos_d_z", "gait_counter_speed", "torques_gravity")


def _quat(eul):
    r, p, y = eul[:, 0] / 2, eul[:, 1] / 2, eul[:, 2] / 2
    q = np.stack([np.cos(r) * np.cos(p) * np.cos(y) + np.sin(r) * np.sin(p) * np.sin(y), np.sin(r) * np.cos(p) * np.cos(y) - np.cos(r) * np.sin(p) * np.sin(y),
                  np.cos(r) * np.sin(p) * np.cos(y) + np.sin(r) * np.cos(p) * np.sin(y), np.cos(r) * np.cos(p) * np.sin(y) - np.sin(r) * np.sin(p) * np.cos(y)], 1)
    return q


def _script(scen):
    """131 ticks of control-tick inputs for 65 robots on the device, computed once: the staggered gait fleet and the stand timetable of the gait-cycle tests, foot forces
    on the thresholds (early contacts part the robots' leg cursors for good), a quaternion and a raw IMU sample per tick for the sensor stage"""
    if "script" not in _SHARED:
        rng = np.random.default_rng(8400)
        gc, spd = gait_cycle_fleet(B_N)
        mm = stand_timetable(B_N, B_BEFORE + B_AFTER)
        ticks = []
        for t in range(B_BEFORE + B_AFTER):
            raw = tick_inputs_timetable(scen, rng, B_N, mm[t], spd, FORCE_TICK)
            d = {k: _t(raw[k]) for k in RAW}
            d.update(quat=_t(_quat(raw["root_euler"])), imu_acc_raw=_t(raw["imu_acc"]), imu_gyro_raw=_t(raw["imu_ang_vel"]))
            ticks.append(d)
        early = (np.array([np.asarray(tk["foot_force"].cpu()) for tk in ticks]) > 30.0).any()
        assert early and (mm == 0).any() and (mm == 1).all(1).any()
        _SHARED["script"] = (gc, ticks)
    return _SHARED["script"]


class _Driven:
    """one handle of 70 with the world of its 65 robots: a tick is a1mpc_sensor_frontend_batch_device (the IMU windows) and a1mpc_control_tick_device (the EKF, the
    contact and terrain filters, the warm start) on the handle's stream"""

    def __init__(self, pkg, scen, warm_start):
        import torch
        self.E = pkg.engine
        self.eng = _engine(pkg, scen.scenario_stand(), B_MAX, warm_start=warm_start)
        self.prm = self.E.TickParams(); self.eng.lib.a1mpc_default_tick_params(C.byref(self.prm))
        gc, self.ticks = _script(scen)
        self.w = tick_world(B_N, _dev(), gc)
        self.front = {k: torch.zeros((B_N, m), dtype=torch.float64, device=_dev()) for k, m in FRONT}
        self.sc = self.eng.sensor_config(imu_window=B_WINDOW)
        torch.cuda.synchronize()   # (the arrays above are filled on torch's stream, the ticks run on the handle's)

    def tick(self, t):
        d, f = self.ticks[t], self.front
        self.eng.sensor_frontend_device(B_N, d["quat"], d["imu_acc_raw"], d["imu_gyro_raw"], *[f[k] for k, _ in FRONT], cfg=self.sc)
        self.eng.control_tick_device(self.prm, tick_buffers(self.E, {**{k: d[k] for k in RAW}, **f}, self.w), B_N)

    def outputs(self):
        """every output array of the tick, as bytes per robot"""
        import torch
        torch.cuda.synchronize()
        arrs = {k: v for g in ("state", "outs", "u8", "i32") for k, v in self.w[g].items()}
        arrs.update(self.front)
        return {k: v.cpu().numpy().reshape(B_N, -1) for k, v in arrs.items()}

    def whole_resets(self, what=RR.ALL):
        L, h = self.eng.lib, self.eng._h
        for bit, f in ((RR.EKF, L.a1mpc_reset_ekf_state), (RR.CONTACT, L.a1mpc_reset_contact_state), (RR.SENSOR, L.a1mpc_reset_sensor_state), (RR.WARM, L.a1mpc_reset_warm_start)):
            if what & bit:
                assert f(h) == 0

    def close(self):
        self.eng.close()


def _rows_equal(a, b, rows):
    return [k for k in a if not RR.bits_equal(a[k][rows], b[k][rows])]


@pytest.mark.parametrize("warm_start", [1, 2])
@pytest.mark.parametrize("kind", RR.MASKS)
def test_a_masked_robot_is_a_robot_of_a_reset_handle_and_the_others_saw_nothing(pkg, scen, kind, warm_start):
    """101 ticks (the terrain window of 100, the leg windows of 60 and the IMU window of 5 have wrapped), then A: the masked reset on the device, B: nothing, C: the
    four whole-handle resets; 30 more ticks, on each of them every output array bit-equal -- the masked rows of A to C's, the other rows of A to B's"""
    import torch
    mask = RR.make_mask(kind, B_N)
    on, off = np.flatnonzero(mask), np.flatnonzero(mask == 0)
    hs = [_Driven(pkg, scen, warm_start) for _ in range(3)]
    try:
        A, B, Cc = hs
        for t in range(B_BEFORE):
            for h in hs:
                h.tick(t)
        a, b = A.outputs(), B.outputs()
        assert _rows_equal(a, b, slice(None)) == []   # (the three runs are reproducible)
        d_mask = torch.cat([_t(mask), torch.ones(B_MAX - B_N, dtype=torch.uint8, device=_dev())])   # (the handle's rows beyond n: masked, and nobody's)
        torch.cuda.synchronize()
        A.eng.respawn_reset_device(B_N, d_mask)
        Cc.whole_resets()
        differs = set()
        for t in range(B_BEFORE, B_BEFORE + B_AFTER):
            for h in hs:
                h.tick(t)
            a, b, c = A.outputs(), B.outputs(), Cc.outputs()
            assert _rows_equal(a, c, on) == [], (t, _rows_equal(a, c, on))
            assert _rows_equal(a, b, off) == [], (t, _rows_equal(a, b, off))
            differs |= set(_rows_equal(b, c, slice(None)))
        # the comparison can fail: a reset handle does give other bits than one that saw nothing, in the estimate, the contacts' filters, the IMU and the forces
        assert {"root_pos", "root_lin_vel", "foot_pos_recent_contact", "imu_acc", "grf"} <= differs, differs
    finally:
        for h in hs:
            h.close()


def test_each_block_alone_is_its_whole_handle_reset(pkg, scen):
    """for each single bit of `what`: the masked rows of a handle that got the masked reset of that block alone (through the HOST entry) equal those of a handle on which
    only that one whole-handle reset was called, its other rows those of a handle that saw nothing; warm_start 2 (the carry is allocated)"""
    mask = RR.make_mask("half", B_N)
    on, off = np.flatnonzero(mask), np.flatnonzero(mask == 0)
    bits = (RR.EKF, RR.CONTACT, RR.SENSOR, RR.WARM)
    hs = [_Driven(pkg, scen, 2) for _ in range(1 + 2 * len(bits))]
    try:
        for t in range(B_BEFORE):
            for h in hs:
                h.tick(t)
        for i, bit in enumerate(bits):
            hs[1 + 2 * i].eng.respawn_reset(mask, what=bit)
            hs[2 + 2 * i].whole_resets(bit)
        moved = {bit: set() for bit in bits}
        for t in range(B_BEFORE, B_BEFORE + B_AFTER):
            for h in hs:
                h.tick(t)
            b = hs[0].outputs()
            for i, bit in enumerate(bits):
                a, c = hs[1 + 2 * i].outputs(), hs[2 + 2 * i].outputs()
                assert _rows_equal(a, c, on) == [] and _rows_equal(a, b, off) == [], (t, bit)
                moved[bit] |= set(_rows_equal(a, b, on))
        assert all(moved[bit] for bit in bits), moved   # (each block's reset does change some output of its robots)
    finally:
        for h in hs:
            h.close()


# ---- c. the rows
ROW_SHAPES = [(1, 0), (4, 0), (8, 0), (96, 0), (4096, 0), (13, 0), (96, 3), (13, 5), (8, 4)]   # (row_bytes, offset of both pointers from a multiple of 8)


@pytest.mark.parametrize("when", [1, 2, 3])
def test_rows_entry_equals_the_restatement(eng, when):
    """the CPU test's shapes at n = 65: rows of 1 .. 4096 bytes, pointers that are no multiple of 8, broadcast and per-robot sources, canaries around every dst and two
    rows behind n inside it"""
    import torch
    n = 65
    rng = np.random.default_rng(8300 + n)
    mask = rng.integers(0, 4, size=n + 2, dtype=np.uint8)
    table, host = [], []
    for rb, off in ROW_SHAPES:
        for per_robot in (False, True):
            store = np.full(64 + (n + 2) * rb + 64 + 8, 0xA5, dtype=np.uint8)
            store[64 + off:64 + off + (n + 2) * rb] = rng.integers(0, 256, size=(n + 2) * rb, dtype=np.uint8)
            src_store = rng.integers(0, 256, size=((n if per_robot else 1) * rb + 8), dtype=np.uint8)
            d_store, d_src = _t(store), _t(src_store)
            dst = d_store[64 + off:64 + off + (n + 2) * rb].reshape(n + 2, rb)
            src = d_src[off:off + (n if per_robot else 1) * rb].reshape(-1, rb)
            assert dst.data_ptr() % 8 == off % 8 and src.data_ptr() % 8 == off % 8
            table.append((dst, src, when)); host.append((store, src_store, off, rb, per_robot, d_store))
    d_mask = _t(mask)
    torch.cuda.synchronize()
    for i in range(0, len(table), RR.ROWS_MAX):
        eng.respawn_rows_device(n, d_mask, table[i:i + RR.ROWS_MAX])
    torch.cuda.synchronize()
    for store, src_store, off, rb, per_robot, d_store in host:
        want = np.array(store)
        dst = want[64 + off:64 + off + (n + 2) * rb].reshape(n + 2, rb)
        src = src_store[off:off + (n if per_robot else 1) * rb].reshape(-1, rb)
        dst[:n] = RR.rows(mask[:n], [(dst[:n], src, when)])[0]
        assert RR.bits_equal(d_store.cpu().numpy(), want), (rb, off, per_robot)
    eng.respawn_rows_device(n, d_mask, [])   # (an empty table is accepted and launches nothing)


# ---- d. the refusals
def test_refusals_leave_the_arrays_untouched(eng, pkg):
    """every refusal of the header from every entry: A1MPC_ERR_INVALID_ARGUMENT (1), the field named in a1mpc_last_error, before any launch; n > max_batch is
    A1MPC_ERR_BATCH_TOO_LARGE; n == 0 is OK and writes nothing; the same arguments, accepted, do write"""
    import torch
    L, engine = eng.lib, pkg.engine
    n = 16
    ep0, life0 = RR.decision_cases(n, seed=8500)
    ep0[:, 2] = 2.0; life0[:, 0] = 0   # (accepted, the default configuration respawns them all)
    big = eng.max_batch + 1
    mk = lambda rows: dict(episode=(_t(np.resize(ep0, (rows, 16))), np.resize(ep0, (rows, 16)).copy()), life=(_t(np.resize(life0, (rows, 2))), np.resize(life0, (rows, 2)).copy()),
                           finished=(torch.full((rows, 16), float("nan"), dtype=torch.float64, device=_dev()), np.full((rows, 16), np.nan)),
                           mask=(torch.full((rows,), 0xEE, dtype=torch.uint8, device=_dev()), np.full(rows, 0xEE, dtype=np.uint8)))
    arr, arr_big = mk(n), mk(big)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ct = {np.dtype("float64"): C.c_double, np.dtype("uint8"): C.c_uint8, np.dtype("int32"): C.c_int32}
    hp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(ct[a.dtype]))

    def decide(cfg=RR.DEFAULT, n_=n, h=eng._h, a=arr, **swap):
        rc = None if cfg is None else C.byref(engine.RespawnConfig(cfg["codes"], cfg["max_ticks"], cfg["hold_ticks"], cfg["what"]))
        x = dict(a)
        x.update(swap)
        dv, hs = {k: v[0] for k, v in x.items()}, {k: v[1] for k, v in x.items()}
        rd = L.a1mpc_respawn_batch_device(h, rc, n_, ptr(dv["episode"]), ptr(dv["life"]), ptr(dv["finished"]), ptr(dv["mask"]), None); md = L.a1mpc_last_error().decode()
        rh = L.a1mpc_respawn_batch(h, rc, n_, hp(hs["episode"]), hp(hs["life"]), hp(hs["finished"]), hp(hs["mask"])); mh = L.a1mpc_last_error().decode()
        return rd, md, rh, mh

    def reset(n_=n, h=eng._h, what=15, a=arr, **swap):
        x = dict(a)
        x.update(swap)
        rd = L.a1mpc_respawn_reset_batch_device(h, n_, ptr(x["mask"][0]), what, None); md = L.a1mpc_last_error().decode()
        rh = L.a1mpc_respawn_reset_batch(h, n_, hp(x["mask"][1]), what); mh = L.a1mpc_last_error().decode()
        return rd, md, rh, mh

    none = (None, None)
    bad = [(dict(h=None), "null handle"), (dict(h=None, cfg=None, n_=-1), "null handle"), (dict(cfg=None), "a1mpc_respawn_config"), (dict(episode=none), "episode"),
           (dict(life=none), "life"), (dict(mask=none), "mask_out"), (dict(n_=-1), "negative n"), (dict(cfg=dict(RR.DEFAULT, what=16)), "what"),
           (dict(cfg=dict(RR.DEFAULT, what=2 ** 31)), "what"), (dict(cfg=dict(RR.DEFAULT, codes=1)), "codes"), (dict(cfg=dict(RR.DEFAULT, codes=0x1E)), "codes"),
           (dict(cfg=dict(RR.DEFAULT, hold_ticks=-1)), "hold_ticks"), (dict(cfg=dict(RR.DEFAULT, max_ticks=2 ** 53)), "max_ticks"),
           (dict(cfg=dict(RR.DEFAULT, max_ticks=2 ** 64 - 1)), "max_ticks"), (dict(finished=arr["episode"]), "finished_out overlaps"),
           (dict(finished=(arr["episode"][0][n - 1:], arr["episode"][1][n - 1:])), "finished_out overlaps"),
           (dict(mask=(arr["episode"][0].view(torch.uint8).reshape(-1)[n * 128 - 1:], arr["episode"][1].view(np.uint8).reshape(-1)[n * 128 - 1:])), "mask_out overlaps")]
    for kw, word in bad:
        rd, md, rh, mh = decide(**kw)
        assert rd == INVALID and rh == INVALID and word in md and word in mh, (word, rd, md, rh, mh)
    for kw, word in [(dict(h=None), "null handle"), (dict(h=None, n_=-1, what=99), "null handle"), (dict(mask=none), "null mask"), (dict(n_=-1), "negative n"),
                     (dict(what=16), "what"), (dict(what=2 ** 32 - 1), "what")]:
        rd, md, rh, mh = reset(**kw)
        assert rd == INVALID and rh == INVALID and word in md and word in mh, (word, rd, md, rh, mh)
    # the rows
    dst, src = torch.full((n, 12), float("nan"), dtype=torch.float64, device=_dev()), torch.zeros((n, 12), dtype=torch.float64, device=_dev())
    d_mask = torch.ones(n, dtype=torch.uint8, device=_dev())
    Row = engine.RespawnRows
    good = dict(dst=dst.data_ptr(), src=src.data_ptr(), row_bytes=96, src_rows=n, when=3)

    def rows(n_=n, h=eng._h, m=d_mask, n_rows=1, table=True, **over):
        t = (Row * 17)(*[Row(**dict(good, **over)) for _ in range(17)])
        t[0] = Row(**good) if n_rows > 1 else t[0]   # (with two entries the bad one is the second)
        r = L.a1mpc_respawn_rows_device(h, n_, ptr(m), t if table else None, n_rows, None)
        return r, L.a1mpc_last_error().decode()

    for kw, word in [(dict(h=None), "null handle"), (dict(h=None, n_=-1, n_rows=40, table=False), "null handle"), (dict(m=None), "null mask"), (dict(table=False), "null rows"),
                     (dict(n_=-1), "negative n"), (dict(n_rows=-1), "n_rows"), (dict(n_rows=17), "n_rows"), (dict(dst=None), "dst"), (dict(src=None), "src"),
                     (dict(row_bytes=0), "row_bytes"), (dict(row_bytes=4097), "row_bytes"), (dict(row_bytes=-8), "row_bytes"), (dict(src_rows=0), "src_rows"),
                     (dict(src_rows=n - 1), "src_rows"), (dict(src_rows=2), "src_rows"), (dict(when=0), "when"), (dict(when=4), "when"), (dict(when=7), "when"),
                     (dict(src=dst.data_ptr()), "overlaps"), (dict(src=dst.data_ptr() + (n - 1) * 96 + 95, src_rows=1), "overlaps"),
                     (dict(src=dst.data_ptr() - 95, src_rows=1), "overlaps"), (dict(n_rows=2, when=0), "rows[1].when")]:
        r, msg = rows(**kw)
        assert r == INVALID and word in msg, (kw, word, r, msg)
    for f, kw in ((decide, dict(n_=big, a=arr_big)), (reset, dict(n_=big, a=arr_big))):
        rd, md, rh, mh = f(**kw)
        assert rd == TOO_LARGE and rh == TOO_LARGE and "max_batch" in md and "max_batch" in mh
    big_dst, big_src, big_mask = torch.full((big, 12), float("nan"), dtype=torch.float64, device=_dev()), torch.zeros((big, 12), dtype=torch.float64, device=_dev()), torch.ones(
        big, dtype=torch.uint8, device=_dev())
    r, msg = rows(n_=big, m=big_mask, dst=big_dst.data_ptr(), src=big_src.data_ptr(), src_rows=big)
    assert r == TOO_LARGE and "max_batch" in msg
    for f in (decide, reset):
        rd, md, rh, mh = f(n_=0)
        assert rd == OK and rh == OK, (md, mh)
    r, msg = rows(n_=0)
    assert r == OK, msg
    torch.cuda.synchronize()
    for a, rows_ in ((arr, n), (arr_big, big)):
        for k, want in (("episode", np.resize(ep0, (rows_, 16))), ("life", np.resize(life0, (rows_, 2)))):
            assert RR.bits_equal(a[k][0].cpu().numpy(), want) and RR.bits_equal(a[k][1], want), k
        assert torch.isnan(a["finished"][0]).all().item() and np.isnan(a["finished"][1]).all() and (a["mask"][0] == 0xEE).all().item() and (a["mask"][1] == 0xEE).all()
    assert torch.isnan(dst).all().item() and torch.isnan(big_dst).all().item()
    # the same arrays, accepted, are written
    rd, md, rh, mh = decide(cfg=dict(codes=0xE, max_ticks=2 ** 53 - 1, hold_ticks=0, what=0))
    assert rd == OK and rh == OK, (md, mh)
    r, msg = rows()
    assert r == OK, msg
    torch.cuda.synchronize()
    re, rl, rf, rm = RR.decide(ep0, life0, dict(codes=0xE, max_ticks=2 ** 53 - 1, hold_ticks=0, what=0), np.full((n, 16), np.nan))
    assert (rm == 1).all()
    for i in (0, 1):
        got = [arr[k][i].cpu().numpy() if i == 0 else arr[k][i] for k in ("episode", "life", "finished", "mask")]
        assert all(RR.bits_equal(g, w) for g, w in zip(got, (re, rl, rf, rm))), i
    assert (dst == 0).all().item()


# ---- e. the closed loop
def _respawn_trot(eng, pkg, scen, cfg, t0=0, pushed=True):
    """the pushed trot of tests/test_gpu_episode.py (_pushed_trot) with the two respawn stages behind the episode update, every stage on every tick: there is no `first`
    and no `t >= PRIME` -- every robot starts held for PRIME ticks (life[:, 0] = PRIME), a held robot's plant rows (state, R, feet, foot velocities, the applied forces
    and contacts) are put back behind its step, and the mode toggle is each robot's own, when its record's clock reaches STAND.  The push belongs to the episode it fells: the wrench
    reaches a robot only while its episodes_done is 0 (applied by the loop's tick alone it would fell the respawned robot again and again until the window closes: 150 N m
    for 60 ticks against a fall within 8 -- measured, three episodes end inside the window).  The loop's ticks are t0 .. T - 1; one copy at the end -> dict"""
    import torch
    E = pkg.engine
    sc = SL.perturbed_standing_robots(scen)
    n, dev = 17, _dev()
    L = eng.lib
    for reset in (L.a1mpc_reset_ekf_state, L.a1mpc_reset_contact_state, L.a1mpc_reset_sensor_state, L.a1mpc_reset_warm_start):
        assert reset(eng._h) == 0
    prm = E.TickParams(); L.a1mpc_default_tick_params(C.byref(prm))
    spawn = dict(state=_t(sc["state"]), R=_t(sc["R"]), foot=_t(sc["foot"]), grf=_t(sc["grf_eq"]), contacts=_t(sc["contact"]))
    state, R, foot = spawn["state"].clone(), spawn["R"].clone(), spawn["foot"].clone()
    w, w0 = tick_world(n, dev, WL.COUNTERS), tick_world(n, dev, WL.COUNTERS)
    w["outs"]["grf"].copy_(spawn["grf"]); w["u8"]["contacts"].copy_(spawn["contacts"])   # (what the first tick's sensors read: the equilibrium forces, all legs in stance)
    Z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)
    syn = dict(quat=Z(n, 4), imu_acc_raw=Z(n, 3), imu_gyro_raw=Z(n, 3), joint_pos=Z(n, 12), joint_vel=Z(n, 12), foot_force=Z(n, 4), reach=Z(n, 4, dt=torch.uint8))
    front = dict(R_world=Z(n, 9), R_z=Z(n, 9), root_euler=Z(n, 3), root_ang_vel=Z(n, 3), imu_acc=Z(n, 3), imu_ang_vel=Z(n, 3), root_lin_vel_d=Z(n, 3), root_ang_vel_d=Z(n, 3),
                 root_pos_d_z=Z(n), movement_mode=Z(n, dt=torch.uint8), mpc_active=Z(n, dt=torch.uint8))
    cs0 = {k: _t(v) for k, v in E.Engine.command_state(n).items() if k != "root_euler_d"}
    cs = {k: v.clone() for k, v in cs0.items()}
    inp = dict(joint_pos=syn["joint_pos"], joint_vel=syn["joint_vel"], foot_force=syn["foot_force"], gait_counter_speed=_t(np.full((n, 4), WL.COUNTER_SPEED)),
               torques_gravity=Z(n, 12), **front)
    stick = dict(cmd=Z(n, 6), mode_toggle=Z(n, dt=torch.uint8))
    walk_cmd = Z(n, 6); walk_cmd[:, 0] = WL.SPEED
    ts = eng.tick_sensors(sensor=eng.sensor_config(imu_window=SL.IMU_WINDOW), quat=syn["quat"], imu_acc_raw=syn["imu_acc_raw"], imu_gyro_raw=syn["imu_gyro_raw"], **stick, **cs)
    bf = tick_buffers(E, inp, w)
    fvb, bias = Z(n, 12), Z(n, 6)
    pushes = [_t(EL.wrench(n, EL.PUSH_FIRST - 1)), _t(EL.wrench(n, EL.PUSH_FIRST))]
    episode, summary, finished = Z(n, ER.WORDS), Z(ER.SUMMARY), Z(n, ER.WORDS)
    life = torch.zeros((n, 2), dtype=torch.int32, device=dev); life[:, 0] = WL.PRIME
    mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    plant_rows = [(state, spawn["state"], 3), (R, spawn["R"], 3), (foot, spawn["foot"], 3), (fvb, Z(1, 12), 3), (w["outs"]["grf"], spawn["grf"], 3),
                  (w["u8"]["contacts"], spawn["contacts"], 3)]
    carried_rows = [(w["state"][k], w0["state"][k], 1) for k in w["state"]] + [(cs[k], cs0[k], 1) for k in cs] + [(bias, Z(1, 6), 1)]
    assert len(plant_rows) + len(carried_rows) > RR.ROWS_MAX >= len(carried_rows)   # (two calls)
    nc = eng.noise_config(**NR.NOMINAL)
    ec = eng.episode_config()
    rc = eng.respawn_config(**cfg)
    wc = eng.walk_config(dt=SL.CONTROL_DT, swing_track=1.0, flat_ground=1, ground_z=0.0)
    T = WL.PRIME + WL.STAND + WL.WALK
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for t in range(t0, T):
        ext = pushes[0]
        if pushed and EL.PUSH_FIRST <= t < EL.PUSH_FIRST + EL.PUSH_TICKS:
            with torch.cuda.stream(stream):
                ext = pushes[1] * (life[:, 1] == 0).to(torch.float64)[:, None]
        with torch.cuda.stream(stream):   # each robot's own schedule, from its own episode clock: stand STAND ticks, toggle to walking, walk
            clock = episode[:, 0]
            stick["mode_toggle"].copy_((clock == float(WL.STAND)).to(torch.uint8)); stick["cmd"].copy_(walk_cmd * (clock >= float(WL.STAND)).to(torch.float64)[:, None])
        eng.walk_sensors_device(n, state, 12, R, foot, w["outs"]["grf"], w["u8"]["contacts"], syn["quat"], syn["imu_acc_raw"], syn["imu_gyro_raw"], syn["joint_pos"],
                                syn["joint_vel"], syn["foot_force"], syn["reach"], d_ext_wrench=ext, d_foot_vel_body=fvb, stream=stream.cuda_stream)
        eng.sensor_noise_device(nc, n, t, syn["quat"], syn["imu_acc_raw"], syn["imu_gyro_raw"], syn["joint_pos"], syn["joint_vel"], syn["foot_force"], bias,
                                stream=stream.cuda_stream)
        eng.control_tick_sensors_device(prm, ts, bf, n, stream=stream.cuda_stream)
        eng.walk_step_device(n, state, 12, R, foot, w["outs"]["grf"], w["u8"]["contacts"], front["R_z"], w["state"]["foot_pos_target_last_time"], fvb, d_ext_wrench=ext,
                             walk=wc, stream=stream.cuda_stream)
        eng.episode_update_device(n, t, episode, state, 12, R, d_root_pos=w["state"]["root_pos"], d_root_lin_vel=w["state"]["root_lin_vel"],
                                  d_root_lin_vel_d=front["root_lin_vel_d"], d_root_pos_d_z=front["root_pos_d_z"], d_grf_body=w["outs"]["grf"],
                                  d_contacts=w["u8"]["contacts"], d_status=w["i32"]["status"], d_reach=syn["reach"], config=ec, stream=stream.cuda_stream)
        eng.respawn_device(n, episode, life, mask, d_finished=finished, config=rc, stream=stream.cuda_stream)
        eng.respawn_rows_device(n, mask, plant_rows, stream=stream.cuda_stream)
        eng.respawn_rows_device(n, mask, carried_rows, stream=stream.cuda_stream)
    eng.episode_summary_device(n, episode, summary, stream=stream.cuda_stream)
    stream.synchronize()
    with torch.cuda.stream(stream):
        out = torch.cat([episode.reshape(-1), summary, finished.reshape(-1), life.to(torch.float64).reshape(-1), state.reshape(-1), R.reshape(-1), foot.reshape(-1)])
    out = out.cpu().numpy()   # the run's ONE copy
    for reset in (L.a1mpc_reset_ekf_state, L.a1mpc_reset_contact_state, L.a1mpc_reset_sensor_state, L.a1mpc_reset_warm_start):
        assert reset(eng._h) == 0
    sizes = dict(episode=(n, 16), summary=(20,), finished=(n, 16), life=(n, 2), state=(n, 12), R=(n, 9), foot=(n, 12))
    res, at = {}, 0
    for k, shape in sizes.items():
        res[k] = out[at:at + int(np.prod(shape))].reshape(shape); at += int(np.prod(shape))
    return res


def test_closed_loop_with_respawn(eng, pkg, scen):
    """Run 1, nobody respawns (codes 0, no time limit): the records and the summary are _pushed_trot's bit for bit -- the hold is the old priming.  Run 2, the default
    configuration: the pushed robot's first episode is in finished_out (ended by tilt or height inside the push window), it was held PRIME ticks and stood up again,
    alive at the end with a clean second record; the other 16 records are run 1's bit for bit.  Run 3, a fresh handle with every robot held from the tick after that
    respawn: robot 5 ends where it ends in run 2, bit for bit -- a respawned robot is a robot of a fresh handle started at that tick"""
    from test_gpu_episode import _pushed_trot
    n, g = 17, EL.ROBOT
    T = WL.PRIME + WL.STAND + WL.WALK
    others = np.arange(n) != g
    ep0, summ0, _ = _pushed_trot(eng, pkg, scen, copying=False)
    r1 = _respawn_trot(eng, pkg, scen, dict(RR.DEFAULT, codes=0, max_ticks=0, hold_ticks=WL.PRIME))
    assert ER.bits_equal(r1["episode"], ep0) and ER.bits_equal(r1["summary"], summ0)
    assert not r1["finished"].any() and not r1["life"].any()
    r2 = _respawn_trot(eng, pkg, scen, dict(RR.DEFAULT, hold_ticks=WL.PRIME))
    first, second = r2["finished"][g], r2["episode"][g]
    print("the pushed robot's first episode:", dict(zip(ER.FIELDS, first)))
    print("its second:", dict(zip(ER.FIELDS, second)), "life", r2["life"][g])
    assert ER.bits_equal(first, ep0[g])   # (its first episode is the one of the loop without respawn)
    assert first[2] in (2, 3) and EL.PUSH_FIRST <= first[1] - 1 < EL.PUSH_FIRST + EL.PUSH_TICKS
    t_fall = int(first[1]) - 1
    assert list(r2["life"][g]) == [0, 1] and not r2["life"][others].any() and not r2["finished"][others].any()
    assert second[2] == 0 and second[1] == 0 and second[0] == T - (t_fall + 1 + WL.PRIME)   # held exactly PRIME ticks, then every tick accumulated
    assert second[11] == 0 and second[12] == 0 and np.isfinite(second).all() and second[5] <= 1 - np.cos(SL.CONDITIONS["tilt"]) ** 2   # (roll and pitch both within the loops' condition)
    assert ER.bits_equal(r2["episode"][others], r1["episode"][others])
    r3 = _respawn_trot(eng, pkg, scen, dict(RR.DEFAULT, hold_ticks=WL.PRIME), t0=t_fall + 1, pushed=False)   # (second episodes: the push was the first one's)
    for k in ("state", "R", "foot", "episode"):
        assert ER.bits_equal(r3[k][g], r2[k][g]), k
    assert list(r3["life"][g]) == [0, 0]
