"""GPU: the balance-QP stance controller (stance_leg_control_type 0 of the reference, S/A1RobotControl.cpp:325-332, 377-444) through the C ABI -- the PD wrench against the
oracle bit for bit, the device-pointer balance solve against the host entry and the oracle, the contact block alone against a1mpc_contact_terrain_batch and the oracle, and
a1mpc_control_tick_balance_device against the *_device entries chained by hand.  Device memory is torch tensors, as in tests/test_gpu_caller_side.py."""
import ctypes as C

import numpy as np
import pytest

import balance_common as BC
from gpu_common import gait_cycle_fleet, gait_loop, threshold_forces, tick_buffers, tick_inputs, tick_world, DEFAULT_FOOT_POS
from helpers import TOL_FORCE_BALANCE_N

pytestmark = pytest.mark.gpu

OK, INVALID, TOO_LARGE = 0, 1, 5


def _cfg(pkg, scen, h=10, **over):
    return pkg.make_config(scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS, h, **over)


def _dev():
    """(torch, the device, host array -> device tensor).  The tests launch on streams of their own, which do not wait for torch's default stream: after the tensors of
    a call have been made (copies, fills) they synchronise the device once before the first launch"""
    import torch
    dev = torch.device("cuda", 0)
    return torch, dev, (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev))


def _wrench_device(torch, dev, T, eng, gains, inp, n, rows, stream=None):
    d = {k: T(v) for k, v in inp.items()}
    out = torch.full((rows, 6), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    eng.balance_wrench_device(n, *[d[k] for k in BC.WRENCH_KEYS], d["R"], out, gains=gains, stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- the wrench
def test_wrench_host_and_device_entries_equal_the_oracle_bit_for_bit(pkg, oracle, scen):
    """the sizes and special rows of tests/test_balance_wrench_host.py (one lane, either side of a wavefront edge, past one workgroup; the yaw wrap on, beside and beyond
    its marks; mixed and zero gains; a NaN row) through a1mpc_balance_wrench_batch and _device on a handle with max_batch 512 > n, a NaN-poisoned tail behind the device
    output; then the handle's cfg.mass: a1mpc_update_config moves element 2 and nothing else"""
    torch, dev, T = _dev()
    cfg = _cfg(pkg, scen)
    m0 = float(cfg.mass)
    with pkg.Engine(cfg, 512, 0) as eng:
        st = torch.cuda.Stream(device=dev)
        for n in BC.WRENCH_SIZES:
            inp = BC.wrench_inputs(scen, np.random.default_rng(40 + n), n)
            BC.yaw_rows_take_their_branch(inp)
            for name, gd in (("default", BC.DEFAULT_GAINS), ("mixed", BC.MIXED_GAINS), ("zero", BC.ZERO_GAINS)):
                gains = eng.balance_gains(**gd)
                ref = BC.oracle_wrench(oracle, gd, inp, m0, rows=n + 19)
                host = eng.balance_wrench(*[inp[k] for k in BC.WRENCH_KEYS], inp["R"], gains=gains)
                BC.assert_wrench_equals_oracle(host, ref[:n], inp, (n, name, "host"))
                got = _wrench_device(torch, dev, T, eng, gains, inp, n, n + 19, stream=st.cuda_stream if n % 2 else None)
                BC.assert_wrench_equals_oracle(got, ref, inp, (n, name, "device"))
        # cfg.mass: with zero gains element 2 IS mass * 9.8, so it moves by exactly m1 * 9.8 - m0 * 9.8 as the host computes it; with the default gains the oracle says where to
        n = 65
        inp = BC.wrench_inputs(scen, np.random.default_rng(5), n, nan_row=False)
        args = [inp[k] for k in BC.WRENCH_KEYS] + [inp["R"]]
        z0 = eng.balance_wrench(*args, gains=eng.balance_gains(**BC.ZERO_GAINS)); d0 = eng.balance_wrench(*args)
        m1 = 13.25
        eng.update_config(_cfg(pkg, scen, mass=m1))
        z1 = eng.balance_wrench(*args, gains=eng.balance_gains(**BC.ZERO_GAINS)); d1 = eng.balance_wrench(*args)
        assert np.array_equal(z0[:, 2], np.full(n, m0 * 9.8)) and np.array_equal(z1[:, 2] - z0[:, 2], np.full(n, m1 * 9.8 - m0 * 9.8))
        assert np.array_equal(d1, BC.oracle_wrench(oracle, BC.DEFAULT_GAINS, inp, m1)) and np.array_equal(d0, BC.oracle_wrench(oracle, BC.DEFAULT_GAINS, inp, m0))
        assert np.array_equal(np.delete(d1, 2, 1), np.delete(d0, 2, 1)) and not np.array_equal(d1[:, 2], d0[:, 2])


def test_wrench_refusals_on_a_live_handle(pkg, scen):
    """every refusal of include/a1mpc.h, none of which touches the output: a null array (each of the ten in turn, named), null gains, a non-finite gain, n < 0,
    n > max_batch; n == 0 is OK and launches nothing"""
    torch, dev, T = _dev()
    with pkg.Engine(_cfg(pkg, scen), 8, 0) as eng:
        lib, h = eng.lib, eng._h
        g = eng.balance_gains()
        ptr = lambda t: C.c_void_p(t.data_ptr())
        arrs = [torch.zeros((8, 3), dtype=torch.float64, device=dev) for _ in range(8)] + [torch.zeros((8, 9), dtype=torch.float64, device=dev)]
        out = torch.full((8, 6), float("nan"), dtype=torch.float64, device=dev)
        names = list(BC.WRENCH_KEYS) + ["R_world", "root_acc_out"]
        full = [ptr(a) for a in arrs] + [ptr(out)]
        for k, name in enumerate(names):
            a = list(full); a[k] = None
            assert lib.a1mpc_balance_wrench_batch_device(h, C.byref(g), 4, *a, None) == INVALID and name.encode() in lib.a1mpc_last_error(), name
        assert lib.a1mpc_balance_wrench_batch_device(h, None, 4, *full, None) == INVALID and b"a1mpc_balance_gains" in lib.a1mpc_last_error()
        for field, bad in (("kp_linear", np.nan), ("kd_angular", np.inf)):
            gb = eng.balance_gains(); getattr(gb, field)[1] = bad
            assert lib.a1mpc_balance_wrench_batch_device(h, C.byref(gb), 4, *full, None) == INVALID and b"gain" in lib.a1mpc_last_error()
        assert lib.a1mpc_balance_wrench_batch_device(h, C.byref(g), -1, *full, None) == INVALID
        assert lib.a1mpc_balance_wrench_batch_device(h, C.byref(g), 9, *full, None) == TOO_LARGE and b"max_batch" in lib.a1mpc_last_error()
        assert lib.a1mpc_balance_wrench_batch_device(h, C.byref(g), 0, *full, None) == OK
        host = [np.zeros((8, 3)) for _ in range(8)] + [np.zeros((8, 9))]
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        assert lib.a1mpc_balance_wrench_batch(h, C.byref(g), 9, *[dp(a) for a in host], dp(np.zeros((9, 6)))) == TOO_LARGE
        assert lib.a1mpc_balance_wrench_batch(h, C.byref(g), 4, *[dp(a) for a in host[:8]], None, dp(np.zeros((4, 6)))) == INVALID and b"R_world" in lib.a1mpc_last_error()
        torch.cuda.synchronize()
        assert torch.isnan(out).all()


# ---------------------------------------------------------------------------------------------------------------- the device balance solve
def _balance_device(torch, dev, T, eng, sc, n, root_acc=None, stream=None, qp=None):
    d = dict(acc=T(sc["root_acc"][:n] if root_acc is None else root_acc), R=T(sc["R"][:n]), Rz=T(sc["Rz"][:n]), foot=T(sc["foot"][:n]), contact=T(sc["contact"][:n]))
    o = dict(grf=torch.zeros((n, 12), dtype=torch.float64, device=dev), f_world=torch.zeros((n, 12), dtype=torch.float64, device=dev),
             iters=torch.zeros(n, dtype=torch.int32, device=dev), status=torch.zeros(n, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    eng.balance_solve_device(n, d["acc"], d["R"], d["Rz"], d["foot"], d["contact"], o["grf"], o["f_world"], o["iters"], o["status"], qp=qp, stream=stream)
    return o, d


@pytest.mark.parametrize("n", [4, 300])
def test_device_balance_solve_equals_the_host_entry_and_the_oracle(pkg, oracle, scen, n):
    """scen.balance_random through a1mpc_balance_solve_batch_device against Engine.balance_solve on a second handle (n = 4: the host entry's pinned block; 300: its staged
    copies) bit for bit, and against the oracle at the bar tests/test_gpu_parity.py::test_balance_qp holds this kernel to: every QP at the oracle's iteration count and
    status, forces within TOL_FORCE_BALANCE_N.  A second call on another stream of the same handle (the batch reversed) is ordered behind the first"""
    torch, dev, T = _dev()
    sc = scen.balance_random(n)
    rev = {k: np.ascontiguousarray(sc[k][::-1]) for k in ("root_acc", "R", "Rz", "foot", "contact")}
    cfg = _cfg(pkg, scen)
    with pkg.Engine(cfg, 512, 0) as e_dev, pkg.Engine(cfg, 512, 0) as e_host:
        s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        o1, keep1 = _balance_device(torch, dev, T, e_dev, sc, n, stream=s1.cuda_stream)
        o2, keep2 = _balance_device(torch, dev, T, e_dev, rev, n, stream=s2.cuda_stream)   # (its synchronisation: the first call has finished -- the ordering proper is
        #                                                                                      the third call below, issued straight behind a fourth on another stream)
        nfact = e_dev.last_nfact(n)           # (synchronises the handle's last stream)
        ms = e_dev.last_kernel_ms()
        torch.cuda.synchronize()
        host = e_host.balance_solve(sc["root_acc"], sc["R"], sc["Rz"], sc["foot"], sc["contact"])
        nfact_host = e_host.last_nfact(n)
        for k in ("grf", "f_world", "iters", "status"):
            assert np.array_equal(o1[k].cpu().numpy(), host[k]), k
            assert np.array_equal(o2[k].cpu().numpy(), host[k][::-1]), (k, "second stream")
        assert np.array_equal(nfact, nfact_host[::-1]) and ms > 0.0
        qp, st = oracle.default_qp_params(), oracle.default_settings()
        grf, fw, it, stt = (o1[k].cpu().numpy() for k in ("grf", "f_world", "iters", "status"))
        worst = 0.0
        for b in range(n):
            r = oracle.balance_solve(qp, st, sc["root_acc"][b], sc["R"][b], sc["Rz"][b], sc["foot"][b], sc["contact"][b])
            assert it[b] == r["info"].iters and stt[b] == r["info"].status, b
            worst = max(worst, np.abs(fw[b] - r["f_world"]).max(), np.abs(grf[b] - r["grf"]).max())
        print(f"device balance solve, n {n}: max |df| vs oracle = {worst:.3e} N, kernel {ms:.3f} ms")
        assert worst < TOL_FORCE_BALANCE_N
        # the optional outputs may be null; an invalid a1mpc_balance_config is refused before anything else is looked at
        g2 = torch.zeros((n, 12), dtype=torch.float64, device=dev); g3 = torch.zeros((n, 12), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        e_dev.balance_solve_device(n, keep2["acc"], keep2["R"], keep2["Rz"], keep2["foot"], keep2["contact"], g3, stream=s1.cuda_stream)
        e_dev.balance_solve_device(n, keep1["acc"], keep1["R"], keep1["Rz"], keep1["foot"], keep1["contact"], g2, stream=s2.cuda_stream)   # back to back, no host wait between
        assert np.array_equal(e_dev.last_nfact(n), nfact_host)   # the handle's nfact scratch holds the LATER call's counts: the two launches did not overlap
        torch.cuda.synchronize()
        assert np.array_equal(g2.cpu().numpy(), host["grf"]) and np.array_equal(g3.cpu().numpy(), host["grf"][::-1])
        lib = e_dev.lib
        for field, bad in (("R", -1.0), ("mu", np.nan), ("F_min", 200.0)):
            q = pkg.BalanceConfig(); lib.a1mpc_default_balance_config(C.byref(q)); setattr(q, field, bad)
            assert lib.a1mpc_balance_solve_batch_device(e_dev._h, C.byref(q), n, *([None] * 9), None) == INVALID and b"balance-QP" in lib.a1mpc_last_error()
        q = pkg.BalanceConfig(); lib.a1mpc_default_balance_config(C.byref(q))
        assert lib.a1mpc_balance_solve_batch_device(e_dev._h, C.byref(q), n, None, *([C.c_void_p(g2.data_ptr())] * 8), None) == INVALID
        assert lib.a1mpc_balance_solve_batch_device(e_dev._h, C.byref(q), 513, *([C.c_void_p(g2.data_ptr())] * 9), None) == TOO_LARGE


def test_device_wrench_into_device_solve_equals_the_host_solve_of_the_oracle_wrench(pkg, oracle, scen):
    """the plumbing of the two entries together (no new tolerance: it follows from the tests above): root_acc from a1mpc_balance_wrench_batch_device, solved in place by
    a1mpc_balance_solve_batch_device on the same stream, equals Engine.balance_solve fed oracle.balance_root_acc, bit for bit"""
    torch, dev, T = _dev()
    n = 130
    sc = scen.balance_random(n, seed=77)
    inp = BC.wrench_inputs(scen, np.random.default_rng(77), n, nan_row=False)
    inp["R"] = sc["R"]
    cfg = _cfg(pkg, scen)
    with pkg.Engine(cfg, 256, 0) as e_dev, pkg.Engine(cfg, 256, 0) as e_host:
        st = torch.cuda.Stream(device=dev)
        d = {k: T(v) for k, v in inp.items()}
        acc = torch.full((n, 6), float("nan"), dtype=torch.float64, device=dev)
        e_dev.balance_wrench_device(n, *[d[k] for k in BC.WRENCH_KEYS], d["R"], acc, stream=st.cuda_stream)
        o = dict(grf=torch.zeros((n, 12), dtype=torch.float64, device=dev), f_world=torch.zeros((n, 12), dtype=torch.float64, device=dev),
                 iters=torch.zeros(n, dtype=torch.int32, device=dev), status=torch.zeros(n, dtype=torch.int32, device=dev))
        Rz, foot, contact = T(sc["Rz"]), T(sc["foot"]), T(sc["contact"])
        torch.cuda.synchronize()
        e_dev.balance_solve_device(n, acc, d["R"], Rz, foot, contact, o["grf"], o["f_world"], o["iters"], o["status"], stream=st.cuda_stream)
        st.synchronize()
        ref_acc = BC.oracle_wrench(oracle, BC.DEFAULT_GAINS, inp, float(cfg.mass))
        assert np.array_equal(acc.cpu().numpy(), ref_acc)
        host = e_host.balance_solve(ref_acc, sc["R"], sc["Rz"], sc["foot"], sc["contact"])
        for k in ("grf", "f_world", "iters", "status"):
            assert np.array_equal(o[k].cpu().numpy(), host[k]), k
        assert (host["status"] == 1).all() and np.abs(host["grf"]).max() > 1.0


# ---------------------------------------------------------------------------------------------------------------- the contact block alone
@pytest.mark.parametrize("n", [1, 65, 300])
def test_contacts_alone_equal_the_contact_terrain_entry_and_leave_the_terrain_filter_alone(pkg, oracle, scen, n):
    """70 ticks (past the recent-contact window of 60) of a staggered walking fleet with foot forces ON the 30 N threshold: a1mpc_contacts_batch on one handle gives, at
    every tick, the contacts and foot_pos_recent_contact of a1mpc_contact_terrain_batch on another and of oracle.contact_terrain_step, bit for bit.  After the run one
    a1mpc_terrain_batch call on the first handle equals the first such call on a fresh handle -- its terrain-angle filter was never advanced -- while the second
    handle's, 70 samples in, answers differently"""
    ticks = 70
    rng = np.random.default_rng(600 + n)
    cfg = _cfg(pkg, scen)
    gc, spd = gait_cycle_fleet(n)
    mm = np.ones(n, np.uint8)
    states = [oracle.contact_state() for _ in range(n)]
    z = np.full(n, 0.3); pitch2 = np.zeros(n); pitch_o = np.zeros(n)
    early = 0
    with pkg.Engine(cfg, 512, 0) as e1, pkg.Engine(cfg, 512, 0) as e2, pkg.Engine(cfg, 512, 0) as e3:
        for t in range(ticks):
            gc, plan = gait_loop(gc, spd, mm)
            ff = threshold_forces(rng, (n, 4))
            foot = DEFAULT_FOOT_POS + rng.normal(0, 0.02, (n, 12))
            a = e1.contacts(gc, plan, ff, foot)
            b = e2.contact_terrain(gc, plan, ff, foot, z, pitch2); pitch2 = b["root_euler_d_pitch"]
            ref = [oracle.contact_terrain_step(states[r], gc[r], plan[r], ff[r], foot[r], z[r], pitch_o[r]) for r in range(n)]
            pitch_o = np.array([r[3] for r in ref])
            for name, other in (("contact_terrain", (b["contacts"], b["foot_pos_recent_contact"])), ("oracle", (np.array([r[0] for r in ref]), np.array([r[1] for r in ref])))):
                assert np.array_equal(a["contacts"], other[0]) and np.array_equal(a["foot_pos_recent_contact"], other[1]), (t, name)
            early += int(((a["contacts"] == 1) & (plan == 0)).sum())
        assert early >= 1 if n == 1 else early >= n * ticks // 16, early   # (early contacts occurred: the flag carried from tick to tick is part of what was compared)
        rec = a["foot_pos_recent_contact"]; p0 = np.full(n, 0.125)
        after = e1.terrain(rec, z, p0); fresh = e3.terrain(rec, z, p0); advanced = e2.terrain(rec, z, p0)
        assert np.array_equal(after[0], fresh[0]) and np.array_equal(after[1], fresh[1])
        assert (fresh[1] > 0).all() and not np.array_equal(advanced[1], fresh[1])


# ---------------------------------------------------------------------------------------------------------------- the one-call tick
def _chain_tick(eng, prm, bt, n, sp, inp, w, extra):
    """one balance tick as the eight *_device entries by hand: the four caller-side stages of gpu_common.TickChain, then contacts, wrench, balance solve, joint torques"""
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    dp_ = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    k = {f: np.array(getattr(prm, f)) for f in ("kp_foot", "kd_foot", "km_foot", "rho_fix", "rho_opt")}
    s7, o7, b7, j7, L, H_ = w["state"], w["outs"], w["u8"], w["i32"], eng.lib, eng._h
    rcs = [L.a1mpc_leg_state_batch_device(H_, n, ptr(inp["joint_pos"]), ptr(inp["joint_vel"]), ptr(inp["R_world"]), ptr(s7["root_pos"]), ptr(s7["root_lin_vel"]),
                                          dp_(k["rho_fix"]), dp_(k["rho_opt"]), ptr(o7["foot_pos_rel"]), ptr(o7["j_foot_blocks"]), ptr(o7["foot_vel_rel"]),
                                          ptr(o7["foot_pos_abs"]), ptr(o7["foot_vel_abs"]), ptr(o7["foot_pos_world"]), ptr(o7["foot_vel_world"]), sp),
           L.a1mpc_ekf_update_batch_device(H_, n, prm.control_dt, prm.assume_flat_ground, ptr(inp["movement_mode"]), ptr(inp["foot_force"]), ptr(inp["R_world"]), ptr(inp["imu_acc"]),
                                           ptr(inp["imu_ang_vel"]), ptr(o7["foot_pos_rel"]), ptr(o7["foot_vel_rel"]), ptr(s7["root_pos"]), ptr(s7["root_lin_vel"]),
                                           ptr(b7["estimated_contacts"]), sp),
           L.a1mpc_update_plan_batch_device(H_, C.byref(prm.gait), n, ptr(inp["movement_mode"]), ptr(s7["gait_counter"]), ptr(inp["gait_counter_speed"]),
                                            ptr(s7["root_lin_vel"]), ptr(inp["R_z"]), ptr(inp["R_world"]), ptr(s7["root_pos"]), ptr(inp["root_lin_vel_d"]),
                                            ptr(b7["plan_contacts"]), ptr(o7["foot_pos_target_rel"]), ptr(o7["foot_pos_target_abs"]), ptr(o7["foot_pos_target_world"]), sp),
           L.a1mpc_swing_legs_batch_device(H_, n, prm.gait.counter_per_swing, prm.control_dt, ptr(inp["R_z"]), ptr(o7["foot_pos_abs"]), ptr(s7["gait_counter"]),
                                           ptr(o7["foot_pos_target_rel"]), dp_(k["kp_foot"]), dp_(k["kd_foot"]), ptr(s7["foot_pos_start"]),
                                           ptr(s7["foot_pos_rel_last_time"]), ptr(s7["foot_pos_target_last_time"]), ptr(o7["foot_pos_cur"]), ptr(o7["foot_forces_kin"]), sp),
           L.a1mpc_contacts_batch_device(H_, C.byref(prm.contact), n, ptr(s7["gait_counter"]), ptr(b7["plan_contacts"]), ptr(inp["foot_force"]), ptr(o7["foot_pos_abs"]),
                                         ptr(b7["contacts"]), ptr(o7["foot_pos_recent_contact"]), sp),
           L.a1mpc_balance_wrench_batch_device(H_, C.byref(bt.gains), n, ptr(extra["root_pos_d"]), ptr(s7["root_pos"]), ptr(inp["root_lin_vel_d"]), ptr(s7["root_lin_vel"]),
                                               ptr(s7["root_euler_d"]), ptr(inp["root_euler"]), ptr(inp["root_ang_vel_d"]), ptr(inp["root_ang_vel"]), ptr(inp["R_world"]),
                                               ptr(extra["root_acc"]), sp),
           L.a1mpc_balance_solve_batch_device(H_, C.byref(bt.qp), n, ptr(extra["root_acc"]), ptr(inp["R_world"]), ptr(inp["R_z"]), ptr(o7["foot_pos_abs"]), ptr(b7["contacts"]),
                                              ptr(o7["grf"]), ptr(extra["f_world"]), ptr(j7["iters"]), ptr(j7["status"]), sp),
           L.a1mpc_joint_torques_batch_device(H_, n, ptr(inp["mpc_active"]), ptr(b7["contacts"]), ptr(o7["j_foot_blocks"]), ptr(o7["grf"]), ptr(o7["foot_forces_kin"]),
                                              dp_(k["km_foot"]), ptr(inp["torques_gravity"]), ptr(s7["joint_torques"]), sp)]
    assert not any(rcs), (rcs, L.a1mpc_last_error())


@pytest.mark.parametrize("n,h,own_buffers", [(64, 10, True), (300, 10, True), (64, 1, False)])
def test_one_call_balance_tick_equals_the_hand_chain(pkg, scen, n, h, own_buffers):
    """a1mpc_control_tick_balance_device on one handle against the eight *_device entries chained by hand on a second, four ticks of gpu_common.tick_inputs with a
    per-robot root_pos_d = [0, 0, 0.3] + N(0, 0.02) and a non-zero root_euler_d: every carried state, every output, root_acc and f_world equal bit for bit (NaN-aware) on
    every tick; root_euler_d and the NaN-filled terrain_angle are never written; every QP solved; the torques are a launch of their own.  (64, 1): a handle of horizon 1
    -- the horizon is irrelevant -- with root_pos_d_z and terrain_angle NULL and root_acc in the handle's own buffer."""
    torch, dev, T = _dev()
    rng = np.random.default_rng(900 + n + h)
    E = pkg.engine
    cfg = _cfg(pkg, scen, h)
    euler_d0 = rng.normal(0, 0.05, (n, 3))
    with pkg.Engine(cfg, n, 0) as e1, pkg.Engine(cfg, n, 0) as e8:
        prm = E.TickParams(); e1.lib.a1mpc_default_tick_params(C.byref(prm))
        st = torch.cuda.Stream(device=dev)
        pos_d = T(np.array([0.0, 0.0, 0.3]) + rng.normal(0, 0.02, (n, 3)))
        worlds, extras = [], []
        for _ in range(2):
            w = tick_world(n, dev, (0.0, 120.0, 120.0, 0.0))
            w["state"]["root_euler_d"].copy_(T(euler_d0)); w["outs"]["terrain_angle"].fill_(float("nan"))
            worlds.append(w)
            extras.append(dict(root_pos_d=pos_d, root_acc=torch.full((n, 6), float("nan"), dtype=torch.float64, device=dev),
                               f_world=torch.full((n, 12), float("nan"), dtype=torch.float64, device=dev)))
        (w1, w8), (x1, x8) = worlds, extras
        bt1 = e1.balance_tick(pos_d, x1["root_acc"] if own_buffers else None, x1["f_world"])
        bt8 = e8.balance_tick(pos_d)
        for t in range(4):
            inp = {k: T(v) for k, v in tick_inputs(scen, rng, n).items()}
            bf = tick_buffers(E, inp, w1)
            torch.cuda.synchronize()
            if not own_buffers:
                bf.root_pos_d_z = None; bf.terrain_angle = None
            e1.control_tick_balance_device(prm, bt1, bf, n, stream=st.cuda_stream)
            ms, fused = e1.last_control_tick_ms()
            assert fused is False and ms > 0.0
            _chain_tick(e8, prm, bt8, n, C.c_void_p(st.cuda_stream), inp, w8, x8)
            st.synchronize()
            for grp in ("state", "outs", "u8", "i32"):
                for k in w1[grp]:
                    a, b = w1[grp][k].cpu().numpy(), w8[grp][k].cpu().numpy()
                    assert np.array_equal(a, b, equal_nan=True), (t, k)
            assert np.array_equal(x1["f_world"].cpu().numpy(), x8["f_world"].cpu().numpy()) and not np.isnan(x1["f_world"].cpu().numpy()).any(), t
            if own_buffers:
                assert np.array_equal(x1["root_acc"].cpu().numpy(), x8["root_acc"].cpu().numpy()) and not np.isnan(x1["root_acc"].cpu().numpy()).any(), t
            assert (w1["i32"]["status"].cpu().numpy() == 1).all(), (t, np.flatnonzero(w1["i32"]["status"].cpu().numpy() != 1)[:8])
            assert np.array_equal(w1["state"]["root_euler_d"].cpu().numpy(), euler_d0) and torch.isnan(w1["outs"]["terrain_angle"]).all(), t
        assert np.abs(w1["state"]["joint_torques"].cpu().numpy()).max() > 0.1 and np.abs(w1["outs"]["grf"].cpu().numpy()).max() > 1.0
        assert w1["u8"]["contacts"].cpu().numpy().any() and np.abs(w1["outs"]["foot_pos_recent_contact"].cpu().numpy()).max() > 0.0
        # refusals: a null root_pos_d, a non-finite gain, a bad QP constant, n > max_batch -- nothing is launched
        lib = e1.lib
        call = lambda b, nn=n: lib.a1mpc_control_tick_balance_device(e1._h, C.byref(prm), C.byref(b), C.byref(bf), nn, None)
        bad = e1.balance_tick(None)
        assert call(bad) == INVALID and b"root_pos_d" in lib.a1mpc_last_error()
        bad = e1.balance_tick(pos_d); bad.gains.kd_linear[2] = float("nan")
        assert call(bad) == INVALID and b"gain" in lib.a1mpc_last_error()
        bad = e1.balance_tick(pos_d); bad.qp.F_min = 500.0
        assert call(bad) == INVALID and b"balance-QP" in lib.a1mpc_last_error()
        assert call(bt1, n + 1) == TOO_LARGE and call(bt1, 0) == OK
