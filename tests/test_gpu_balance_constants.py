"""GPU, through the C ABI: the balance-QP stance controller (a1mpc_balance_solve_batch, a1mpc_balance_solve_batch_device, a1mpc_control_tick_balance_device) OFF the
reference's constants and OFF the default OSQP settings.  Every other balance test of the suite passes a1mpc_default_balance_config -- Q = (1, 1, 1, 400, 400, 100), F_min = 0,
an F_max that hardly ever binds -- under which a swap inside a weight triple, a force weight read for a torque weight in the Hessian or the gradient alone, an F_min not
gated by the contact flag or an F_max never applied all compute the same forces; and the library's argument fill (balance_kernel_args: Q re-ordered torque-first, the rest of
the block copied from the handle's MPC configuration) is exercised by nothing else, because the host-fiber build of the kernel text is handed a restatement of that order.

The yardstick is the oracle with the same constants and settings (the reference keeps them private; tests/test_balance_constants_host.py anchors the oracle off the
defaults), the gate balance_common.balance_held_to_oracle: the oracle's iteration count and status on every QP, grf and f_world within TOL_FORCE_BALANCE_N; the caps on QPs
settled by the 80-bit build are gpu_common's and the CPU file shows the oracle alone needs none of them on these batches.  Every solver test first shows on the oracle that
each of the nine balance_variants() moves the forces of its own batch by more than 100 x TOL_FORCE_BALANCE_N on at least half of the QPs."""
import ctypes as C

import numpy as np
import pytest

import balance_common as BC
from gpu_common import GENERIC_CONSTANTS, assert_all_three_outcomes, assert_worlds_equal, case_id, generic_params, generic_warm_ticks, tick_buffers, tick_inputs, tick_world
from test_gpu_balance_tick import _chain_tick

pytestmark = pytest.mark.gpu

OK, INVALID = 0, 1
POISON = -12345
CASES = BC.balance_settings_cases()
CONSTANTS = dict(default=BC.DEFAULT_BALANCE, generic=BC.GENERIC_BALANCE)
_id = lambda c: case_id(c) or "default"
_REFS = {}


def _cfg(pkg, scen, h=10, params=None, **over):
    return pkg.make_config((scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS) if params is None else params, h, **over)


def _dev():
    import torch
    dev = torch.device("cuda", 0)
    return torch, dev, (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev))


def _batch(scen, which):
    if ("batch", which) not in _REFS:
        _REFS["batch", which] = BC.balance_batch(scen, *which)
    return _REFS["batch", which]


def _oracle(oracle, scen, which, cname, case=None):
    """the oracle's answer to a batch at a constant set and a settings case, solved once per session and never written to"""
    key = (which, cname, _id(case or {}))
    if key not in _REFS:
        c = CONSTANTS.get(cname) or BC.BALANCE_EDGE_CONSTANTS[cname]
        _REFS[key] = BC.oracle_balance(oracle, c, oracle.default_settings(**(case or {})), _batch(scen, which))
        for v in _REFS[key].values():
            v.setflags(write=False)
    return _REFS[key]


def _host(eng, sc, qp):
    return eng.balance_solve(sc["root_acc"], sc["R"], sc["Rz"], sc["foot"], sc["contact"], qp=qp)


def _rows(d, lo, hi):
    return {k: d[k][lo:hi] for k in BC.BALANCE_KEYS}


def _poisoned(torch, dev, rows):
    return dict(grf=torch.full((rows, 12), float("nan"), dtype=torch.float64, device=dev), f_world=torch.full((rows, 12), float("nan"), dtype=torch.float64, device=dev),
                iters=torch.full((rows,), POISON, dtype=torch.int32, device=dev), status=torch.full((rows,), POISON, dtype=torch.int32, device=dev))


def _untouched(o, n):
    """every word beyond row n still holds its poison"""
    a = {k: v.cpu().numpy() for k, v in o.items()}
    return np.isnan(a["grf"][n:]).all() and np.isnan(a["f_world"][n:]).all() and (a["iters"][n:] == POISON).all() and (a["status"][n:] == POISON).all()


# ---------------------------------------------------------------------------------------------------------------- 1. the host entry
def test_host_entry_at_the_generic_constants(pkg, oracle, scen):
    """a1mpc_balance_solve_batch with GENERIC_BALANCE: 256 QPs with all sixteen contact patterns (staged copies) and the first 4 and 8 rows of a 9-QP batch (the pinned
    small-batch block) held to the oracle; the small calls equal the first rows of the n = 9 call bit for bit"""
    main, small = _batch(scen, BC.BATCH_MAIN), _batch(scen, BC.BATCH_SMALL)
    BC.assert_balance_variants_move(oracle, main); BC.assert_balance_variants_move(oracle, small)
    qp = BC.balance_config(pkg, BC.GENERIC_BALANCE)
    with pkg.Engine(_cfg(pkg, scen), 256, 0) as eng:
        out = _host(eng, main, qp)
        nine = _host(eng, small, qp)
        few = {n: _host(eng, BC.balance_rows(small, 0, n), qp) for n in (4, 8)}
    BC.balance_held_to_oracle(out, _oracle(oracle, scen, BC.BATCH_MAIN, "generic"), BC.x87_balance(BC.GENERIC_BALANCE, {}, main), {}, "host entry")
    ref9 = _oracle(oracle, scen, BC.BATCH_SMALL, "generic")
    BC.balance_held_to_oracle(nine, ref9, BC.x87_balance(BC.GENERIC_BALANCE, {}, small), {}, "host entry")
    for n, a in few.items():
        BC.balance_held_to_oracle(a, _rows(ref9, 0, n), BC.x87_balance(BC.GENERIC_BALANCE, {}, small), {}, "host entry, pinned block")
        for k in BC.BALANCE_KEYS:
            assert np.array_equal(a[k], nine[k][:n]), (n, k)
    assert np.abs(out["grf"]).max() > 10.0 and (out["status"] == 1).all()


# ---------------------------------------------------------------------------------------------------------------- 2. the device entry at the batch edges
@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 257])
def test_device_entry_batch_edges(pkg, oracle, scen, n):
    """a1mpc_balance_solve_batch_device with GENERIC_BALANCE on n rows cut from the middle of a 257-QP batch (all-stance rows and the patterns b % 16 on either side of the
    cut; a balance QP is one DPP row, four to a wavefront): outputs 8 rows longer than n and poisoned -- rows below n equal the host entry's bit for bit and are held to the
    oracle, every word beyond n is untouched; null optional outputs are accepted and leave the others alone; two calls with different constants back to back on two streams
    of one handle each give their own constants' answer (the by-value a1mpc_balance_config is not shared state)"""
    torch, dev, T = _dev()
    whole = _batch(scen, BC.BATCH_EDGES)
    BC.assert_balance_variants_move(oracle, whole)
    lo = 0 if n == 257 else 128 - (n + 1) // 2
    sc = BC.balance_rows(whole, lo, lo + n)
    assert sc["contact"][0].all() and (n == 1 or not sc["contact"].all())       # all-stance rows first, then other patterns
    gen, dft = BC.balance_config(pkg, BC.GENERIC_BALANCE), BC.balance_config(pkg, BC.DEFAULT_BALANCE)
    cfg = _cfg(pkg, scen)
    with pkg.Engine(cfg, 512, 0) as e_dev, pkg.Engine(cfg, 512, 0) as e_host:
        s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        d = [T(sc[k]) for k in BC.BALANCE_INPUTS]
        o = _poisoned(torch, dev, n + 8)
        torch.cuda.synchronize()
        e_dev.balance_solve_device(n, *d, o["grf"], o["f_world"], o["iters"], o["status"], qp=gen, stream=s1.cuda_stream)
        s1.synchronize()
        host = _host(e_host, sc, gen); host_dft = _host(e_host, sc, dft)
        got = {k: o[k].cpu().numpy()[:n] for k in BC.BALANCE_KEYS}
        x87_solve = BC.x87_balance(BC.GENERIC_BALANCE, {}, sc)
        BC.balance_held_to_oracle(got, _rows(_oracle(oracle, scen, BC.BATCH_EDGES, "generic"), lo, lo + n), x87_solve, {}, f"device entry n = {n}")
        for k in BC.BALANCE_KEYS:
            assert np.array_equal(got[k], host[k]), (n, k)
        assert _untouched(o, n), n
        # null optional outputs: grf alone is written, the three others keep what the first call left
        g2 = torch.full((n + 8, 12), float("nan"), dtype=torch.float64, device=dev)
        before = {k: o[k].clone() for k in ("f_world", "iters", "status")}
        torch.cuda.synchronize()
        e_dev.balance_solve_device(n, *d, g2, qp=gen, stream=s2.cuda_stream)
        s2.synchronize()
        assert np.array_equal(g2.cpu().numpy()[:n], host["grf"]) and torch.isnan(g2[n:]).all(), n
        for k in before:
            assert np.array_equal(o[k].cpu().numpy(), before[k].cpu().numpy(), equal_nan=True), (n, k)
        # two constant sets back to back on two streams, no host wait in between
        oa, ob = _poisoned(torch, dev, n + 8), _poisoned(torch, dev, n + 8)
        torch.cuda.synchronize()
        e_dev.balance_solve_device(n, *d, oa["grf"], oa["f_world"], oa["iters"], oa["status"], qp=gen, stream=s1.cuda_stream)
        e_dev.balance_solve_device(n, *d, ob["grf"], ob["f_world"], ob["iters"], ob["status"], qp=dft, stream=s2.cuda_stream)
        torch.cuda.synchronize()
        for k in BC.BALANCE_KEYS:
            assert np.array_equal(oa[k].cpu().numpy()[:n], host[k]), (n, k, "generic constants, first stream")
            assert np.array_equal(ob[k].cpu().numpy()[:n], host_dft[k]), (n, k, "default constants, second stream")
        assert _untouched(oa, n) and _untouched(ob, n)
        BC.balance_held_to_oracle(host_dft, _rows(_oracle(oracle, scen, BC.BATCH_EDGES, "default"), lo, lo + n), BC.x87_balance(BC.DEFAULT_BALANCE, {}, sc), {},
                                  f"default constants n = {n}")
        assert not np.array_equal(host["grf"], host_dft["grf"])


# ---------------------------------------------------------------------------------------------------------------- 3. settings on the H = 1 kernel
@pytest.mark.parametrize("cname", list(CONSTANTS))
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_settings_on_the_balance_kernel(pkg, oracle, scen, case, cname):
    """the fifteen gpu_common.SETTINGS_CASES and one Ruiz pass, set on the HANDLE ("the handle's OSQP settings"), on launch<1, kModeBalance> with the default and the generic
    constants, 256 QPs.  max_iter = 30: the oracle's answer holds MAX_ITER_REACHED, SOLVED_INACCURATE and SOLVED (asserted first), and every QP, the failed ones included,
    is held to its iteration count, status and forces.  (The variant precondition is shown under the default settings, a property of the batch; under which settings it
    holds as well is in tests/test_balance_constants_host.py.)"""
    sc = _batch(scen, BC.BATCH_MAIN)
    BC.assert_balance_variants_move(oracle, sc)
    ref = _oracle(oracle, scen, BC.BATCH_MAIN, cname, case)
    if case.get("max_iter") == 30:
        print(cname, "oracle statuses at max_iter = 30:", assert_all_three_outcomes(ref["status"]))
    with pkg.Engine(_cfg(pkg, scen, 10, warm_start=0, **case), 256, 0) as eng:
        out = _host(eng, sc, BC.balance_config(pkg, CONSTANTS[cname]))
    BC.balance_held_to_oracle(out, ref, BC.x87_balance(CONSTANTS[cname], case, sc), case, f"{cname} constants")


@pytest.mark.parametrize("mode", [1, 2])
def test_warm_start_is_forced_off(pkg, oracle, scen, mode):
    """an h = 10 handle made with warm_start = 1 / 2: two successive calls give identical bits, the bits of a warm_start = 0 handle, and the oracle's cold answer"""
    sc = _batch(scen, BC.BATCH_MAIN)
    BC.assert_balance_variants_move(oracle, sc)
    qp = BC.balance_config(pkg, BC.GENERIC_BALANCE)
    with pkg.Engine(_cfg(pkg, scen, 10, warm_start=mode), 256, 0) as eng, pkg.Engine(_cfg(pkg, scen, 10, warm_start=0), 256, 0) as cold:
        a = _host(eng, sc, qp); b = _host(eng, sc, qp); c = _host(cold, sc, qp)
    for k in BC.BALANCE_KEYS:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), (mode, k)
    BC.balance_held_to_oracle(a, _oracle(oracle, scen, BC.BATCH_MAIN, "generic"), BC.x87_balance(BC.GENERIC_BALANCE, {}, sc), {}, f"warm_start = {mode} handle")


# ---------------------------------------------------------------------------------------------------------------- 4. constants at the edge of what is accepted
@pytest.mark.parametrize("name", list(BC.BALANCE_EDGE_CONSTANTS))
def test_edge_constants_are_accepted_and_solved(pkg, oracle, scen, name):
    """mu = 0, F_min = F_max, R = 0, two zero weights, Q = 0 (each the generic set with that one change) under the default settings: the same gate; the all-swing rows return
    the oracle's (near-zero) forces with status SOLVED"""
    sc = _batch(scen, BC.BATCH_MAIN)
    BC.assert_balance_variants_move(oracle, sc)
    c = BC.BALANCE_EDGE_CONSTANTS[name]
    ref = _oracle(oracle, scen, BC.BATCH_MAIN, name)
    swing = ~sc["contact"].any(1)
    assert swing.sum() == 8 and (ref["status"] == 1).all() and np.abs(ref["grf"][swing]).max() < BC.TOL_FORCE_BALANCE_N
    with pkg.Engine(_cfg(pkg, scen), 256, 0) as eng:
        out = _host(eng, sc, BC.balance_config(pkg, c))
    BC.balance_held_to_oracle(out, ref, BC.x87_balance(c, {}, sc), {}, name)
    assert (out["status"][swing] == 1).all() and np.abs(out["grf"][swing]).max() < BC.TOL_FORCE_BALANCE_N


# ---------------------------------------------------------------------------------------------------------------- 5. the handle's MPC configuration is irrelevant
def test_the_handles_mpc_configuration_is_not_read(pkg, oracle, scen):
    """balance_kernel_args starts from the handle's MPC block (mass, inertia, q, r, mu, fz_*, dt) and overwrites part of it: one generic-constants batch on three handles
    with the same OSQP settings -- the gazebo set at h = 10, gpu_common.GENERIC_CONSTANTS at h = 16 with mu = 0.6, fz_min = 5, fz_max = 120, and h = 1 -- gives bit-equal
    outputs, held to the oracle"""
    sc = _batch(scen, BC.BATCH_MAIN)
    BC.assert_balance_variants_move(oracle, sc)
    qp = BC.balance_config(pkg, BC.GENERIC_BALANCE)
    base = scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS
    other = generic_params(base, mu=0.6, fz_min=5.0, fz_max=120.0)
    assert other["mass"] == GENERIC_CONSTANTS["mass"] != base["mass"]
    outs = []
    for h, params in ((10, base), (16, other), (1, base)):
        with pkg.Engine(_cfg(pkg, scen, h, params), 256, 0) as eng:
            outs.append(_host(eng, sc, qp))
    for k in BC.BALANCE_KEYS:
        assert np.array_equal(outs[0][k], outs[1][k]) and np.array_equal(outs[0][k], outs[2][k]), k
    BC.balance_held_to_oracle(outs[1], _oracle(oracle, scen, BC.BATCH_MAIN, "generic"), BC.x87_balance(BC.GENERIC_BALANCE, {}, sc), {}, "h = 16 handle, generic MPC constants")


def test_balance_solves_between_mpc_ticks_leave_the_warm_start_alone(pkg, oracle, scen):
    """three ticks of a warm_start = 1 MPC sequence (h = 10, n = 64) with a balance solve after each tick -- 64 QPs through the staged copies, 4 through the pinned block --
    equal the same sequence without them bit for bit in grf, u, iters and status: the balance launch is handed none of the handle's warm buffers"""
    ticks = generic_warm_ticks(scen, 10, 64)[:3]
    main = _batch(scen, BC.BATCH_MAIN)
    BC.assert_balance_variants_move(oracle, main)
    b64, b4 = BC.balance_rows(main, 96, 160), BC.balance_rows(main, 126, 130)
    qp = BC.balance_config(pkg, BC.GENERIC_BALANCE)
    cfg = _cfg(pkg, scen, 10, ticks[0]["params"], warm_start=1)
    args = lambda sc: (sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"])
    with pkg.Engine(cfg, 64, 0) as plain, pkg.Engine(cfg, 64, 0) as mixed:
        between = []
        for t, sc in enumerate(ticks):
            a = plain.solve(*args(sc), want_u=True)
            b = mixed.solve(*args(sc), want_u=True)
            for k in ("grf", "u", "iters", "status"):
                assert np.array_equal(a[k], b[k]), (t, k)
            between.append((_host(mixed, b64, qp), _host(mixed, b4, qp)))
        assert (a["status"] == 1).all() and plain.last_warm_start_mode() == 1
    ref = _oracle(oracle, scen, BC.BATCH_MAIN, "generic")
    for big, few in between:      # the balance answers themselves do not depend on the MPC solve before them either
        for k in BC.BALANCE_KEYS:
            assert np.array_equal(big[k], between[0][0][k]) and np.array_equal(few[k], big[k][30:34]), k
    BC.balance_held_to_oracle(between[0][0], _rows(ref, 96, 160), BC.x87_balance(BC.GENERIC_BALANCE, {}, b64), {}, "between MPC ticks")


# ---------------------------------------------------------------------------------------------------------------- 6. the one-call tick
def test_one_call_tick_with_generic_constants(pkg, oracle, scen):
    """a1mpc_control_tick_balance_device with bt.qp = GENERIC_BALANCE and MIXED_GAINS, n = 65, four ticks of gpu_common.tick_inputs, against the eight *_device entries
    chained by hand on a second handle: every output word and every carried state bit for bit.  On tick 0 the balance stage is held to the oracle, fed the chain's own
    root_acc, feet and contacts read back from the device (the oracle and its 80-bit build are first held to each other on those inputs).

    On tick 0 the robots STAND (movement_mode = 0, four stance legs; the balance QP is the stance controller), root_euler_d starts within 0.02 rad of the measured attitude
    and root_pos_d is spread by 0.05 m; ticks 1 - 3 walk as tick_inputs has them.  The reason is the variant precondition: in tick_inputs' trot two legs carry the 118 N
    of the body, so with F_max = 50 every QP sits on its upper bound and neither R nor F_min shows in the oracle's forces (measured on the inputs read back from the device:
    R -> 1e-3 moves 6 % of 65 QPs, F_min -> 0 40 %) -- a BalanceTick that handed on a wrong R or F_min would pass.  Standing, each of the nine variants moves more than
    half of the batch; that is asserted on the inputs read back, before any output is looked at"""
    torch, dev, T = _dev()
    n = 65
    rng = np.random.default_rng(4246)
    E = pkg.engine
    cfg = _cfg(pkg, scen)
    qp = BC.balance_config(pkg, BC.GENERIC_BALANCE)
    with pkg.Engine(cfg, n, 0) as e1, pkg.Engine(cfg, n, 0) as e8:
        prm = E.TickParams(); e1.lib.a1mpc_default_tick_params(C.byref(prm))
        st = torch.cuda.Stream(device=dev)
        pos_d = T(np.array([0.0, 0.0, 0.3]) + rng.normal(0, 0.05, (n, 3)))
        first = tick_inputs(scen, rng, n)
        first["movement_mode"] = np.zeros(n, np.uint8)
        euler_d0 = first["root_euler"] + rng.normal(0, 0.02, (n, 3))
        worlds = [tick_world(n, dev, (0.0, 120.0, 120.0, 0.0)) for _ in range(2)]
        for w in worlds:
            w["state"]["root_euler_d"].copy_(T(euler_d0))
        extras = [dict(root_pos_d=pos_d, root_acc=torch.full((n, 6), float("nan"), dtype=torch.float64, device=dev),
                       f_world=torch.full((n, 12), float("nan"), dtype=torch.float64, device=dev)) for _ in range(2)]
        (w1, w8), (x1, x8) = worlds, extras
        gains = e1.balance_gains(**BC.MIXED_GAINS)
        bt1 = e1.balance_tick(pos_d, x1["root_acc"], x1["f_world"], gains=gains, qp=qp)
        bt8 = e8.balance_tick(pos_d, gains=gains, qp=qp)
        for t in range(4):
            inp = {k: T(v) for k, v in (first if t == 0 else tick_inputs(scen, rng, n)).items()}
            bf = tick_buffers(E, inp, w1)
            torch.cuda.synchronize()
            e1.control_tick_balance_device(prm, bt1, bf, n, stream=st.cuda_stream)
            _chain_tick(e8, prm, bt8, n, C.c_void_p(st.cuda_stream), inp, w8, x8)
            st.synchronize()
            assert_worlds_equal(t, w1, w8)
            for k in ("root_acc", "f_world"):
                assert np.array_equal(x1[k].cpu().numpy(), x8[k].cpu().numpy(), equal_nan=True), (t, k)
            if t == 0:
                sc = dict(root_acc=x8["root_acc"].cpu().numpy(), R=inp["R_world"].cpu().numpy(), Rz=inp["R_z"].cpu().numpy(), foot=w8["outs"]["foot_pos_abs"].cpu().numpy(),
                          contact=w8["u8"]["contacts"].cpu().numpy())
                assert not any(np.isnan(sc[k]).any() for k in ("root_acc", "R", "Rz", "foot"))
                got = dict(grf=w1["outs"]["grf"].cpu().numpy(), f_world=x1["f_world"].cpu().numpy(), iters=w1["i32"]["iters"].cpu().numpy(), status=w1["i32"]["status"].cpu().numpy())
                BC.assert_balance_variants_move(oracle, sc, label="tick 0")
                ref = BC.oracle_balance(oracle, BC.GENERIC_BALANCE, oracle.default_settings(), sc)
                x87_solve = BC.x87_balance(BC.GENERIC_BALANCE, {}, sc)
                BC.balance_yardstick_alone("tick 0", ref, x87_solve, {})
                BC.balance_held_to_oracle(got, ref, x87_solve, {}, "one-call tick, tick 0")
        assert np.abs(w1["state"]["joint_torques"].cpu().numpy()).max() > 0.1 and np.abs(w1["outs"]["grf"].cpu().numpy()).max() > 1.0


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def _bad_configs(pkg):
    def make(**f):
        q = BC.balance_config(pkg, BC.GENERIC_BALANCE)
        for k, v in f.items():
            if k.startswith("Q"):
                q.Q[int(k[1:])] = v
            else:
                setattr(q, k, v)
        return q
    return {"Q[2] < 0": make(Q2=-1.0), "Q[0] < 0": make(Q0=-1e-300), "Q[4] NaN": make(Q4=np.nan), "R < 0": make(R=-1e-3), "mu < 0": make(mu=-0.1),
            "F_min > F_max": make(F_min=60.0), "F_max < 0": make(F_min=-2.0, F_max=-1.0), "F_max infinite": make(F_max=np.inf), "Q[5] infinite": make(Q5=np.inf),
            "R NaN": make(R=np.nan), "mu infinite": make(mu=np.inf), "F_min -infinite": make(F_min=-np.inf)}


def test_invalid_constants_are_refused_by_all_three_entries(pkg, scen):
    """a negative or NaN weight, R < 0, mu < 0, F_min > F_max, F_max < 0 and an infinite field, each through a1mpc_balance_solve_batch, _device and
    a1mpc_control_tick_balance_device: A1MPC_ERR_INVALID_ARGUMENT, a1mpc_last_error names the balance QP, and no poisoned output or carried state is touched.  (Zero
    weights, mu = 0 and F_min = F_max are accepted: test_edge_constants_are_accepted_and_solved.)"""
    torch, dev, T = _dev()
    n = 8
    E = pkg.engine
    sc = BC.balance_rows(_batch(scen, BC.BATCH_MAIN), 124, 132)
    rng = np.random.default_rng(4247)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)); ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    with pkg.Engine(_cfg(pkg, scen), n, 0) as eng:
        lib, h = eng.lib, eng._h
        d = [T(sc[k]) for k in BC.BALANCE_INPUTS]
        o = _poisoned(torch, dev, n)
        hg, hf = np.full((n, 12), np.nan), np.full((n, 12), np.nan); hi, hs = np.full(n, POISON, np.int32), np.full(n, POISON, np.int32)
        prm = E.TickParams(); lib.a1mpc_default_tick_params(C.byref(prm))
        pos_d = T(np.tile([0.0, 0.0, 0.3], (n, 1)))
        w = tick_world(n, dev, (0.0, 120.0, 120.0, 0.0))
        for k in w["outs"]:
            w["outs"][k].fill_(float("nan"))
        for k in w["i32"]:
            w["i32"][k].fill_(POISON)
        keep = {(g, k): w[g][k].cpu().numpy().copy() for g in w for k in w[g]}
        x = dict(root_acc=torch.full((n, 6), float("nan"), dtype=torch.float64, device=dev), f_world=torch.full((n, 12), float("nan"), dtype=torch.float64, device=dev))
        inp = {k: T(v) for k, v in tick_inputs(scen, rng, n).items()}
        bf = tick_buffers(E, inp, w)
        torch.cuda.synchronize()
        for name, q in _bad_configs(pkg).items():
            rc = lib.a1mpc_balance_solve_batch(h, C.byref(q), n, dp(sc["root_acc"]), dp(sc["R"]), dp(sc["Rz"]), dp(sc["foot"]), sc["contact"].ctypes.data_as(C.POINTER(C.c_uint8)),
                                               dp(hg), dp(hf), ip(hi), ip(hs))
            assert rc == INVALID and b"balance-QP" in lib.a1mpc_last_error(), (name, "host", rc, lib.a1mpc_last_error())
            rc = lib.a1mpc_balance_solve_batch_device(h, C.byref(q), n, *[ptr(t) for t in d], ptr(o["grf"]), ptr(o["f_world"]), ptr(o["iters"]), ptr(o["status"]), None)
            assert rc == INVALID and b"balance-QP" in lib.a1mpc_last_error(), (name, "device", rc, lib.a1mpc_last_error())
            bt = eng.balance_tick(pos_d, x["root_acc"], x["f_world"], qp=q)
            rc = lib.a1mpc_control_tick_balance_device(h, C.byref(prm), C.byref(bt), C.byref(bf), n, None)
            assert rc == INVALID and b"balance-QP" in lib.a1mpc_last_error(), (name, "tick", rc, lib.a1mpc_last_error())
        torch.cuda.synchronize()
        assert np.isnan(hg).all() and np.isnan(hf).all() and (hi == POISON).all() and (hs == POISON).all()
        assert _untouched(o, 0) and torch.isnan(x["root_acc"]).all() and torch.isnan(x["f_world"]).all()
        for (g, k), v in keep.items():
            assert np.array_equal(w[g][k].cpu().numpy(), v, equal_nan=True), (g, k)
        # the handle still works, and the valid generic set goes through all three entries
        good = BC.balance_config(pkg, BC.GENERIC_BALANCE)
        out = _host(eng, sc, good)
        eng.balance_solve_device(n, *d, o["grf"], o["f_world"], o["iters"], o["status"], qp=good)
        eng.control_tick_balance_device(prm, eng.balance_tick(pos_d, x["root_acc"], x["f_world"], qp=good), bf, n)
        torch.cuda.synchronize()
        assert all(np.array_equal(o[k].cpu().numpy(), out[k]) for k in BC.BALANCE_KEYS) and not torch.isnan(x["f_world"]).any()
