"""CPU: the predicted horizon states at the C ABI -- a1mpc_horizon_states_batch(_device) and a1mpc_horizon_states_ticks_batch(_device) are declared in include/a1mpc.h with
the argument order of the strided solve entries, exported by liba1mpc.so, listed in engine.EXPORTS and bound with argument types; the engine wrappers have the documented
signatures; every refusal is reported without a device; the kernel is in the code object and uses no scratch memory.  And the yardstick the GPU tests use where the
reference library does not exist (other horizons, large n) -- the longdouble recurrence of tests/horizon_states_ref.py -- is pinned to the reference's own A_qp / B_qp.
No compute on a GPU (there is none here)."""
import ctypes as C
import importlib
import inspect
import json
import os
import re

import numpy as np
import pytest

import horizon_states_ref as HS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("a1mpc_horizon_states_batch", "a1mpc_horizon_states_batch_device", "a1mpc_horizon_states_ticks_batch", "a1mpc_horizon_states_ticks_batch_device")


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "a1mpc.h")).read(), flags=re.S)


def _params(code, name):
    """the parameter names of `name`'s declaration, in order"""
    m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m, f"{name} is not declared in include/a1mpc.h"
    return [re.search(r"(\w+)\s*$", p.strip()).group(1) for p in m.group(1).split(",")]


def test_new_symbols_are_declared_exported_and_listed(pkg):
    pkg.build.build()
    code = _code()
    lib = C.CDLL(pkg.build.LIB_PATH)
    bound = pkg.load_library()
    for name in NEW:
        _params(code, name)
        assert hasattr(lib, name), f"{name} is not exported by liba1mpc.so"
        assert name in pkg.engine.EXPORTS
        assert getattr(bound, name).argtypes is not None, name   # bound with argument types (a pointer passed as a bare int would be truncated)
        assert len(getattr(bound, name).argtypes) == len(_params(code, name)), name


def test_argument_order_is_the_strided_solve_entries_for_the_shared_inputs():
    code = _code()
    shared = lambda ps: [p for p in ps if re.sub(r"^d_", "", p) in ("h", "n", "x0", "x_ref", "tick", "R_world", "foot_abs", "foot_stride", "yaw_A", "hip_stream")]
    for new, old in (("a1mpc_horizon_states_batch", "a1mpc_solve_batch_strided"), ("a1mpc_horizon_states_batch_device", "a1mpc_solve_batch_strided_device"),
                     ("a1mpc_horizon_states_ticks_batch", "a1mpc_solve_batch_ticks_strided"), ("a1mpc_horizon_states_ticks_batch_device", "a1mpc_solve_batch_ticks_strided_device")):
        a, b = _params(code, new), _params(code, old)
        assert shared(a) == shared(b), (new, a, b)
        rest = [re.sub(r"^d_", "", p) for p in a if p not in shared(a)]
        assert rest == ["u_full", "x_pred_out", "cost_out"], (new, rest)   # what a solve returns goes in right behind what it took; then the two outputs
        names = [re.sub(r"^d_", "", p) for p in a]
        assert names.index("u_full") == names.index("yaw_A") + 1, (new, a)


def test_engine_wrappers_have_the_documented_signatures(pkg):
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()][1:]
    E = inspect.Parameter.empty
    assert sig(pkg.Engine.horizon_states) == [("x0", E), ("R", E), ("foot", E), ("u", None), ("xref", None), ("foot_stride", 0), ("yaw_A", None)]
    assert sig(pkg.Engine.horizon_states_ticks) == [("tick", E), ("R", E), ("foot", E), ("u", None), ("foot_stride", 0), ("yaw_A", None), ("want_cost", True)]
    assert sig(pkg.Engine.horizon_states_device) == [("n", E), ("d_x0", E), ("d_xref", E), ("d_R", E), ("d_foot", E), ("foot_stride", E), ("d_u", E), ("d_x_pred", None),
                                                     ("d_cost", None), ("d_yaw_A", None), ("stream", None)]
    assert sig(pkg.Engine.horizon_states_ticks_device) == [("n", E), ("d_tick", E), ("d_R", E), ("d_foot", E), ("foot_stride", E), ("d_u", E), ("d_x_pred", None),
                                                           ("d_cost", None), ("d_yaw_A", None), ("stream", None)]


def test_refusals_are_reported_without_a_device(pkg):
    """a null handle with good and with bad arguments: A1MPC_ERR_INVALID_ARGUMENT (1) from all four entries, and a1mpc_last_error names what was refused.  (The refusals
    that need a live handle -- n > max_batch, cost_out without x_ref, the null inputs, both outputs null -- are checked on the GPU, tests/test_gpu_horizon_states.py.)"""
    lib = pkg.load_library()
    d = lambda k: (C.c_double * k)()
    x0, tick, xref, R, foot, u, xp, cost = d(13), d(22), d(130), d(9), d(120), d(120), d(130), d(2)
    for n, fs, xo, co in ((1, 0, xp, cost), (-1, 0, xp, cost), (1, 7, xp, cost), (1, 0, None, None), (1, 12, xp, None)):
        assert lib.a1mpc_horizon_states_batch(None, n, x0, xref, R, foot, fs, None, u, xo, co) == 1
        assert b"null handle" in lib.a1mpc_last_error()
        assert lib.a1mpc_horizon_states_batch_device(None, n, None, None, None, None, fs, None, None, None, None, None) == 1
        assert lib.a1mpc_horizon_states_ticks_batch(None, n, tick, R, foot, fs, None, u, xo, co) == 1
        assert lib.a1mpc_horizon_states_ticks_batch_device(None, n, None, None, None, fs, None, None, None, None, None) == 1
        assert b"null handle" in lib.a1mpc_last_error()
    assert lib.a1mpc_horizon_states_batch(None, 1, None, None, None, None, 0, None, None, xp, cost) == 1   # null x0 / R_world / foot_abs, cost_out without x_ref


def test_kernel_is_in_the_code_object_and_uses_no_scratch(pkg):
    pkg.build.build()
    res = json.load(open(pkg.build.RESOURCES_PATH))["kernels"]
    isa_check = importlib.import_module(pkg.__name__ + ".isa_check")
    assert isa_check.resource_gaps(res, no_scratch=("a1mpc_horizon_states_kernel",)) == []
    k = next(v for name, v in res.items() if "a1mpc_horizon_states_kernel" in name)
    print("a1mpc_horizon_states_kernel:", k)
    assert k["lds_static_bytes"] <= 20480 and k["max_flat_workgroup_size"] == 64   # one wavefront per workgroup, eight of them in a CU's 160 KB of LDS


@pytest.mark.parametrize("h", [10, 16, 20])
def test_longdouble_recurrence_equals_the_reference_A_qp_B_qp(scen, h):
    """The yardstick's own check: the recurrence restated in tests/horizon_states_ref.py agrees with A_qp x0 + B_qp u on the A_qp / B_qp that S/ConvexMpc.cpp (compiled
    verbatim, oracle/_ref) fills, within 1e-12 x S, S = |A_qp||x0| + |B_qp||u| -- broadcast and per-step feet, the A_c yaw from x0 and one of its own, forces uniform in
    [-60, 180] N (not a solution: every block of B_qp carries weight), 8 QPs each.  The abs-sum accumulated step by step is never below the matrices'."""
    import ref as REF
    if not REF.build():
        pytest.skip("oracle/_ref not built and the reference sources are absent")
    from gpu_common import _strided_inputs
    rng = np.random.default_rng(700 + h)
    sc, feet, fs, _, _ = _strided_inputs(scen, rng, h, 8, True, False)
    u = rng.uniform(-60.0, 180.0, (8, 12 * h)); yaw = sc["x0"][:, 2] + rng.uniform(-0.5, 0.5, 8)
    worst = 0.0
    for foot, stride in ((sc["foot"], 0), (feet, fs)):
        for ya in (None, yaw):
            for uu in (u, None):
                ref = HS.reference_states(REF, sc["params"], h, sc["x0"], sc["xref"], sc["R"], foot, stride, sc["contact"], uu, ya)
                X, S = HS.rollout(sc["params"], h, sc["x0"], sc["R"], foot, stride, uu, ya)
                assert (S[..., :12] > 0).all() and (ref["S"][..., :12] > 0).all()
                ratio = HS.states_ratio(X, ref["X"], ref["S"])
                worst = max(worst, ratio)
                assert ratio <= HS.BAR, (h, stride, ya is not None, ratio)
                assert np.array_equal(X[..., 12], np.broadcast_to(sc["x0"][:, 12:13], (8, h)))
                assert (ref["S"] <= S * (1 + 1e-12)).all()   # |A^k B| <= |A|^k |B|: the step-by-step abs-sum is the looser scale of the two, never the tighter
    print(f"h {h}: longdouble recurrence vs reference A_qp x0 + B_qp u, worst |dx| / S = {worst:.2e}")
