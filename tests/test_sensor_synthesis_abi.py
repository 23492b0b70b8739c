"""CPU: sensor synthesis at the C ABI -- a1mpc_sensor_synthesis_batch and a1mpc_sensor_synthesis_batch_device are declared in include/a1mpc.h, exported by liba1mpc.so,
listed in engine.EXPORTS and bound with argument types; the two entries name their arguments alike; no exported symbol of theirs contains `plant` (tests/test_plant_abi.py
counts those); the engine wrappers' signatures; the refusals that need no device; the kernel is in the code object, uses no scratch memory and is covered by the build's
gate.  No compute on a GPU (there is none here)."""
import ctypes as C
import importlib
import inspect
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("a1mpc_sensor_synthesis_batch", "a1mpc_sensor_synthesis_batch_device")
KERNEL = "a1mpc_sensor_synthesis_kernel"
HOST_ARGS = ["h", "n", "state", "state_stride", "R_world", "foot_abs", "grf_body", "contacts", "ext_wrench", "rho_fix", "rho_opt", "quat_out", "imu_acc_raw_out",
             "imu_gyro_raw_out", "joint_pos_out", "joint_vel_out", "foot_force_out", "reach_out", "foot_pos_rel_out", "foot_vel_rel_out"]


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "a1mpc.h")).read(), flags=re.S)


def _params(code, name):
    m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m, f"{name} is not declared in include/a1mpc.h"
    return [re.search(r"(\w+)\s*$", p.strip()).group(1) for p in m.group(1).split(",")]


def test_symbols_are_declared_exported_listed_and_bound(pkg):
    pkg.build.build()
    code = _code()
    lib = C.CDLL(pkg.build.LIB_PATH)
    bound = pkg.load_library()
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported by liba1mpc.so"
        assert name in pkg.engine.EXPORTS
        assert len(getattr(bound, name).argtypes) == len(_params(code, name)), name
    assert _params(code, NEW[0]) == HOST_ARGS
    dev = _params(code, NEW[1])
    assert [re.sub(r"^d_", "", p) for p in dev] == HOST_ARGS + ["hip_stream"]
    assert [p for p in dev if not p.startswith("d_")] == ["h", "n", "state_stride", "rho_fix", "rho_opt", "hip_stream"]   # the geometry stays a host array
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.build.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in nm.splitlines() if re.search(r" T a1mpc_\w*synthesis", l))
    assert exported == sorted(NEW), exported
    assert not [s for s in exported if "plant" in s]


def test_the_engine_wrappers(pkg):
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()][1:]
    E = inspect.Parameter.empty
    assert sig(pkg.Engine.sensor_synthesis) == [("state", E), ("R", E), ("foot", E), ("grf", E), ("contacts", E), ("ext_wrench", None), ("rho_fix", None), ("rho_opt", None),
                                                ("want_foot_rel", True)]
    assert sig(pkg.Engine.sensor_synthesis_device) == [("n", E), ("d_state", E), ("state_stride", E), ("d_R", E), ("d_foot", E), ("d_grf", E), ("d_contacts", E), ("d_quat", E),
                                                       ("d_imu_acc_raw", E), ("d_imu_gyro_raw", E), ("d_joint_pos", E), ("d_joint_vel", E), ("d_foot_force", E), ("d_reach", E),
                                                       ("d_foot_pos_rel", None), ("d_foot_vel_rel", None), ("d_ext_wrench", None), ("rho_fix", None), ("rho_opt", None),
                                                       ("stream", None)]
    assert pkg.Engine.SYNTHESIS_OUTPUTS == ("quat", "imu_acc_raw", "imu_gyro_raw", "joint_pos", "joint_vel", "foot_force", "reach", "foot_pos_rel", "foot_vel_rel")


def test_refusals_are_reported_without_a_device(pkg):
    """a null handle is refused first by both entries, with good and with bad arguments (the refusals that need a live handle are checked on the GPU)"""
    lib = pkg.load_library()
    d = lambda k: (C.c_double * k)()
    st, R, foot, grf, ct, fix, opt = d(22), d(9), d(12), d(12), (C.c_uint8 * 4)(), d(20), d(12)
    outs = [d(4), d(3), d(3), d(12), d(12), d(4), (C.c_uint8 * 4)(), d(12), d(12)]
    for n, stride in ((1, 12), (-1, 12), (1, 7)):
        assert lib.a1mpc_sensor_synthesis_batch(None, n, st, stride, R, foot, grf, ct, None, fix, opt, *outs) == 1
        assert b"null handle" in lib.a1mpc_last_error()
        assert lib.a1mpc_sensor_synthesis_batch_device(None, n, None, stride, None, None, None, None, None, fix, opt, *([None] * 9), None) == 1
        assert b"null handle" in lib.a1mpc_last_error()


def test_kernel_is_in_the_code_object_uses_no_scratch_and_is_gated(pkg):
    pkg.build.build()
    res = json.load(open(pkg.build.RESOURCES_PATH))["kernels"]
    isa_check = importlib.import_module(pkg.__name__ + ".isa_check")
    assert KERNEL in isa_check.NO_SCRATCH   # the build's own gate covers it
    assert isa_check.resource_gaps(res, no_scratch=(KERNEL,)) == []
    k = next(v for name, v in res.items() if KERNEL in name)
    print(KERNEL + ":", k)
    assert k["scratch_bytes"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["max_flat_workgroup_size"] == 64 and k["lds_static_bytes"] <= 8192
    spilled = dict(res); spilled["x_" + KERNEL + "_x"] = dict(k, scratch_bytes=16)
    assert isa_check.resource_gaps(spilled, no_scratch=(KERNEL,)) != []   # the gate does fail on a spill
