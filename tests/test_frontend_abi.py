"""CPU: the sensor / command front end at the C ABI -- a1mpc_sensor_frontend_batch(_device), a1mpc_reset_sensor_state, a1mpc_command_batch(_device),
a1mpc_control_tick_sensors_device, a1mpc_balance_wrench_kp_batch(_device) and the two defaults are declared in include/a1mpc.h, exported by liba1mpc.so, listed in
engine.EXPORTS and bound with as many argument types as parameters; the ctypes structs have the header's sizes; the defaults are the reference's constants; every entry
refuses a null handle without a device and names it; the new kernels are in the build's no-scratch gate and clean in its resource record.  The refusals that need a live
handle are checked on the GPU (tests/test_gpu_sensor_frontend.py).  No compute on a GPU (there is none here)."""
import ctypes as C
import importlib
import json
import os
import re
import subprocess
import tempfile

import numpy as np

import frontend_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("a1mpc_default_sensor_config", "a1mpc_default_command_config", "a1mpc_reset_sensor_state", "a1mpc_sensor_frontend_batch", "a1mpc_sensor_frontend_batch_device",
       "a1mpc_command_batch", "a1mpc_command_batch_device", "a1mpc_control_tick_sensors_device", "a1mpc_balance_wrench_kp_batch", "a1mpc_balance_wrench_kp_batch_device")
KERNELS = ("a1mpc_sensor_frontend_kernel", "a1mpc_command_kernel", "a1mpc_balance_wrench_kp_kernel")


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "a1mpc.h")).read(), flags=re.S)


def _params(code, name):
    m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m, f"{name} is not declared in include/a1mpc.h"
    return [re.search(r"(\w+)\s*$", p.strip()).group(1) for p in m.group(1).split(",")]


def test_new_symbols_are_declared_exported_listed_and_bound(pkg):
    pkg.build.build()
    code = _code()
    lib = C.CDLL(pkg.build.LIB_PATH)
    bound = pkg.load_library()
    for name in NEW:
        params = _params(code, name)
        assert hasattr(lib, name), f"{name} is not exported by liba1mpc.so"
        assert name in pkg.engine.EXPORTS
        assert getattr(bound, name).argtypes is not None and len(getattr(bound, name).argtypes) == len(params), name
    strip = lambda ps: [re.sub(r"^d_", "", p) for p in ps]
    for host in ("a1mpc_sensor_frontend_batch", "a1mpc_command_batch", "a1mpc_balance_wrench_kp_batch"):
        assert strip(_params(code, host + "_device")) == _params(code, host) + ["hip_stream"], host
    # the per-robot wrench takes the batch-wide wrench's arguments with kp_linear_xy in front of the arrays
    plain = _params(code, "a1mpc_balance_wrench_batch")
    assert _params(code, "a1mpc_balance_wrench_kp_batch") == plain[:3] + ["kp_linear_xy"] + plain[3:]
    for wrapper in ("sensor_frontend", "sensor_frontend_device", "reset_sensor_state", "command", "command_device", "command_state", "control_tick_sensors_device",
                    "balance_wrench_kp", "balance_wrench_kp_device"):
        assert callable(getattr(pkg.Engine, wrapper)), wrapper
    assert pkg.SensorConfig is pkg.engine.SensorConfig and pkg.CommandConfig is pkg.engine.CommandConfig and pkg.TickSensors is pkg.engine.TickSensors


def test_ctypes_structs_have_the_header_sizes_and_offsets(pkg):
    src = r'''#include <stdio.h>
#include <stddef.h>
#include "a1mpc.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(a1mpc_sensor_config), sizeof(a1mpc_command_config), sizeof(a1mpc_tick_sensors), sizeof(a1mpc_tick_buffers),
           offsetof(a1mpc_command_config, mpc_init_ticks), offsetof(a1mpc_tick_sensors, command), offsetof(a1mpc_tick_sensors, quat),
           offsetof(a1mpc_tick_sensors, mpc_init_counter), A1MPC_IMU_WINDOW_MAX);
    return 0;
}
'''
    with tempfile.TemporaryDirectory(prefix="a1mpc_abi_") as d:
        c = os.path.join(d, "sizes.c"); exe = os.path.join(d, "sizes")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    E = pkg.engine
    want = [C.sizeof(E.SensorConfig), C.sizeof(E.CommandConfig), C.sizeof(E.TickSensors), C.sizeof(E.TickBuffers), E.CommandConfig.mpc_init_ticks.offset,
            E.TickSensors.command.offset, E.TickSensors.quat.offset, E.TickSensors.mpc_init_counter.offset, 64]
    assert got == want, (got, want)
    assert got[3] == len(E.TICK_BUFFER_FIELDS) * C.sizeof(C.c_void_p)   # a1mpc_tick_buffers is what it was: one pointer per field


def test_defaults_are_the_reference_constants(pkg):
    lib = pkg.load_library()
    s = pkg.SensorConfig(); c = pkg.CommandConfig()
    lib.a1mpc_default_sensor_config(C.byref(s)); lib.a1mpc_default_command_config(C.byref(c))
    assert s.imu_window == 5                                                   # MovingWindowFilter(5), S/GazeboA1ROS.cpp:99-104
    assert {k: getattr(c, k) for k in FR.COMMAND_DEFAULTS} == FR.COMMAND_DEFAULTS   # S/A1Params.h:16-17, S/A1CtrlStates.h:273-274, S/GazeboA1ROS.cpp:180, S/A1RobotControl.cpp:294
    lib.a1mpc_default_sensor_config(None); lib.a1mpc_default_command_config(None)   # (like the other defaults: a null pointer is ignored)
    st = pkg.Engine.command_state(3); ref = FR.initial_state(3)
    assert list(st) == list(FR.STATE_KEYS) == list(pkg.engine.COMMAND_STATE_FIELDS)
    for k in FR.STATE_KEYS:
        assert st[k].dtype == ref[k].dtype and np.array_equal(st[k], ref[k]), k


def test_every_new_entry_refuses_a_null_handle_without_a_device(pkg):
    lib = pkg.load_library()
    E = pkg.engine
    s = E.SensorConfig(); lib.a1mpc_default_sensor_config(C.byref(s))
    c = E.CommandConfig(); lib.a1mpc_default_command_config(C.byref(c))
    g = E.BalanceGains(); lib.a1mpc_default_balance_gains(C.byref(g))
    prm = E.TickParams(); lib.a1mpc_default_tick_params(C.byref(prm))
    ts = E.TickSensors(); bf = E.TickBuffers()
    for n in (1, 0, -1):
        calls = [lib.a1mpc_sensor_frontend_batch(None, C.byref(s), n, *([None] * 9)),
                 lib.a1mpc_sensor_frontend_batch_device(None, C.byref(s), n, *([None] * 9), None),
                 lib.a1mpc_command_batch(None, C.byref(c), n, None, None, None, 0.0025, *([None] * 11)),
                 lib.a1mpc_command_batch_device(None, C.byref(c), n, None, None, None, 0.0025, *([None] * 11), None),
                 lib.a1mpc_control_tick_sensors_device(None, C.byref(prm), C.byref(ts), C.byref(bf), n, None),
                 lib.a1mpc_balance_wrench_kp_batch(None, C.byref(g), n, *([None] * 11)),
                 lib.a1mpc_balance_wrench_kp_batch_device(None, C.byref(g), n, *([None] * 11), None),
                 lib.a1mpc_reset_sensor_state(None)]
        assert calls == [1] * len(calls), (n, calls)
        assert b"null handle" in lib.a1mpc_last_error()


def test_new_kernels_are_gated_and_use_no_scratch(pkg):
    pkg.build.build()
    res = json.load(open(pkg.build.RESOURCES_PATH))["kernels"]
    isa_check = importlib.import_module(pkg.__name__ + ".isa_check")
    for name in KERNELS:
        assert name in isa_check.NO_SCRATCH, name
    assert isa_check.resource_gaps(res, no_scratch=KERNELS) == []
    for name in KERNELS:
        k = next(v for key, v in res.items() if name in key)
        print(name, k)
        assert k["scratch_bytes"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch_instrs"] == 0
        assert k["lds_static_bytes"] == 0 and k["max_flat_workgroup_size"] == 256   # one lane per robot, workgroups of 256, no LDS
    assert next(v for key, v in res.items() if "a1mpc_sensor_frontend_kernel" in key)["vgpr"] <= 256   # two waves per SIMD at the least (the four libm calls set the count)
    # the batch-wide wrench kernel is still there beside its per-robot twin, under its own name
    assert sum("a1mpc_balance_wrench_kernel" in key for key in res) == 1 and sum("a1mpc_balance_wrench_kp_kernel" in key for key in res) == 1
