"""CPU: the walking plant at the C ABI -- a1mpc_default_walk_config, a1mpc_walk_step_batch(_device) and a1mpc_walk_sensors_batch(_device) are declared in
include/a1mpc.h, exported by liba1mpc.so, listed in engine.EXPORTS and bound with argument types; the struct and its defaults; the engine wrappers' signatures; the
refusals that need no device; both kernels are in the code object, use no scratch memory and are covered by the build's gate.  No compute on a GPU (there is none here)."""
import ctypes as C
import importlib
import inspect
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("a1mpc_default_walk_config", "a1mpc_walk_step_batch", "a1mpc_walk_step_batch_device", "a1mpc_walk_sensors_batch", "a1mpc_walk_sensors_batch_device")
STEP_ARGS = ["h", "cfg", "n", "state_in", "state_stride", "R_world", "foot_abs", "grf_body", "contacts", "ext_wrench", "R_z", "foot_target", "state_out", "R_world_out",
             "foot_abs_out", "foot_vel_body_out"]
KERNELS = ("a1mpc_walk_step_kernel", "a1mpc_walk_sensors_kernel")


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "a1mpc.h")).read(), flags=re.S)


def _params(code, name):
    m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m, f"{name} is not declared in include/a1mpc.h"
    return [re.search(r"(\w+)\s*$", p.strip()).group(1) for p in m.group(1).split(",")]


def test_symbols_are_declared_exported_and_listed(pkg):
    pkg.build.build()
    code = _code()
    lib = C.CDLL(pkg.build.LIB_PATH)
    bound = pkg.load_library()
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported by liba1mpc.so"
        assert name in pkg.engine.EXPORTS
        assert len(getattr(bound, name).argtypes) == len(_params(code, name)), name
    assert _params(code, "a1mpc_walk_step_batch") == STEP_ARGS
    assert [re.sub(r"^d_", "", p) for p in _params(code, "a1mpc_walk_step_batch_device")] == STEP_ARGS + ["hip_stream"]
    # the sensors: the synthesis's parameters with foot_vel_body after ext_wrench, in both entries
    for suffix in ("", "_device"):
        syn, walk = _params(code, "a1mpc_sensor_synthesis_batch" + suffix), _params(code, "a1mpc_walk_sensors_batch" + suffix)
        k = syn.index("d_ext_wrench" if suffix else "ext_wrench") + 1
        assert walk == syn[:k] + ["d_foot_vel_body" if suffix else "foot_vel_body"] + syn[k:], walk
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.build.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in nm.splitlines() if re.search(r" T a1mpc_\w*walk", l))
    assert exported == sorted(NEW), exported
    assert not any("plant" in s or "synthesis" in s for s in NEW)   # (tests/test_plant_abi.py and tests/test_sensor_synthesis_abi.py list those families whole)
    assert re.search(r"typedef struct a1mpc_walk_config \{ a1mpc_plant_config plant; double swing_track; int32_t flat_ground; double ground_z; \} a1mpc_walk_config;", code)


def test_struct_defaults_and_the_engine_wrappers(pkg):
    lib = pkg.load_library()
    E = pkg.engine
    wc = E.WalkConfig(plant=E.PlantConfig(dt=-1.0, substeps=-1, gravity_z=0.0), swing_track=-1.0, flat_ground=7, ground_z=3.0)
    lib.a1mpc_default_walk_config(C.byref(wc))
    assert (wc.plant.dt, wc.plant.substeps, wc.plant.gravity_z, wc.swing_track, wc.flat_ground, wc.ground_z) == (0.0025, 1, -9.8, 1.0, 0, 0.0)
    lib.a1mpc_default_walk_config(None)   # (a null pointer is ignored, like the other defaults)
    assert [f[0] for f in E.WalkConfig._fields_] == ["plant", "swing_track", "flat_ground", "ground_z"] and C.sizeof(E.WalkConfig) == 48
    pc = E.PlantConfig(); lib.a1mpc_default_plant_config(C.byref(pc))
    assert (pc.dt, pc.substeps, pc.gravity_z) == (0.0025, 1, -9.8)
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()][1:]
    N = inspect.Parameter.empty
    assert sig(pkg.Engine.walk_step) == [("state", N), ("R", N), ("foot", N), ("grf", N), ("contacts", N), ("R_z", None), ("foot_target", None), ("ext_wrench", None),
                                         ("walk", None)]
    assert sig(pkg.Engine.walk_step_device) == [("n", N), ("d_state", N), ("state_stride", N), ("d_R", N), ("d_foot", N), ("d_grf", N), ("d_contacts", N), ("d_R_z", N),
                                                ("d_foot_target", N), ("d_foot_vel_body", N), ("d_ext_wrench", None), ("d_state_out", None), ("d_R_out", None),
                                                ("d_foot_out", None), ("walk", None), ("stream", None)]
    assert [k for k, _ in sig(pkg.Engine.walk_sensors)][:6] == ["state", "R", "foot", "grf", "contacts", "foot_vel_body"]
    assert "d_foot_vel_body" in [k for k, _ in sig(pkg.Engine.walk_sensors_device)] and [k for k, _ in sig(pkg.Engine.walk_config)] == ["fields"]


def test_refusals_are_reported_without_a_device(pkg):
    """a null handle is refused first by all four entries, with good and with bad arguments (the refusals that need a live handle are checked on the GPU)"""
    lib = pkg.load_library()
    wc = pkg.engine.WalkConfig(); lib.a1mpc_default_walk_config(C.byref(wc))
    d = lambda k: (C.c_double * k)()
    st, R, foot, grf, ct, vel = d(22), d(9), d(12), d(12), (C.c_uint8 * 4)(), d(12)
    for n, stride in ((1, 12), (-1, 12), (1, 7)):
        assert lib.a1mpc_walk_step_batch(None, C.byref(wc), n, st, stride, R, foot, grf, ct, None, R, foot, st, R, foot, vel) == 1
        assert b"null handle" in lib.a1mpc_last_error()
        assert lib.a1mpc_walk_step_batch_device(None, C.byref(wc), n, None, stride, *([None] * 12)) == 1
        assert b"null handle" in lib.a1mpc_last_error()
        assert lib.a1mpc_walk_sensors_batch(None, n, st, stride, R, foot, grf, ct, None, vel, d(20), d(12), d(4), d(3), d(3), d(12), d(12), d(4), ct, None, None) == 1
        assert b"null handle" in lib.a1mpc_last_error()
        assert lib.a1mpc_walk_sensors_batch_device(None, n, None, stride, *([None] * 6), d(20), d(12), *([None] * 10)) == 1
        assert b"null handle" in lib.a1mpc_last_error()
    assert lib.a1mpc_walk_step_batch(None, None, 1, st, 12, R, foot, grf, ct, None, R, foot, st, R, foot, vel) == 1


def test_kernels_are_in_the_code_object_use_no_scratch_and_are_gated(pkg):
    pkg.build.build()
    res = json.load(open(pkg.build.RESOURCES_PATH))["kernels"]
    isa_check = importlib.import_module(pkg.__name__ + ".isa_check")
    for name in KERNELS:
        assert name in isa_check.NO_SCRATCH   # the build's own gate covers it
        assert "a1mpc_plant_step_kernel" not in name and "a1mpc_sensor_synthesis_kernel" not in name
        assert isa_check.resource_gaps(res, no_scratch=(name,)) == []
        hits = [v for k, v in res.items() if name in k]
        assert len(hits) == 1, name
        k = hits[0]
        print(name + ":", k)
        assert k["scratch_bytes"] == 0 and k["vgpr_spill"] == 0 and k["max_flat_workgroup_size"] == 64 and k["lds_static_bytes"] <= 8192
        spilled = dict(res); spilled["x_" + name + "_x"] = dict(k, scratch_bytes=16)
        assert isa_check.resource_gaps(spilled, no_scratch=(name,)) != []   # the gate does fail on a spill
    # the two kernels beside them are still found under their own names alone
    assert len([k for k in res if "a1mpc_plant_step_kernel" in k]) == 1 and len([k for k in res if "a1mpc_sensor_synthesis_kernel" in k]) == 1
