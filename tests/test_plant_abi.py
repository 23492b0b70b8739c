"""CPU: the plant step at the C ABI -- a1mpc_default_plant_config, a1mpc_plant_step_batch and a1mpc_plant_step_batch_device are declared in include/a1mpc.h, exported by
liba1mpc.so (and nothing else of the plant is), listed in engine.EXPORTS and bound with argument types; the defaults; the engine wrappers' signatures; the refusals that
need no device; the kernel is in the code object, uses no scratch memory and is covered by the build's gate.  No compute on a GPU (there is none here)."""
import ctypes as C
import importlib
import inspect
import json
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("a1mpc_default_plant_config", "a1mpc_plant_step_batch", "a1mpc_plant_step_batch_device")
HOST_ARGS = ["h", "cfg", "n", "state_in", "state_stride", "R_world", "foot_abs", "grf_body", "contacts", "ext_wrench", "state_out", "R_world_out", "foot_abs_out"]


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
    assert _params(code, "a1mpc_plant_step_batch") == HOST_ARGS
    dev = _params(code, "a1mpc_plant_step_batch_device")
    assert [re.sub(r"^d_", "", p) for p in dev] == HOST_ARGS + ["hip_stream"]
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.build.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in nm.splitlines() if re.search(r" T a1mpc_\w*plant", l))
    assert exported == sorted(NEW), exported   # the header and the exports name the same three
    assert re.search(r"typedef struct a1mpc_plant_config \{ double dt; int32_t substeps; double gravity_z; \} a1mpc_plant_config;", code)


def test_defaults_and_the_engine_wrappers(pkg):
    lib = pkg.load_library()
    pc = pkg.engine.PlantConfig(dt=-1.0, substeps=-1, gravity_z=0.0)
    lib.a1mpc_default_plant_config(C.byref(pc))
    assert (pc.dt, pc.substeps, pc.gravity_z) == (0.0025, 1, -9.8)
    lib.a1mpc_default_plant_config(None)   # (a null pointer is ignored, like the other defaults)
    assert [f[0] for f in pkg.engine.PlantConfig._fields_] == ["dt", "substeps", "gravity_z"] and C.sizeof(pkg.engine.PlantConfig) == 24
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()][1:]
    E = inspect.Parameter.empty
    assert sig(pkg.Engine.plant_step) == [("state", E), ("R", E), ("foot", E), ("grf", E), ("contacts", E), ("ext_wrench", None), ("plant", None)]
    assert sig(pkg.Engine.plant_step_device) == [("n", E), ("d_state", E), ("state_stride", E), ("d_R", E), ("d_foot", E), ("d_grf", E), ("d_contacts", E), ("d_ext_wrench", None),
                                                 ("d_state_out", None), ("d_R_out", None), ("d_foot_out", None), ("plant", None), ("stream", None)]
    assert [k for k, _ in sig(pkg.Engine.plant_config)] == ["fields"]


def test_refusals_are_reported_without_a_device(pkg):
    """a null handle is refused first by both entries, with good and with bad arguments (the refusals that need a live handle are checked on the GPU)"""
    lib = pkg.load_library()
    pc = pkg.engine.PlantConfig(); lib.a1mpc_default_plant_config(C.byref(pc))
    d = lambda k: (C.c_double * k)()
    st, R, foot, grf, ct = d(22), d(9), d(12), d(12), (C.c_uint8 * 4)()
    for n, stride in ((1, 12), (-1, 12), (1, 7)):
        assert lib.a1mpc_plant_step_batch(None, C.byref(pc), n, st, stride, R, foot, grf, ct, None, st, R, foot) == 1
        assert b"null handle" in lib.a1mpc_last_error()
        assert lib.a1mpc_plant_step_batch_device(None, C.byref(pc), n, None, stride, None, None, None, None, None, None, None, None, None) == 1
        assert b"null handle" in lib.a1mpc_last_error()
    assert lib.a1mpc_plant_step_batch(None, None, 1, st, 12, R, foot, grf, ct, None, st, R, foot) == 1


def test_kernel_is_in_the_code_object_uses_no_scratch_and_is_gated(pkg):
    pkg.build.build()
    res = json.load(open(pkg.build.RESOURCES_PATH))["kernels"]
    isa_check = importlib.import_module(pkg.__name__ + ".isa_check")
    assert "a1mpc_plant_step_kernel" in isa_check.NO_SCRATCH   # the build's own gate covers it
    assert isa_check.resource_gaps(res, no_scratch=("a1mpc_plant_step_kernel",)) == []
    k = next(v for name, v in res.items() if "a1mpc_plant_step_kernel" in name)
    print("a1mpc_plant_step_kernel:", k)
    assert k["scratch_bytes"] == 0 and k["vgpr_spill"] == 0 and k["max_flat_workgroup_size"] == 64 and k["lds_static_bytes"] <= 8192
    spilled = dict(res); spilled["x_a1mpc_plant_step_kernel_x"] = dict(k, scratch_bytes=16)
    assert isa_check.resource_gaps(spilled, no_scratch=("a1mpc_plant_step_kernel",)) != []   # the gate does fail on a spill
