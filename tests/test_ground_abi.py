"""CPU: sloped ground and sensed touchdowns at the C ABI -- a1mpc_ground_step_batch(_device) and a1mpc_touch_sensors_batch(_device) are declared in include/a1mpc.h
with the walk entries' parameters and the new ones where the header says, exported by liba1mpc.so (and nothing else of theirs is), listed in engine.EXPORTS and bound
with argument types; the engine wrappers' signatures; the refusals that need no device (the ones that need a live handle, the poisoned outputs and n = 0 are checked on
the GPU: tests/test_gpu_ground.py); both kernels are in the code object, use no scratch memory and are covered by the build's gate.  No compute on a GPU."""
import ctypes as C
import importlib
import inspect
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("a1mpc_ground_step_batch", "a1mpc_ground_step_batch_device", "a1mpc_touch_sensors_batch", "a1mpc_touch_sensors_batch_device")
KERNELS = ("a1mpc_walk_step_ground_kernel", "a1mpc_walk_sensors_touch_kernel")


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
        assert getattr(bound, name).restype is C.c_int
    for d in ("", "d_"):
        suffix = "_device" if d else ""
        # the step: the walk step's parameters with ground after foot_target and touch_out after foot_vel_body_out
        walk, ground = _params(code, "a1mpc_walk_step_batch" + suffix), _params(code, "a1mpc_ground_step_batch" + suffix)
        i, j = walk.index(d + "foot_target") + 1, walk.index(d + "foot_vel_body_out") + 1
        assert ground == walk[:i] + [d + "ground"] + walk[i:j] + [d + "touch_out"] + walk[j:], ground
        # the sensors: the walk sensors' parameters with touch and touch_force after foot_vel_body
        walk, touch = _params(code, "a1mpc_walk_sensors_batch" + suffix), _params(code, "a1mpc_touch_sensors_batch" + suffix)
        k = walk.index(d + "foot_vel_body") + 1
        assert touch == walk[:k] + [d + "touch", "touch_force"] + walk[k:], touch
    assert bound.a1mpc_touch_sensors_batch.argtypes[11] is C.c_double and bound.a1mpc_touch_sensors_batch_device.argtypes[11] is C.c_double   # (by value)
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.build.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in nm.splitlines() if re.search(r" [TW] a1mpc_\w*(ground|touch)", l))
    assert exported == sorted(NEW), exported


def test_the_engine_wrappers(pkg):
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()][1:]
    N = inspect.Parameter.empty
    assert sig(pkg.Engine.walk_step_ground) == [("state", N), ("R", N), ("foot", N), ("grf", N), ("contacts", N), ("R_z", None), ("foot_target", None), ("ground", None),
                                                ("ext_wrench", None), ("walk", None)]
    assert sig(pkg.Engine.walk_step_ground_device) == [("n", N), ("d_state", N), ("state_stride", N), ("d_R", N), ("d_foot", N), ("d_grf", N), ("d_contacts", N), ("d_R_z", N),
                                                       ("d_foot_target", N), ("d_foot_vel_body", N), ("d_touch", N), ("d_ground", None), ("d_ext_wrench", None),
                                                       ("d_state_out", None), ("d_R_out", None), ("d_foot_out", None), ("walk", None), ("stream", None)]
    assert [k for k, _ in sig(pkg.Engine.walk_sensors_touch)][:8] == ["state", "R", "foot", "grf", "contacts", "foot_vel_body", "touch", "touch_force"]
    names = [k for k, _ in sig(pkg.Engine.walk_sensors_touch_device)]
    assert "d_touch" in names and "touch_force" in names and dict(sig(pkg.Engine.walk_sensors_touch_device))["touch_force"] == 0.0


def test_refusals_are_reported_without_a_device(pkg):
    """a null handle is refused first by all four entries, with good and with bad arguments"""
    lib = pkg.load_library()
    wc = pkg.engine.WalkConfig(); lib.a1mpc_default_walk_config(C.byref(wc))
    d = lambda k: (C.c_double * k)()
    st, R, foot, grf, ct, vel, gr, tc = d(22), d(9), d(12), d(12), (C.c_uint8 * 4)(), d(12), d(3), (C.c_uint8 * 4)()
    for n, stride, force in ((1, 12, 60.0), (-1, 12, 60.0), (1, 7, 60.0), (1, 12, -1.0), (1, 12, float("nan"))):
        assert lib.a1mpc_ground_step_batch(None, C.byref(wc), n, st, stride, R, foot, grf, ct, None, R, foot, gr, st, R, foot, vel, tc) == 1
        assert b"null handle" in lib.a1mpc_last_error()
        assert lib.a1mpc_ground_step_batch_device(None, C.byref(wc), n, None, stride, *([None] * 14)) == 1
        assert b"null handle" in lib.a1mpc_last_error()
        assert lib.a1mpc_touch_sensors_batch(None, n, st, stride, R, foot, grf, ct, None, vel, tc, force, d(20), d(12), d(4), d(3), d(3), d(12), d(12), d(4), ct, None, None) == 1
        assert b"null handle" in lib.a1mpc_last_error()
        assert lib.a1mpc_touch_sensors_batch_device(None, n, None, stride, *([None] * 7), force, d(20), d(12), *([None] * 10)) == 1
        assert b"null handle" in lib.a1mpc_last_error()
    assert lib.a1mpc_ground_step_batch(None, None, 1, st, 12, R, foot, grf, ct, None, R, foot, gr, st, R, foot, vel, tc) == 1


def test_kernels_are_in_the_code_object_use_no_scratch_and_are_gated(pkg):
    pkg.build.build()
    res = json.load(open(pkg.build.RESOURCES_PATH))["kernels"]
    isa_check = importlib.import_module(pkg.__name__ + ".isa_check")
    for name in KERNELS:
        assert name in isa_check.NO_SCRATCH   # the build's own gate covers it
        assert isa_check.resource_gaps(res, no_scratch=(name,)) == []
        hits = [v for k, v in res.items() if name in k]
        assert len(hits) == 1, name
        k = hits[0]
        print(name + ":", k)
        assert k["scratch_bytes"] == 0 and k["vgpr_spill"] == 0 and k["max_flat_workgroup_size"] == 64 and k["lds_static_bytes"] <= 8192
        spilled = dict(res); spilled["x_" + name + "_x"] = dict(k, scratch_bytes=16)
        assert isa_check.resource_gaps(spilled, no_scratch=(name,)) != []   # the gate does fail on a spill
    # the walk kernels beside them are still found under their own names alone
    assert len([k for k in res if "a1mpc_walk_step_kernel" in k]) == 1 and len([k for k in res if "a1mpc_walk_sensors_kernel" in k]) == 1
