"""CPU: sensor noise and IMU bias at the C ABI -- a1mpc_default_noise_config and a1mpc_sensor_noise_batch(_device) are declared in include/a1mpc.h with the parameters the
header's block names, exported by liba1mpc.so (and nothing else of theirs is), listed in engine.EXPORTS and bound with argument types; the configuration's layout and
defaults; the engine wrappers' signatures; the refusal that needs no device (a null handle comes first, with good and with bad arguments; the ones that need a live
handle, the poisoned arrays and n = 0 are checked on the GPU: tests/test_gpu_noise.py); the kernel is in the code object, uses no scratch memory and is covered by the
build's gate.  No compute on a GPU."""
import ctypes as C
import importlib
import inspect
import json
import os
import re
import subprocess

import numpy as np

import noise_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("a1mpc_default_noise_config", "a1mpc_sensor_noise_batch", "a1mpc_sensor_noise_batch_device")
KERNEL = "a1mpc_sensor_noise_kernel"
ARRAYS = ["quat", "imu_acc_raw", "imu_gyro_raw", "joint_pos", "joint_vel", "foot_force", "imu_bias", "z_out"]


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "a1mpc.h")).read(), flags=re.S)


def _params(code, name):
    m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m, f"{name} is not declared in include/a1mpc.h"
    return [(re.sub(r"\s*\w+\s*$", "", p.strip()), re.search(r"(\w+)\s*$", p.strip()).group(1)) for p in m.group(1).split(",")]


def test_symbols_are_declared_exported_listed_and_bound(pkg):
    pkg.build.build()
    code = _code()
    lib = C.CDLL(pkg.build.LIB_PATH)
    bound = pkg.load_library()
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported by liba1mpc.so"
        assert name in pkg.engine.EXPORTS
        assert len(getattr(bound, name).argtypes) == len(_params(code, name)), name
    assert bound.a1mpc_default_noise_config.restype is None and bound.a1mpc_sensor_noise_batch.restype is C.c_int and bound.a1mpc_sensor_noise_batch_device.restype is C.c_int
    head = [("a1mpc_handle", "h"), ("const a1mpc_noise_config*", "cfg"), ("int32_t", "n"), ("uint64_t", "robot0"), ("uint64_t", "tick")]
    assert _params(code, "a1mpc_sensor_noise_batch") == head + [("double*", k) for k in ARRAYS]   # (in place: none of them const)
    assert _params(code, "a1mpc_sensor_noise_batch_device") == head + [("double*", "d_" + k) for k in ARRAYS] + [("void*", "hip_stream")]
    for f in (bound.a1mpc_sensor_noise_batch, bound.a1mpc_sensor_noise_batch_device):
        assert f.argtypes[3] is C.c_uint64 and f.argtypes[4] is C.c_uint64   # (by value, 64 bits)
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.build.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in nm.splitlines() if re.search(r" [TW] a1mpc_\w*noise", l))
    assert exported == sorted(NEW), exported


def test_the_configuration(pkg):
    """the header's struct, field for field, and its defaults: seed 0 and every level +0 (off), whatever the memory held"""
    code = _code()
    m = re.search(r"typedef struct a1mpc_noise_config \{(.*?)\} a1mpc_noise_config;", code, flags=re.S)
    assert m
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ty, names = decl.split(None, 1)
            fields += [(ty, k.strip()) for k in names.split(",")]
    ctype = {"uint64_t": C.c_uint64, "double": C.c_double}
    assert [(k, t) for k, t in pkg.engine.NoiseConfig._fields_] == [(k, ctype[ty]) for ty, k in fields]
    assert [k for _, k in fields] == ["seed"] + list(NR.LEVELS) and C.sizeof(pkg.engine.NoiseConfig) == 72
    lib = pkg.load_library()
    nc = pkg.engine.NoiseConfig()
    C.memset(C.byref(nc), 0xFF, C.sizeof(nc))
    lib.a1mpc_default_noise_config(C.byref(nc))
    assert bytes(nc) == bytes(72)
    lib.a1mpc_default_noise_config(None)   # (a null pointer is ignored)


def test_the_engine_wrappers(pkg):
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()][1:]
    N = inspect.Parameter.empty
    assert [k for k, _ in sig(pkg.Engine.noise_config)] == ["fields"]
    assert sig(pkg.Engine.sensor_noise) == [("noise", N), ("tick", N)] + [(k, None) for k in ARRAYS[:7]] + [("robot0", 0), ("want_z", False)]
    assert sig(pkg.Engine.sensor_noise_device) == [("noise", N), ("n", N), ("tick", N)] + [("d_" + k, None) for k in ARRAYS[:7]] + [("d_z", None), ("robot0", 0), ("stream", None)]
    assert pkg.NoiseConfig is pkg.engine.NoiseConfig and tuple(pkg.engine.NOISE_SENSORS) == NR.SENSORS and pkg.engine.NOISE_WIDTHS == NR.WIDTHS


def test_a_null_handle_is_refused_first_without_a_device(pkg):
    """both entries, with good and with bad arguments (a negative n, a NaN sigma, a walk without a bias, robot0 + n beyond 2^32, two arrays that are one): status 1,
    `null handle` named, and the poisoned arrays keep their bits"""
    lib = pkg.load_library()
    n = 4
    arr = {k: np.full((n, NR.WIDTHS.get(k, 44)), np.nan) for k in ARRAYS}
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    v = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    good = dict(NR.NOMINAL)
    cases = [(good, n, 0, {}), (good, -1, 0, {}), (dict(good, gyro_sigma=float("nan")), n, 0, {}), (dict(good, foot_force_sigma=-1.0), n, 0, {}),
             (good, n, 0, dict(imu_bias=None)), (good, n, 2 ** 32 - 3, {}), (good, n, 0, dict(joint_vel=arr["joint_pos"])), (None, n, 0, {})]
    for cfg, n_, robot0, swap in cases:
        nc = None
        if cfg is not None:
            nc = pkg.engine.NoiseConfig(); lib.a1mpc_default_noise_config(C.byref(nc))
            for k, val in cfg.items():
                setattr(nc, k, val)
        a = dict(arr, **swap)
        ref = None if nc is None else C.byref(nc)
        assert lib.a1mpc_sensor_noise_batch(None, ref, n_, robot0, 7, *[p(a[k]) for k in ARRAYS]) == 1
        assert b"null handle" in lib.a1mpc_last_error()
        assert lib.a1mpc_sensor_noise_batch_device(None, ref, n_, robot0, 7, *[v(a[k]) for k in ARRAYS], None) == 1
        assert b"null handle" in lib.a1mpc_last_error()
    assert all(np.isnan(a).all() for a in arr.values())


def test_the_kernel_is_in_the_code_object_uses_no_scratch_and_is_gated(pkg):
    pkg.build.build()
    res = json.load(open(pkg.build.RESOURCES_PATH))["kernels"]
    isa_check = importlib.import_module(pkg.__name__ + ".isa_check")
    assert KERNEL in isa_check.NO_SCRATCH   # the build's own gate covers it
    assert isa_check.resource_gaps(res, no_scratch=(KERNEL,)) == []
    hits = [v for k, v in res.items() if KERNEL in k]
    assert len(hits) == 1
    k = hits[0]
    print(KERNEL + ":", k)
    assert k["scratch_bytes"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["max_flat_workgroup_size"] == 64 and k["lds_static_bytes"] == 16 * 44 * 8
    assert k["vgpr"] <= 128   # (four waves per SIMD at the least)
    spilled = dict(res); spilled["x_" + KERNEL + "_x"] = dict(k, scratch_bytes=16)
    assert isa_check.resource_gaps(spilled, no_scratch=(KERNEL,)) != []   # the gate does fail on a spill
    # the sensor kernels beside it are still found under their own names alone
    for other in ("a1mpc_sensor_synthesis_kernel", "a1mpc_walk_sensors_kernel", "a1mpc_walk_sensors_touch_kernel", "a1mpc_sensor_frontend_kernel"):
        assert len([key for key in res if other in key]) == 1, other
