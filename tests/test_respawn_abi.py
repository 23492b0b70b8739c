"""CPU: the respawn family at the C ABI -- a1mpc_default_respawn_config, a1mpc_respawn_reset_batch(_device), a1mpc_respawn_batch(_device) and
a1mpc_respawn_rows_device are declared in include/a1mpc.h with the parameters the header's block names, exported by liba1mpc.so (and nothing else of theirs is),
listed in engine.EXPORTS and bound with argument types; the two structs' layouts and the defaults; the engine's wrappers; the refusal that needs no device (a null
handle comes first, with good and with bad arguments; the ones that need a live handle are checked on the GPU: tests/test_gpu_respawn.py); both kernels are in the code
object once each, use neither scratch memory nor LDS and are covered by the build's gate.  No compute on a GPU."""
import ctypes as C
import importlib
import inspect
import json
import os
import re
import subprocess

import numpy as np

import respawn_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("a1mpc_default_respawn_config", "a1mpc_respawn_reset_batch", "a1mpc_respawn_reset_batch_device", "a1mpc_respawn_batch", "a1mpc_respawn_batch_device",
       "a1mpc_respawn_rows_device")
KERNELS = ("a1mpc_respawn_kernel", "a1mpc_respawn_rows_kernel")
OTHER_WORDS = ("plant", "synthesis", "walk", "ground", "touch", "noise", "episode")


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
        assert getattr(bound, name).restype is (None if name == NEW[0] else C.c_int)
    h, n = ("a1mpc_handle", "h"), ("int32_t", "n")
    cfg = ("const a1mpc_respawn_config*", "cfg")
    assert _params(code, "a1mpc_respawn_reset_batch") == [h, n, ("const uint8_t*", "mask"), ("uint32_t", "what")]
    assert _params(code, "a1mpc_respawn_reset_batch_device") == [h, n, ("const uint8_t*", "d_mask"), ("uint32_t", "what"), ("void*", "hip_stream")]
    tail = [("double*", "episode"), ("int32_t*", "life"), ("double*", "finished_out"), ("uint8_t*", "mask_out")]
    assert _params(code, "a1mpc_respawn_batch") == [h, cfg, n] + tail
    assert _params(code, "a1mpc_respawn_batch_device") == [h, cfg, n] + [(t, "d_" + k) for t, k in tail] + [("void*", "hip_stream")]
    assert _params(code, "a1mpc_respawn_rows_device") == [h, n, ("const uint8_t*", "d_mask"), ("const a1mpc_respawn_rows*", "rows"), ("int32_t", "n_rows"),
                                                          ("void*", "hip_stream")]
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.build.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in nm.splitlines() if re.search(r" [TW] a1mpc_\w*respawn", l))   # (the C symbols; a kernel's host stub is a mangled C++ name)
    assert exported == sorted(NEW), exported
    # the closed symbol lists of the other families match on these substrings: no name of this family may carry one
    assert not [name for name in NEW + KERNELS for word in OTHER_WORDS if word in name]
    for word, value in (("EKF", 1), ("CONTACT", 2), ("SENSOR", 4), ("WARM", 8), ("ROWS_MAX", 16)):
        m = re.search(r"#define A1MPC_RESPAWN_" + word + r" (\d+)u?\s", code)
        assert m and int(m.group(1)) == value == getattr(pkg.engine, "RESPAWN_" + word)
    assert (RR.EKF, RR.CONTACT, RR.SENSOR, RR.WARM, RR.ROWS_MAX) == (1, 2, 4, 8, 16)


def test_the_structs_and_the_defaults(pkg):
    """the header's structs, field for field, against the engine's and the restatement's; the defaults whatever the memory held"""
    code = _code()
    E = pkg.engine
    ctype = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int32_t": C.c_int32, "void*": C.c_void_p, "const void*": C.c_void_p}
    for name, cls, want, size in (("a1mpc_respawn_config", E.RespawnConfig, RR.FIELDS, 24), ("a1mpc_respawn_rows", E.RespawnRows, RR.ROWS_FIELDS, 32)):
        m = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", code, flags=re.S)
        assert m, name
        fields = [(re.sub(r"\s*\w+$", "", d.strip()), re.search(r"(\w+)$", d.strip()).group(1)) for d in m.group(1).split(";") if d.strip()]
        assert tuple(fields) == want
        assert [(k, t) for k, t in cls._fields_] == [(k, ctype[t]) for t, k in fields] and C.sizeof(cls) == size
    lib = pkg.load_library()
    rc = E.RespawnConfig()
    C.memset(C.byref(rc), 0xFF, C.sizeof(rc))
    lib.a1mpc_default_respawn_config(C.byref(rc))
    assert dict(codes=rc.codes, max_ticks=rc.max_ticks, hold_ticks=rc.hold_ticks, what=rc.what) == RR.DEFAULT == dict(codes=0xE, max_ticks=0, hold_ticks=10, what=0xF)
    assert bytes(rc) == bytes(E.RespawnConfig(0xE, 0, 10, 0xF))   # (the padding too)
    lib.a1mpc_default_respawn_config(None)   # (a null pointer is ignored)
    assert pkg.RespawnConfig is E.RespawnConfig and pkg.RespawnRows is E.RespawnRows
    import sensor_loop
    assert RR.DEFAULT["hold_ticks"] == sensor_loop.PRIME


def test_the_engine_wrappers(pkg):
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()][1:]
    N = inspect.Parameter.empty
    assert [k for k, _ in sig(pkg.Engine.respawn_config)] == ["fields"]
    assert sig(pkg.Engine.respawn_reset) == [("mask", N), ("what", 15)]
    assert sig(pkg.Engine.respawn_reset_device) == [("n", N), ("d_mask", N), ("what", 15), ("stream", None)]
    assert sig(pkg.Engine.respawn) == [("episode", N), ("life", N), ("finished", None), ("config", None)]
    assert sig(pkg.Engine.respawn_device) == [("n", N), ("d_episode", N), ("d_life", N), ("d_mask", N), ("d_finished", None), ("config", None), ("stream", None)]
    assert sig(pkg.Engine.respawn_rows_device) == [("n", N), ("d_mask", N), ("rows", N), ("stream", None)]


def test_a_null_handle_is_refused_first_without_a_device(pkg):
    """all five entries, with good and with bad arguments: status 1, `null handle` named, and the arrays keep their bits"""
    lib = pkg.load_library()
    E = pkg.engine
    n = 4
    ep = np.full((n, 16), np.nan); life = np.full((n, 2), 7, dtype=np.int32); fin = np.full((n, 16), np.nan); mask = np.full(n, 9, dtype=np.uint8)
    dp, ip, bp = (lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))), (
        lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8)))
    v = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    good = E.RespawnConfig(0xE, 0, 10, 0xF)
    for n_, m, what in ((n, mask, 15), (-1, mask, 15), (n, None, 15), (n, mask, 16)):
        assert lib.a1mpc_respawn_reset_batch(None, n_, bp(m), what) == 1 and b"null handle" in lib.a1mpc_last_error()
        assert lib.a1mpc_respawn_reset_batch_device(None, n_, v(m), what, None) == 1 and b"null handle" in lib.a1mpc_last_error()
    for cfg, n_, e, l, f, m in ((good, n, ep, life, fin, mask), (None, n, ep, life, fin, mask), (good, -1, ep, life, None, mask), (E.RespawnConfig(1, 0, 10, 15), n, ep, life, fin, mask),
                                (E.RespawnConfig(0xE, 2 ** 53, -1, 31), n, ep, life, fin, mask), (good, n, None, None, None, None), (good, n, ep, life, ep, mask)):
        ref = None if cfg is None else C.byref(cfg)
        assert lib.a1mpc_respawn_batch(None, ref, n_, dp(e), ip(l), dp(f), bp(m)) == 1 and b"null handle" in lib.a1mpc_last_error()
        assert lib.a1mpc_respawn_batch_device(None, ref, n_, v(e), v(l), v(f), v(m), None) == 1 and b"null handle" in lib.a1mpc_last_error()
    table = (E.RespawnRows * 2)(E.RespawnRows(ep.ctypes.data, fin.ctypes.data, 128, n, 3), E.RespawnRows(None, None, 0, 0, 0))
    for n_, m, t, k in ((n, mask, table, 1), (n, mask, table, 2), (n, mask, None, 0), (n, None, table, 1), (-1, mask, table, 17)):
        assert lib.a1mpc_respawn_rows_device(None, n_, v(m), t, k, None) == 1 and b"null handle" in lib.a1mpc_last_error()
    assert np.isnan(ep).all() and np.isnan(fin).all() and (life == 7).all() and (mask == 9).all()


def test_the_kernels_are_in_the_code_object_use_no_scratch_and_are_gated(pkg):
    pkg.build.build()
    res = json.load(open(pkg.build.RESOURCES_PATH))["kernels"]
    isa_check = importlib.import_module(pkg.__name__ + ".isa_check")
    for kernel in KERNELS:
        assert kernel in isa_check.NO_SCRATCH   # the build's own gate covers it
        assert isa_check.resource_gaps(res, no_scratch=(kernel,)) == []
        hits = [v for k, v in res.items() if kernel in k]
        assert len(hits) == 1, kernel
        k = hits[0]
        print(kernel + ":", k)
        assert k["scratch_bytes"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["max_flat_workgroup_size"] == 64 and k["lds_static_bytes"] == 0
        assert k["vgpr"] <= 64 and k["agpr"] == 0   # (eight waves per SIMD)
        spilled = dict(res); spilled["x_" + kernel + "_x"] = dict(k, scratch_bytes=16)
        assert isa_check.resource_gaps(spilled, no_scratch=(kernel,)) != []   # the gate does fail on a spill
    # no other kernel's name lies inside a new one or the other way round: tests look kernels up with `in`
    names = [re.search(r"a1mpc_\w+_kernel", key).group(0) for key in res if re.search(r"a1mpc_\w+_kernel", key)]
    for kernel in KERNELS:
        assert [x for x in set(names) if x != kernel and (x in kernel or kernel in x)] == []
    for other in ("a1mpc_episode_update_kernel", "a1mpc_episode_reduce_kernel", "a1mpc_sensor_noise_kernel", "a1mpc_ekf_init_kernel"):
        assert len([key for key in res if other in key]) == 1, other
