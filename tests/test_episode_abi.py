"""CPU: the episode record and batch summary at the C ABI -- a1mpc_default_episode_config, a1mpc_episode_update_batch(_device) and a1mpc_episode_summary_batch(_device)
are declared in include/a1mpc.h with the parameters the header's block names, exported by liba1mpc.so (and nothing else of theirs is), listed in engine.EXPORTS and bound
with argument types; the configuration's layout and defaults; the engine's constants and wrappers; the refusal that needs no device (a null handle comes first, with good
and with bad arguments; the ones that need a live handle, the poisoned device arrays and n = 0 are checked on the GPU: tests/test_gpu_episode.py); both kernels are in the
code object once each, use no scratch memory and are covered by the build's gate.  No compute on a GPU."""
import ctypes as C
import importlib
import inspect
import json
import os
import re
import subprocess

import numpy as np

import episode_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("a1mpc_default_episode_config", "a1mpc_episode_update_batch", "a1mpc_episode_update_batch_device", "a1mpc_episode_summary_batch", "a1mpc_episode_summary_batch_device")
KERNELS = ("a1mpc_episode_update_kernel", "a1mpc_episode_reduce_kernel")
INPUTS = [("const double*", "root_pos"), ("const double*", "root_lin_vel"), ("const double*", "root_lin_vel_d"), ("const double*", "root_pos_d_z"), ("const double*", "ground"),
          ("const double*", "grf_body"), ("const uint8_t*", "contacts"), ("const int32_t*", "status"), ("const uint8_t*", "reach")]


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
    head = [("a1mpc_handle", "h"), ("const a1mpc_episode_config*", "cfg"), ("int32_t", "n"), ("uint64_t", "tick")]
    assert _params(code, "a1mpc_episode_update_batch") == head + [("const double*", "state"), ("int32_t", "state_stride"), ("const double*", "R_world")] + INPUTS + [
        ("double*", "episode")]
    assert _params(code, "a1mpc_episode_update_batch_device") == head + [("const double*", "d_state"), ("int32_t", "state_stride"), ("const double*", "d_R_world")] + [
        (t, "d_" + k) for t, k in INPUTS] + [("double*", "d_episode"), ("void*", "hip_stream")]
    assert _params(code, "a1mpc_episode_summary_batch") == [("a1mpc_handle", "h"), ("int32_t", "n"), ("const double*", "episode"), ("double*", "summary_out")]
    assert _params(code, "a1mpc_episode_summary_batch_device") == [("a1mpc_handle", "h"), ("int32_t", "n"), ("const double*", "d_episode"), ("double*", "d_summary_out"),
                                                                   ("void*", "hip_stream")]
    for f in (bound.a1mpc_episode_update_batch, bound.a1mpc_episode_update_batch_device):
        assert f.argtypes[3] is C.c_uint64   # (the tick by value, 64 bits)
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.build.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in nm.splitlines() if re.search(r" [TW] a1mpc_\w*episode", l))
    assert exported == sorted(NEW), exported
    # the closed symbol lists of the families beside it match on these substrings: no name of this family may carry one
    assert not [name for name in NEW + KERNELS for word in ("plant", "synthesis", "walk", "ground", "touch", "noise") if word in name]


def test_the_configuration_and_the_constants(pkg):
    """the header's struct, field for field, and its defaults whatever the memory held; the record's and the summary's field lists are the restatement's"""
    code = _code()
    m = re.search(r"typedef struct a1mpc_episode_config \{(.*?)\} a1mpc_episode_config;", code, flags=re.S)
    assert m
    fields = [tuple(decl.split()) for decl in m.group(1).split(";") if decl.strip()]
    assert fields == [("double", "min_up"), ("double", "min_height")]
    E = pkg.engine
    assert [(k, t) for k, t in E.EpisodeConfig._fields_] == [(k, C.c_double) for _, k in fields] and C.sizeof(E.EpisodeConfig) == 16
    lib = pkg.load_library()
    ec = E.EpisodeConfig()
    C.memset(C.byref(ec), 0xFF, C.sizeof(ec))
    lib.a1mpc_default_episode_config(C.byref(ec))
    assert (ec.min_up, ec.min_height) == (0.5, 0.12) == (ER.DEFAULT["min_up"], ER.DEFAULT["min_height"])
    lib.a1mpc_default_episode_config(None)   # (a null pointer is ignored)
    assert pkg.EpisodeConfig is E.EpisodeConfig
    assert E.EPISODE_WORDS == 16 == ER.WORDS == len(E.EPISODE_FIELDS) and tuple(E.EPISODE_FIELDS) == ER.FIELDS
    assert tuple(E.SUMMARY_FIELDS) == ER.SUMMARY_FIELDS and len(E.SUMMARY_FIELDS) == 20 == ER.SUMMARY
    assert [k for k, _, _ in E.EPISODE_INPUTS] == [k for _, k in INPUTS]


def test_the_engine_wrappers(pkg):
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()][1:]
    N = inspect.Parameter.empty
    names = [k for _, k in INPUTS]
    assert [k for k, _ in sig(pkg.Engine.episode_config)] == ["fields"]
    assert sig(pkg.Engine.episode_update) == [("episode", N), ("tick", N), ("state", N), ("R_world", N)] + [(k, None) for k in names] + [("config", None)]
    assert sig(pkg.Engine.episode_update_device) == [("n", N), ("tick", N), ("d_episode", N), ("d_state", N), ("state_stride", N), ("d_R_world", N)] + [
        ("d_" + k, None) for k in names] + [("config", None), ("stream", None)]
    assert sig(pkg.Engine.episode_summary) == [("episode", N)]
    assert sig(pkg.Engine.episode_summary_device) == [("n", N), ("d_episode", N), ("d_summary", N), ("stream", None)]


def test_a_null_handle_is_refused_first_without_a_device(pkg):
    """all four entries, with good and with bad arguments (a negative n, a stride of 14, a NaN threshold, a tick of 2^53, half a pair, a null state, the records over an
    input, the summary over the records): status 1, `null handle` named, and the poisoned arrays keep their bits"""
    lib = pkg.load_library()
    n = 4
    d = {k: np.array(v) for k, v in ER.random_inputs(n, seed=9950)[0].items()}
    ep = np.full((n, 16), np.nan); out = np.full(20, np.nan)
    keep = {k: v.copy() for k, v in d.items()}
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER({np.dtype("float64"): C.c_double, np.dtype("uint8"): C.c_uint8, np.dtype("int32"): C.c_int32}[a.dtype]))
    v = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    names = [k for _, k in INPUTS]
    good = dict(min_up=0.5, min_height=0.12)
    cases = [(good, n, 7, 12, {}), (good, -1, 7, 12, {}), (good, n, 7, 14, {}), (dict(good, min_up=float("nan")), n, 7, 12, {}), (dict(good, min_up=1.5), n, 7, 12, {}),
             (dict(good, min_height=float("inf")), n, 7, 12, {}), (good, n, 2 ** 53, 12, {}), (good, n, 7, 12, dict(root_pos=None)), (good, n, 7, 12, dict(contacts=None)),
             (good, n, 7, 12, dict(state=None)), (good, n, 7, 12, dict(R=None)), (good, n, 7, 12, dict(episode=None)), (good, n, 7, 12, dict(episode=d["grf_body"])),
             (None, n, 7, 12, {})]
    for cfg, n_, tick, stride, swap in cases:
        ec = None
        if cfg is not None:
            ec = pkg.engine.EpisodeConfig(); ec.min_up, ec.min_height = cfg["min_up"], cfg["min_height"]
        a = dict(dict(d, episode=ep), **swap)
        ref = None if ec is None else C.byref(ec)
        assert lib.a1mpc_episode_update_batch(None, ref, n_, tick, p(a["state"]), stride, p(a["R"]), *[p(a[k]) for k in names], p(a["episode"])) == 1
        assert b"null handle" in lib.a1mpc_last_error()
        assert lib.a1mpc_episode_update_batch_device(None, ref, n_, tick, v(a["state"]), stride, v(a["R"]), *[v(a[k]) for k in names], v(a["episode"]), None) == 1
        assert b"null handle" in lib.a1mpc_last_error()
    for n_, e, o in ((n, ep, out), (-1, ep, out), (n, None, out), (n, ep, None), (n, ep, ep[1])):
        assert lib.a1mpc_episode_summary_batch(None, n_, p(e), p(o)) == 1 and b"null handle" in lib.a1mpc_last_error()
        assert lib.a1mpc_episode_summary_batch_device(None, n_, v(e), v(o), None) == 1 and b"null handle" in lib.a1mpc_last_error()
    assert np.isnan(ep).all() and np.isnan(out).all() and all(ER.bits_equal(d[k].astype(np.float64), keep[k].astype(np.float64)) for k in d)


def test_the_kernels_are_in_the_code_object_use_no_scratch_and_are_gated(pkg):
    pkg.build.build()
    res = json.load(open(pkg.build.RESOURCES_PATH))["kernels"]
    isa_check = importlib.import_module(pkg.__name__ + ".isa_check")
    lds = {KERNELS[0]: (16 * 22 + 16 * 9 + 16 * 16 + 4 * 48 + 16) * 8, KERNELS[1]: 64 * 20 * 8}
    for kernel in KERNELS:
        assert kernel in isa_check.NO_SCRATCH   # the build's own gate covers it
        assert isa_check.resource_gaps(res, no_scratch=(kernel,)) == []
        hits = [v for k, v in res.items() if kernel in k]
        assert len(hits) == 1, kernel
        k = hits[0]
        print(kernel + ":", k)
        assert k["scratch_bytes"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["max_flat_workgroup_size"] == 64 and k["lds_static_bytes"] == lds[kernel]
        assert k["vgpr"] <= 128   # (four waves per SIMD at the least)
        spilled = dict(res); spilled["x_" + kernel + "_x"] = dict(k, scratch_bytes=16)
        assert isa_check.resource_gaps(spilled, no_scratch=(kernel,)) != []   # the gate does fail on a spill
    # no existing kernel's name lies inside a new one or the other way round: tests look kernels up with `in`
    names = [re.search(r"a1mpc_\w+_kernel", key).group(0) for key in res if re.search(r"a1mpc_\w+_kernel", key)]
    for kernel in KERNELS:
        assert [x for x in set(names) if x != kernel and (x in kernel or kernel in x)] == []
    for other in ("a1mpc_sensor_noise_kernel", "a1mpc_walk_sensors_kernel", "a1mpc_walk_sensors_touch_kernel", "a1mpc_plant_step_kernel"):
        assert len([key for key in res if other in key]) == 1, other
