"""CPU: the gait-aware horizon at the C ABI -- the new entry points are declared in include/a1mpc.h, exported by liba1mpc.so and listed in engine.EXPORTS; the preview
configuration has the header's layout and defaults; what can be refused without a device is refused there.  No compute (there is no GPU here)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("a1mpc_default_preview_config", "a1mpc_horizon_preview_batch", "a1mpc_horizon_preview_batch_device", "a1mpc_solve_batch_ticks_strided",
       "a1mpc_solve_batch_ticks_strided_device", "a1mpc_control_tick_preview_device")


def _header():
    return open(os.path.join(ROOT, "include", "a1mpc.h")).read()


def test_new_symbols_are_declared_exported_and_listed(pkg):
    pkg.build.build()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = C.CDLL(pkg.build.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in include/a1mpc.h"
        assert hasattr(lib, name), f"{name} is not exported by liba1mpc.so"
        assert name in pkg.engine.EXPORTS
    bound = pkg.load_library()
    for name in NEW:
        assert getattr(bound, name).argtypes is not None, name   # bound with argument types (a pointer passed as a bare int would be truncated)
    assert pkg.PreviewConfig is pkg.engine.PreviewConfig
    for method in ("horizon_preview", "solve_ticks_strided", "control_tick_preview_device"):
        assert callable(getattr(pkg.Engine, method))


def test_preview_config_layout_and_defaults(pkg):
    lib = pkg.load_library()
    m = re.search(r"typedef struct a1mpc_preview_config \{(.*?)\} a1mpc_preview_config;", _header(), flags=re.S)
    fields = re.findall(r"\b(int32_t|double|float|int64_t|uint8_t)\s+(\w+)\s*;", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [("int32_t", "contact_schedule"), ("int32_t", "foot_preview"), ("int32_t", "ticks_per_step")]
    assert [f[0] for f in pkg.PreviewConfig._fields_] == [f[1] for f in fields] and all(f[1] is C.c_int32 for f in pkg.PreviewConfig._fields_)
    assert C.sizeof(pkg.PreviewConfig) == 3 * C.sizeof(C.c_int32)
    pv = pkg.PreviewConfig(-5, -5, -5)
    lib.a1mpc_default_preview_config(C.byref(pv))
    assert (pv.contact_schedule, pv.foot_preview, pv.ticks_per_step) == (1, 0, 1)
    lib.a1mpc_default_preview_config(None)   # tolerated like the other a1mpc_default_* calls


def test_null_handle_and_null_config_are_refused_without_a_device(pkg):
    lib = pkg.load_library()
    pv = pkg.PreviewConfig(1, 0, 1); gait = pkg.GaitConfig(); lib.a1mpc_default_gait_config(C.byref(gait))
    assert lib.a1mpc_horizon_preview_batch(None, C.byref(pv), C.byref(gait), 1, None, None, None, None, None, None, None, None, None) == 1
    assert lib.a1mpc_horizon_preview_batch_device(None, C.byref(pv), C.byref(gait), 1, None, None, None, None, None, None, None, None, None, None) == 1
    assert lib.a1mpc_control_tick_preview_device(None, None, C.byref(pv), None, 1, None) == 1
    assert lib.a1mpc_solve_batch_ticks_strided(None, 1, None, None, None, 12, None, 4, None, None, None, None, None) == 1
    assert lib.a1mpc_solve_batch_ticks_strided(None, 1, None, None, None, 3, None, 4, None, None, None, None, None) == 1 and b"foot_stride" in lib.a1mpc_last_error()
    assert lib.a1mpc_solve_batch_ticks_strided_device(None, 1, None, None, None, 12, None, 4, None, None, None, None, None, None) == 1
