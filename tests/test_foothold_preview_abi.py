"""CPU: the foothold preview at the C ABI -- a1mpc_horizon_preview_footholds_batch(_device), a1mpc_control_tick_preview_footholds_device and
a1mpc_pipeline_submit_ticks_strided_device are declared in include/a1mpc.h with the documented argument order, exported by liba1mpc.so, listed in engine.EXPORTS and bound
with argument types; the engine wrappers have the documented signatures; a1mpc_preview_config keeps its three fields.  No compute (there is no GPU here)."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("a1mpc_horizon_preview_footholds_batch", "a1mpc_horizon_preview_footholds_batch_device", "a1mpc_control_tick_preview_footholds_device",
       "a1mpc_pipeline_submit_ticks_strided_device")


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


def test_argument_order_is_the_existing_entries_with_the_new_arguments_inserted():
    code = _code()
    for new, old in (("a1mpc_horizon_preview_footholds_batch", "a1mpc_horizon_preview_batch"), ("a1mpc_horizon_preview_footholds_batch_device", "a1mpc_horizon_preview_batch_device")):
        a, b = _params(code, new), _params(code, old)
        k = next(i for i, p in enumerate(b) if p.endswith("root_lin_vel_d")) + 1
        assert a[:k] == b[:k] and a[k].endswith("foot_pos_target_abs") and a[k + 1:] == b[k:], (a, b)   # the target sits right after root_lin_vel_d
    assert _params(code, "a1mpc_control_tick_preview_footholds_device") == _params(code, "a1mpc_control_tick_preview_device")
    # the tick-record submit with foot_stride, contact_stride and d_yaw_A where a1mpc_pipeline_submit_strided_device has them
    a, t, s = (_params(code, n) for n in ("a1mpc_pipeline_submit_ticks_strided_device", "a1mpc_pipeline_submit_ticks_device", "a1mpc_pipeline_submit_strided_device"))
    assert [p for p in a if p not in ("foot_stride", "contact_stride", "d_yaw_A")] == t
    assert a[a.index("d_R_world"):] == s[s.index("d_R_world"):]


def test_engine_wrappers_have_the_documented_signatures(pkg):
    hp = inspect.signature(pkg.Engine.horizon_preview).parameters
    assert "foot_target_abs" in hp and hp["foot_target_abs"].default is None
    assert list(inspect.signature(pkg.Engine.control_tick_preview_footholds_device).parameters) == list(inspect.signature(pkg.Engine.control_tick_preview_device).parameters)
    sub = list(inspect.signature(pkg.Pipeline.submit_ticks_strided_device).parameters)
    assert sub[:8] == ["self", "n", "d_tick", "d_R", "d_foot", "foot_stride", "d_contact", "contact_stride"] and "d_yaw_A" in sub
    assert {"slot", "fresh", "after_stream"} <= set(sub)


def test_preview_config_keeps_its_three_fields(pkg):
    m = re.search(r"typedef struct a1mpc_preview_config \{(.*?)\} a1mpc_preview_config;", open(os.path.join(ROOT, "include", "a1mpc.h")).read(), flags=re.S)
    fields = re.findall(r"\b(int32_t|double|float|int64_t|uint8_t)\s+(\w+)\s*;", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [("int32_t", "contact_schedule"), ("int32_t", "foot_preview"), ("int32_t", "ticks_per_step")]
    assert C.sizeof(pkg.PreviewConfig) == 3 * C.sizeof(C.c_int32) and all(f[1] is C.c_int32 for f in pkg.PreviewConfig._fields_)


def test_null_handle_and_bad_strides_are_refused_without_a_device(pkg):
    lib = pkg.load_library()
    pv = pkg.PreviewConfig(1, 1, 1); gait = pkg.GaitConfig(); lib.a1mpc_default_gait_config(C.byref(gait))
    assert lib.a1mpc_horizon_preview_footholds_batch(None, C.byref(pv), C.byref(gait), 1, None, None, None, None, None, None, None, None, None, None) == 1
    assert lib.a1mpc_horizon_preview_footholds_batch_device(None, C.byref(pv), C.byref(gait), 1, None, None, None, None, None, None, None, None, None, None, None) == 1
    assert lib.a1mpc_control_tick_preview_footholds_device(None, None, C.byref(pv), None, 1, None) == 1
    assert lib.a1mpc_pipeline_submit_ticks_strided_device(None, -1, 1, 1, None, None, None, 12, None, 4, None, None, None, None, None, None, None) == 1
