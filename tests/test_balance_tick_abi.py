"""CPU: the balance-QP stance controller at the C ABI -- a1mpc_default_balance_gains, a1mpc_balance_wrench_batch(_device), a1mpc_balance_solve_batch_device,
a1mpc_contacts_batch(_device) and a1mpc_control_tick_balance_device are declared in include/a1mpc.h, exported by liba1mpc.so, listed in engine.EXPORTS and bound with as
many argument types as parameters; the ctypes structs have the header's sizes (a C compiler says which); the default gains are the reference's; every entry refuses a null
handle without a device; the new kernels are in the code object and use no scratch memory.  No compute on a GPU (there is none here)."""
import ctypes as C
import importlib
import json
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("a1mpc_default_balance_gains", "a1mpc_balance_wrench_batch", "a1mpc_balance_wrench_batch_device", "a1mpc_balance_solve_batch_device", "a1mpc_contacts_batch",
       "a1mpc_contacts_batch_device", "a1mpc_control_tick_balance_device")


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "a1mpc.h")).read(), flags=re.S)


def _params(code, name):
    """the parameter names of `name`'s declaration, in order"""
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
    # the device entries take the host entries' arguments in their order (d_ prefixed), then the stream; the device solve takes a1mpc_balance_solve_batch's
    strip = lambda ps: [re.sub(r"^d_", "", p) for p in ps]
    for host, dev in (("a1mpc_balance_wrench_batch", "a1mpc_balance_wrench_batch_device"), ("a1mpc_contacts_batch", "a1mpc_contacts_batch_device"),
                      ("a1mpc_balance_solve_batch", "a1mpc_balance_solve_batch_device")):
        assert strip(_params(code, dev)) == _params(code, host) + ["hip_stream"], (host, dev)
    for wrapper in ("balance_wrench", "balance_solve_device", "contacts", "control_tick_balance_device"):
        assert callable(getattr(pkg.Engine, wrapper))
    assert pkg.BalanceGains is pkg.engine.BalanceGains and pkg.BalanceTick is pkg.engine.BalanceTick


def test_ctypes_structs_have_the_header_sizes_and_offsets(pkg):
    """sizeof / offsetof as a C compiler sees include/a1mpc.h; a1mpc_tick_buffers (which this controller shares with the MPC tick) is still one pointer per field"""
    src = r'''#include <stdio.h>
#include <stddef.h>
#include "a1mpc.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(a1mpc_balance_gains), sizeof(a1mpc_balance_tick), sizeof(a1mpc_balance_config), sizeof(a1mpc_tick_buffers),
           offsetof(a1mpc_balance_tick, qp), offsetof(a1mpc_balance_tick, root_pos_d), offsetof(a1mpc_balance_tick, root_acc), offsetof(a1mpc_balance_tick, f_world),
           sizeof(a1mpc_tick_params));
    return 0;
}
'''
    with tempfile.TemporaryDirectory(prefix="a1mpc_abi_") as d:
        c = os.path.join(d, "sizes.c"); exe = os.path.join(d, "sizes")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    E = pkg.engine
    want = [C.sizeof(E.BalanceGains), C.sizeof(E.BalanceTick), C.sizeof(E.BalanceConfig), C.sizeof(E.TickBuffers), E.BalanceTick.qp.offset, E.BalanceTick.root_pos_d.offset,
            E.BalanceTick.root_acc.offset, E.BalanceTick.f_world.offset, C.sizeof(E.TickParams)]
    assert got == want, (got, want)
    assert C.sizeof(E.BalanceGains) == 12 * 8 and C.sizeof(E.TickBuffers) == len(E.TICK_BUFFER_FIELDS) * C.sizeof(C.c_void_p)


def test_default_gains_are_the_reference_constants(pkg):
    lib = pkg.load_library()
    g = pkg.BalanceGains()
    lib.a1mpc_default_balance_gains(C.byref(g))
    assert [list(g.kp_linear), list(g.kd_linear), list(g.kp_angular), list(g.kd_angular)] == [[1000.0] * 3, [200.0, 70.0, 120.0], [650.0, 35.0, 1.0], [4.5, 4.5, 30.0]]   # S/A1CtrlStates.h:117-120
    lib.a1mpc_default_balance_gains(None)   # (like the other defaults: a null pointer is ignored)


def test_every_new_entry_refuses_a_null_handle_without_a_device(pkg):
    """A1MPC_ERR_INVALID_ARGUMENT (1) and a1mpc_last_error names the handle, whatever the other arguments are: the handle is looked at first.  (The refusals that need a
    live handle -- n > max_batch, a null array, a non-finite gain, a bad QP config, a null root_pos_d -- are checked on the GPU, tests/test_gpu_balance_tick.py.)"""
    lib = pkg.load_library()
    E = pkg.engine
    d = lambda k: (C.c_double * k)()
    u8 = lambda k: (C.c_uint8 * k)()
    g = E.BalanceGains(); lib.a1mpc_default_balance_gains(C.byref(g))
    qp = E.BalanceConfig(); lib.a1mpc_default_balance_config(C.byref(qp))
    cc = E.ContactConfig(); lib.a1mpc_default_contact_config(C.byref(cc))
    prm = E.TickParams(); lib.a1mpc_default_tick_params(C.byref(prm))
    bt = E.BalanceTick(); bf = E.TickBuffers()
    v3 = [d(3) for _ in range(8)]
    for n in (1, 0, -1):
        calls = [lib.a1mpc_balance_wrench_batch(None, C.byref(g), n, *v3, d(9), d(6)),
                 lib.a1mpc_balance_wrench_batch(None, None, n, *([None] * 10)),
                 lib.a1mpc_balance_wrench_batch_device(None, C.byref(g), n, *([None] * 10), None),
                 lib.a1mpc_balance_solve_batch_device(None, C.byref(qp), n, *([None] * 9), None),
                 lib.a1mpc_contacts_batch(None, C.byref(cc), n, d(4), u8(4), d(4), d(12), u8(4), d(12)),
                 lib.a1mpc_contacts_batch_device(None, C.byref(cc), n, *([None] * 6), None),
                 lib.a1mpc_control_tick_balance_device(None, C.byref(prm), C.byref(bt), C.byref(bf), n, None)]
        assert calls == [1] * len(calls), (n, calls)
        assert b"null handle" in lib.a1mpc_last_error()


def test_new_kernels_are_in_the_code_object_and_use_no_scratch(pkg):
    pkg.build.build()
    res = json.load(open(pkg.build.RESOURCES_PATH))["kernels"]
    isa_check = importlib.import_module(pkg.__name__ + ".isa_check")
    new = ("a1mpc_balance_wrench_kernel", "a1mpc_contacts_kernel")
    assert isa_check.resource_gaps(res, no_scratch=new) == []
    for name in new:
        k = next(v for key, v in res.items() if name in key)
        print(name, k)
        assert k["scratch_bytes"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0
    w = next(v for key, v in res.items() if "a1mpc_balance_wrench_kernel" in key)
    assert w["lds_static_bytes"] == 0 and w["max_flat_workgroup_size"] == 256 and w["vgpr"] <= 128   # element-wise: no LDS, four waves per SIMD at the least
    c = next(v for key, v in res.items() if "a1mpc_contacts_kernel" in key)
    t = next(v for key, v in res.items() if "a1mpc_contact_terrain_kernel" in key)
    assert c["lds_static_bytes"] == t["lds_static_bytes"] and c["max_flat_workgroup_size"] == 64   # the same record staging as the kernel it is cut from
