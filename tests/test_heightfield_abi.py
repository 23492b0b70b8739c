"""CPU: height-field terrain at the C ABI -- a1mpc_default_heightfield, a1mpc_heightfield_step_batch(_device) and a1mpc_heightfield_sample_batch(_device) are declared in
include/a1mpc.h with the ground step's parameters and the new ones where the header says, exported by liba1mpc.so (and nothing else of theirs is), listed in
engine.EXPORTS and bound with argument types; the struct's layout and default; the engine wrappers' signatures; every refusal of the field, which the entries check in
front of the handle and so report without a device (the refusals that need a live handle, the poisoned outputs and n = 0 are checked on the GPU:
tests/test_gpu_heightfield.py); both kernels are in the code object and use no scratch memory; the generators of heightfields.py.  No compute on a GPU."""
import ctypes as C
import importlib
import inspect
import json
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("a1mpc_default_heightfield", "a1mpc_heightfield_step_batch", "a1mpc_heightfield_step_batch_device", "a1mpc_heightfield_sample_batch",
       "a1mpc_heightfield_sample_batch_device")
KERNELS = ("a1mpc_walk_step_heightfield_kernel", "a1mpc_heightfield_sample_kernel")
INVALID, TOO_LARGE = 1, 5


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
        assert getattr(bound, name).restype is (None if name == "a1mpc_default_heightfield" else C.c_int)
    for d in ("", "d_"):
        suffix = "_device" if d else ""
        # the step: the ground step's parameters with (field, origin) where ground is and ground_out after touch_out
        ground, hf = _params(code, "a1mpc_ground_step_batch" + suffix), _params(code, "a1mpc_heightfield_step_batch" + suffix)
        i, j = ground.index(d + "ground"), ground.index(d + "touch_out") + 1
        assert hf == ground[:i] + ["field", d + "origin"] + ground[i + 1:j] + [d + "ground_out"] + ground[j:], hf
        assert _params(code, "a1mpc_heightfield_sample_batch" + suffix) == ["h", "field", "n", d + "xy", d + "origin", d + "height_out"] + (["hip_stream"] if d else [])
    hfp = C.POINTER(pkg.engine.Heightfield)
    assert bound.a1mpc_heightfield_step_batch.argtypes[12] is hfp and bound.a1mpc_heightfield_step_batch_device.argtypes[12] is hfp
    assert bound.a1mpc_heightfield_sample_batch.argtypes[1] is hfp and bound.a1mpc_heightfield_sample_batch_device.argtypes[1] is hfp
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.build.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in nm.splitlines() if re.search(r" [TW] a1mpc_\w*heightfield", l))
    assert exported == sorted(NEW), exported
    taken = ("ground", "touch", "walk", "plant", "episode", "respawn", "noise", "synthesis")   # the substrings by which the other families' ABI tests list their exports
    assert not [n for n in NEW for t in taken if t in n]


def test_the_struct_layout_and_default(pkg):
    """a1mpc_heightfield as the header declares it, field by field, with the C layout (int32 pair, four doubles, an int32 and its padding, a pointer); the default"""
    code = _code()
    m = re.search(r"typedef struct a1mpc_heightfield \{(.*?)\} a1mpc_heightfield;", code, flags=re.S)
    assert m
    flat = []
    for d in (x.strip() for x in m.group(1).split(";") if x.strip()):
        ty, rest = re.match(r"(const double\*|int32_t|double)\s*(.*)", re.sub(r"\s+", " ", d)).groups()
        flat += [(n.strip(), ty) for n in rest.split(",")]
    assert flat == [("nx", "int32_t"), ("ny", "int32_t"), ("x0", "double"), ("y0", "double"), ("dx", "double"), ("dy", "double"), ("interp", "int32_t"),
                    ("height", "const double*")], flat
    H = pkg.engine.Heightfield
    want = {"int32_t": C.c_int32, "double": C.c_double, "const double*": C.c_void_p}
    assert [(k, t) for k, t in H._fields_] == [(k, want[t]) for k, t in flat]
    assert [getattr(H, k).offset for k, _ in H._fields_] == [0, 4, 8, 16, 24, 32, 40, 48] and C.sizeof(H) == 56
    f = H(7, 7, 7.0, 7.0, 7.0, 7.0, 7, 7)
    lib = pkg.load_library()
    lib.a1mpc_default_heightfield(C.byref(f))
    assert (f.nx, f.ny, f.x0, f.y0, f.dx, f.dy, f.interp, f.height) == (0, 0, 0.0, 0.0, 1.0, 1.0, 0, None)
    lib.a1mpc_default_heightfield(None)   # (a null descriptor is left alone)


def test_the_engine_wrappers(pkg):
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()][1:]
    N = inspect.Parameter.empty
    E = pkg.Engine
    # the ground methods' argument order with field, origin where ground is, and ground_out last
    g = sig(E.walk_step_ground); i = [k for k, _ in g].index("ground")
    assert sig(E.walk_step_heightfield) == g[:i] + [("field", None), ("origin", None)] + g[i + 1:] + [("ground_out", True)]
    g = sig(E.walk_step_ground_device); i = [k for k, _ in g].index("d_ground")
    assert sig(E.walk_step_heightfield_device) == g[:i] + [("field", None), ("d_origin", None)] + g[i + 1:] + [("d_ground_out", None)]
    assert sig(E.heightfield) == [("heights", N), ("x0", 0.0), ("y0", 0.0), ("dx", 1.0), ("dy", 1.0), ("interp", 0)]
    assert sig(E.heightfield_sample) == [("field", N), ("xy", N), ("origin", None)]
    assert sig(E.heightfield_sample_device) == [("field", N), ("n", N), ("d_xy", N), ("d_height_out", N), ("d_origin", None), ("stream", None)]


def _field(pkg, **kw):
    f = pkg.engine.Heightfield()
    pkg.load_library().a1mpc_default_heightfield(C.byref(f))
    keep = np.zeros(16)
    f.nx, f.ny, f.interp, f.height = 4, 4, 0, keep.ctypes.data
    for k, v in kw.items():
        setattr(f, k, v)
    return f, keep


def test_refusals_are_reported_without_a_device(pkg):
    """the field is checked in front of the handle: every refusal of the header's list comes back from all four entries with the field named, handle or no handle; a
    good field with a null handle is refused for the handle; a field of more than 2^20 nodes is A1MPC_ERR_BATCH_TOO_LARGE from the host-pointer entries only when the
    arguments before it are good, which needs a handle (GPU file)"""
    lib = pkg.load_library()
    wc = pkg.engine.WalkConfig(); lib.a1mpc_default_walk_config(C.byref(wc))
    d = lambda k: (C.c_double * k)()
    st, R, foot, grf, ct, vel, og, tc, go, xy, out = d(22), d(9), d(12), d(12), (C.c_uint8 * 4)(), d(12), d(3), (C.c_uint8 * 4)(), d(3), d(2), d(1)

    def all_four(fp):
        got = []
        got.append((lib.a1mpc_heightfield_step_batch(None, C.byref(wc), 1, st, 12, R, foot, grf, ct, None, R, foot, fp, og, st, R, foot, vel, tc, go), lib.a1mpc_last_error().decode()))
        got.append((lib.a1mpc_heightfield_step_batch_device(None, C.byref(wc), 1, None, 12, *([None] * 7), fp, *([None] * 8)), lib.a1mpc_last_error().decode()))
        got.append((lib.a1mpc_heightfield_sample_batch(None, fp, 1, xy, og, out), lib.a1mpc_last_error().decode()))
        got.append((lib.a1mpc_heightfield_sample_batch_device(None, fp, 1, None, None, None, None), lib.a1mpc_last_error().decode()))
        return got

    nan, inf = float("nan"), float("inf")
    bad = [(dict(interp=2), "interp"), (dict(interp=-1), "interp"), (dict(nx=0), "nx"), (dict(ny=0), "ny"), (dict(nx=-3), "nx"), (dict(interp=1, nx=1), "nx"),
           (dict(interp=1, ny=1), "ny"), (dict(nx=32769), "nx"), (dict(ny=32769), "ny"), (dict(dx=0.0), "dx"), (dict(dx=-1.0), "dx"), (dict(dx=nan), "dx"), (dict(dx=inf), "dx"),
           (dict(dy=0.0), "dy"), (dict(dy=-0.5), "dy"), (dict(dy=nan), "dy"), (dict(dy=inf), "dy"), (dict(x0=nan), "x0"), (dict(x0=-inf), "x0"), (dict(y0=nan), "y0"),
           (dict(y0=inf), "y0"), (dict(dx=1e-320), "1 / dx"), (dict(dy=4e-324), "1 / dy"), (dict(height=None), "height")]
    for kw, word in bad:
        f, keep = _field(pkg, **kw)
        for rc, msg in all_four(C.byref(f)):
            assert rc == INVALID and "a1mpc_heightfield" in msg and word in msg, (kw, rc, msg)
    for rc, msg in all_four(None):
        assert rc == INVALID and "null a1mpc_heightfield" in msg, (rc, msg)
    for kw in (dict(), dict(interp=1, nx=2, ny=2), dict(nx=1, ny=1), dict(nx=32768, ny=32768)):   # (accepted fields: then the handle is what is missing)
        f, keep = _field(pkg, **kw)
        for rc, msg in all_four(C.byref(f)):
            assert rc == INVALID and "null handle" in msg, (kw, rc, msg)
    assert st[0] == 0.0 and out[0] == 0.0 and tc[0] == 0


def test_kernels_are_in_the_code_object_and_use_no_scratch(pkg):
    pkg.build.build()
    res = json.load(open(pkg.build.RESOURCES_PATH))["kernels"]
    isa_check = importlib.import_module(pkg.__name__ + ".isa_check")
    for name in KERNELS:
        assert isa_check.resource_gaps(res, no_scratch=(name,)) == []
        hits = [v for k, v in res.items() if name in k]
        assert len(hits) == 1, name
        k = hits[0]
        print(name + ":", k)
        assert k["scratch_bytes"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["max_flat_workgroup_size"] == 64 and k["lds_static_bytes"] <= 8192
    # the ground kernels beside them are still found under their own names alone
    assert len([k for k in res if "a1mpc_walk_step_ground_kernel" in k]) == 1 and len([k for k in res if "a1mpc_walk_sensors_touch_kernel" in k]) == 1


def test_the_kernel_sits_in_the_plant_step_section_and_the_older_emulations_still_compile():
    """between the section's two markers, so that plant_host.section() cuts it; the modules that compile that section for the host build with it inside"""
    import plant_host, walk_step_host, walk_step_ground_host, heightfield_host
    s = plant_host.section()
    assert all(k in s for k in KERNELS) and s.index("a1mpc_walk_step_ground_kernel") < s.index("a1mpc_walk_step_heightfield_kernel")
    assert s.count("__device__ __forceinline__ double hf_sample(") == 1 and s.count("hf_sample(") == 1 + 4 + 2   # one function, called by both kernels
    for m in (plant_host, walk_step_host, walk_step_ground_host, heightfield_host):
        assert m.load() is not None


def test_the_generators(pkg):
    G = pkg.heightfields
    r = G.ramp(5, 3, 0.5, 0.25, 0.1, -0.2)
    assert r.shape == (3, 5) and r[0, 0] == 0.0 and np.allclose(r[2, 4], 0.1 * 2.0 - 0.2 * 0.5, atol=1e-15) and np.allclose(np.diff(r, axis=1), 0.05) and np.allclose(np.diff(r, axis=0), -0.05)
    s = G.stairs(13, 2, 0.05, 0.05, 0.08, 0.30, 0)
    assert s.shape == (2, 13) and np.array_equal(s[0], s[1]) and np.allclose(s[0], 0.08 * np.array([0] * 6 + [1] * 6 + [2]))
    assert np.array_equal(G.stairs(2, 13, 0.05, 0.05, 0.08, 0.30, 1), s.T)
    a, b = G.rough(64, 48, 5, 0.05), G.rough(64, 48, 5, 0.05)
    assert a.shape == (48, 64) and np.array_equal(a, b) and np.abs(a).max() <= 0.05 and a.std() > 0.02 and not np.array_equal(a, G.rough(64, 48, 6, 0.05))
    t, o = G.tiles([r, s, np.ones((1, 2))], dx=0.5)
    assert t.shape == (3, 5 + 13 + 2) and np.array_equal(t[:, :5], r) and np.array_equal(t[:2, 5:18], s) and np.array_equal(t[2, 5:18], s[1]) and (t[:, 18:] == 1.0).all()
    assert np.array_equal(o, [[0.0, 0.0, 0.0], [-2.5, 0.0, 0.0], [-9.0, 0.0, 0.0]])
    for k in (r, s, a, t):
        assert k.dtype == np.float64 and k.flags.c_contiguous
