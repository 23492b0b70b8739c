"""The height-field kernels' text under the host sanitizers, on exact-fit buffers (the pattern of tests/test_host_sanitizers.py).  tests/emu/heightfield_host.py is built
as a stand-alone program (tests/emu/sanitize.py: its own `main`, the sanitizer's runtime linked statically, nothing loaded into python) under AddressSanitizer + UBSan
and under ThreadSanitizer.  The height array is an allocation of its own of exactly nx * ny * 8 bytes: the clamped edges are where a gather reads one element past the
end, and the redzone begins right there.  The build's float-cast-overflow check is what holds "only clamped values are converted to an integer" on the NaN and inf
points.  In both runs the outputs are held to tests/heightfield_ref.py, never to the unsanitized emulation."""
import os, sys
import numpy as np
import pytest
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import sanitize
import heightfield_host as host
import heightfield_cases as HC
import heightfield_ref as HR
import plant_ref as PR

SANITIZERS = ("asan", "tsan")
_LIBS = {}


@pytest.fixture(scope="module")
def programs():
    def lib(sanitizer):
        if sanitizer not in _LIBS:
            _LIBS[sanitizer] = sanitize.Library(host, sanitizer)
        return _LIBS[sanitizer]
    return lib


@pytest.fixture(params=SANITIZERS)
def sanitizer(request):
    return request.param


def test_the_height_array_is_an_exact_fit_allocation(pkg):
    """what the marshalling hands the program: nx * ny doubles and not a byte more (sanitize.py gives every array an allocation of exactly its bytes)"""
    for f in HC.fields(pkg).values():
        _, H = host._field_args(f)
        assert H.nbytes == f.nx * f.ny * 8 and H.flags.c_contiguous and H.ndim == 1


@pytest.mark.parametrize("with_origin", [False, True])
def test_sample_on_the_edge_cases(pkg, programs, sanitizer, with_origin):
    """every field, every edge point (the last node of each axis, beyond every side and corner, -1e-300, +-inf, NaN): no read past the height array, no conversion of a
    value that does not fit, and the restatement's bits.  Two of the fields stand at the world's origin, where X = -1e-300 and X = -0.0 reach the rule as a tiny negative
    ux and as ux = -0.0 (asserted)"""
    rng = np.random.default_rng(9700)
    tiny = 0
    with sanitize.instead_of_load(host, programs(sanitizer)):
        for name, f in HC.point_fields(pkg).items():
            pts = HC.edge_points_few(f)
            n = len(pts)
            origin = None
            if with_origin:
                origin, pts = HC.point_origins(rng, pts)
            tiny += HC.tiny_points_reach_the_rule(f, pts, origin)
            out = host.sample(f, pts, origin)
            assert out.shape == (n,) and HR.same_heights(out, HR.sample(f, pts[:, 0], pts[:, 1], origin)), name
            assert np.isnan(out).sum() == 4 and np.isinf(pts).any(axis=1).sum() >= 6
    assert tiny == 2   # on the two fields at the world's origin ux = -1e-300 / dx and ux = -0.0 did reach the conversion to an index


STEP_CASES = [   # n, stride, configuration of heightfield_cases.CONFIGS (sub-steps, swing_track, field; origin / ground_out / in place by its flags)
    (1, 12, 0), (15, 13, 9), (16, 22, 18), (17, 12, 27), (33, 13, 36), (33, 22, 45), (17, 22, 7), (16, 13, 38), (15, 12, 20), (1, 22, 29), (33, 12, 6), (17, 13, 47)]


def _the_step_cases_cover_every_field_and_flag():
    seen = [(HC.CONFIGS[k][2],) + HC.flags(k) for _, _, k in STEP_CASES]
    assert {s[0] for s in seen} == {c[2] for c in HC.CONFIGS}
    for flag in (1, 2, 3):
        assert {s[flag] for s in seen} == {False, True}
    assert {HC.CONFIGS[k][0] for _, _, k in STEP_CASES} == {1, 3} and {HC.CONFIGS[k][1] for _, _, k in STEP_CASES} == {0.0, 0.5, 1.0}


@pytest.mark.parametrize("n,stride,k", STEP_CASES)
def test_step(pkg, scen, programs, sanitizer, n, stride, k):
    """the step on exact-fit arrays: every output of exactly n rows, the height array of exactly nx * ny doubles, the optional pointers null and given, in place and out of
    place; under tsan the 64 lanes' LDS traffic is ordered by the barriers; the restatement's bits"""
    _the_step_cases_cover_every_field_and_flag()
    sc = HC.walkers(scen)
    sub, track, name = HC.CONFIGS[k]
    with_origin, with_out, in_place = HC.flags(k)
    tracked = track != 0.0
    state = sc["wide"][:n, :stride]
    with sanitize.instead_of_load(host, programs(sanitizer)):
        out = host.run(sc["params"], state, sc["R"][:n], sc["foot"][:n], sc["grf"][:n], sc["contacts"][:n], sc["Rz"][:n] if tracked else None,
                       sc["target"][:n] if tracked else None, HC.fields(pkg)[name], sc["origin"][:n] if with_origin else None, sc["ext"][:n] if sub == 3 else None, 0.0025, sub,
                       swing_track=track, in_place=in_place, ground_out=with_out)
    ref = HC.ref(pkg, scen, k)
    so, Ro, fo, vo, to, go = out
    assert so.shape == (n, stride) and Ro.shape == (n, 9) and fo.shape == (n, 12) and vo.shape == (n, 12) and to.shape == (n, 4)
    assert PR.bits_equal(so[:, 3:12], ref[0][:n, 3:12]) and PR.bits_equal(Ro, ref[1][:n]) and PR.bits_equal(fo, ref[2][:n]) and PR.bits_equal(vo, ref[3][:n])
    assert np.array_equal(to, ref[4][:n]) and np.abs(so[:, :3] - ref[0][:n, :3]).max() <= PR.ANGLE_BAR
    assert np.array_equal(so[:, 12:], state[:, 12:]) if in_place else np.isnan(so[:, 12:]).all()
    assert (go is None) if not with_out else (go.shape == (n, 3) and PR.bits_equal(go, ref[5][:n]))
