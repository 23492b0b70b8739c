"""N2b on the CPU: the product's contact / terrain kernel text compiled for the host (tests/emu/n2b_host.py) stepped against the oracle -- the shipped
arithmetic AND the shipped state layout (records + sector-sized ring slots), window wrap of both filter lengths included.  The same sequence runs on the
GPU in tests/test_gpu_caller_side.py::test_contact_terrain_N2b_sequence."""
import os, sys
import numpy as np
import pytest
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import n2b_host


def test_n2b_kernel_text_on_the_host_matches_the_oracle(oracle):
    rng = np.random.default_rng(21)
    n, ticks = 24, 260   # terrain window 100 and leg window 60 both wrap; max_batch > n: the ring regions start behind max_batch records
    H = n2b_host.HostN2b(40)
    states = [oracle.contact_state() for _ in range(n)]
    pg = np.zeros(n); po = np.zeros(n)
    base = np.outer([0.2, 0.2, -0.2, -0.2], [1.0, 0.0, 0.3]).reshape(12) + np.outer([1, -1, 1, -1], [0.0, 0.13, 0.0]).reshape(12)
    gcs = rng.uniform(0, 240, (n, 4))
    for t in range(ticks):
        gcs = np.fmod(gcs + 2.0, 240.0); plan = (gcs <= 120).astype(np.uint8); ff = rng.uniform(0, 80, (n, 4))
        foot = base + rng.normal(0, 0.03, (n, 12)) + np.tile([0.0, 0.0, -0.3], 4); z = np.where(rng.random(n) < 0.9, 0.3, 0.05)
        out = H.tick(gcs, plan, ff, foot, z, pg); pg = out["root_euler_d_pitch"]
        for b in range(n):
            ct, rec, ang, po[b] = oracle.contact_terrain_step(states[b], gcs[b], plan[b], ff[b], foot[b], z[b], po[b])
            assert (out["contacts"][b] == ct).all() and (out["foot_pos_recent_contact"][b] == rec).all(), (t, b)
            assert out["terrain_angle"][b] == ang and pg[b] == po[b], (t, b)   # same libm on the host: exact (1e-13 on the GPU, whose acos is the device library's)


def test_n2b_terrain_only_entry_shares_the_terrain_filter(oracle):
    """recent_in given (a1mpc_terrain_batch): the leg filters are not touched, the terrain filter advances exactly as in the full entry fed the same positions"""
    rng = np.random.default_rng(5)
    n = 8
    A = n2b_host.HostN2b(n); B = n2b_host.HostN2b(n)
    pa = np.zeros(n); pb = np.zeros(n)
    gcs = rng.uniform(0, 240, (n, 4))
    for t in range(130):
        gcs = np.fmod(gcs + 2.0, 240.0); plan = (gcs <= 120).astype(np.uint8); ff = rng.uniform(0, 80, (n, 4)); foot = rng.normal(0, 0.2, (n, 12)); z = np.full(n, 0.3)
        oa = A.tick(gcs, plan, ff, foot, z, pa); pa = oa["root_euler_d_pitch"]
        ob = B.tick(gcs, plan, ff, foot, z, pb, recent_in=oa["foot_pos_recent_contact"]); pb = ob["root_euler_d_pitch"]
        assert np.array_equal(oa["terrain_angle"], ob["terrain_angle"]) and np.array_equal(pa, pb)


def test_n2b_kernel_text_at_the_phase_and_force_thresholds(oracle):
    """The comparisons of the contact logic ON their thresholds, where uniform random counters never land: gait_counter = 180 against the next double, foot_force = 30
    against the next double, the early-contact flag kept from tick to tick and cleared in stance, root_pos_z = 0.1 (not standing) against the next double, and a plane steep
    enough that the terrain angle reaches its 0.5 clamp with both signs of the pitch (gpu_common.contact_threshold_run / steep_plane_run: the oracle is held to the
    tabulated contacts first, then the kernel text to the oracle; the same rows run on the GPU in tests/test_gpu_gait_cycle.py).  Same libm on the host: the angles are exact."""
    import gpu_common
    n = 67
    H = n2b_host.HostN2b(80)
    gpu_common.contact_threshold_run(H.tick, oracle, n, 0.0)
    S = n2b_host.HostN2b(8)
    gpu_common.steep_plane_run(S.tick, oracle, 0.0)


def _oracle_contact_run(oracle, gcs, plans, ffs, foots, zs, pitch0, **kw):
    """oracle.contact_terrain_step over a recorded input sequence (ticks, n, ...) -> (contacts, recent, angle, pitch), each (n, ticks, ...)"""
    ticks, n = gcs.shape[:2]
    states = [oracle.contact_state() for _ in range(n)]
    pitch = np.array(pitch0, dtype=np.float64)
    ct = np.zeros((n, ticks, 4), np.uint8); rec = np.zeros((n, ticks, 12)); ang = np.zeros((n, ticks)); pit = np.zeros((n, ticks))
    for t in range(ticks):
        for b in range(n):
            ct[b, t], rec[b, t], ang[b, t], pitch[b] = oracle.contact_terrain_step(states[b], gcs[t, b], plans[t, b], ffs[t, b], foots[t, b], zs[t, b], pitch[b], **kw)
        pit[:, t] = pitch
    return ct, rec, ang, pit


@pytest.mark.parametrize("adapt", [0, 1])
@pytest.mark.parametrize("name", ["A", "B"])
def test_n2b_kernel_text_at_other_contact_configs(oracle, name, adapt):
    """The host-compiled kernel text at the contact configs of gpu_common.PARAM_SETS (A: counter_per_swing 100 -- the early-contact mark is 150 --, B: 160 -- mark 240 --;
    foot_force_low 45; use_terrain_adapt 0 and 1), bit for bit against the oracle: (i) 230 ticks of the set's staggered fleet (both filter windows wrap) with forces drawn
    ON 45 N and 50 N; (ii) the threshold scripts at the set's marks -- 150 / 240 and the next double, 45 N and the next double.  use_terrain_adapt = 0: the pitch comes back
    bit-unchanged on every tick.  Before the kernel text is stepped, the oracle alone shows that each parameter matters on these inputs: put back to 120, to 30 N or to
    use_terrain_adapt = 1, its result differs (gpu_common.assert_sensitive), and the fleet's counters hit the lift-off mark, the early-contact mark and the wrap."""
    import gpu_common as G
    ps = G.PARAM_SETS[name]
    rng = np.random.default_rng(2100 + adapt + ord(name))
    n, ticks = 12, 230
    kw = dict(counter_per_swing=ps["contact_per_swing"], foot_force_low=ps["foot_force_low"], use_terrain_adapt=adapt)
    gk = G.gait_kw(ps)
    gc, spd = G.gait_cycle_fleet(n, G.PARAM_SPEEDS, per_gait=gk["per_gait"], reset=gk["reset"])
    mm = np.ones((ticks, n), np.uint8)
    G.assert_thresholds_are_hit(gc, spd, mm, early_mark=G.early_mark(ps), **gk)
    base = np.outer([0.2, 0.2, -0.2, -0.2], [1.0, 0.0, 0.3]).reshape(12) + np.outer([1, -1, 1, -1], [0.0, 0.13, 0.0]).reshape(12)
    gcs = np.zeros((ticks, n, 4)); plans = np.zeros((ticks, n, 4), np.uint8)
    for t in range(ticks):
        gc, plans[t] = G.gait_loop(gc, spd, mm[t], **gk); gcs[t] = gc
    ffs = rng.choice(G.force_values(ps), size=(ticks, n, 4))
    foots = base + rng.normal(0, 0.03, (ticks, n, 12)) + np.tile([0.0, 0.0, -0.3], 4)
    zs = np.where(rng.random((ticks, n)) < 0.9, 0.3, 0.05)
    pitch0 = np.full(n, 0.0625)
    full = _oracle_contact_run(oracle, gcs, plans, ffs, foots, zs, pitch0, **kw)
    back = dict(counter_per_swing=dict(kw, counter_per_swing=120.0), foot_force_low=dict(kw, foot_force_low=30.0))
    if adapt == 0:
        back["use_terrain_adapt"] = dict(kw, use_terrain_adapt=1)
    G.assert_sensitive(f"N2b host, set {name}, adapt {adapt}", full, {k: _oracle_contact_run(oracle, gcs, plans, ffs, foots, zs, pitch0, **v) for k, v in back.items()})
    early = int(((full[0] == 1) & (plans.transpose(1, 0, 2) == 0)).sum())
    assert early >= n * ticks // 8, early
    H = n2b_host.HostN2b(20)
    pitch = pitch0.copy()
    for t in range(ticks):
        out = H.tick(gcs[t], plans[t], ffs[t], foots[t], zs[t], pitch, **kw); pitch = out["root_euler_d_pitch"]
        assert np.array_equal(out["contacts"], full[0][:, t]) and np.array_equal(out["foot_pos_recent_contact"], full[1][:, t]), t
        assert np.array_equal(out["terrain_angle"], full[2][:, t]) and np.array_equal(pitch, full[3][:, t]), t
        if adapt == 0:
            assert np.array_equal(pitch, pitch0), t
    assert np.abs(full[2]).max() > 0.0 and (adapt == 0 or not np.array_equal(full[3][:, -1], pitch0))
    T = n2b_host.HostN2b(80)
    scripts = G.contact_scripts(ps["counter_per_swing"], ps["foot_force_low"], ps["contact_per_swing"], ps["counter_per_gait"])
    worst = G.contact_threshold_run(lambda *a: T.tick(*a, **kw), oracle, 67, 0.0, scripts=scripts, adapt=adapt, counter_per_swing=ps["contact_per_swing"],
                                    foot_force_low=ps["foot_force_low"])
    print(f"N2b host, set {name}, adapt {adapt}: {early} early contacts, worst angle / pitch distance on the scripts {worst:.1e} (same libm: exact)")
