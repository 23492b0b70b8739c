#!/usr/bin/env python3
"""Runs ON THE GPU BOX: what the gait-aware horizon costs (profiles/horizon_preview.md).

  python tools/preview_probe.py tick [--parent OTHER_LIB.so] [--rounds 5] [--ticks 100] [--n 4096] [--only plain|sched|feet]
      steady-state control ticks of n warm-started robots at h = 10 (the inputs of bench.py's full_control_tick block), one handle per variant:
        parent   a1mpc_control_tick_device of another build of the library (--parent: the commit before the preview existed), if given
        plain    a1mpc_control_tick_device of the in-tree library
        sched    a1mpc_control_tick_preview_device {1, 0, 1}
        feet     a1mpc_control_tick_preview_device {1, 1, 1}
      The variants take turns, `rounds` times (what a run measures follows its position in the sequence, profiles/r06_control_tick_timeline.md): per run the mean over
      `ticks` back-to-back ticks between two events on the caller's stream, and the last tick by the handle's own events (a1mpc_last_control_tick_ms).
  python tools/preview_probe.py kernel [--n 65536] [--h 20]
      a1mpc_horizon_preview_batch_device alone (schedule + feet mode 2), ticks_per_step 1 and 16: ms per launch by the handle's events (a1mpc_last_kernel_ms), bytes moved, TB/s
One JSON line per call."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
E = pkg.engine


def tick_world(n, dev, seed=7):
    """device arrays of one handle's control ticks: bench.full_tick_probe's inputs"""
    import torch
    rng = np.random.default_rng(seed); scen = pkg.scenarios
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    eul = rng.normal(0, 0.03, (n, 3)); eul[:, 2] = rng.uniform(-1, 1, n)
    inp = dict(joint_pos=np.tile([0.0, 0.8, -1.6], (n, 4)) + rng.normal(0, 0.05, (n, 12)), joint_vel=rng.normal(0, 0.3, (n, 12)),
               R_world=scen.rot_zyx(eul[:, 0], eul[:, 1], eul[:, 2]).reshape(n, 9), R_z=scen.rot_zyx(0 * eul[:, 0], 0 * eul[:, 0], eul[:, 2]).reshape(n, 9), root_euler=eul,
               root_ang_vel=rng.normal(0, 0.1, (n, 3)), imu_acc=np.array([0, 0, 9.81]) + rng.normal(0, 0.1, (n, 3)), imu_ang_vel=rng.normal(0, 0.1, (n, 3)),
               foot_force=rng.uniform(20, 120, (n, 4)), movement_mode=np.ones(n, np.uint8), mpc_active=np.ones(n, np.uint8),
               root_lin_vel_d=np.c_[rng.uniform(-0.3, 0.3, (n, 2)), np.zeros(n)], root_ang_vel_d=np.c_[np.zeros((n, 2)), rng.uniform(-0.3, 0.3, n)], root_pos_d_z=np.full(n, 0.3),
               gait_counter_speed=np.full((n, 4), 2.0), torques_gravity=rng.normal(0, 0.3, (n, 12)),
               gait_counter=np.tile([0.0, 120.0, 120.0, 0.0], (n, 1)), root_euler_d=np.c_[np.zeros((n, 2)), eul[:, 2]])
    f64 = dict(foot_pos_start=12, foot_pos_rel_last_time=12, foot_pos_target_last_time=12, joint_torques=12, root_pos=3, root_lin_vel=3, foot_pos_rel=12, j_foot_blocks=36,
               foot_vel_rel=12, foot_pos_abs=12, foot_vel_abs=12, foot_pos_world=12, foot_vel_world=12, foot_pos_target_rel=12, foot_pos_target_abs=12, foot_pos_target_world=12,
               foot_pos_cur=12, foot_forces_kin=12, foot_pos_recent_contact=12, terrain_angle=1, grf=12)
    d = {k: T(v) for k, v in inp.items()}
    d.update({k: torch.zeros((n, m), dtype=torch.float64, device=dev) for k, m in f64.items()})
    d.update({k: torch.zeros((n, 4), dtype=torch.uint8, device=dev) for k in ("estimated_contacts", "plan_contacts", "contacts")})
    d.update({k: torch.zeros(n, dtype=torch.int32, device=dev) for k in ("iters", "status")})
    bf = E.TickBuffers()
    for k in E.TICK_BUFFER_FIELDS:
        setattr(bf, k, d[k].data_ptr())
    return d, bf


def probe_ticks(a):
    import torch
    dev = torch.device("cuda", 0); st = torch.cuda.Stream(device=dev); sp = C.c_void_p(st.cuda_stream)
    n = a.n
    cfg = pkg.make_config(pkg.scenarios.PARAM_SETS["gazebo"] | pkg.scenarios.MPC_CONSTANTS, 10, warm_start=1)
    here = pkg.load_library()
    variants = []   # (name, library, preview config or None)
    if a.parent:
        variants.append(("parent", pkg.load_library(a.parent), None))
    variants += [("plain", here, None), ("sched", here, E.PreviewConfig(1, 0, 1)), ("feet", here, E.PreviewConfig(1, 1, 1))]
    if a.only:
        variants = [v for v in variants if v[0] == a.only]
    runs = {}
    live = []
    for name, lib, pv in variants:
        h = C.c_void_p()
        assert lib.a1mpc_create(C.byref(cfg), n, 0, C.byref(h)) == 0, lib.a1mpc_last_error()
        prm = E.TickParams(); lib.a1mpc_default_tick_params(C.byref(prm))
        d, bf = tick_world(n, dev)
        if pv is None:
            tick = lambda lib=lib, h=h, prm=prm, bf=bf: lib.a1mpc_control_tick_device(h, C.byref(prm), C.byref(bf), n, sp)
        else:
            tick = lambda lib=lib, h=h, prm=prm, bf=bf, pv=pv: lib.a1mpc_control_tick_preview_device(h, C.byref(prm), C.byref(pv), C.byref(bf), n, sp)
        for _ in range(32):   # (the first tick runs the split pipeline; the GPU needs a few ms of work to reach its steady clocks)
            assert tick() == 0, lib.a1mpc_last_error()
        st.synchronize()
        live.append((name, lib, h, tick, d))
        runs[name] = {"ms_per_tick": [], "last_tick_ms": []}
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for name, lib, h, tick, d in live:
            tick()
            e0.record(st)
            for _ in range(a.ticks):
                tick()
            e1.record(st)
            st.synchronize()
            ms = C.c_float(0); fused = C.c_int32(0)
            assert lib.a1mpc_last_control_tick_ms(h, C.byref(ms), C.byref(fused)) == 0
            runs[name]["ms_per_tick"].append(round(e0.elapsed_time(e1) / a.ticks, 5)); runs[name]["last_tick_ms"].append(round(float(ms.value), 5))
            runs[name]["torques_fused"] = int(fused.value)
    for name, lib, h, tick, d in live:
        r = runs[name]
        r["mean_ms_per_tick"] = round(float(np.mean(r["ms_per_tick"])), 5); r["spread_ms"] = round(float(np.max(r["ms_per_tick"]) - np.min(r["ms_per_tick"])), 5)
        r["mean_mpc_iters"] = float(d["iters"].float().mean().item()); r["solved_frac"] = float((d["status"] == 1).float().mean().item())
        lib.a1mpc_destroy(h)
    print(json.dumps({"probe": "tick", "n": n, "h": 10, "ticks_per_run": a.ticks, "rounds": a.rounds, "order": [v[0] for v in variants], "runs": runs}))


def probe_kernel(a):
    import torch
    dev = torch.device("cuda", 0)
    n, h = a.n, a.h
    rng = np.random.default_rng(3)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    cfg = pkg.make_config(pkg.scenarios.PARAM_SETS["gazebo"] | pkg.scenarios.MPC_CONSTANTS, h)
    mm = T(np.ones(n, np.uint8)); gc = T(rng.uniform(0, 240, (n, 4))); spd = T(rng.choice([1.0, 1.5, 2.0, 3.0], size=(n, 4))); ct = T(np.ones((n, 4), np.uint8))
    foot = T(rng.normal(0, 0.2, (n, 12))); R = T(np.tile(np.eye(3).reshape(9), (n, 1))); vd = T(rng.normal(0, 0.5, (n, 3)))
    sched = torch.zeros((n, 4 * h), dtype=torch.uint8, device=dev); feet = torch.zeros((n, 12 * h), dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    out = {"probe": "kernel", "n": n, "h": h, "bytes_written_per_robot": 4 * h + 96 * h, "bytes_read_per_robot": 1 + 32 + 32 + 4 + 96 + 72 + 24}
    with pkg.Engine(cfg, n, 0) as eng:
        gait = E.GaitConfig(); eng.lib.a1mpc_default_gait_config(C.byref(gait))
        for tps in (1, 16):
            for what, s_, f_ in (("schedule+feet", sched, feet), ("schedule", sched, None), ("feet", None, feet)):
                pv = E.PreviewConfig(1, 2, tps)
                ms = []
                for i in range(40):
                    rc = eng.lib.a1mpc_horizon_preview_batch_device(eng._h, C.byref(pv), C.byref(gait), n, p(mm), p(gc), p(spd), p(ct), p(foot), p(R), p(vd),
                                                                    p(s_) if s_ is not None else None, p(f_) if f_ is not None else None, None)
                    assert rc == 0, eng.lib.a1mpc_last_error()
                    if i >= 10:
                        ms.append(eng.last_kernel_ms())
                med = float(np.median(ms))
                moved = n * ((4 * h if s_ is not None else 0) + (96 * h if f_ is not None else 0) + ((1 + 32 + 32 + 4) if s_ is not None else 0) + ((96 + 72 + 24) if f_ is not None else 0))
                out[f"tps{tps}_{what}"] = {"ms_median": round(med, 5), "ms_min": round(float(np.min(ms)), 5), "TB_per_s": round(moved / (med * 1e-3) / 1e12, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["tick", "kernel"])
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--h", type=int, default=20)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    if a.n is None:
        a.n = 4096 if a.what == "tick" else 65536
    probe_ticks(a) if a.what == "tick" else probe_kernel(a)
