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
  python tools/preview_probe.py footholds [--parent OTHER_LIB.so] [--rounds 5] [--n N --h H] [--only null_target|target|parent]
      the preview launch (schedule + feet mode 2, one tick per step) at 4096 and 65 536 robots, h = 10 and 20, three ways that take turns: a null target (the existing
      entry), a non-null target (a1mpc_horizon_preview_footholds_batch_device) and the existing entry of --parent; half of the robots land a leg inside the horizon.
      ms per launch by the handle's events; under `rocprofv3 --kernel-trace --stats` the two kernels' own times are in the trace (the parent's kernel has the name of the
      null-target one: trace it in a run with --only parent)
  python tools/preview_probe.py tick-footholds [--parent OTHER_LIB.so] [--rounds 5] [--ticks 100] [--n 4096]
      steady-state control ticks at h = 10 whose legs 1 / 2 land inside the horizon: a1mpc_control_tick_preview_device {1, 2, 1} of --parent and of this build, and
      a1mpc_control_tick_preview_footholds_device {1, 2, 1}
  python tools/preview_probe.py pipeline [--rounds 5] [--n 4096]
      first solves (no warm start) of tick records + foothold feet + schedule at h = 10: a lone handle's a1mpc_solve_batch_ticks_strided_device against a depth-2
      a1mpc_pipeline_submit_ticks_strided_device over four distinct batches cycled eight times per round, solves per second
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


def _landing_inputs(rng, n, h, dev):
    """gait inputs in which leg 0 of every second robot crosses 240 inside the horizon (one tick per step), and random targets"""
    import torch
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    gc = rng.uniform(0, 240, (n, 4)); spd = rng.choice([1.0, 1.5, 2.0, 3.0], size=(n, 4))
    gc[::2, 0] = np.mod(240.0 - rng.uniform(0.05, 0.95, (n + 1) // 2) * (h - 1) * spd[::2, 0], 240.0)
    return dict(mm=T(np.ones(n, np.uint8)), gc=T(gc), spd=T(spd), ct=T((gc <= 120.0).astype(np.uint8)), foot=T(rng.normal(0, 0.2, (n, 12))),
                R=T(np.tile(np.eye(3).reshape(9), (n, 1))), vd=T(rng.normal(0, 0.5, (n, 3))), tg=T(rng.normal(0, 0.2, (n, 12))),
                sched=torch.zeros((n, 4 * h), dtype=torch.uint8, device=dev), feet=torch.zeros((n, 12 * h), dtype=torch.float64, device=dev))


def probe_footholds(a):
    import torch
    dev = torch.device("cuda", 0)
    p = lambda t: C.c_void_p(t.data_ptr())
    here = pkg.load_library()
    libs = [("null_target", here, False), ("target", here, True)] + ([("parent", pkg.load_library(a.parent), False)] if a.parent else [])
    if a.only:
        libs = [v for v in libs if v[0] == a.only]
    out = {"probe": "footholds", "rounds": a.rounds, "launches_per_round": 30, "order": [v[0] for v in libs]}
    for n in ((a.n,) if "--n" in sys.argv else (4096, 65536)):   # (--n / --h: that one shape, for a kernel trace whose statistics are per kernel name)
        for h in ((a.h,) if "--h" in sys.argv else (10, 20)):
            cfg = pkg.make_config(pkg.scenarios.PARAM_SETS["gazebo"] | pkg.scenarios.MPC_CONSTANTS, h)
            d = _landing_inputs(np.random.default_rng(3), n, h, dev)
            pv = E.PreviewConfig(1, 2, 1)
            live = []
            for name, lib, tgt in libs:
                hd = C.c_void_p(); assert lib.a1mpc_create(C.byref(cfg), n, 0, C.byref(hd)) == 0, lib.a1mpc_last_error()
                gait = E.GaitConfig(); lib.a1mpc_default_gait_config(C.byref(gait))
                if tgt:
                    run = lambda lib=lib, hd=hd, gait=gait: lib.a1mpc_horizon_preview_footholds_batch_device(hd, C.byref(pv), C.byref(gait), n, p(d["mm"]), p(d["gc"]), p(d["spd"]), p(d["ct"]), p(d["foot"]), p(d["R"]), p(d["vd"]), p(d["tg"]), p(d["sched"]), p(d["feet"]), None)
                else:
                    run = lambda lib=lib, hd=hd, gait=gait: lib.a1mpc_horizon_preview_batch_device(hd, C.byref(pv), C.byref(gait), n, p(d["mm"]), p(d["gc"]), p(d["spd"]), p(d["ct"]), p(d["foot"]), p(d["R"]), p(d["vd"]), p(d["sched"]), p(d["feet"]), None)
                for _ in range(20):
                    assert run() == 0, lib.a1mpc_last_error()
                live.append((name, lib, hd, run, []))
            for _ in range(a.rounds):
                for name, lib, hd, run, meds in live:
                    ms = []
                    for _ in range(30):
                        assert run() == 0
                        v = C.c_float(0); assert lib.a1mpc_last_kernel_ms(hd, C.byref(v)) == 0
                        ms.append(float(v.value))
                    meds.append(float(np.median(ms)))
            torch.cuda.synchronize()
            landed = None
            for name, lib, hd, run, meds in live:
                out[f"n{n}_h{h}_{name}"] = {"us_median_of_rounds": round(1e3 * float(np.median(meds)), 3), "us_rounds": [round(1e3 * m, 3) for m in meds]}
                lib.a1mpc_destroy(hd)
            c = d["sched"].cpu().numpy().reshape(n, h, 4)
            out[f"n{n}_h{h}_robots_with_a_touchdown"] = round(float(((c[:, 1:] == 1) & (c[:, :-1] == 0)).any(axis=(1, 2)).mean()), 3)
    print(json.dumps(out))


def probe_tick_footholds(a):
    import torch
    dev = torch.device("cuda", 0); st = torch.cuda.Stream(device=dev); sp = C.c_void_p(st.cuda_stream)
    n = a.n
    cfg = pkg.make_config(pkg.scenarios.PARAM_SETS["gazebo"] | pkg.scenarios.MPC_CONSTANTS, 10, warm_start=1)
    here = pkg.load_library()
    variants = ([("parent_feet2", pkg.load_library(a.parent), False)] if a.parent else []) + [("feet2", here, False), ("footholds", here, True)]
    if a.only:
        variants = [v for v in variants if v[0] == a.only]
    pv = E.PreviewConfig(1, 2, 1)
    live, runs = [], {}
    for name, lib, fh in variants:
        h = C.c_void_p(); assert lib.a1mpc_create(C.byref(cfg), n, 0, C.byref(h)) == 0, lib.a1mpc_last_error()
        prm = E.TickParams(); lib.a1mpc_default_tick_params(C.byref(prm))
        d, bf = tick_world(n, dev)
        fn = lib.a1mpc_control_tick_preview_footholds_device if fh else lib.a1mpc_control_tick_preview_device
        start = torch.from_numpy(np.tile([110.0, 230.0, 230.0, 110.0], (n, 1))).to(dev)   # legs 1 / 2 in swing, landing within the horizon's 18 counts
        def tick(fn=fn, h=h, prm=prm, bf=bf, d=d, start=start):
            with torch.cuda.stream(st):
                d["gait_counter"].copy_(start)   # every tick sees the same phase: the landing stays inside the horizon however many ticks run
            return fn(h, C.byref(prm), C.byref(pv), C.byref(bf), n, sp)
        for _ in range(32):
            assert tick() == 0, lib.a1mpc_last_error()
        st.synchronize()
        live.append((name, lib, h, tick, d)); runs[name] = {"ms_per_tick": []}
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for name, lib, h, tick, d in live:
            tick(); e0.record(st)
            for _ in range(a.ticks):
                tick()
            e1.record(st); st.synchronize()
            runs[name]["ms_per_tick"].append(round(e0.elapsed_time(e1) / a.ticks, 5))
    for name, lib, h, tick, d in live:
        r = runs[name]
        r["mean_ms_per_tick"] = round(float(np.mean(r["ms_per_tick"])), 5); r["spread_ms"] = round(float(np.max(r["ms_per_tick"]) - np.min(r["ms_per_tick"])), 5)
        r["mean_mpc_iters"] = float(d["iters"].float().mean().item()); r["solved_frac"] = float((d["status"] == 1).float().mean().item())
        lib.a1mpc_destroy(h)
    print(json.dumps({"probe": "tick-footholds", "n": n, "h": 10, "ticks_per_run": a.ticks, "rounds": a.rounds, "order": [v[0] for v in variants], "runs": runs}))


def probe_pipeline(a):
    import time
    import torch
    dev = torch.device("cuda", 0)
    n, h, NB, CYCLES = a.n, 10, 4, 8   # 32 first solves per timed round: the pipeline's start and drain are a thirty-second of it
    T = lambda x, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dtype=dt)
    scs = [pkg.scenarios.config3_random_flat(nb=n, horizon=h, seed=40 + k) for k in range(NB)]
    cfg = pkg.make_config(scs[0]["params"], h, warm_start=0)
    rng = np.random.default_rng(11)
    ins = []
    with pkg.Engine(cfg, n, 0) as eng:
        pv = eng.preview_config(contact_schedule=1, foot_preview=2, ticks_per_step=3)
        for sc in scs:
            gc = rng.uniform(0, 240, (n, 4)); spd = rng.choice([1.0, 1.5, 2.0, 3.0], size=(n, 4))
            gc[::2, 0] = np.mod(240.0 - rng.uniform(0.05, 0.95, (n + 1) // 2) * (h - 1) * 3 * spd[::2, 0], 240.0)
            tg = sc["foot"] + rng.normal(0, 0.05, (n, 12))
            p = eng.horizon_preview(np.ones(n, np.uint8), gc, spd, (gc <= 120.0).astype(np.uint8), sc["foot"], sc["R"], sc["tick"][:, 15:18], preview=pv, foot_target_abs=tg)
            ins.append([T(sc["tick"]), T(sc["R"]), T(p["foot_steps"]), T(p["contact_sched"], torch.uint8)])
        outs = [(torch.zeros(n, 12, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)) for _ in range(NB)]
        ptr = lambda t: C.c_void_p(t.data_ptr())
        lone = []
        for r in range(a.rounds + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for (tk, R, ft, ct), o in list(zip(ins, outs)) * CYCLES:
                eng.set_schedule(True)   # a fresh batch: no history of the previous one
                assert eng.lib.a1mpc_solve_batch_ticks_strided_device(eng._h, n, ptr(tk), ptr(R), ptr(ft), 12, ptr(ct), 4, None, ptr(o[0]), None, ptr(o[1]), ptr(o[2]), None) == 0
            torch.cuda.synchronize(); lone.append(CYCLES * NB * n / (time.perf_counter() - t0))
        solved = float(np.mean([(o[2] == 1).float().mean().item() for o in outs]))
    piped = []
    with pkg.Pipeline(cfg, n, 0, depth=2) as pipe:
        for r in range(a.rounds + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for (tk, R, ft, ct), o in list(zip(ins, outs)) * CYCLES:   # (a batch's output set is overwritten by its next turn: only the time is read here)
                pipe.submit_ticks_strided_device(n, tk, R, ft, 12, ct, 4, o[0], None, o[1], o[2])
            pipe.wait(); piped.append(CYCLES * NB * n / (time.perf_counter() - t0))
    print(json.dumps({"probe": "pipeline", "n": n, "h": h, "batches": NB, "solves_per_round": CYCLES * NB, "solved_frac": solved, "lone_solves_per_s": [round(v) for v in lone[1:]],
                      "pipelined_solves_per_s": [round(v) for v in piped[1:]], "lone_median": round(float(np.median(lone[1:]))), "pipelined_median": round(float(np.median(piped[1:])))}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["tick", "kernel", "footholds", "tick-footholds", "pipeline"])
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--h", type=int, default=20)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    if a.n is None:
        a.n = 65536 if a.what == "kernel" else 4096
    {"tick": probe_ticks, "kernel": probe_kernel, "footholds": probe_footholds, "tick-footholds": probe_tick_footholds, "pipeline": probe_pipeline}[a.what](a)
