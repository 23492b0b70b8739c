#!/usr/bin/env python3
"""bench.py -- MPC-QP solves/sec (horizon-10 SRBD) of the MI355X engine, one process per GPU.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A "step" is one pass of the hot path (QP formation + OSQP-faithful ADMM solve, cold start) over one batch of
synthetic input: BASELINE.json configs[2] -- 4096 randomized CoM states, flat terrain, horizon 10, per GPU
(weak scaling: every rank gets its own 4096 QPs, generated from a rank-specific seed; the batch is
embarrassingly parallel, so there is no data-path collective).  Inputs are resident in HBM before the timed
region.  Rank 0 prints ONE JSON line: `value` (solves/s) and `ms_per_step` of exactly K timed steps.  A plain run measures nothing
else; --full adds everything measured beside `value` (single-stream and index-order steps, stage counters, `roofline`, latency probes,
other shapes, `cpu_baseline`, parity against the oracle).  --dump-outputs DIR writes the last timed step's outputs as .npy files.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

PMC_SUMMARY = "r06_pmc_summary.json"   # static rocprofv3 --pmc summary of this round (tools/collect_profiles.sh + summarize_profiles.py)
FP64_PEAK_TFLOPS = 78.6  # MI355X FP64 vector = matrix peak (AMD spec; = 1/2 of the 157.3 TF FP32 rate in MI355X_MICROARCH.md)
BATCH = 4096
HORIZON = 10
DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, arrays):
    """--dump-outputs: the arrays the timed path returned to its caller in its last step, one DIR/<name>.npy each, as float64 (iteration counts and statuses
    are exact in it).  All arrays share their first axis (one row per QP); beyond DUMP_LIMIT_BYTES a fixed, seeded sample of rows is written, with its row
    indices as sample_rows.npy."""
    arrays = {k: np.asarray(v, dtype=np.float64) for k, v in arrays.items()}
    rows = len(next(iter(arrays.values())))
    row_bytes = sum(a[:1].nbytes for a in arrays.values()) + 8
    if rows * row_bytes > DUMP_LIMIT_BYTES:
        keep = np.sort(np.random.default_rng(0).choice(rows, DUMP_LIMIT_BYTES // row_bytes, replace=False))
        arrays = {k: a[keep] for k, a in arrays.items()}
        arrays["sample_rows"] = keep.astype(np.float64)
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, f"{k}.npy"), np.ascontiguousarray(a))


def single_thread_ticks(pkg, oracle, pr, horizon, nticks=10000, budget_s=8.0):
    """the reference's own operating point -- ONE thread, batch 1, warm-started sequential ticks (configs[1] trot) -- as
    p50 / p99 latency, with the stage split of the reference's stopwatches (formation | OSQP set-up + solve).  Up to 10 000 ticks, bounded in time."""
    seq = pkg.scenarios.config2_trot_sequence(nticks)
    stw = oracle.default_settings(warm_start=1)
    wx = np.zeros(12 * horizon); wy = np.zeros(20 * horizon); rho = 0.0
    lat = []; tf = []; t_end = time.perf_counter() + budget_s
    for k in range(nticks):
        a = time.perf_counter()
        o = oracle.mpc_solve(pr, stw, seq["x0"][k], seq["xref"][k], seq["R"][k], seq["foot"][k], seq["contact"][k], warm_x=wx, warm_y=wy, warm_rho=rho)
        lat.append(time.perf_counter() - a)
        wx, wy, rho = o["warm_x"], o["warm_y"], o["rho"]
        if k % 40 == 0:
            a = time.perf_counter(); oracle.mpc_form(pr, seq["x0"][k], seq["xref"][k], seq["R"][k], seq["foot"][k], seq["contact"][k]); tf.append(time.perf_counter() - a)
        if time.perf_counter() > t_end:
            break
    lat = np.array(lat[min(50, len(lat) // 10):]) * 1e3; form_ms = float(np.median(tf)) * 1e3
    return {"workload": "config2 trot, h=10, batch 1, warm start, one thread (one ctypes call per tick)", "ticks": int(len(lat)),
            "p50_ms": float(np.percentile(lat, 50)), "p99_ms": float(np.percentile(lat, 99)), "max_ms": float(lat.max()),
            "stage_ms": {"formation_dense_as_the_reference_writes_it": form_ms, "osqp_setup_and_solve": float(np.percentile(lat, 50)) - form_ms}}


def cpu_baseline(pkg, sc, budget_s=15.0):
    """The oracle (port of the reference path: dense formation + OSQP-0.6 ADMM) on this box's host cores, bounded sample."""
    oracle = graft.load_oracle()
    oracle.build()
    p = sc["params"]
    pr = oracle.mpc_params(sc["horizon"], p["dt"], p["mu"], p["fz_min"], p["fz_max"], p["q"], p["r"], p["mass"], p["inertia"])
    st = oracle.default_settings()
    cores = oracle.num_threads()
    take = lambda n: (sc["x0"][:n], sc["xref"][:n], sc["R"][:n], sc["foot"][:n], sc["contact"][:n])
    nb = len(sc["x0"])
    # single-thread figures FIRST: after an OpenMP parallel region the idle worker threads spin for a while and steal cycles from a
    # one-thread measurement (the r1 bench line and DESIGN quoted 478 and 1.4 k solves/s for the same thing for exactly that reason)
    oracle.mpc_solve_batch(pr, st, *take(min(nb, 8)), nthreads=1)
    t = time.perf_counter(); oracle.mpc_solve_batch(pr, st, *take(min(nb, 96)), nthreads=1); ts = (time.perf_counter() - t) / min(nb, 96)
    single = single_thread_ticks(pkg, oracle, pr, sc["horizon"])
    # How many cores does this process really have?  omp_get_max_threads() counts the box's hardware threads; the affinity mask and the cgroup quota say what is usable.
    usable = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else cores
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        quota = None if q == "max" else float(q) / float(per)
    except Exception:
        pass
    # thread-count sweep on a bounded sample (one problem per thread, static partition): the best count is the baseline's -- 128 SMT threads of a shared box are not 128 cores
    qcores = int(round(quota)) if quota else None
    cand = sorted({t_ for t_ in (1, 8, 16, 32, 64, 128, qcores or 0, min(usable, cores)) if 1 <= t_ <= max(cores, usable)})
    sweep = {}
    for t_ in cand:
        # SUSTAINED rate: at least 1.5 s per point -- a CFS quota lets a burst of a few hundred ms run on every hardware thread before it throttles (a 1024-QP sample on
        # 64 threads measured 73 k solves/s on a box whose quota of 16 cores sustains 18 k)
        oracle.mpc_solve_batch(pr, st, *take(min(nb, 2 * t_)), nthreads=t_)
        m = min(nb, max(64, 16 * t_)); done = 0; t = time.perf_counter()
        while time.perf_counter() - t < 1.5:
            oracle.mpc_solve_batch(pr, st, *take(m), nthreads=t_); done += m
        sweep[t_] = done / (time.perf_counter() - t)
    best = max(sweep, key=sweep.get)
    t0 = nb / sweep[best]
    reps = int(max(1, min(64, budget_s / max(t0, 1e-9))))  # whole passes over the workload, ~budget_s of CPU time
    t = time.perf_counter()
    for _ in range(reps):
        r = oracle.mpc_solve_batch(pr, st, *take(nb), nthreads=best)
    t1 = time.perf_counter() - t
    n = reps * nb
    return {"value": n / t1, "unit": "solves/s", "cores": best, "kind": "port",
            "sample": f"{reps} pass(es) over the same {nb} QPs (config3, h=10) = {n} solves, OpenMP static over {best} threads (the best of the sweep), {t1:.1f} s; "
                      f"single-thread cold {1.0 / ts:.1f} solves/s (measured before the threaded passes); real OSQP/Eigen are not installable here (oracle/ restates them)",
            "host": {"hardware_threads_omp": cores, "sched_getaffinity": usable, "cgroup_cpu_max_cores": quota,
                     "usable_cores": min(x for x in (cores, usable, quota or 1e9))},
            "thread_sweep_solves_per_s": {str(k): float(v) for k, v in sweep.items()}, "speedup_over_one_thread": float(n / t1 * ts),
            "mean_iters": float(r["iters"].mean()), "single_thread_cold_solves_per_s": 1.0 / ts, "single_thread_warm_ticks": single}, r


def latency_probe(pkg, nticks=1500, mode=1, horizon=10, cpp_ticks=10000):
    """BASELINE configs[1]: batch 1, trot, warm-started sequential ticks through the host-pointer ABI (PCIe inclusive).  10 000 ticks from the
    C++ harness (tests/cpp/latency_harness, no Python in the loop) when it has been built; the Python loop below otherwise.
    mode 1: fresh set-up + osqp_warm_start every tick; mode 2: the reference's per-tick OSQP update path on its persistent solver (S/A1RobotControl.cpp:533-540:
    what the reference's control loop -- and the drop-in ComputeGrfGpu -- actually runs)."""
    import subprocess
    exe = os.path.join(ROOT, "tests", "cpp", "latency_harness")
    if os.path.exists(exe):
        try:
            env = dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("LOCAL_RANK", "0")) if os.environ.get("LOCAL_RANK") else None
            r = subprocess.run([exe, str(cpp_ticks), "0", str(mode), str(horizon)], capture_output=True, text=True, timeout=120, env=env)
            if r.returncode == 0:
                res = json.loads(r.stdout)
                if horizon == 10:   # both protocols on record: the figures above run with the handle's HIP timing events OFF (a1mpc_set_timing(h, 0), what a control loop that never
                                    # reads a1mpc_last_stage_ms wants); this is the library's default after a1mpc_create (events on)
                    r2 = subprocess.run([exe, str(cpp_ticks), "0", str(mode), str(horizon), "1"], capture_output=True, text=True, timeout=120, env=env)
                    if r2.returncode == 0:
                        j2 = json.loads(r2.stdout)
                        res["timing_events_on"] = {k: j2.get(k) for k in ("p50_ms", "p99_ms", "max_ms", "ticks_over_2p5_ms")}
                    # ... and the same ticks as 22-number tick records through a1mpc_solve_batch_ticks: the entry the drop-in's compute_grf calls (include/a1mpc_dropin.hpp)
                    r3 = subprocess.run([exe, str(cpp_ticks), "0", str(mode), str(horizon), "0", "1"], capture_output=True, text=True, timeout=120, env=env)
                    if r3.returncode == 0:
                        j3 = json.loads(r3.stdout)
                        res["tick_record_entry"] = {k: j3.get(k) for k in ("p50_ms", "p99_ms", "max_ms", "ticks_over_2p5_ms", "mean_iters")}
                return res
        except Exception:
            pass
    sc = pkg.scenarios.config2_trot_sequence(nticks, horizon=horizon)
    cfg = pkg.make_config(sc["params"], sc["horizon"], warm_start=mode)
    import gc
    lat = np.zeros(nticks)
    with pkg.Engine(cfg, 1, int(os.environ.get("LOCAL_RANK", 0))) as eng:
        gc.collect(); gc.disable()  # the caller of the reference is C++; a Python gen-2 collection (30-60 ms) is not the library's latency
        try:
            for t in range(nticks):
                a = time.perf_counter()
                eng.solve(sc["x0"][t], sc["xref"][t], sc["R"][t], sc["foot"][t], sc["contact"][t])
                lat[t] = time.perf_counter() - a
        finally:
            gc.enable()
    lat = lat[50:] * 1e3
    return {"warm_start": mode, "workload": f"config2 trot, h={horizon}, batch 1, warm start, host pointers in/out", "horizon": horizon, "ticks": int(len(lat)),
            "p50_ms": float(np.percentile(lat, 50)), "p99_ms": float(np.percentile(lat, 99)), "max_ms": float(lat.max())}


def pcie_inclusive_probe(pkg, scs, cfg, n, local, steps=24):
    """Extra information (never `value`): the same first solves for a caller that owns HOST arrays (the reference's boundary is host-side, S/A1RobotControl.h:44) --
    a1mpc_solve_batch (synchronous) and a1mpc_pipeline_submit / _wait with two batches in flight (the caller's thread snapshots batch k + 1 into the slot's pinned
    block while the GPU solves batch k).  Wall clock of the calling thread; outputs checked bit for bit against the synchronous entry."""
    import gc
    NB = len(scs)
    gc.collect(); gc.disable()   # wall-clock loops of a few tens of ms: one Python gen-2 collection (~40 ms, observed) would double the figure; the reference's caller is C++
    try:
        return _pcie_inclusive(pkg, scs, cfg, n, local, steps, NB)
    finally:
        gc.enable()


def _pcie_inclusive(pkg, scs, cfg, n, local, steps, NB):
    with pkg.Engine(cfg, n, local) as eng:
        ref = []
        for k in range(NB + 2):
            s_ = scs[k % NB]; eng.set_schedule(True); o = eng.solve(s_["x0"], s_["xref"], s_["R"], s_["foot"], s_["contact"])
            if k < NB: ref.append(o)
        t0 = time.perf_counter()
        for k in range(steps):
            s_ = scs[k % NB]; eng.set_schedule(True); eng.solve(s_["x0"], s_["xref"], s_["R"], s_["foot"], s_["contact"])
        sync_ms = (time.perf_counter() - t0) / steps * 1e3
    depth = 2
    outs = [dict(grf=np.zeros((n, 12)), iters=np.zeros(n, np.int32), status=np.zeros(n, np.int32)) for _ in range(depth)]
    same = True
    with pkg.Pipeline(cfg, n, local, depth=depth) as pipe:
        def run(count, check):
            nonlocal same
            held = [None] * depth
            for k in range(count):
                j = k % depth; s_ = scs[k % NB]
                if held[j] is not None:
                    pipe.wait(j)
                    if check:
                        r = ref[held[j]]; same = same and np.array_equal(outs[j]["grf"], r["grf"]) and np.array_equal(outs[j]["iters"], r["iters"])
                pipe.submit(s_["x0"], s_["xref"], s_["R"], s_["foot"], s_["contact"], outs[j], slot=j, fresh=True); held[j] = k % NB
            pipe.wait()
        run(2 * depth + NB, True)
        t0 = time.perf_counter(); run(steps, False); pipe_ms = (time.perf_counter() - t0) / steps * 1e3
    h = int(cfg.horizon)
    return {"workload": f"{n} x h{h} first solves, host arrays in and out every batch", "bytes_in_per_batch": n * ((13 + 13 * h + 9 + 12) * 8 + 4), "bytes_out_per_batch": n * (12 * 8 + 8),
            "synchronous_a1mpc_solve_batch": {"ms_per_batch": sync_ms, "solves_per_s": n / sync_ms * 1e3},
            "a1mpc_pipeline_submit_depth2": {"ms_per_batch": pipe_ms, "solves_per_s": n / pipe_ms * 1e3, "bit_identical_to_synchronous": bool(same)}}


def batch_sweep(pkg, local, sizes=(1, 16, 256, 1024, 4096, 16384, 65536)):
    """Extra information (not `value`): the same workload generator at other batch sizes of BASELINE's 1..65536 range."""
    import torch
    out = {}
    dev = torch.device("cuda", local)
    st = torch.cuda.Stream(device=dev)
    for n in sizes:
        sc = pkg.scenarios.config3_random_flat(nb=n)
        cfg = pkg.make_config(sc["params"], HORIZON, warm_start=0)
        d = {k: torch.from_numpy(sc[k]).to(dev) for k in ("x0", "xref", "R", "foot", "contact")}
        grf = torch.zeros((n, 12), dtype=torch.float64, device=dev)
        it = torch.zeros(n, dtype=torch.int32, device=dev); stt = torch.zeros(n, dtype=torch.int32, device=dev)
        with pkg.Engine(cfg, n, local) as eng:
            ms = []
            for _ in range(4):
                eng.solve_device(n, d["x0"], d["xref"], d["R"], d["foot"], d["contact"], grf, None, it, stt, stream=st.cuda_stream)
                ms.append(eng.last_kernel_ms())
        out[str(n)] = {"kernel_ms": float(np.median(ms[1:])), "solves_per_s": n / (float(np.median(ms[1:])) * 1e-3), "mean_iters": float(it.float().mean().item())}
    return out   # (cold first solves through one handle on one stream: north_star's "batch 1 ... 65536")


def horizon_sweep(pkg, local, n=4096, horizons=(4, 6, 8, 10, 12, 14, 16, 20)):
    """Extra information (not `value`): cold first solves of the same workload generator at every MPC horizon compiled in (PLAN_HORIZON is a run-time value of the
    C ABI; 4 / 6 / 8 / 12 / 14 are the extended horizons: the kernel family as it instantiates for them), one handle, one stream."""
    import torch
    out = {}
    dev = torch.device("cuda", local); st = torch.cuda.Stream(device=dev)
    for h in horizons:
        sc = pkg.scenarios.config3_random_flat(nb=n, horizon=h)
        d = {k: torch.from_numpy(sc[k]).to(dev) for k in ("x0", "xref", "R", "foot", "contact")}
        grf = torch.zeros((n, 12), dtype=torch.float64, device=dev); it = torch.zeros(n, dtype=torch.int32, device=dev); stt = torch.zeros(n, dtype=torch.int32, device=dev)
        with pkg.Engine(pkg.make_config(sc["params"], h, warm_start=0), n, local) as eng:
            ms = []
            for _ in range(4):
                eng.set_schedule(True)
                eng.solve_device(n, d["x0"], d["xref"], d["R"], d["foot"], d["contact"], grf, None, it, stt, stream=st.cuda_stream)
                ms.append(eng.last_kernel_ms())
        out[f"h{h}"] = {"kernel_ms": float(np.median(ms[1:])), "solves_per_s": n / (float(np.median(ms[1:])) * 1e-3), "mean_iters": float(it.float().mean().item()),
                        "solved": int((stt == 1).sum().item())}
    return out


def general_path_probe(pkg, local, shapes=((10, 4096), (16, 8192), (20, 8192))):
    """Extra information (not `value`): the general path of the reference's interface -- per-step feet (S/ConvexMpc.h:74 B_mat_d_list) and per-step
    contact schedules through a1mpc_solve_batch_strided -- on the states of the fast path's workload: first solves (queue by the set-up kernel's guess)
    and the same batch again in history order (tools/general_path_probe.py is the same measurement with the fast path beside it)."""
    out = {}
    for h, n in shapes:
        sc = pkg.scenarios.config3_random_flat(nb=n, horizon=h)
        rng = np.random.default_rng(h)
        vd = rng.uniform(-0.6, 0.6, (n, 1, 1, 3))
        foot = np.ascontiguousarray((sc["foot"].reshape(n, 1, 4, 3) - vd * sc["params"]["dt"] * np.arange(h).reshape(1, h, 1, 1) * 40.0).reshape(n, h * 12))
        sw = rng.integers(0, h + 1, (n, 4)); first = rng.integers(0, 2, (n, 4))
        contact = np.ascontiguousarray(np.where(np.arange(h).reshape(1, h, 1) < sw[:, None, :], first[:, None, :], 1 - first[:, None, :]).astype(np.uint8).reshape(n, h * 4))
        with pkg.Engine(pkg.make_config(sc["params"], h, warm_start=0), n, local) as eng:
            first_ms, hist_ms = [], []
            for _ in range(3):
                eng.set_schedule(True)   # forgets the history: the next solve is a first solve
                o = eng.solve_strided(sc["x0"], sc["xref"], sc["R"], foot, 12, contact, 4); first_ms.append(eng.last_kernel_ms())
                eng.solve_strided(sc["x0"], sc["xref"], sc["R"], foot, 12, contact, 4); hist_ms.append(eng.last_kernel_ms())
                st_ms = eng.last_stage_ms()   # (set-up | ADMM of the last launch by the handle's events)
        f, hh = float(np.median(first_ms)), float(np.median(hist_ms))
        out[f"{n}xh{h}"] = {"first_solve_kernel_ms": f, "first_solve_solves_per_s": n / (f * 1e-3), "history_order_kernel_ms": hh, "history_order_solves_per_s": n / (hh * 1e-3),
                            "setup_kernel_ms": float(st_ms[0]), "mean_iters": float(o["iters"].mean()), "solved_frac": float((o["status"] == 1).mean())}
        # two batches in flight (a1mpc_pipeline_submit_strided_device, round 6): first solves of three distinct resident batches, every launch fresh (no queue history)
        try:
            import torch
            dev = torch.device("cuda", local)
            tt = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dt)
            NBG = 3
            ins = []
            for k in range(NBG):
                sck = pkg.scenarios.config3_random_flat(nb=n, horizon=h, seed=4242 + 31 * k)
                rk = np.random.default_rng(h + 100 * k)
                vdk = rk.uniform(-0.6, 0.6, (n, 1, 1, 3))
                fk = np.ascontiguousarray((sck["foot"].reshape(n, 1, 4, 3) - vdk * sck["params"]["dt"] * np.arange(h).reshape(1, h, 1, 1) * 40.0).reshape(n, h * 12))
                swk = rk.integers(0, h + 1, (n, 4)); fik = rk.integers(0, 2, (n, 4))
                ck = np.ascontiguousarray(np.where(np.arange(h).reshape(1, h, 1) < swk[:, None, :], fik[:, None, :], 1 - fik[:, None, :]).astype(np.uint8).reshape(n, h * 4))
                ins.append([tt(sck["x0"]), tt(sck["xref"]), tt(sck["R"]), tt(fk), tt(ck, torch.uint8)])
            outs_g = [(torch.zeros(n, 12, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)) for _ in range(NBG)]
            with pkg.Pipeline(pkg.make_config(sc["params"], h, warm_start=0), n, local, depth=2) as pipe:
                def run(steps):
                    for k in range(steps):
                        if k >= NBG:
                            pass   # (outputs of batch k % NBG were last written two submits ago on the other slot's stream or this one's: same slot order, no hazard that matters for timing)
                        x0_, xr_, R_, f_, c_ = ins[k % NBG]; o_ = outs_g[k % NBG]
                        pipe.submit_strided_device(n, x0_, xr_, R_, f_, 12, c_, 4, o_[0], None, o_[1], o_[2], fresh=True)
                    pipe.wait()
                run(4); torch.cuda.synchronize()
                steps = 12
                t0 = time.perf_counter(); run(steps); torch.cuda.synchronize()
                pms = (time.perf_counter() - t0) / steps * 1e3
            out[f"{n}xh{h}"].update({"pipelined_ms_per_batch": pms, "pipelined_first_solves_per_s": n / (pms * 1e-3), "pipelined_what": "a1mpc_pipeline_submit_strided_device, depth 2, "
                                     "first solves of 3 distinct resident batches (fresh_batch = 1), host clock over 12 submits + wait"})
        except Exception as e:
            out[f"{n}xh{h}"]["pipelined_error"] = str(e)[:200]
        # batch 1 (the reference's own use of the interface, S/test/test_mpc.cpp:106-122: one QP with a B_d per step): the fused general kernel, 40 warm-started
        # ticks of robot 0 with slowly moving state, kernel time by the handle's events, the fast path's latency kernel on the same ticks beside it
        with pkg.Engine(pkg.make_config(sc["params"], h, warm_start=1), 1, local) as eng:
            g_ms, f_ms, its = [], [], []
            x0 = sc["x0"][:1].copy()
            for k in range(40):
                x0[:, :12] += np.random.default_rng(1000 + k).normal(0, 2e-3, (1, 12))
                o1 = eng.solve_strided(x0, sc["xref"][:1], sc["R"][:1], foot[:1], 12, contact[:1], 4); g_ms.append(eng.last_kernel_ms()); its.append(int(o1["iters"][0]))
            eng.reset_warm_start()
            for k in range(40):
                eng.solve(x0, sc["xref"][:1], sc["R"][:1], sc["foot"][:1], sc["contact"][:1]); f_ms.append(eng.last_kernel_ms())
        out[f"{n}xh{h}"].update({"batch1_warm_tick_kernel_ms": float(np.median(g_ms[5:])), "batch1_warm_tick_mean_iters": float(np.mean(its[5:])),
                                 "batch1_warm_tick_kernel_ms_fast_path": float(np.median(f_ms[5:]))})
    return out


def warm_tick_probe(pkg, local, n=4096, ticks=12, mode=1):
    """Extra information (not `value`): the closed-loop regime -- the same n robots tick after tick with warm start (the carried OSQP
    workspace of the reference) and slowly moving states (two nearby batches alternate), queue order from the previous tick."""
    import torch
    dev = torch.device("cuda", local); st = torch.cuda.Stream(device=dev)
    a = pkg.scenarios.config3_random_flat(nb=n)
    rng = np.random.default_rng(5)
    b = {k: a[k].copy() for k in ("x0", "xref", "R", "foot", "contact")}
    b["x0"][:, :12] += rng.normal(0, 0.002, (n, 12)); b["foot"] += rng.normal(0, 0.001, (n, 12))
    cfg = pkg.make_config(a["params"], HORIZON, warm_start=mode)   # 1: fresh set-up + warm start; 2: the reference's per-tick OSQP update path (include/a1mpc.h)
    da = {k: torch.from_numpy(a[k]).to(dev) for k in b}; db = {k: torch.from_numpy(b[k]).to(dev) for k in b}
    grf = torch.zeros((n, 12), dtype=torch.float64, device=dev)
    it = torch.zeros(n, dtype=torch.int32, device=dev); stt = torch.zeros(n, dtype=torch.int32, device=dev)
    ms, iters = [], []
    with pkg.Engine(cfg, n, local) as eng:
        for t in range(ticks):
            d = da if t % 2 == 0 else db
            eng.solve_device(n, d["x0"], d["xref"], d["R"], d["foot"], d["contact"], grf, None, it, stt, stream=st.cuda_stream)
            ms.append(eng.last_kernel_ms()); iters.append(float(it.float().mean().item()))
    return {"workload": "4096 robots, h=10, warm start, states move ~2 mm / 2 mrad between ticks", "warm_start_mode": mode, "kernel_ms_per_tick": float(np.median(ms[4:])),
            "ticks_per_s_x_robots": n / (float(np.median(ms[4:])) * 1e-3), "mean_iters_cold_first_tick": iters[0], "mean_iters_warm": float(np.mean(iters[4:]))}


def warm_tick_stage_counters(pkg, local, n=4096, mode=1, ticks=8):
    """where a warm-started tick spends its cycles -- the profiling instantiation of the fused (n > 256) / latency (n <= 256) kernel
    (a1mpc_set_profiling + a1mpc_last_tick_stage_cycles: same arithmetic, same bits, shader-clock stamps between the stages), one profiled tick behind `ticks` plain ones.
    Shares of the tick's cycles, cycles per QP and the plain kernel's ms per tick beside them."""
    import torch
    dev = torch.device("cuda", local); st = torch.cuda.Stream(device=dev)
    a = pkg.scenarios.config3_random_flat(nb=n) if n > 1 else None
    if n == 1:   # BASELINE configs[1]: the trot sequence, one robot
        seq = pkg.scenarios.config2_trot_sequence(ticks + 2)
        frames = [{k: np.ascontiguousarray(seq[k][t:t + 1]) for k in ("x0", "xref", "R", "foot", "contact")} for t in range(ticks + 2)]
        params = seq["params"]
    else:
        rng = np.random.default_rng(5)
        b = {k: a[k].copy() for k in ("x0", "xref", "R", "foot", "contact")}
        b["x0"][:, :12] += rng.normal(0, 0.002, (n, 12)); b["foot"] += rng.normal(0, 0.001, (n, 12))
        frames = [a if t % 2 == 0 else b for t in range(ticks + 2)]
        params = a["params"]
    cfg = pkg.make_config(params, HORIZON, warm_start=mode)
    grf = torch.zeros((n, 12), dtype=torch.float64, device=dev); it = torch.zeros(n, dtype=torch.int32, device=dev); stt = torch.zeros(n, dtype=torch.int32, device=dev)
    ms = []
    with pkg.Engine(cfg, n, local) as eng:
        def tick(t):
            d = {k: torch.from_numpy(frames[t][k]).to(dev) for k in ("x0", "xref", "R", "foot", "contact")}
            eng.solve_device(n, d["x0"], d["xref"], d["R"], d["foot"], d["contact"], grf, None, it, stt, stream=st.cuda_stream)
            return eng.last_kernel_ms()
        for t in range(ticks):
            ms.append(tick(t))
        eng.set_profiling(True); prof_ms = tick(ticks); cyc = eng.last_tick_stage_cycles(); iters = float(it.float().mean().item()); eng.set_profiling(False)
        ms.append(tick(ticks + 1))
    if cyc["qps"] != n or cyc["total"] <= 0:
        return {"error": f"the tick was not profiled (qps {cyc['qps']})"}
    tot = cyc["total"]
    return {"robots": n, "warm_start_mode": mode, "kernel": "latency (coop) kernel" if n <= 256 else "fused kernel",
            "kernel_ms_per_tick": float(np.median(ms[3:])), "profiled_tick_ms": prof_ms, "mean_iters": iters,
            "share": {k: cyc[k] / tot for k in pkg.Engine.TICK_STAGES[:-1]}, "cycles_per_qp": {k: cyc[k] / n for k in pkg.Engine.TICK_STAGES},
            "stages": "[formation | Ruiz passes | hot state + hand-off | factor passes | iterations | residual checks | outputs + carry], shader-clock cycles of the "
                      "wavefront summed over the QPs (a QP's cycles include its wave-mate's)"}


def full_tick_probe(pkg, local, n=4096, ticks=10, only=None):
    """Extra information (not `value`): one whole control tick per robot in ONE C call (a1mpc_control_tick_device, round 5) -- leg state, EKF, gait plan, swing legs,
    contacts / terrain, warm-started MPC from tick records, joint torques in the MPC kernel's output stage -- sensors resident in HBM, one stream, HIP events around
    `ticks` ticks.  (Until round 4 the same stages were seven entry points chained from Python with the tick record assembled by torch: 0.577 ms.)"""
    import ctypes as C
    import torch
    dev = torch.device("cuda", local); st = torch.cuda.Stream(device=dev)
    rng = np.random.default_rng(7); scen = pkg.scenarios; E = pkg.engine
    P = scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS
    cfg = pkg.make_config(P, HORIZON, warm_start=1)
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
    with pkg.Engine(cfg, n, local) as eng:
        prm = E.TickParams(); eng.lib.a1mpc_default_tick_params(C.byref(prm))
        for _ in range(32):   # (the first tick runs the split pipeline; the GPU needs a few ms of work to reach its steady clocks)
            eng.control_tick_device(prm, bf, n, stream=st.cuda_stream)
        st.synchronize()
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)

        def run(timing):
            eng.set_timing(timing)   # the handle's own timing events off = as a control loop would run it (a1mpc_set_timing): four event records less per tick
            eng.control_tick_device(prm, bf, n, stream=st.cuda_stream)
            e0.record(st)
            for _ in range(ticks):
                eng.control_tick_device(prm, bf, n, stream=st.cuda_stream)
            e1.record(st)
            st.synchronize()
            return e0.elapsed_time(e1) / ticks
        if only is not None and not isinstance(only, (list, tuple)):   # (tools/control_tick_timeline.py: ONE setting of a1mpc_set_timing, for a kernel / HIP trace of exactly these ticks)
            return {"timing_events": bool(only), "ms_per_tick": [run(bool(only)) for _ in range(3)]}
        if only is not None:   # (tools/control_tick_markers.py: an explicit sequence of settings, e.g. [1, 0, 1, 0, 1, 0] -- the position of a run in the sequence matters, see there)
            return {"sequence": list(only), "ms_per_tick": [run(bool(x)) for x in only]}
        # Round 6 (profiles/r06_control_tick_timeline.md): what a run of ten ticks (4 ms of work behind a synchronisation) measures is decided by its POSITION in the sequence of runs
        # -- the part's clocks ramp: 0.47 / 0.43 / 0.55 / 0.38 / 0.38 / 0.45 ms per tick for six identical runs -- not by the setting; round 5's (off, on) x 3 protocol therefore
        # reported "timing off is 7 % slower", an artefact.  The figures are now taken from runs of `long_ticks` ticks (steady clocks) in on / off / off / on order; the
        # ten-tick runs are kept beside them, six in a row with the default setting.
        long_ticks = 100
        ticks_short = ticks
        ticks = long_ticks
        r = [(x, run(bool(x))) for x in (1, 0, 0, 1)]
        ms = float(np.mean([v for x, v in r if x])); ms_off = float(np.mean([v for x, v in r if not x]))   # `ms_per_tick`: the handle as a1mpc_create leaves it (timing events on)
        ticks = ticks_short
        short_runs = [run(True) for _ in range(6)]
        last_ms, fused = eng.last_control_tick_ms()
        mpc_ms = eng.last_kernel_ms()
    return {"workload": f"{n} robots: leg state + EKF + gait plan + swing legs + contacts/terrain + warm-started MPC (h=10, tick records) + joint torques per tick, device-resident, "
                        "ONE C call per tick (a1mpc_control_tick_device)", "ms_per_tick": ms, "robot_ticks_per_s": n / (ms * 1e-3), "ms_per_tick_with_a1mpc_set_timing_off": ms_off,
            "protocol": f"runs of {long_ticks} back-to-back ticks between HIP events on the caller's stream, timing events on / off / off / on, means; `ms_per_tick` = on (the library's default)",
            "ms_per_tick_runs_of_10_ticks_in_sequence": short_runs, "runs_of_10_ticks_note": "six identical runs (timing on): the figure follows the position in the sequence (clock ramp after "
            "each synchronisation), which is what round 5's alternating ten-tick protocol mistook for an effect of the timing events", "last_tick_ms_by_its_own_events": last_ms,
            "mpc_launch_ms_of_the_last_tick": mpc_ms, "joint_torques_in_the_mpc_output_stage": bool(fused), "mean_mpc_iters": float(d["iters"].float().mean().item()),
            "solved_frac": float((d["status"] == 1).float().mean().item())}


def other_config_rooflines(pkg, local, steps=4):
    """roofline blocks for the shapes of BASELINE configs[3] (h = 16, one GPU's share of 65536 / 8) and configs[4] (32768 x h = 20),
    first solves, device-resident inputs (extra information, not `value`)."""
    import torch
    dev = torch.device("cuda", local); st = torch.cuda.Stream(device=dev)
    res = []
    pmc = {}
    try:
        pmc = json.load(open(os.path.join(ROOT, "profiles", PMC_SUMMARY))).get("executed_fp64_flops_per_launch_by_config", {})
    except Exception:
        pass
    for name, gen, n, h in (("BASELINE's upper batch: 65536 x h10 (configs[2]'s generator)", "config3_random_flat", 65536, 10), ("configs[3] share: 8192 x h16", "config4_random_h16", 8192, 16),
                            ("configs[4]: 32768 x h20 mixed contacts, 0.5 rad pitch", "config5_divergent", 32768, 20)):
        sc = getattr(pkg.scenarios, gen)(nb=n)
        cfg = pkg.make_config(sc["params"], h, warm_start=0)
        d = {k: torch.from_numpy(sc[k]).to(dev) for k in ("x0", "xref", "R", "foot", "contact")}
        grf = torch.zeros((n, 12), dtype=torch.float64, device=dev)
        it = torch.zeros(n, dtype=torch.int32, device=dev); stt = torch.zeros(n, dtype=torch.int32, device=dev)
        with pkg.Engine(cfg, n, local) as eng:
            ms = []
            for k in range(steps + 1):
                eng.set_schedule(True)
                eng.solve_device(n, d["x0"], d["xref"], d["R"], d["foot"], d["contact"], grf, None, it, stt, stream=st.cuda_stream)
                ms.append(eng.last_kernel_ms())
            nf = eng.last_nfact(n)
        avg = float(np.mean(ms[1:]))
        fl = float(pkg.algorithmic_flops(h, it.cpu().numpy(), nf).sum())
        ach = fl / (avg * 1e-3) / 1e12
        entry = {"config": name, "batch": n, "horizon": h, "avg_kernel_ms": avg, "solves_per_s": n / (avg * 1e-3), "bound": "fp64-valu", "achieved": ach,
                 "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": ach / FP64_PEAK_TFLOPS, "mean_iters": float(it.float().mean().item()),
                 "algorithmic_bytes_per_launch": pkg.algorithmic_bytes(h) * n, "solved_frac": float((stt == 1).float().mean().item())}
        entry["lanes_live"] = {10: "48 of 64 (two QPs per wavefront)",
                               16: "48 of 64: a CU-wide workgroup of four wavefronts carries five QPs (wave 0 two as twin pairs = 48 lanes; waves 1-3 one each as a quad of rows = 48 lanes "
                                   "in the sweeps, whose rows 1 / 3 repeat rows 0 / 2, and 4 x 12 distinct lanes in the element-wise steps)",
                               20: "48 of 64 (one QP per wavefront as a quad of rows: 40 KB of LDS per QP, four per CU; rows 1 / 3 repeat the sweeps of rows 0 / 2 and hold their own quarter of the "
                                   "per-lane state -- executed_fp64_frac counts the work of ONE pair, from the twin-pair kernel's PMC pass)"}[h]
        ex = pmc.get(f"{n}x{h}")   # SQ_INSTS_VALU_{FMA,ADD,MUL}_F64 x live lanes of a first solve of this batch (static: profiles/, rocprofv3 --pmc of tools/prof_shapes.py)
        if ex:
            entry["executed_fp64_flops_per_launch"] = ex; entry["executed_fp64_frac"] = ex / (avg * 1e-3) / 1e12 / FP64_PEAK_TFLOPS
        exq = pmc.get(f"{n}x{h}q") or pmc.get(f"{n}x{h}cu")   # the quad-of-rows kernels as they run (h = 20; the CU-wide kernel at h = 16): rows 1 / 3 of a quad repeat the sweeps of rows 0 / 2 -- what the FP64 pipe issues, repeats included
        if exq:
            entry["issued_fp64_frac_repeats_included"] = exq / (avg * 1e-3) / 1e12 / FP64_PEAK_TFLOPS
        if n <= 8192:   # a batch of this size leaves a tail: the same first solves with two batches in flight (a1mpc_pipeline; batches of tens of thousands fill the chip alone)
            outs = [(torch.zeros((n, 12), dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)) for _ in range(2)]
            with pkg.Pipeline(cfg, n, local, depth=2) as pipe:
                sub = lambda k, after=None: pipe.submit_device(n, d["x0"], d["xref"], d["R"], d["foot"], d["contact"], outs[k % 2][0], None, outs[k % 2][1], outs[k % 2][2], fresh=True, after_stream=after)
                for k in range(2):
                    sub(k)
                pipe.wait(); torch.cuda.synchronize()
                e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for k in range(2 * steps):
                    sub(k, st.cuda_stream if k < 2 else None)
                pipe.join(st.cuda_stream); e1.record(st); torch.cuda.synchronize()
                pms = e0.elapsed_time(e1) / (2 * steps)
            entry["two_in_flight"] = {"ms_per_batch": pms, "solves_per_s": n / (pms * 1e-3), "frac": fl / (pms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS}
        res.append(entry)
    return res


def device_identity(local):
    """which physical GPU this rank drives: PCI bus id + UUID (HIP runtime through ctypes, torch's device properties as the fall-back), host name"""
    import socket
    import ctypes as C
    ident = {"host": socket.gethostname(), "local_device": int(local), "pci_bus_id": None, "uuid": None}
    try:
        hip = C.CDLL("libamdhip64.so")
        buf = C.create_string_buffer(64)
        if hip.hipDeviceGetPCIBusId(buf, 64, int(local)) == 0:
            ident["pci_bus_id"] = buf.value.decode()
        uu = (C.c_ubyte * 16)()
        if hip.hipDeviceGetUuid(C.byref(uu), int(local)) == 0:
            ident["uuid"] = bytes(uu).hex()
    except Exception:
        pass
    try:
        import torch
        pr = torch.cuda.get_device_properties(int(local))
        if ident["uuid"] is None and getattr(pr, "uuid", None) is not None:
            ident["uuid"] = str(pr.uuid)
        if ident["pci_bus_id"] is None and getattr(pr, "pci_bus_id", None) is not None:
            ident["pci_bus_id"] = f"{getattr(pr, 'pci_domain_id', 0):04x}:{pr.pci_bus_id:02x}:{getattr(pr, 'pci_device_id', 0):02x}.0"
        ident["name"] = pr.name
    except Exception:
        pass
    return ident


def participation(dist, rank, world, local, backend):
    """Round 6: an N > 1 line proves which devices took part.  Every rank's (rank, host, PCI bus id, UUID) is gathered on rank 0; `distinct_devices` counts
    the different physical GPUs among them, and the line is a SCALING POINT only if that equals the world size and the ranks talk over RCCL -- ranks sharing a GPU
    (the one-GPU smoke test of this code path) are labelled, never counted."""
    ident = dict(device_identity(local), rank=int(rank))
    if world > 1:
        allid = [None] * world
        dist.all_gather_object(allid, ident)
    else:
        allid = [ident]
    keys = {(d["host"], d.get("uuid") or d.get("pci_bus_id") or f"local{d['local_device']}") for d in allid}
    return {"distinct_devices": len(keys), "world_size": int(world), "rccl_world_size": int(world) if (backend == "nccl" and world > 1) else 0, "backend": backend if world > 1 else "none",
            "is_scaling_point": bool(len(keys) == world and (world == 1 or backend == "nccl")),
            "device_ids": ";".join(f"r{d['rank']}@{d['host']}:{d.get('pci_bus_id')}:{(d.get('uuid') or '')[:16]}" for d in allid)}


def strong_scaling_config4(pkg, args, rank, world, local, backend, dist):
    """BASELINE configs[3]: 65536 QPs, horizon 16, the whole batch resident in rank 0's HBM; a step = scatter the shards' inputs (one group of
    ncclSend / ncclRecv over xGMI), solve, gather GRFs + iterations + status back to rank 0 -- all inside the timed region.  Strong scaling."""
    import torch
    H = 16
    N = args.batch if args.batch != BATCH else 65536
    dev = torch.device("cuda", local)
    cdev = dev if backend == "nccl" else torch.device("cpu")      # gloo smoke test: communication through host tensors
    sh = pkg.sharding
    sc = pkg.scenarios.config4_random_h16(nb=N) if rank == 0 else None
    params = (pkg.scenarios.PARAM_SETS["gazebo"] | pkg.scenarios.MPC_CONSTANTS)
    cfg = pkg.make_config(params, H, warm_start=0)
    rec, ct = sh.pack_inputs(sc, H, cdev) if rank == 0 else (None, None)
    parts = sh.partition(N, world); cnt = parts[rank][1]
    eng = pkg.Engine(cfg, max(cnt, 1), local)
    stream = torch.cuda.Stream(device=dev)
    grf = torch.zeros((cnt, 12), dtype=torch.float64, device=dev); meta = torch.zeros((cnt, 2), dtype=torch.int32, device=dev)
    it = torch.zeros(cnt, dtype=torch.int32, device=dev); stt = torch.zeros(cnt, dtype=torch.int32, device=dev)
    out_bufs = (torch.empty((N, 12), dtype=torch.float64, device=cdev), torch.empty((N, 2), dtype=torch.int32, device=cdev)) if rank == 0 else None
    t_comm = [0.0]
    on_device = cdev == dev   # nccl: scatter, solve and gather are queued on ONE stream (torch's current stream; RCCL orders its own stream against it), no host
                              # synchronisation and no staging hop inside a step; the communication share is read from HIP events after the loop.
                              # gloo (the CPU smoke test of this code path): host tensors, host clocks, a synchronisation per phase.
    torch.cuda.synchronize()
    if on_device:
        torch.cuda.set_stream(stream)   # a real (non-null) stream becomes torch's current stream: tensor ops, RCCL's stream dependencies and the engine's launches share it
    cur = stream
    evs = []

    def step():
        if on_device:
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record(cur)
            lrec, lct = sh.scatter(rec, ct, N, H, cdev, None, 0) if world > 1 else (rec, ct)
            e[1].record(cur)
            f = sh.unpack_record(lrec, H)
            eng.set_schedule(True)
            eng.solve_device(cnt, f["x0"], f["xref"], f["R"], f["foot"], lct, grf, None, it, stt, stream=cur.cuda_stream)
            meta[:, 0] = it; meta[:, 1] = stt
            e[2].record(cur)
            if world > 1:
                sh.gather(grf, meta, N, cdev, None, 0, out_bufs)
            else:
                out_bufs[0].copy_(grf); out_bufs[1].copy_(meta)
            e[3].record(cur)
            evs.append(e)
            return
        a = time.perf_counter()
        lrec, lct = sh.scatter(rec, ct, N, H, cdev, None, 0) if world > 1 else (rec, ct)
        lrec = lrec.to(dev); lct = lct.to(dev)
        torch.cuda.synchronize(); b = time.perf_counter()
        f = sh.unpack_record(lrec, H)
        torch.cuda.current_stream().synchronize()
        eng.set_schedule(True)
        eng.solve_device(cnt, f["x0"], f["xref"], f["R"], f["foot"], lct.contiguous(), grf, None, it, stt, stream=stream.cuda_stream)
        stream.synchronize()
        meta[:, 0] = it; meta[:, 1] = stt
        torch.cuda.synchronize(); c = time.perf_counter()
        if world > 1:
            sh.gather(grf.to(cdev), meta.to(cdev), N, cdev, None, 0, out_bufs)
        else:
            out_bufs[0].copy_(grf); out_bufs[1].copy_(meta)
        torch.cuda.synchronize(); d = time.perf_counter()
        t_comm[0] += (b - a) + (d - c)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t_comm[0] = 0.0; evs.clear()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if on_device:
        t_comm[0] = sum(e[0].elapsed_time(e[1]) + e[2].elapsed_time(e[3]) for e in evs) * 1e-3
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=cdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    res = None
    part = participation(dist, rank, world, local, backend)   # (a collective: every rank calls it)
    if rank == 0:
        iters = out_bufs[1][:, 0].cpu().numpy(); status = out_bufs[1][:, 1].cpu().numpy()
        if args.dump_outputs:   # what the last timed step gathered on rank 0
            dump_outputs(args.dump_outputs, {"grf": out_bufs[0].cpu().numpy(), "iters": iters, "status": status})
        res = {"metric": "MPC QP solves/sec (horizon=16 SRBD), BASELINE configs[3]", "value": N * args.steps / elapsed, "unit": "solves/s", "n_gpus": world,
               "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
               "dtype": "f64", "data": "synthetic",
               "config": {"workload": "BASELINE configs[3]: batch=65536 randomized CoM states, horizon=16, the batch resident on rank 0, sharded contiguously over the "
                                      "GPUs; scatter inputs + solve (cold start, first solve) + gather GRFs per step", "global_batch": N, "horizon": H,
                          "parallelism": f"batch-sharded x{world}, {backend} grouped send/recv", "mean_iters": float(iters.mean()), "solved_frac": float((status == 1).mean())},
               "scatter_gather_ms_per_step_rank0": t_comm[0] / args.steps * 1e3,
               "scatter_bytes_per_step": int(N - parts[0][1]) * (sh.record_width(H) * 8 + 4), "gather_bytes_per_step": int(N - parts[0][1]) * (12 * 8 + 8)}
        # flat in `config` (the driver's record keeps the scalar members of `config`): who took part, and what scatter + gather moved and cost
        res["config"].update(part)
        res["config"].update({"scatter_bytes_per_step": res["scatter_bytes_per_step"], "gather_bytes_per_step": res["gather_bytes_per_step"],
                              "scatter_gather_ms_per_step_rank0": res["scatter_gather_ms_per_step_rank0"],
                              "scatter_gather_share_of_step": res["scatter_gather_ms_per_step_rank0"] / res["ms_per_step"]})
        if not part["is_scaling_point"]:
            res["config"]["parallelism"] += f" -- {part['distinct_devices']} distinct GPU(s) for {world} rank(s): NOT a scaling point"
    eng.close()
    return res


def metric_line(n, world, args, elapsed, depth, untimed, it, stt, part, backend):
    """the line of BASELINE configs[2]'s metric (everything a plain run prints): `value`, `ms_per_step`, the workload and who took part; `it` / `stt` are the
    iterations and statuses of batch 0"""
    import torch
    out = {
        "metric": "MPC QP solves/sec (horizon=10 SRBD)", "value": world * n * args.steps / elapsed, "unit": "solves/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": "BASELINE configs[2]: batch=4096 randomized CoM states + flat terrain, horizon=10, cold-start "
                               "OSQP-default ADMM, per GPU; 4 distinct batches cycled, every step a first solve (no queue-order history); "
                               f"{depth} batch(es) in flight (a1mpc_pipeline: one engine handle + HIP stream per slot, round-robin)",
                   "batch_per_gpu": n, "horizon": HORIZON, "parallelism": f"batch-sharded x{world}" + (f" ({backend}, ranks SHARING {torch.cuda.device_count()} physical GPU(s): a smoke "
                                                                                                   "test of the N > 1 path, not a scaling point)" if os.environ.get("A1_BENCH_SHARE_GPU") else ""),
                   "batches_in_flight": depth, "untimed_launches_before_timing": untimed,
                   "mean_iters": float(it.mean()), "max_iters": int(it.max()), "solved_frac": float((stt == 1).mean())},
    }
    out["config"].update(part)   # who took part: distinct_devices, rccl_world_size, is_scaling_point, device_ids (flat scalars of `config`)
    if not part["is_scaling_point"]:
        out["config"]["parallelism"] += f" -- {part['distinct_devices']} distinct GPU(s) for {world} rank(s): NOT a scaling point"
    return out


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher around it: start the N ranks here (one process per GPU through torch.distributed.run, the way the driver launches
    N > 1) and hand their JSON line through.  A box with fewer than N GPUs runs the N ranks on the GPUs it has over gloo (A1_BENCH_SHARE_GPU: a smoke test of the
    N > 1 code path, said so in config.parallelism) -- the line still says n_gpus = N ranks, never a scaling claim."""
    import socket
    import subprocess
    import torch
    have = torch.cuda.device_count()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if have < args.gpus:
        env["A1_BENCH_SHARE_GPU"] = "1"; env["A1_BENCH_BACKEND"] = "gloo"
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0)); port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + sys.argv[1:]
    rc = subprocess.call(cmd, env=env)
    if rc != 0:
        raise SystemExit(rc)


def native_sharded(args):
    """One process, all GPUs: the C ABI's own sharding (a1mpc_sharded_*, SURVEY 8b `device = -1`, 8e "measure both transports").  Host arrays in, host arrays out -- the
    PCIe-inclusive rate of a caller on the reference's side of the boundary, both transports side by side over the same batches.  On a box with fewer GPUs than --gpus
    the shards of transport 0 share the GPUs that exist (a plumbing run); transport 1 needs distinct devices and is run over the devices that exist."""
    import torch
    pkg = graft.load_package()
    pkg.load_library()
    have = torch.cuda.device_count()
    cfg4 = args.config == 4
    h = 16 if cfg4 else HORIZON
    n = (args.batch if args.batch != BATCH else 65536) if cfg4 else args.batch * args.gpus
    gen = pkg.scenarios.config4_random_h16 if cfg4 else pkg.scenarios.config3_random_flat
    NB = 2 if cfg4 else 4
    scs = [gen(nb=n, seed=0xA1 + 3 + 17 * k) for k in range(NB)]
    cfg = pkg.make_config(scs[0]["params"], h, warm_start=0)
    res, last = {}, {}
    for transport in (0, 1):
        devs = [g % have for g in range(args.gpus)] if transport == 0 else list(range(min(args.gpus, have)))
        try:
            with pkg.engine.ShardedEngine(cfg, n, devices=devs, transport=transport) as sh:
                for k in range(max(1, args.warmup // 2)):
                    s = scs[k % NB]; o = sh.solve(s["x0"], s["xref"], s["R"], s["foot"], s["contact"])
                t0 = time.perf_counter()
                for k in range(args.steps):
                    s = scs[k % NB]; o = sh.solve(s["x0"], s["xref"], s["R"], s["foot"], s["contact"])
                el = time.perf_counter() - t0
                last[transport] = o
                res[transport] = {"transport": "pinned fan-out, one hipMemcpyAsync per device each way" if transport == 0 else "RCCL grouped ncclSend / ncclRecv through shard 0's GPU",
                                  "devices": devs, "solves_per_s": n * args.steps / el, "ms_per_step": el / args.steps * 1e3, "mean_iters": float(o["iters"].mean()),
                                  "solved_frac": float((o["status"] == 1).mean())}
        except Exception as e:   # (e.g. RCCL not loadable: reported, the other transport still counts)
            res[transport] = {"error": str(e)[:300], "devices": devs}
    pick = res[args.native]
    if "error" in pick:
        raise SystemExit(f"--native {args.native}: {pick['error']}")
    if args.dump_outputs:   # the chosen transport's last timed step
        o = last[args.native]
        dump_outputs(args.dump_outputs, {"grf": o["grf"], "iters": o["iters"], "status": o["status"]})
    out = {"metric": f"MPC QP solves/sec (horizon={h} SRBD), host arrays in / out through a1mpc_sharded_* (PCIe inclusive)", "value": pick["solves_per_s"], "unit": "solves/s",
           "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup, "ms_per_step": pick["ms_per_step"], "higher_is_better": True, "scaling": "strong" if cfg4 else "weak",
           "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {"workload": ("BASELINE configs[3]: 65536 x h16" if cfg4 else f"BASELINE configs[2]: {args.batch} x h10 per GPU") + ", one process, batch sharded contiguously over the devices inside the C ABI, "
                                  "cold-start first solves of distinct batches, host arrays in and out every step", "global_batch": n, "horizon": h,
                      "parallelism": f"a1mpc_sharded x{args.gpus} ({have} physical GPU(s) on this box)", "transport": args.native},
           "transports": {"0": res[0], "1": res[1]}}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--batch", type=int, default=BATCH, help="QPs per GPU per step")
    ap.add_argument("--config", type=int, default=2, choices=(2, 4), help="2 (default): BASELINE configs[2], 4096 x h10 per GPU, weak scaling (the `metric`); "
                    "4: BASELINE configs[3], 65536 x h16 in total, sharded over the GPUs with scatter + gather inside the timed region (strong scaling)")
    ap.add_argument("--depth", type=int, default=2, help="batches in flight (a1mpc_pipeline: one engine handle + HIP stream each, submitted round-robin); "
                    "1 = one handle, launches serialised on one stream")
    ap.add_argument("--full", action="store_true", help="measure everything beside `value` as well: single-stream and index / history-order steps, stage counters, "
                    "roofline, latency probes, other shapes and horizons, CPU baseline and parity against the oracle.  Without it the run sets up, warms up, "
                    "times the steps and prints the metric's line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the timed path computed in its last step as DIR/<name>.npy "
                    "(float64; the inputs are seeded, so two builds can be compared output for output)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(with --full) skip the CPU baseline and the parity block")
    ap.add_argument("--no-latency", action="store_true", help="(with --full) skip the latency probes, sweeps and other shapes")
    ap.add_argument("--no-index-order", action="store_true", help="(with --full) skip the extra index-order steps (profiling runs)")
    ap.add_argument("--native", type=int, default=-1, choices=(-1, 0, 1), help="one process, all --gpus GPUs through the C ABI's own sharding (a1mpc_sharded_*, host arrays in / out): "
                    "0 = pinned fan-out (one hipMemcpyAsync per device each way), 1 = RCCL grouped send / recv through shard 0's GPU; both are measured, the chosen one is `value`")
    args = ap.parse_args()
    if not args.full:   # a plain run measures `value` and nothing else
        args.no_cpu_baseline = args.no_latency = args.no_index_order = True

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (there is no CPU path for the solver)")
    if args.native >= 0:
        return native_sharded(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn_ranks(args)
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", 0)); world = int(os.environ.get("WORLD_SIZE", 1)); local = int(os.environ.get("LOCAL_RANK", 0))
    backend = os.environ.get("A1_BENCH_BACKEND", "nccl")  # "gloo" + A1_BENCH_SHARE_GPU=1: two ranks on ONE GPU, a smoke test of the N > 1 code path
    if os.environ.get("A1_BENCH_SHARE_GPU"):
        local = 0
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    pkg = graft.load_package()
    try:
        pkg.load_library()
    except Exception:
        if rank == 0:
            pkg.build.build()
        if world > 1:
            dist.barrier()
        pkg.load_library()

    if args.config == 4:
        out = strong_scaling_config4(pkg, args, rank, world, local, backend, dist)
        if rank == 0:
            print(json.dumps(out), flush=True)
        if world > 1:
            dist.barrier(); dist.destroy_process_group()
        return

    n = args.batch
    # NB distinct batches, resident in HBM, cycled through the steps: no step re-solves the inputs of the step before it, and every step
    # is a FIRST solve (a1mpc_set_schedule drops the handle's queue-order history before each launch) -- `value` cannot profit from
    # having seen the same QPs before.  Rank 0 / batch 0 = the documented seed of BASELINE configs[2].
    NB = 4
    scs = [pkg.scenarios.config3_random_flat(nb=n, seed=0xA1 + 3 + 1000 * rank + 17 * k) for k in range(NB)]
    sc = scs[0]
    cfg = pkg.make_config(sc["params"], HORIZON, warm_start=0)                   # cold start every step: no work is skipped
    dev = torch.device("cuda", local)
    ds = [{k: torch.from_numpy(s_[k]).to(dev) for k in ("x0", "xref", "R", "foot", "contact")} for s_ in scs]
    grf = torch.zeros((n, 12), dtype=torch.float64, device=dev)
    iters = torch.zeros(n, dtype=torch.int32, device=dev); status = torch.zeros(n, dtype=torch.int32, device=dev)
    outs = [(torch.zeros((n, 12), dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
            for _ in range(NB)]           # one output set per resident batch: a batch in flight never shares its outputs with the next one
    depth = max(1, min(args.depth, NB))
    eng = pkg.Engine(cfg, n, local)       # the lone handle: single-stream figures, index / history order, work collection (--full; created in a plain run too,
                                          #  so that the timed pipeline is set up exactly as in a --full run)
    pipe = pkg.Pipeline(cfg, n, local, depth=depth)   # `value`: `depth` batches in flight, the next batch fills the tail of the one before
    stream = torch.cuda.Stream(device=dev)  # a real (non-null) HIP stream: kernels and the timing events share it
    torch.cuda.synchronize()

    def step(k=0, fresh=True):            # the lone handle, one stream
        d = ds[k % NB]
        if fresh:
            eng.set_schedule(True)   # forget the previous solve: the queue is ordered by the set-up kernel's own cost guess
        eng.solve_device(n, d["x0"], d["xref"], d["R"], d["foot"], d["contact"], grf, None, iters, status, stream=stream.cuda_stream)

    def submit(k, after=None):            # the pipeline: every batch a first solve (fresh: the slot's history is dropped), round-robin over the slots
        d = ds[k % NB]; o = outs[k % NB]
        return pipe.submit_device(n, d["x0"], d["xref"], d["R"], d["foot"], d["contact"], o[0], None, o[1], o[2], fresh=True, after_stream=after)

    spin_up = max(0, int(os.environ.get("A1_BENCH_SPIN_UP", "32")) - args.warmup)   # (untimed, like the warm-up steps, reported as config.untimed_launches_before_timing: the GPU
                                          #  needs some ms of work to reach its steady clocks -- 0.72 ms per step with 3 launches behind the timed region, 0.65 with 8,
                                          #  tools/pipe_start_probe.py; a property of the power management, not of a step)

    def region(steps):
        """`steps` batches through the pipeline exactly the way the timed region issues them: the first launch of every slot starts behind an event on `stream`, an
        event sits behind the last launch of every slot.  The warm-up runs through here too: the first use of the cross-stream waits and of the events costs the
        HIP runtime ~0.7 ms on the GPU timeline and several ms on the host (tools/pipe_start_probe.py: first region 0.66 ms per batch, every later one 0.625) --
        a one-off of the process, not of a step, so it belongs to the warm-up."""
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for k in range(steps):
            submit(k, after=stream.cuda_stream if k < depth else None)   # the first launch of every slot starts behind e0
        pipe.join(stream.cuda_stream)     # ... and e1 sits behind the last launch of every slot: HIP events around the region
        e1.record(stream)
        torch.cuda.synchronize()
        return e0, e1

    if spin_up + args.warmup > 0:
        region(spin_up + args.warmup)     # W untimed warm-up steps (+ the spin-up launches)
    pipe.wait()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0, e1 = region(args.steps)           # EXACTLY K timed steps, bracketed by a barrier + synchronize on both sides
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    pipe_ms = e0.elapsed_time(e1) / args.steps   # device time per batch with `depth` batches in flight
    pipe_out0 = tuple(t_.cpu().numpy().copy() for t_ in outs[0])   # what the timed region left for batch 0 (GRFs, iterations, status): the parity block checks THESE
    if args.dump_outputs and rank == 0:   # the batch of the last timed step, before anything below launches again
        last = outs[(args.steps - 1) % NB]
        dump_outputs(args.dump_outputs, {"grf": last[0].cpu().numpy(), "iters": last[1].cpu().numpy(), "status": last[2].cpu().numpy()})
    # continuity with the round-3 protocol (ADVICE r4 / VERDICT r4 item 7): the same K steps behind only 8 untimed launches, the GPU idle for a second before them
    # (round 3 timed exactly that; round 4 moved to 32 untimed launches, which is worth ~5 % through the clocks alone).  Reported beside `value`, never instead of it.
    value8 = None
    if args.full and world == 1 and os.environ.get("A1_BENCH_VALUE8", "1") != "0":
        time.sleep(1.0)
        region(8); pipe.wait(); torch.cuda.synchronize()
        t8 = time.perf_counter(); region(args.steps); torch.cuda.synchronize()
        value8 = n * args.steps / (time.perf_counter() - t8)
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if not args.full:
        part = participation(dist, rank, world, local, backend)   # (a collective: every rank calls it)
        if rank == 0:
            print(json.dumps(metric_line(n, world, args, elapsed, depth, spin_up + args.warmup, pipe_out0[1], pipe_out0[2], part, backend)), flush=True)
        eng.close(); pipe.close()
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    # the same steps through the lone handle on one stream (launches serialised): per-launch durations by HIP events, what a kernel trace shows
    for k in range(2):
        step(k)
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    evs[0].record(stream)
    for k in range(args.steps):
        step(k)
        evs[k + 1].record(stream)
    torch.cuda.synchronize()
    kern_ms = np.array([evs[k].elapsed_time(evs[k + 1]) for k in range(args.steps)])  # HIP events on the launch stream

    # per-batch work (iterations, factorisations: deterministic) for the flop model, collected outside the timed region
    work = []
    for k in range(NB):
        step(k); torch.cuda.synchronize()
        work.append((iters.cpu().numpy().copy(), status.cpu().numpy().copy(), eng.last_nfact(n).copy()))
    gpu_grf0 = None
    step(0); torch.cuda.synchronize(); gpu_grf0 = grf.cpu().numpy().copy()
    it, stt = work[0][0], work[0][1]
    # stage counters (the reference's t1..t6 stopwatches): set-up | solve by HIP events, the solve stage split into factor passes | iterations | residual checks by
    # the clock-stamped instantiation of the ADMM kernel (a1mpc_set_profiling; the same results bit for bit) -- one extra solve of batch 0, outside every timed region
    stage = None
    try:
        eng.set_profiling(True); step(0); torch.cuda.synchronize()
        cyc = eng.last_stage_cycles(); sms = eng.last_stage_ms(); eng.set_profiling(False)
        tot = cyc["factor"] + cyc["iterate"] + cyc["check"]
        if cyc["qps"] == n and tot > 0:
            stage = {"setup_ms": sms[0], "solve_ms": sms[1], "solve_split": {"factor_passes": cyc["factor"] / tot, "iterations": cyc["iterate"] / tot, "residual_checks": cyc["check"] / tot},
                     "cycles_per_iteration": cyc["iterate"] / float(work[0][0].sum()), "cycles_per_factor_pass": cyc["factor"] / float(work[0][2].sum()),
                     "source": "a1mpc_last_stage_ms (HIP events) + a1mpc_last_stage_cycles (shader-clock stamps in the profiling instantiation of the persistent ADMM kernel; a QP's cycles "
                               "include its wave-mate's divergent stages)"}
    except Exception as e:   # (a library without the profiling entry points)
        stage = {"error": str(e)}
    pipe_same = bool(np.array_equal(pipe_out0[0], gpu_grf0) and np.array_equal(pipe_out0[1], it) and np.array_equal(pipe_out0[2], stt))
    # the same batches with the queue ordered by history (each batch re-solved right after itself) and in plain index order: reported beside `value`
    index_ms = hist_ms = None
    if not args.no_index_order:
        def timed(fn):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(stream); fn(); e1.record(stream); torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.steps
        eng.set_schedule(False)
        step(0, fresh=False); torch.cuda.synchronize()
        index_ms = timed(lambda: [step(k, fresh=False) for k in range(args.steps)])
        eng.set_schedule(True)
        step(0, fresh=False); torch.cuda.synchronize()
        hist_ms = timed(lambda: [step(0, fresh=False) for _ in range(args.steps)])   # identical inputs again and again: hindsight order
    part = participation(dist, rank, world, local, backend)   # (a collective: every rank calls it)
    if rank == 0:
        h = HORIZON
        flops_b = [float(pkg.algorithmic_flops(h, w[0], w[2]).sum()) for w in work]
        flops = float(np.mean([flops_b[k % NB] for k in range(args.steps)]))   # mean algorithmic flops of a timed launch
        single_ms = float(kern_ms.mean())          # one launch alone on one stream (what a kernel trace shows per launch: set-up + order + ADMM kernel)
        avg_ms = float(pipe_ms)                    # device time per launch over the timed region (HIP events), `depth` launches in flight
        achieved = flops / (avg_ms * 1e-3) / 1e12
        pmc = {}
        try:
            pmc = json.load(open(os.path.join(ROOT, "profiles", PMC_SUMMARY)))
        except Exception:
            pass
        traffic = float(pmc["hbm_bytes_per_launch"]) if (n == BATCH and "hbm_bytes_per_launch" in pmc) else None
        out = metric_line(n, world, args, elapsed, depth, spin_up + args.warmup, it, stt, part, backend)
        out.update({
            "roofline": {"bound": "fp64-valu", "achieved": achieved, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / FP64_PEAK_TFLOPS, "traffic": traffic,
                         "traffic_source": f"static: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, profiles/{PMC_SUMMARY}" if traffic else None,
                         "kernel": "a1mpc_setup_kernel<10,1> + a1mpc_admm_kernel<10,2> (+ a1mpc_order_kernel, ~5 us) = one solve", "avg_kernel_ms": avg_ms,
                         "avg_kernel_ms_is": f"timed region (HIP events on the launch stream, behind the first and after the last launch of every slot) / launches, {depth} launches in flight: "
                                             "with overlapping launches this is the rate a launch completes at, not the span of one launch",
                         "lanes_live": "48 of 64 (two QPs per wavefront, each on a main / twin pair of 16-lane rows with 12 live lanes)",
                         "single_stream": {"avg_kernel_ms": single_ms, "achieved": flops / (single_ms * 1e-3) / 1e12, "frac": flops / (single_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
                                           "solves_per_s": n / (single_ms * 1e-3),
                                           "executed_fp64_frac": (pmc["executed_fp64_flops_per_launch"] / (single_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS) if pmc.get("executed_fp64_flops_per_launch") else None,
                                           "what": "the same first solves through ONE handle on one stream, launches serialised: the sum of the three kernels' durations in a kernel trace "
                                                   "(profiles/r06_kernel_stats_bench_depth1_batch4096_h10.csv)"},
                         "algorithmic_flops_per_launch": flops, "algorithmic_bytes_per_launch": pkg.algorithmic_bytes(h) * n,
                         "executed_fp64_flops_per_launch": pmc.get("executed_fp64_flops_per_launch"),
                         "executed_fp64_frac": (pmc["executed_fp64_flops_per_launch"] / (avg_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS) if pmc.get("executed_fp64_flops_per_launch") else None,
                         "note": "bound: FP64 VALU issue / LDS latency (no MFMA in the kernel: profiles/r02_mfma_trial.md); the peak is the dense FP64 peak (vector = matrix "
                                 "on MI355X).  TWO fractions, always side by side: `frac` prices the SURVEY 8(d) dense-condensed flop model F(h,iters,nfact) (what a dense solver "
                                 "would execute; the structured Riccati solve executes 1.5x / 2.8x / 3.9x fewer flops at h = 10 / 16 / 20), `executed_fp64_frac` prices the FP64 flops "
                                 "the kernels really issue (SQ_INSTS_VALU_{FMA,ADD,MUL}_F64 x live lanes from the static PMC profile) -- the hardware fraction"},
        })
        out["stage_counters"] = stage
        # ---- scalars a reader of this line needs first; repeated inside `roofline` and `config`, which the driver keeps whole
        admm_ms = stage.get("solve_ms") if isinstance(stage, dict) else None   # the persistent ADMM kernel (+ the ~6 us order kernel) of one launch alone, by HIP events
        admm_flops = flops_b[0] - n * float(pkg.algorithmic_flops(h, np.zeros(1, np.int64), np.zeros(1, np.int64))[0])   # F(h, iters, nfact) minus F_cond: what the ADMM kernel itself owes
        scal = {"value_with_8_untimed_launches": value8, "single_stream_solves_per_s": n / (single_ms * 1e-3), "single_stream_frac": flops / (single_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
                "admm_kernel_ms": admm_ms, "admm_kernel_model_frac": (admm_flops / (admm_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS) if admm_ms else None,
                "admm_kernel_executed_frac": (pmc["executed_fp64_flops_admm_kernel"] / (admm_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS) if (admm_ms and pmc.get("executed_fp64_flops_admm_kernel")) else None}
        out.update(scal); out["roofline"]["scalars"] = dict(scal)
        out["scheduling"] = {
            "mode": "value: first solves (no history; queue ordered by the set-up kernel's per-QP cost guess).  Beside it: plain index order, and "
                    "'history' = the same batch solved again right after itself with the queue in longest-first order of the previous solve "
                    "(the closed-loop regime's order; hindsight for identical inputs, never `value`)",
            "index_order_ms_per_step": index_ms, "index_order_solves_per_s_per_gpu": (n / (index_ms * 1e-3)) if index_ms else None,
            "history_ms_per_step": hist_ms, "history_solves_per_s_per_gpu": (n / (hist_ms * 1e-3)) if hist_ms else None}
        if not args.no_latency and world == 1:
            out["roofline_other_configs"] = other_config_rooflines(pkg, local)
    if world > 1 and backend == "nccl" and os.environ.get("A1_BENCH_SCATTER_GATHER") == "1":   # opt-in: an extra collective phase must not be able to take the metric's run down
        # Extra information (not `value`, which needs no collective): what scattering this step's inputs from rank 0 and gathering the results
        # back over RCCL / xGMI would cost -- the north_star's "scatter inputs / gather GRFs" -- one grouped send/recv each way.
        sh = pkg.sharding
        NT = n * world
        rec = torch.zeros((NT if rank == 0 else 0, sh.record_width(HORIZON)), dtype=torch.float64, device=dev)
        ctt = torch.zeros((NT if rank == 0 else 0, 4), dtype=torch.uint8, device=dev)
        mg = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        for _ in range(2):
            sh.scatter(rec, ctt, NT, HORIZON, dev); sh.gather(grf, mg, NT, dev)
        torch.cuda.synchronize(); dist.barrier()
        t1 = time.perf_counter()
        for _ in range(10):
            sh.scatter(rec, ctt, NT, HORIZON, dev); sh.gather(grf, mg, NT, dev)
        torch.cuda.synchronize(); dist.barrier()
        sg_ms = (time.perf_counter() - t1) / 10 * 1e3
        if rank == 0:
            out["config"].update({"scatter_gather_ms_per_step": sg_ms, "scatter_bytes_per_step": int(n * (world - 1) * (sh.record_width(HORIZON) * 8 + 4)),
                                  "gather_bytes_per_step": int(n * (world - 1) * (12 * 8 + 8))})
            out["scatter_gather"] = {"ms_per_step": sg_ms, "bytes_out_of_rank0": int(n * (world - 1) * (sh.record_width(HORIZON) * 8 + 4)),
                                     "bytes_into_rank0": int(n * (world - 1) * (12 * 8 + 8)), "transport": "torch.distributed nccl (RCCL) batch_isend_irecv",
                                     "note": "not part of `value`: ranks generate their own inputs in the weak-scaling metric; --config 4 puts scatter + gather inside the timed region"}
    if rank == 0:
        # everything below is extra information measured on ONE GPU / the host; N > 1 runs (the scaling curve) print the metric's line only,
        # the other ranks are not kept waiting in the final barrier for a minute of single-GPU probes
        if world > 1:
            args.no_latency = args.no_cpu_baseline = True
        if not args.no_latency:
            out["pcie_inclusive"] = pcie_inclusive_probe(pkg, scs, cfg, n, local)
            out["latency"] = latency_probe(pkg)
            out["latency_update_path"] = latency_probe(pkg, mode=2)   # warm_start = 2: the reference's operating point (its persistent OsqpEigen solver, update calls + solve per tick)
            out["latency_update_path_h16"] = latency_probe(pkg, mode=2, horizon=16, cpp_ticks=4000)
            out["latency_update_path_h20"] = latency_probe(pkg, mode=2, horizon=20, cpp_ticks=4000)
            out["throughput_by_batch"] = batch_sweep(pkg, local)
            out["throughput_by_horizon_4096"] = horizon_sweep(pkg, local)
            out["warm_start_ticks"] = warm_tick_probe(pkg, local)
            out["warm_start_ticks_update_path"] = warm_tick_probe(pkg, local, mode=2)
            out["stage_counters_warm"] = {f"{n_}_robots_mode{m_}": warm_tick_stage_counters(pkg, local, n=n_, mode=m_) for n_ in (4096, 1) for m_ in (1, 2)}
            out["full_control_tick"] = full_tick_probe(pkg, local)
            out["general_path"] = general_path_probe(pkg, local)
            meas = {"latency_p50_ms": out["latency"].get("p50_ms"), "latency_p99_ms": out["latency"].get("p99_ms"),
                    "latency_update_path_p50_ms": out["latency_update_path"].get("p50_ms"), "latency_update_path_p99_ms": out["latency_update_path"].get("p99_ms"),
                    "latency_update_path_h16_p50_p99_ms": [out["latency_update_path_h16"].get("p50_ms"), out["latency_update_path_h16"].get("p99_ms")],
                    "latency_update_path_h20_p50_p99_ms": [out["latency_update_path_h20"].get("p50_ms"), out["latency_update_path_h20"].get("p99_ms")],
                    "warm_tick_kernel_ms_4096_robots": out["warm_start_ticks"]["kernel_ms_per_tick"],
                    "warm_tick_update_path_kernel_ms_4096_robots": out["warm_start_ticks_update_path"]["kernel_ms_per_tick"],
                    "full_control_tick_ms_4096_robots": out["full_control_tick"]["ms_per_tick"],
                    "throughput_by_batch_solves_per_s": {k: v["solves_per_s"] for k, v in out["throughput_by_batch"].items()},
                    "general_path_first_solves_per_s": {k: v["first_solve_solves_per_s"] for k, v in out["general_path"].items()},
                    "other_shapes": [{"config": e["config"], "solves_per_s": e["solves_per_s"], "model_frac": e["frac"], "executed_fp64_frac": e.get("executed_fp64_frac"),
                                      "issued_fp64_frac": e.get("issued_fp64_frac_repeats_included")} for e in out.get("roofline_other_configs", [])]}
            out["config"]["measured_beside_value"] = meas
            # Round 6: the driver's record keeps (a) the SCALAR members of `config` / `roofline` / `cpu_baseline` and (b) the last ~2 KB of the line.
            # BASELINE's metric is "solves/sec + p99 solve latency": the latency half and the other shapes go into both places as flat scalars -- `summary` is
            # appended as the LAST key of the line (see the end of main), the same numbers sit flat in `config` (latency) and `roofline` (fractions).
            shp = {"65536xh10": None, "8192xh16": None, "32768xh20": None}
            for e in out.get("roofline_other_configs", []):
                key = f"{e['batch']}xh{e['horizon']}"
                if key in shp:
                    shp[key] = e
            def r3(v, nd=4):
                return None if v is None else round(float(v), nd)
            summ = {"value_solves_per_s": r3(out["value"], 0), "ms_per_step": r3(out["ms_per_step"]),
                    "latency_p50_ms": r3(out["latency"].get("p50_ms")), "latency_p99_ms": r3(out["latency"].get("p99_ms")), "latency_max_ms": r3(out["latency"].get("max_ms")),
                    "latency_mode2_p50_ms": r3(out["latency_update_path"].get("p50_ms")), "latency_mode2_p99_ms": r3(out["latency_update_path"].get("p99_ms")),
                    "latency_timing_events_on_p50_ms": r3(out["latency"].get("timing_events_on", {}).get("p50_ms")), "latency_timing_events_on_p99_ms": r3(out["latency"].get("timing_events_on", {}).get("p99_ms")),
                    "latency_tick_record_entry_p50_ms": r3(out["latency"].get("tick_record_entry", {}).get("p50_ms")), "latency_tick_record_entry_p99_ms": r3(out["latency"].get("tick_record_entry", {}).get("p99_ms")),
                    "latency_h16_mode2_p50_ms": r3(out["latency_update_path_h16"].get("p50_ms")), "latency_h16_mode2_p99_ms": r3(out["latency_update_path_h16"].get("p99_ms")),
                    "latency_h20_mode2_p50_ms": r3(out["latency_update_path_h20"].get("p50_ms")), "latency_h20_mode2_p99_ms": r3(out["latency_update_path_h20"].get("p99_ms")),
                    "latency_budget_ms": 2.5, "single_stream_solves_per_s": r3(out.get("single_stream_solves_per_s"), 0), "value_with_8_untimed_launches": r3(out.get("value_with_8_untimed_launches"), 0),
                    "frac": r3(out["roofline"]["frac"]), "executed_fp64_frac": r3(out["roofline"].get("executed_fp64_frac")),
                    "admm_kernel_ms": r3(out.get("admm_kernel_ms")), "admm_kernel_model_frac": r3(out.get("admm_kernel_model_frac")), "admm_kernel_executed_frac": r3(out.get("admm_kernel_executed_frac")),
                    "warm_tick_ms_4096": r3(meas["warm_tick_kernel_ms_4096_robots"]), "warm_tick_mode2_ms_4096": r3(meas["warm_tick_update_path_kernel_ms_4096_robots"]),
                    "control_tick_ms_4096": r3(meas["full_control_tick_ms_4096_robots"])}
            for key, e in shp.items():
                if e is not None:
                    summ[f"{key}_solves_per_s"] = r3(e["solves_per_s"], 0); summ[f"{key}_frac"] = r3(e["frac"]); summ[f"{key}_executed_frac"] = r3(e.get("executed_fp64_frac"))
            for key, v in meas["general_path_first_solves_per_s"].items():
                summ[f"general_{key}_first_solves_per_s"] = r3(v, 0)
            for key, v in out["general_path"].items():
                if isinstance(v, dict) and v.get("setup_kernel_ms") is not None:
                    summ[f"general_{key}_setup_ms"] = r3(v["setup_kernel_ms"])
                if isinstance(v, dict) and v.get("pipelined_first_solves_per_s") is not None:
                    summ[f"general_{key}_two_in_flight_solves_per_s"] = r3(v["pipelined_first_solves_per_s"], 0)
            out["config"].update({k: v for k, v in summ.items() if k.startswith("latency")})
            out["roofline"].update({k: v for k, v in summ.items() if k.endswith("_frac") and k not in out["roofline"]})
            out["roofline"]["latency_p50_ms"] = summ["latency_p50_ms"]; out["roofline"]["latency_p99_ms"] = summ["latency_p99_ms"]
            out["_summary"] = summ
        if not args.no_cpu_baseline:
            out["cpu_baseline"], ref = cpu_baseline(pkg, sc)
            # parity of the timed workload against the checker (same leg: the oracle is only ever the baseline / the checker)
            dg = np.abs(pipe_out0[0] - ref["grf"])
            out["parity"] = {"checked_qps": int(n), "max_abs_dgrf_N": float(dg.max()), "iteration_mismatches": int((pipe_out0[1] != ref["iters"]).sum()),
                             "status_mismatches": int((pipe_out0[2] != ref["status"]).sum()), "tolerance_N": 1e-5,
                             "checked": "the outputs the timed region left for batch 0 (pipelined launches)", "pipelined_outputs_bit_identical_to_lone_handle": pipe_same,
                             "against": "oracle/a1mpc_oracle.c (formation pinned to the reference's ConvexMpc.cpp by oracle/_ref; the OSQP solve restated, unpinned)"}
        if "_summary" in out:   # LAST key of the line: the driver's record keeps the line's tail
            summ = out.pop("_summary")
            if "parity" in out:
                summ["parity_max_abs_dgrf_N"] = out["parity"]["max_abs_dgrf_N"]; summ["parity_iteration_mismatches"] = out["parity"]["iteration_mismatches"]
            if "cpu_baseline" in out:
                summ["cpu_baseline_solves_per_s"] = round(out["cpu_baseline"]["value"], 0); summ["cpu_cores"] = out["cpu_baseline"]["cores"]
            out["summary"] = summ
            assert len(json.dumps(summ)) < 2000, "the summary block must fit the tail the driver keeps"
        print(json.dumps(out), flush=True)
    eng.close(); pipe.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
