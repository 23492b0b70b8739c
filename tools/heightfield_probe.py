"""a1mpc_walk_step_heightfield_kernel: time per launch beside a1mpc_walk_step_ground_kernel, which it copies, in one process, by the method of tools/ground_walk_probe.py:
torch events around back-to-back launches on one stream, the variants taking turns inside every round (the order reversed on odd rounds), after a second of launches for
the clock and 20 warm launches of every variant.  Variants: the ground step on a plane per robot; the height-field step on a 1024 x 1024 rough field (8 MiB: gathers that
miss) and on a 16 x 16 field that stays in cache, each cell-constant and bilinear.  The robots stand uniformly over the field, so a wavefront's gathers are scattered.
Run under `rocprofv3 --kernel-trace` the dispatches are in the trace in the order of the plan this writes (json: one entry per batch), which gives the kernels' own
durations without the gaps between launches."""
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
out_path = sys.argv[1] if len(sys.argv) > 1 else "heightfield_probe.json"
dev = torch.device("cuda:0")
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
h, ROUNDS, SPAN = 4, 7, 2.5
G = pkg.heightfields
res, plan = [], []
for n, launches in ((4096, 200), (65536, 50)):
    sc = pkg.scenarios.config3_random_flat(nb=n, horizon=h)
    rng = np.random.default_rng(1)
    R, foot = T(sc["R"]), T(sc["foot"])
    grf = T(rng.normal(0, 15, (n, 12)) + np.tile([0.0, 0.0, 30.0], 4))
    ct = T((rng.random((n, 4)) < 0.7).astype(np.uint8))
    x = np.array(sc["x0"][:, :12]); x[:, 3:5] = rng.uniform(-SPAN, SPAN, (n, 2))
    state = T(x)
    yaw = np.arctan2(sc["R"].reshape(n, 9)[:, 3], sc["R"].reshape(n, 9)[:, 0])
    Rz = T(pkg.scenarios.rot_zyx(0 * yaw, 0 * yaw, yaw).reshape(n, 9)); target = T(np.asarray(sc["foot"]).reshape(n, 12) + rng.uniform(-0.1, 0.1, (n, 12)))
    ground = T(np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)], 1))
    Z = lambda w, dt=torch.float64: torch.zeros((n, w), dtype=dt, device=dev)
    so, Ro, fo, vo, to, go = Z(12), Z(9), Z(12), Z(12), Z(4, torch.uint8), Z(3)   # (out of place: the timed launches all read the same state)
    cfg = pkg.make_config(sc["params"], h, warm_start=0)
    with pkg.Engine(cfg, n, 0) as eng:
        eng.set_timing(False)
        st = torch.cuda.Stream(); torch.cuda.synchronize()
        s = st.cuda_stream
        w1 = eng.walk_config(substeps=1, swing_track=1.0)
        fields = {}
        for interp in (0, 1):
            fields[f"heightfield 1024 x 1024, interp {interp}"] = eng.heightfield(G.rough(1024, 1024, 1, 0.05), -SPAN, -SPAN, 2 * SPAN / 1023, 2 * SPAN / 1023, interp)
            fields[f"heightfield 16 x 16, interp {interp}"] = eng.heightfield(G.rough(16, 16, 2, 0.05), -SPAN, -SPAN, 2 * SPAN / 15, 2 * SPAN / 15, interp)
        calls = {"ground step": lambda: eng.walk_step_ground_device(n, state, 12, R, foot, grf, ct, Rz, target, vo, to, ground, None, so, Ro, fo, walk=w1, stream=s)}
        for label, f in fields.items():
            calls[label] = lambda f=f: eng.walk_step_heightfield_device(n, state, 12, R, foot, grf, ct, Rz, target, vo, to, f, None, None, so, Ro, fo, walk=w1, stream=s,
                                                                        d_ground_out=go)
        t0 = time.time()
        while time.time() - t0 < 1.0:   # the clock ramp
            for call in calls.values():
                call()
        for call in calls.values():
            for _ in range(20):
                call()
        torch.cuda.synchronize()
        plan.append(dict(n=n, phase="warm"))
        times = {k: [] for k in calls}
        for rep in range(ROUNDS):
            order = list(calls) if rep % 2 == 0 else list(calls)[::-1]
            for k in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(launches):
                    calls[k]()
                e1.record(st); torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / launches)
                plan.append(dict(n=n, phase="timed", round=rep, variant=k, launches=launches))
        for label, all_us in times.items():
            ratios = [a / b for a, b in zip(all_us, times["ground step"])]
            r = dict(kernel=label, n=n, us_per_launch_median=float(np.median(all_us)), us_per_launch_all=[round(t, 3) for t in all_us], launches=launches,
                     ratio_to_ground_step_median=float(np.median(ratios)), ratio_all=[round(v, 3) for v in ratios])
            print(json.dumps(r), flush=True); res.append(r)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(dict(results=res, plan=plan), open(out_path, "w"), indent=1)
