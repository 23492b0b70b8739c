"""a1mpc_walk_step_ground_kernel and a1mpc_walk_sensors_touch_kernel: time per launch against a1mpc_walk_step_kernel and a1mpc_walk_sensors_kernel, which they copy,
by the method of tools/walk_step_probe.py: torch events around back-to-back launches on one stream, the kernels taking turns inside every round, so that a ratio is
formed from launches a few milliseconds apart; the median of five rounds and every round's figure are reported beside the byte ratio from the shapes (the step: 24 B more
in and 4 B more out per robot; the sensors: 4 B more in)."""
import json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
launches = int(sys.argv[1]) if len(sys.argv) > 1 else 300
out_path = sys.argv[2] if len(sys.argv) > 2 else "ground_walk_probe.json"
dev = torch.device("cuda:0")
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
h, ROUNDS = 4, 5


def timed(calls, st):
    """calls: {label: launch} -> {label: microseconds per launch of each round}"""
    for call in calls.values():
        for _ in range(20):
            call()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for rep in range(ROUNDS):
        for k, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(launches):
                call()
            e1.record(st); torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / launches)
    return times


res = []
for n in (4096, 65536):
    sc = pkg.scenarios.config3_random_flat(nb=n, horizon=h)
    rng = np.random.default_rng(1)
    R, foot = T(sc["R"]), T(sc["foot"])
    grf = T(rng.normal(0, 15, (n, 12)) + np.tile([0.0, 0.0, 30.0], 4)); ext = T(rng.normal(0, 5, (n, 6)))
    ct = T((rng.random((n, 4)) < 0.7).astype(np.uint8)); state = T(sc["x0"][:, :12])
    yaw = np.arctan2(sc["R"].reshape(n, 9)[:, 3], sc["R"].reshape(n, 9)[:, 0])
    Rz = T(pkg.scenarios.rot_zyx(0 * yaw, 0 * yaw, yaw).reshape(n, 9)); target = T(np.asarray(sc["foot"]).reshape(n, 12) + rng.uniform(-0.1, 0.1, (n, 12)))
    vel = T(rng.normal(0, 1, (n, 12)))
    ground = T(np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)], 1))
    touch_in = T((rng.random((n, 4)) < 0.5).astype(np.uint8))
    Z = lambda w, dt=torch.float64: torch.zeros((n, w), dtype=dt, device=dev)
    so, Ro, fo, vo, to = Z(12), Z(9), Z(12), Z(12), Z(4, torch.uint8)   # (out of place: the timed launches all read the same state)
    sens = [Z(4), Z(3), Z(3), Z(12), Z(12), Z(4), Z(4, torch.uint8), Z(12), Z(12)]
    cfg = pkg.make_config(sc["params"], h, warm_start=0)
    walk_bytes = (12 + 9 + 12 + 12 + 6 + 12 + 9 + 12) * 8 + 4 + (9 + 12 + 12) * 8
    sensor_bytes = (12 + 9 + 12 + 12 + 6) * 8 + 4 + (4 + 3 + 3 + 12 + 12 + 4 + 12 + 12) * 8 + 4 + 12 * 8
    with pkg.Engine(cfg, n, 0) as eng:
        eng.set_timing(False)
        st = torch.cuda.Stream(); torch.cuda.synchronize()
        s = st.cuda_stream
        for sub in (1, 4):
            w1 = eng.walk_config(substeps=sub, swing_track=1.0, flat_ground=1)
            calls = {"walk_step": lambda: eng.walk_step_device(n, state, 12, R, foot, grf, ct, Rz, target, vo, ext, so, Ro, fo, walk=w1, stream=s),
                     "walk_step_ground": lambda: eng.walk_step_ground_device(n, state, 12, R, foot, grf, ct, Rz, target, vo, to, ground, ext, so, Ro, fo, walk=w1, stream=s),
                     "walk_step_ground, ground NULL": lambda: eng.walk_step_ground_device(n, state, 12, R, foot, grf, ct, Rz, target, vo, to, None, ext, so, Ro, fo, walk=w1,
                                                                                           stream=s)}
            nbytes = {"walk_step": walk_bytes, "walk_step_ground": walk_bytes + 28, "walk_step_ground, ground NULL": walk_bytes + 4}
            if sub == 1:
                calls["walk_sensors"] = lambda: eng.walk_sensors_device(n, state, 12, R, foot, grf, ct, *sens, d_ext_wrench=ext, d_foot_vel_body=vel, stream=s)
                calls["walk_sensors_touch"] = lambda: eng.walk_sensors_touch_device(n, state, 12, R, foot, grf, ct, *sens, d_ext_wrench=ext, d_foot_vel_body=vel,
                                                                                    d_touch=touch_in, touch_force=60.0, stream=s)
                nbytes.update({"walk_sensors": sensor_bytes, "walk_sensors_touch": sensor_bytes + 4})
            times = timed(calls, st)
            for label, all_us in times.items():
                us = float(np.median(all_us))
                base = "walk_sensors" if "sensors" in label else "walk_step"
                ratios = [a / b for a, b in zip(all_us, times[base])]
                r = dict(kernel=label, n=n, substeps=sub, us_per_launch_median=us, us_per_launch_all=[round(t, 3) for t in all_us], bytes=n * nbytes[label],
                         TB_per_s=n * nbytes[label] / us * 1e-6, launches=launches, against=base, ratio_median=float(np.median(ratios)), ratio_all=[round(x, 3) for x in ratios],
                         byte_ratio=nbytes[label] / nbytes[base])
                print(json.dumps(r), flush=True); res.append(r)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
