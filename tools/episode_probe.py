"""a1mpc_episode_update_kernel and a1mpc_episode_reduce_kernel: time per launch beside a1mpc_walk_sensors_kernel, by the method of tools/sensor_noise_probe.py: torch
events around back-to-back launches on one stream, the kernels taking turns inside every round, so that a ratio is formed from launches a few milliseconds apart; the
median of five rounds and every round's figure are reported.  The update is timed with every input given and with the truth alone (state and R_world); the summary's
figure is one whole summary, all its levels.  Usage: episode_probe.py [launches] [out.json]"""
import json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
launches = int(sys.argv[1]) if len(sys.argv) > 1 else 300
out_path = sys.argv[2] if len(sys.argv) > 2 else "episode_probe.json"
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
    ct = T((rng.random((n, 4)) < 0.7).astype(np.uint8)); state = T(sc["x0"][:, :12]); vel = T(rng.normal(0, 1, (n, 12)))
    Z = lambda w, dt=torch.float64: torch.zeros((n, w), dtype=dt, device=dev)
    sens = [Z(4), Z(3), Z(3), Z(12), Z(12), Z(4), Z(4, torch.uint8), Z(12), Z(12)]
    est_pos, est_vel, cmd, ground = T(rng.normal(0, 1, (n, 3))), T(rng.normal(0, 1, (n, 3))), T(rng.normal(0, 0.3, (n, 3))), T(rng.normal(0, 0.01, (n, 3)))
    pdz, status, reach = T(np.full(n, 0.3)), T(np.ones(n, np.int32)), Z(4, torch.uint8)
    episode, truth_only, summary = Z(16), Z(16), torch.zeros(20, dtype=torch.float64, device=dev)
    cfg = pkg.make_config(sc["params"], h, warm_start=0)
    sensor_bytes = (12 + 9 + 12 + 12 + 6) * 8 + 4 + (4 + 3 + 3 + 12 + 12 + 4 + 12 + 12) * 8 + 4 + 12 * 8
    update_bytes = (12 + 9 + 3 + 3 + 3 + 1 + 3 + 12) * 8 + 4 + 4 + 4 + 2 * 16 * 8
    levels, m = 0, n
    while True:
        m = (m + 63) // 64; levels += 1
        if m == 1:
            break
    with pkg.Engine(cfg, n, 0) as eng:
        eng.set_timing(False)
        st = torch.cuda.Stream(); torch.cuda.synchronize()
        s = st.cuda_stream
        ec = eng.episode_config(min_up=-1.0, min_height=-1e9)   # (nobody ends: every launch accumulates every word)
        tick = [0]

        def update(rec, **inputs):
            tick[0] += 1
            eng.episode_update_device(n, tick[0], rec, state, 12, R, config=ec, stream=s, **inputs)

        every = dict(d_root_pos=est_pos, d_root_lin_vel=est_vel, d_root_lin_vel_d=cmd, d_root_pos_d_z=pdz, d_ground=ground, d_grf_body=grf, d_contacts=ct, d_status=status,
                     d_reach=reach)
        calls = {"walk_sensors": lambda: eng.walk_sensors_device(n, state, 12, R, foot, grf, ct, *sens, d_ext_wrench=ext, d_foot_vel_body=vel, stream=s),
                 "episode_update": lambda: update(episode, **every),
                 "episode_update, truth alone": lambda: update(truth_only),
                 "episode_summary": lambda: eng.episode_summary_device(n, episode, summary, stream=s)}
        nbytes = {"walk_sensors": sensor_bytes, "episode_update": update_bytes, "episode_update, truth alone": (12 + 9) * 8 + 2 * 16 * 8, "episode_summary": 16 * 8}
        times = timed(calls, st)
        for label, all_us in times.items():
            us = float(np.median(all_us))
            ratios = [a / b for a, b in zip(all_us, times["walk_sensors"])]
            r = dict(kernel=label, n=n, us_per_launch_median=us, us_per_launch_all=[round(t, 3) for t in all_us], bytes=n * nbytes[label], TB_per_s=n * nbytes[label] / us * 1e-6,
                     launches=launches, against="walk_sensors", ratio_median=float(np.median(ratios)), ratio_all=[round(x, 3) for x in ratios])
            if label == "episode_summary":
                r["levels"] = levels
            print(json.dumps(r), flush=True); res.append(r)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
