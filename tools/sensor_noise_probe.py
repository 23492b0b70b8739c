"""a1mpc_sensor_noise_kernel: time per launch beside a1mpc_walk_sensors_kernel, whose outputs it works on, by the method of tools/ground_walk_probe.py: torch events around
back-to-back launches on one stream, the kernels taking turns inside every round, so that a ratio is formed from launches a few milliseconds apart; the median of five
rounds and every round's figure are reported.  The noise kernel is timed with every channel on, with z_out as well, and with the IMU channels alone (16 of its 22 draws
skipped).  Usage: sensor_noise_probe.py [launches] [out.json]"""
import json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
launches = int(sys.argv[1]) if len(sys.argv) > 1 else 300
out_path = sys.argv[2] if len(sys.argv) > 2 else "sensor_noise_probe.json"
dev = torch.device("cuda:0")
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
h, ROUNDS = 4, 5
LEVELS = dict(seed=2026, gyro_sigma=0.01, acc_sigma=0.1, gyro_bias_walk=1e-5, acc_bias_walk=1e-4, att_sigma=0.002, joint_pos_sigma=0.001, joint_vel_sigma=0.05,
              foot_force_sigma=5.0)


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
    noisy = [T(np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))), Z(3), Z(3), Z(12), Z(12), Z(4)]   # (arrays of their own: the timed launches keep adding noise to them)
    bias, z = Z(6), Z(44)
    cfg = pkg.make_config(sc["params"], h, warm_start=0)
    sensor_bytes = (12 + 9 + 12 + 12 + 6) * 8 + 4 + (4 + 3 + 3 + 12 + 12 + 4 + 12 + 12) * 8 + 4 + 12 * 8
    noise_bytes = 2 * (4 + 3 + 3 + 12 + 12 + 4 + 6) * 8
    with pkg.Engine(cfg, n, 0) as eng:
        eng.set_timing(False)
        st = torch.cuda.Stream(); torch.cuda.synchronize()
        s = st.cuda_stream
        every, imu = eng.noise_config(**LEVELS), eng.noise_config(seed=2026, gyro_sigma=0.01, acc_sigma=0.1, gyro_bias_walk=1e-5, acc_bias_walk=1e-4)
        tick = [0]

        def noise(nc, arrays, d_z=None):
            tick[0] += 1
            eng.sensor_noise_device(nc, n, tick[0], *arrays, bias, d_z=d_z, stream=s)

        calls = {"walk_sensors": lambda: eng.walk_sensors_device(n, state, 12, R, foot, grf, ct, *sens, d_ext_wrench=ext, d_foot_vel_body=vel, stream=s),
                 "sensor_noise": lambda: noise(every, noisy),
                 "sensor_noise, z_out": lambda: noise(every, noisy, z),
                 "sensor_noise, IMU alone": lambda: noise(imu, [None, noisy[1], noisy[2], None, None, None])}
        nbytes = {"walk_sensors": sensor_bytes, "sensor_noise": noise_bytes, "sensor_noise, z_out": noise_bytes + 44 * 8, "sensor_noise, IMU alone": 2 * (3 + 3 + 6) * 8}
        times = timed(calls, st)
        for label, all_us in times.items():
            us = float(np.median(all_us))
            ratios = [a / b for a, b in zip(all_us, times["walk_sensors"])]
            r = dict(kernel=label, n=n, us_per_launch_median=us, us_per_launch_all=[round(t, 3) for t in all_us], bytes=n * nbytes[label], TB_per_s=n * nbytes[label] / us * 1e-6,
                     launches=launches, against="walk_sensors", ratio_median=float(np.median(ratios)), ratio_all=[round(x, 3) for x in ratios])
            print(json.dumps(r), flush=True); res.append(r)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
