"""a1mpc_horizon_states_kernel: time per launch (torch events around back-to-back launches on one stream) -> bytes moved per second."""
import json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
launches = int(sys.argv[1]) if len(sys.argv) > 1 else 300
out_path = sys.argv[2] if len(sys.argv) > 2 else "horizon_states_probe.json"
dev = torch.device("cuda:0")
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
res = []
for n, h in ((4096, 10), (65536, 20)):
    sc = pkg.scenarios.config3_random_flat(nb=n, horizon=h)
    rng = np.random.default_rng(1)
    u = T(rng.uniform(-60, 180, (n, 12 * h))); feet = T(np.tile(sc["foot"], (1, h)) + rng.normal(0, 1e-3, (n, 12 * h)))
    x0, xref, R, foot = T(sc["x0"]), T(sc["xref"]), T(sc["R"]), T(sc["foot"])
    xp = torch.zeros((n, h * 13), dtype=torch.float64, device=dev); cost = torch.zeros((n, 2), dtype=torch.float64, device=dev)
    cfg = pkg.make_config(sc["params"], h, warm_start=0)
    with pkg.Engine(cfg, n, 0) as eng:
        eng.set_timing(False)
        st = torch.cuda.Stream(); torch.cuda.synchronize()
        for label, f, fs in (("broadcast", foot, 0), ("per_step", feet, 12)):
            for _ in range(20):
                eng.horizon_states_device(n, x0, xref, R, f, fs, u, xp, cost, stream=st.cuda_stream)
            torch.cuda.synchronize()
            times = []
            for rep in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(launches):
                    eng.horizon_states_device(n, x0, xref, R, f, fs, u, xp, cost, stream=st.cuda_stream)
                e1.record(st); torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3 / launches)
            doubles = n * (13 + 9 + (12 * h if fs else 12) + 12 * h + 13 * h + 13 * h + 2)
            us = float(np.median(times))
            r = dict(n=n, h=h, feet=label, us_per_launch_median=us, us_per_launch_all=[round(t, 3) for t in times], bytes=doubles * 8, TB_per_s=doubles * 8 / us * 1e-6,
                     launches=launches)
            print(json.dumps(r), flush=True); res.append(r)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
