"""a1mpc_plant_step_kernel: time per launch (torch events around back-to-back launches on one stream) -> bytes moved per second, with a1mpc_horizon_states_kernel at
h = 4 in the same run as the yardstick of a memory-bound kernel of this size."""
import json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
launches = int(sys.argv[1]) if len(sys.argv) > 1 else 300
out_path = sys.argv[2] if len(sys.argv) > 2 else "plant_step_probe.json"
dev = torch.device("cuda:0")
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
h = 4


def timed(call, st):
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    times = []
    for rep in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(launches):
            call()
        e1.record(st); torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / launches)
    return float(np.median(times)), [round(t, 3) for t in times]


res = []
for n in (4096, 65536):
    sc = pkg.scenarios.config3_random_flat(nb=n, horizon=h)
    rng = np.random.default_rng(1)
    x0, xref, R, foot = T(sc["x0"]), T(sc["xref"]), T(sc["R"]), T(sc["foot"])
    u = T(rng.uniform(-60, 180, (n, 12 * h))); grf = T(rng.normal(0, 15, (n, 12)) + np.tile([0.0, 0.0, 30.0], 4)); ext = T(rng.normal(0, 5, (n, 6)))
    ct = T((rng.random((n, 4)) < 0.7).astype(np.uint8)); state = T(sc["x0"][:, :12])
    xp = torch.zeros((n, h * 13), dtype=torch.float64, device=dev); cost = torch.zeros((n, 2), dtype=torch.float64, device=dev)
    so, Ro, fo = torch.zeros_like(state), torch.zeros_like(R), torch.zeros_like(foot)   # (out of place: the timed launches all read the same state)
    cfg = pkg.make_config(sc["params"], h, warm_start=0)
    with pkg.Engine(cfg, n, 0) as eng:
        eng.set_timing(False)
        st = torch.cuda.Stream(); torch.cuda.synchronize()
        rows = [("horizon_states h4", None, lambda: eng.horizon_states_device(n, x0, xref, R, foot, 0, u, xp, cost, stream=st.cuda_stream),
                 n * (13 + 9 + 12 + 12 * h + 13 * h + 13 * h + 2) * 8)]
        for sub in (1, 4):
            pc = eng.plant_config(substeps=sub)
            rows.append(("plant_step", sub, (lambda pc=pc: eng.plant_step_device(n, state, 12, R, foot, grf, ct, ext, so, Ro, fo, plant=pc, stream=st.cuda_stream)),
                         n * ((12 + 9 + 12 + 12 + 6 + 12 + 9 + 12) * 8 + 4)))
        for label, sub, call, nbytes in rows:
            us, all_us = timed(call, st)
            r = dict(kernel=label, n=n, substeps=sub, us_per_launch_median=us, us_per_launch_all=all_us, bytes=nbytes, TB_per_s=nbytes / us * 1e-6, launches=launches)
            print(json.dumps(r), flush=True); res.append(r)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
