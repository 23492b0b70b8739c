"""a1mpc_sensor_synthesis_kernel: time per launch (torch events around back-to-back launches on one stream) -> bytes moved per second, with a1mpc_plant_step_kernel (one
sub-step, out of place) in the same run: the two kernels share the layout and move comparable traffic."""
import json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
launches = int(sys.argv[1]) if len(sys.argv) > 1 else 300
out_path = sys.argv[2] if len(sys.argv) > 2 else "sensor_synthesis_probe.json"
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
    R = T(sc["R"])
    footb = np.array(pkg.scenarios.PARAM_SETS["gazebo"]["foot"], float).reshape(1, 4, 3) + rng.uniform(-0.03, 0.03, (n, 4, 3))   # within every leg's reach
    foot = T(np.einsum("bij,blj->bli", sc["R"].reshape(n, 3, 3), footb).reshape(n, 12))
    grf = T(rng.normal(0, 15, (n, 12)) + np.tile([0.0, 0.0, 30.0], 4)); ext = T(rng.normal(0, 5, (n, 6)))
    ct = T((rng.random((n, 4)) < 0.7).astype(np.uint8)); state = T(sc["x0"][:, :12])
    Z = lambda w, dt=torch.float64: torch.zeros((n, w), dtype=dt, device=dev)
    so, Ro, fo = torch.zeros_like(state), torch.zeros_like(R), torch.zeros_like(foot)
    o = dict(quat=Z(4), acc=Z(3), gyro=Z(3), jp=Z(12), jv=Z(12), ff=Z(4), reach=Z(4, torch.uint8), pr=Z(12), vr=Z(12))
    cfg = pkg.make_config(sc["params"], h, warm_start=0)
    with pkg.Engine(cfg, n, 0) as eng:
        eng.set_timing(False)
        st = torch.cuda.Stream(); torch.cuda.synchronize()
        pc = eng.plant_config(substeps=1)
        rows = [("plant_step", lambda: eng.plant_step_device(n, state, 12, R, foot, grf, ct, ext, so, Ro, fo, plant=pc, stream=st.cuda_stream),
                 n * ((12 + 9 + 12 + 12 + 6 + 12 + 9 + 12) * 8 + 4)),
                ("sensor_synthesis", lambda: eng.sensor_synthesis_device(n, state, 12, R, foot, grf, ct, o["quat"], o["acc"], o["gyro"], o["jp"], o["jv"], o["ff"], o["reach"],
                                                                         o["pr"], o["vr"], d_ext_wrench=ext, stream=st.cuda_stream),
                 n * ((12 + 9 + 12 + 12 + 6 + 4 + 3 + 3 + 12 + 12 + 4 + 12 + 12) * 8 + 8)),
                ("sensor_synthesis, no foot_rel outputs", lambda: eng.sensor_synthesis_device(n, state, 12, R, foot, grf, ct, o["quat"], o["acc"], o["gyro"], o["jp"], o["jv"],
                                                                                              o["ff"], o["reach"], d_ext_wrench=ext, stream=st.cuda_stream),
                 n * ((12 + 9 + 12 + 12 + 6 + 4 + 3 + 3 + 12 + 12 + 4) * 8 + 8))]
        for label, call, nbytes in rows:
            us, all_us = timed(call, st)
            r = dict(kernel=label, n=n, us_per_launch_median=us, us_per_launch_all=all_us, bytes=nbytes, TB_per_s=nbytes / us * 1e-6, launches=launches)
            print(json.dumps(r), flush=True); res.append(r)
        torch.cuda.synchronize()
        assert not o["reach"].any().item(), "the probe's feet are meant to be reachable"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
