"""Runs on the GPU: the balance-QP controller's numbers for profiles/balance_tick.md -- the PD-wrench kernel (time per launch, achieved bytes per second: 27 doubles in,
6 out per robot) at 4096 and 65 536 robots, and a1mpc_control_tick_balance_device at n = 1 and 4096 (runs of 100 back-to-back ticks between events on the caller's
stream, the handle's timing events on / off / off / on) with the MPC control tick of the same build and session beside it (bench.full_tick_probe, the same protocol).
usage: python tools/balance_tick_probe.py [out.json]"""
import ctypes as C, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
import __graft_entry__ as g
pkg = g.load_package()
out_path = sys.argv[1] if len(sys.argv) > 1 else "balance_tick_probe.json"
dev = torch.device("cuda:0")
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
scen, E = pkg.scenarios, pkg.engine
P = scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS
res = dict(wrench=[], balance_tick=[], mpc_tick=[])

for n in (4096, 65536):
    rng = np.random.default_rng(n)
    v3 = [T(rng.normal(0, 0.3, (n, 3))) for _ in range(8)]
    eul = rng.normal(0, 0.3, (n, 3))
    R = T(scen.rot_zyx(eul[:, 0], eul[:, 1], eul[:, 2]).reshape(n, 9)); acc = torch.zeros((n, 6), dtype=torch.float64, device=dev)
    with pkg.Engine(pkg.make_config(P, 10), n, 0) as eng:
        eng.set_timing(False)
        st = torch.cuda.Stream(); torch.cuda.synchronize()
        launches = 300
        for _ in range(50):
            eng.balance_wrench_device(n, *v3, R, acc, stream=st.cuda_stream)
        torch.cuda.synchronize()
        times = []
        for rep in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(launches):
                eng.balance_wrench_device(n, *v3, R, acc, stream=st.cuda_stream)
            e1.record(st); torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / launches)
        us = float(np.median(times)); nbytes = n * 33 * 8
        r = dict(n=n, us_per_launch_median=us, us_per_launch_all=[round(t, 3) for t in times], bytes=nbytes, GB_per_s=nbytes / us * 1e-3, launches=launches)
        print(json.dumps(dict(wrench=r)), flush=True); res["wrench"].append(r)


def balance_tick(n, long_ticks=100):
    rng = np.random.default_rng(7)
    eul = rng.normal(0, 0.03, (n, 3)); eul[:, 2] = rng.uniform(-1, 1, n)
    inp = dict(joint_pos=np.tile([0.0, 0.8, -1.6], (n, 4)) + rng.normal(0, 0.05, (n, 12)), joint_vel=rng.normal(0, 0.3, (n, 12)),
               R_world=scen.rot_zyx(eul[:, 0], eul[:, 1], eul[:, 2]).reshape(n, 9), R_z=scen.rot_zyx(0 * eul[:, 0], 0 * eul[:, 0], eul[:, 2]).reshape(n, 9), root_euler=eul,
               root_ang_vel=rng.normal(0, 0.1, (n, 3)), imu_acc=np.array([0, 0, 9.81]) + rng.normal(0, 0.1, (n, 3)), imu_ang_vel=rng.normal(0, 0.1, (n, 3)),
               foot_force=rng.uniform(20, 120, (n, 4)), movement_mode=np.ones(n, np.uint8), mpc_active=np.ones(n, np.uint8),
               root_lin_vel_d=np.c_[rng.uniform(-0.3, 0.3, (n, 2)), np.zeros(n)], root_ang_vel_d=np.c_[np.zeros((n, 2)), rng.uniform(-0.3, 0.3, n)], root_pos_d_z=np.full(n, 0.3),
               gait_counter_speed=np.full((n, 4), 2.0), torques_gravity=rng.normal(0, 0.3, (n, 12)),
               gait_counter=np.tile([0.0, 120.0, 120.0, 0.0], (n, 1)), root_euler_d=np.c_[np.zeros((n, 2)), eul[:, 2]])   # (the sensors of bench.full_tick_probe)
    f64 = dict(foot_pos_start=12, foot_pos_rel_last_time=12, foot_pos_target_last_time=12, joint_torques=12, root_pos=3, root_lin_vel=3, foot_pos_rel=12, j_foot_blocks=36,
               foot_vel_rel=12, foot_pos_abs=12, foot_vel_abs=12, foot_pos_world=12, foot_vel_world=12, foot_pos_target_rel=12, foot_pos_target_abs=12, foot_pos_target_world=12,
               foot_pos_cur=12, foot_forces_kin=12, foot_pos_recent_contact=12, terrain_angle=1, grf=12)
    d = {k: T(v) for k, v in inp.items()}
    d.update({k: torch.zeros((n, m), dtype=torch.float64, device=dev) for k, m in f64.items()})
    d.update({k: torch.zeros((n, 4), dtype=torch.uint8, device=dev) for k in ("estimated_contacts", "plan_contacts", "contacts")})
    d.update({k: torch.zeros(n, dtype=torch.int32, device=dev) for k in ("iters", "status")})
    pos_d = T(np.tile([0.0, 0.0, 0.3], (n, 1)))
    bf = E.TickBuffers()
    for k in E.TICK_BUFFER_FIELDS:
        setattr(bf, k, d[k].data_ptr())
    with pkg.Engine(pkg.make_config(P, 10), n, 0) as eng:
        prm = E.TickParams(); eng.lib.a1mpc_default_tick_params(C.byref(prm))
        bt = eng.balance_tick(pos_d)
        st = torch.cuda.Stream(device=dev); torch.cuda.synchronize()
        for _ in range(64):
            eng.control_tick_balance_device(prm, bt, bf, n, stream=st.cuda_stream)
        st.synchronize()
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)

        def run(timing):
            eng.set_timing(timing)
            eng.control_tick_balance_device(prm, bt, bf, n, stream=st.cuda_stream)
            e0.record(st)
            for _ in range(long_ticks):
                eng.control_tick_balance_device(prm, bt, bf, n, stream=st.cuda_stream)
            e1.record(st); st.synchronize()
            return e0.elapsed_time(e1) / long_ticks
        runs = [(x, run(bool(x))) for x in (1, 0, 0, 1)]
        last_ms, fused = eng.last_control_tick_ms(); qp_ms = eng.last_kernel_ms()
        return dict(n=n, ms_per_tick_timing_on=float(np.mean([v for x, v in runs if x])), ms_per_tick_timing_off=float(np.mean([v for x, v in runs if not x])),
                    runs_on_off_off_on=[round(v, 5) for _, v in runs], last_tick_ms_by_its_own_events=last_ms, balance_qp_launch_ms_of_the_last_tick=qp_ms, torques_fused=bool(fused),
                    mean_qp_iters=float(d["iters"].float().mean().item()), solved_frac=float((d["status"] == 1).float().mean().item()))


for n in (1, 4096):
    r = balance_tick(n); print(json.dumps(dict(balance_tick=r)), flush=True); res["balance_tick"].append(r)
    m = bench.full_tick_probe(pkg, 0, n=n)
    m = {k: m[k] for k in ("ms_per_tick", "ms_per_tick_with_a1mpc_set_timing_off", "last_tick_ms_by_its_own_events", "mpc_launch_ms_of_the_last_tick", "mean_mpc_iters")} | dict(n=n)
    print(json.dumps(dict(mpc_tick=m)), flush=True); res["mpc_tick"].append(m)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
