"""Runs on the GPU: the sensor / command front end's numbers for profiles/sensor_frontend.md --
  kernels  a1mpc_sensor_frontend_batch_device and a1mpc_command_batch_device alone at 65 536 robots: time per launch of 300 back-to-back launches between events (five
           rounds, median; at this size that is the host's enqueue rate, the kernels' own durations come from a kernel trace of the `kernels` run) and the bytes each moves (sensor: 10 doubles in, 30 out, 14 doubles and 2 words of filter state read and written; command: 19 doubles, 2 bytes
           and a word in, 21 doubles, 3 bytes and a word out);
  copy     what the front end replaces: the eleven fields it produces (298 bytes per robot) from pinned host memory to the device, and the raw inputs a host
           implementation would need first (quaternion, IMU sample, command: 129 bytes per robot) from the device to pinned host memory, per tick, same protocol;
  ticks    a1mpc_control_tick_sensors_device beside a1mpc_control_tick_device of the same build on the same inputs at n = 1, 4096 and 65 536: runs of 100 back-to-back
           ticks between events on the caller's stream, the handle's timing events on / off / off / on (the protocol of bench.full_tick_probe, which supplies the
           second figure).
usage: python tools/sensor_frontend_probe.py [out.json] [sizes, comma separated | kernels]
       rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/sensor_frontend_probe.py out.json kernels     (kernel durations: a run of its own)"""
import ctypes as C, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
import __graft_entry__ as g
pkg = g.load_package()
out_path = sys.argv[1] if len(sys.argv) > 1 else "sensor_frontend_probe.json"
kernels_only = len(sys.argv) > 2 and sys.argv[2] == "kernels"   # the two kernels alone and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`
sizes = [] if kernels_only else [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 4096, 65536]
dev = torch.device("cuda:0")
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
scen, E = pkg.scenarios, pkg.engine
P = scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS
res = dict(kernels=[], copy=[], ticks=[])
SENSOR_OUT = (("R_world", 9), ("R_z", 9), ("root_euler", 3), ("imu_acc", 3), ("imu_ang_vel", 3), ("root_ang_vel", 3))
COMMAND_OUT = (("root_lin_vel_d", 3, torch.float64), ("root_ang_vel_d", 3, torch.float64), ("movement_mode", 1, torch.uint8), ("mpc_active", 1, torch.uint8),
               ("root_pos_d_z", 1, torch.float64))


def quat_of_euler(eul):
    cr, sr, cp, sp, cy, sy = np.cos(eul[:, 0] / 2), np.sin(eul[:, 0] / 2), np.cos(eul[:, 1] / 2), np.sin(eul[:, 1] / 2), np.cos(eul[:, 2] / 2), np.sin(eul[:, 2] / 2)
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], axis=1)


def timed(st, launch, launches=300, rounds=5, warm=50):
    for _ in range(warm):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(launches):
            launch()
        e1.record(st); torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / launches)
    return float(np.median(times)), [round(t, 3) for t in times]


def raw_inputs(n, rng):
    eul = rng.normal(0, 0.03, (n, 3)); eul[:, 2] = rng.uniform(-1, 1, n)
    return dict(quat=quat_of_euler(eul), imu_acc_raw=np.array([0, 0, 9.81]) + rng.normal(0, 0.1, (n, 3)), imu_gyro_raw=rng.normal(0, 0.1, (n, 3)),
                cmd=np.c_[rng.uniform(-0.3, 0.3, (n, 2)), np.zeros((n, 3)), rng.uniform(-0.3, 0.3, n)], mode_toggle=np.zeros(n, np.uint8)), eul


def command_state(n):
    return {k: T(v) for k, v in pkg.Engine.command_state(n).items()}


# ---- the two kernels alone
n = 65536
with pkg.Engine(pkg.make_config(P, 10), n, 0) as eng:
    eng.set_timing(False)
    raw, _ = raw_inputs(n, np.random.default_rng(n)); d = {k: T(v) for k, v in raw.items()}
    so = [torch.zeros((n, w), dtype=torch.float64, device=dev) for _, w in SENSOR_OUT]
    co = [torch.zeros((n, w) if w > 1 else (n,), dtype=t, device=dev) for _, w, t in COMMAND_OUT]
    cs = command_state(n); pos = T(np.tile([0.0, 0.0, 0.3], (n, 1)))
    st = torch.cuda.Stream(); torch.cuda.synchronize()
    us, runs = timed(st, lambda: eng.sensor_frontend_device(n, d["quat"], d["imu_acc_raw"], d["imu_gyro_raw"], *so, stream=st.cuda_stream))
    nbytes = n * ((10 + 30 + 2 * 14) * 8 + 2 * 2 * 4)
    r = dict(kernel="a1mpc_sensor_frontend_kernel", n=n, us_per_launch_median=us, us_per_launch_all=runs, bytes=nbytes, GB_per_s=nbytes / us * 1e-3)
    print(json.dumps(r), flush=True); res["kernels"].append(r)
    us, runs = timed(st, lambda: eng.command_device(n, d["cmd"], d["mode_toggle"], pos, 0.0025, *[cs[k] for k in E.COMMAND_STATE_FIELDS], *co, stream=st.cuda_stream))
    nbytes = n * ((6 + 3 + 1 + 3 + 3 + 2) * 8 + 2 + 4 + (1 + 3 + 3 + 2 + 3 + 3 + 1) * 8 + 3 + 4)   # (root_pos: the xy pair is used, the lines travel whole)
    r = dict(kernel="a1mpc_command_kernel", n=n, us_per_launch_median=us, us_per_launch_all=runs, bytes=nbytes, GB_per_s=nbytes / us * 1e-3)
    print(json.dumps(r), flush=True); res["kernels"].append(r)

# ---- the copy the front end replaces
for n in sizes:
    produced = [torch.zeros((n, 37), dtype=torch.float64, device=dev), torch.zeros((n, 2), dtype=torch.uint8, device=dev)]         # 9 + 9 + 3 + 3 + 3 + 3 + 3 + 3 + 1 doubles, 2 bytes
    produced_h = [torch.zeros((n, 37), dtype=torch.float64).pin_memory(), torch.zeros((n, 2), dtype=torch.uint8).pin_memory()]
    rawd = [torch.zeros((n, 16), dtype=torch.float64, device=dev), torch.zeros((n, 1), dtype=torch.uint8, device=dev)]              # 4 + 3 + 3 + 6 doubles, 1 byte
    rawh = [torch.zeros((n, 16), dtype=torch.float64).pin_memory(), torch.zeros((n, 1), dtype=torch.uint8).pin_memory()]
    st = torch.cuda.Stream(); torch.cuda.synchronize()

    def up():
        with torch.cuda.stream(st):
            for a, b in zip(produced, produced_h): a.copy_(b, non_blocking=True)

    def round_trip():
        with torch.cuda.stream(st):
            for a, b in zip(rawh, rawd): a.copy_(b, non_blocking=True)
            for a, b in zip(produced, produced_h): a.copy_(b, non_blocking=True)
    us_up, runs_up = timed(st, up, launches=100)
    us_rt, runs_rt = timed(st, round_trip, launches=100)
    r = dict(n=n, produced_bytes=n * 298, raw_bytes=n * 129, us_upload_of_the_eleven_fields=us_up, us_upload_all=runs_up, us_round_trip=us_rt, us_round_trip_all=runs_rt,
             note="back-to-back asynchronous copies on one stream: no host wait between the two directions, which a host implementation would add")
    print(json.dumps(dict(copy=r)), flush=True); res["copy"].append(r)


# ---- the tick from raw inputs beside the tick of the same build
def sensors_tick(n, long_ticks=100):
    rng = np.random.default_rng(7)
    raw, eul = raw_inputs(n, rng)
    inp = dict(joint_pos=np.tile([0.0, 0.8, -1.6], (n, 4)) + rng.normal(0, 0.05, (n, 12)), joint_vel=rng.normal(0, 0.3, (n, 12)), foot_force=rng.uniform(20, 120, (n, 4)),
               gait_counter_speed=np.full((n, 4), 2.0), torques_gravity=rng.normal(0, 0.3, (n, 12)), gait_counter=np.tile([0.0, 120.0, 120.0, 0.0], (n, 1)),
               root_euler_d=np.c_[np.zeros((n, 2)), eul[:, 2]])
    f64 = dict(foot_pos_start=12, foot_pos_rel_last_time=12, foot_pos_target_last_time=12, joint_torques=12, root_pos=3, root_lin_vel=3, foot_pos_rel=12, j_foot_blocks=36,
               foot_vel_rel=12, foot_pos_abs=12, foot_vel_abs=12, foot_pos_world=12, foot_vel_world=12, foot_pos_target_rel=12, foot_pos_target_abs=12, foot_pos_target_world=12,
               foot_pos_cur=12, foot_forces_kin=12, foot_pos_recent_contact=12, terrain_angle=1, grf=12,
               R_world=9, R_z=9, root_euler=3, root_ang_vel=3, imu_acc=3, imu_ang_vel=3, root_lin_vel_d=3, root_ang_vel_d=3, root_pos_d_z=1)
    d = {k: T(v) for k, v in inp.items()}
    d.update({k: torch.zeros((n, m), dtype=torch.float64, device=dev) for k, m in f64.items()})
    d.update({k: torch.zeros((n, 4), dtype=torch.uint8, device=dev) for k in ("estimated_contacts", "plan_contacts", "contacts")})
    d.update({k: torch.zeros(n, dtype=torch.uint8, device=dev) for k in ("movement_mode", "mpc_active")})
    d.update({k: torch.zeros(n, dtype=torch.int32, device=dev) for k in ("iters", "status")})
    bf = E.TickBuffers()
    for k in E.TICK_BUFFER_FIELDS:
        setattr(bf, k, d[k].data_ptr())
    rd = {k: T(v) for k, v in raw.items()}
    cs = command_state(n); cs.pop("root_euler_d")
    with pkg.Engine(pkg.make_config(P, bench.HORIZON, warm_start=1), n, 0) as eng:
        prm = E.TickParams(); eng.lib.a1mpc_default_tick_params(C.byref(prm))
        ts = eng.tick_sensors(**rd, **cs)
        st = torch.cuda.Stream(device=dev); torch.cuda.synchronize()
        rd["mode_toggle"].fill_(1); torch.cuda.synchronize()
        eng.control_tick_sensors_device(prm, ts, bf, n, stream=st.cuda_stream); st.synchronize()       # the first tick switches every robot to walking
        rd["mode_toggle"].fill_(0); torch.cuda.synchronize()
        for _ in range(32):
            eng.control_tick_sensors_device(prm, ts, bf, n, stream=st.cuda_stream)
        st.synchronize()
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)

        def run(timing):
            eng.set_timing(timing)
            eng.control_tick_sensors_device(prm, ts, bf, n, stream=st.cuda_stream)
            e0.record(st)
            for _ in range(long_ticks):
                eng.control_tick_sensors_device(prm, ts, bf, n, stream=st.cuda_stream)
            e1.record(st); st.synchronize()
            return e0.elapsed_time(e1) / long_ticks
        runs = [(x, run(bool(x))) for x in (1, 0, 0, 1)]
        return dict(n=n, ms_per_tick_timing_on=float(np.mean([v for x, v in runs if x])), ms_per_tick_timing_off=float(np.mean([v for x, v in runs if not x])),
                    runs_on_off_off_on=[round(v, 5) for _, v in runs], walking_frac=float(d["movement_mode"].float().mean().item()),
                    mpc_active_frac=float(d["mpc_active"].float().mean().item()), mean_mpc_iters=float(d["iters"].float().mean().item()),
                    solved_frac=float((d["status"] == 1).float().mean().item()))


for n in sizes:
    r = sensors_tick(n); print(json.dumps(dict(sensors_tick=r)), flush=True)
    m = bench.full_tick_probe(pkg, 0, n=n)
    m = {k: m[k] for k in ("ms_per_tick", "ms_per_tick_with_a1mpc_set_timing_off", "mean_mpc_iters", "solved_frac")} | dict(n=n)
    print(json.dumps(dict(mpc_tick=m)), flush=True); res["ticks"].append(dict(sensors_tick=r, mpc_tick=m))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
