"""a1mpc_respawn_kernel and a1mpc_respawn_rows_kernel: time per launch at 65 536 robots, h = 10, IMU window 5, by the method of tools/episode_probe.py: torch events
around back-to-back launches on one stream, the calls taking turns inside every round, the median of five rounds and every round's figure reported.
  decision   a1mpc_respawn_batch_device with nobody respawning, beside a1mpc_episode_update_batch_device on the same records
  reset      the same kernel through a1mpc_respawn_reset_batch_device (a respawned robot's record is zero on the next launch, so a decision cannot respawn launch after
             launch; the masked reset can) with nobody, one robot per wavefront and everybody masked, beside a fill of the same bytes (torch zero_ on four tensors of the
             blocks' sizes: what the four whole-handle memsets write, without their synchronisation)
  rows       a1mpc_respawn_rows_device with a closed loop's table (6 plant rows when = 3, 14 carried rows when = 1: two calls) at the same three densities
  ekf init   the control tick alone, behind a masked reset that clears nothing of the EKF, and behind one that names the EKF (which makes the tick launch its init kernel)
  tick       control_tick_sensors + episode_update per tick, without and with respawn + the two rows calls behind it
Usage: respawn_probe.py [launches] [out.json]"""
import ctypes as C, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
launches = int(sys.argv[1]) if len(sys.argv) > 1 else 200
out_path = sys.argv[2] if len(sys.argv) > 2 else "respawn_probe.json"
dev = torch.device("cuda:0")
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
E, scen = pkg.engine, pkg.scenarios
n, H, WINDOW, ROUNDS = 65536, 10, 5, 5


def timed(calls, st, launches=launches):
    """calls: {label: launch} -> {label: microseconds per launch of each round}"""
    for call in calls.values():
        for _ in range(10):
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


def report(section, times, against, extra=None):
    for label, all_us in times.items():
        ratios = [a / b for a, b in zip(all_us, times[against])]
        r = dict(section=section, call=label, n=n, us_per_launch_median=float(np.median(all_us)), us_per_launch_all=[round(t, 3) for t in all_us], against=against,
                 ratio_median=float(np.median(ratios)), ratio_all=[round(x, 3) for x in ratios], **(extra or {}).get(label, {}))
        print(json.dumps(r), flush=True); res.append(r)


def quat_of_euler(eul):
    cr, sr, cp, sp, cy, sy = np.cos(eul[:, 0] / 2), np.sin(eul[:, 0] / 2), np.cos(eul[:, 1] / 2), np.sin(eul[:, 1] / 2), np.cos(eul[:, 2] / 2), np.sin(eul[:, 2] / 2)
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], axis=1)


res = []
rng = np.random.default_rng(7)
eul = rng.normal(0, 0.03, (n, 3)); eul[:, 2] = rng.uniform(-1, 1, n)
raw = dict(quat=quat_of_euler(eul), imu_acc_raw=np.array([0, 0, 9.81]) + rng.normal(0, 0.1, (n, 3)), imu_gyro_raw=rng.normal(0, 0.1, (n, 3)),
           cmd=np.c_[rng.uniform(-0.3, 0.3, (n, 2)), np.zeros((n, 3)), rng.uniform(-0.3, 0.3, n)], mode_toggle=np.zeros(n, np.uint8))
inp = dict(joint_pos=np.tile([0.0, 0.8, -1.6], (n, 4)) + rng.normal(0, 0.05, (n, 12)), joint_vel=rng.normal(0, 0.3, (n, 12)), foot_force=rng.uniform(20, 120, (n, 4)),
           gait_counter_speed=np.full((n, 4), 2.0), torques_gravity=rng.normal(0, 0.3, (n, 12)), gait_counter=np.tile([0.0, 120.0, 120.0, 0.0], (n, 1)),
           root_euler_d=np.c_[np.zeros((n, 2)), eul[:, 2]])
CARRIED = dict(gait_counter=4, foot_pos_start=12, foot_pos_rel_last_time=12, foot_pos_target_last_time=12, root_euler_d=3, joint_torques=12, root_pos=3, root_lin_vel=3)
f64 = dict(foot_pos_start=12, foot_pos_rel_last_time=12, foot_pos_target_last_time=12, joint_torques=12, root_pos=3, root_lin_vel=3, foot_pos_rel=12, j_foot_blocks=36,
           foot_vel_rel=12, foot_pos_abs=12, foot_vel_abs=12, foot_pos_world=12, foot_vel_world=12, foot_pos_target_rel=12, foot_pos_target_abs=12, foot_pos_target_world=12,
           foot_pos_cur=12, foot_forces_kin=12, foot_pos_recent_contact=12, terrain_angle=1, grf=12,
           R_world=9, R_z=9, root_euler=3, root_ang_vel=3, imu_acc=3, imu_ang_vel=3, root_lin_vel_d=3, root_ang_vel_d=3, root_pos_d_z=1)
d = {k: T(v) for k, v in inp.items()}
d.update({k: torch.zeros((n, m), dtype=torch.float64, device=dev) for k, m in f64.items()})
d["root_pos"][:, 2] = 0.3
d.update({k: torch.zeros((n, 4), dtype=torch.uint8, device=dev) for k in ("estimated_contacts", "plan_contacts", "contacts")})
d.update({k: torch.zeros(n, dtype=torch.uint8, device=dev) for k in ("movement_mode", "mpc_active")})
d.update({k: torch.zeros(n, dtype=torch.int32, device=dev) for k in ("iters", "status")})
bf = E.TickBuffers()
for k in E.TICK_BUFFER_FIELDS:
    setattr(bf, k, d[k].data_ptr())
rd = {k: T(v) for k, v in raw.items()}
cs = {k: T(v) for k, v in pkg.Engine.command_state(n).items()}; cs.pop("root_euler_d")
state = torch.zeros((n, 12), dtype=torch.float64, device=dev); state[:, 5] = 0.3
R = T(np.tile(np.eye(3).reshape(9), (n, 1))); foot = T(np.tile([0.17, 0.15, -0.35, 0.17, -0.15, -0.35, -0.17, 0.15, -0.35, -0.17, -0.15, -0.35], (n, 1)))
fvb, bias = torch.zeros((n, 12), dtype=torch.float64, device=dev), torch.zeros((n, 6), dtype=torch.float64, device=dev)
episode, finished = torch.zeros((n, 16), dtype=torch.float64, device=dev), torch.zeros((n, 16), dtype=torch.float64, device=dev)
life, mask_out = torch.zeros((n, 2), dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
masks = {"nobody": torch.zeros(n, dtype=torch.uint8, device=dev), "one per wavefront": torch.zeros(n, dtype=torch.uint8, device=dev), "everybody": torch.ones(n, dtype=torch.uint8, device=dev)}
masks["one per wavefront"][::64] = 1
plant = [(state, state.clone(), 3), (R, R.clone(), 3), (foot, foot.clone(), 3), (fvb, torch.zeros((1, 12), dtype=torch.float64, device=dev), 3), (d["grf"], d["grf"].clone(), 3),
         (d["contacts"], torch.ones((n, 4), dtype=torch.uint8, device=dev), 3)]
carried = [(d[k], d[k].clone(), 1) for k in CARRIED] + [(cs[k], cs[k].clone(), 1) for k in cs] + [(bias, torch.zeros((1, 6), dtype=torch.float64, device=dev), 1)]
row_bytes = sum(t[0][0].numel() * t[0].element_size() for t in plant + carried)
cfg = pkg.make_config(scen.PARAM_SETS["gazebo"] | scen.MPC_CONSTANTS, H, warm_start=2)
with pkg.Engine(cfg, n, 0) as eng:
    eng.set_timing(False)
    prm = E.TickParams(); eng.lib.a1mpc_default_tick_params(C.byref(prm))
    ts = eng.tick_sensors(sensor=eng.sensor_config(imu_window=WINDOW), **rd, **cs)
    st = torch.cuda.Stream(device=dev); torch.cuda.synchronize()
    s = st.cuda_stream
    tick = lambda: eng.control_tick_sensors_device(prm, ts, bf, n, stream=s)
    rd["mode_toggle"].fill_(1); torch.cuda.synchronize()
    tick(); st.synchronize()                      # the first tick switches every robot to walking; every state block of the handle is allocated from here on
    rd["mode_toggle"].fill_(0); torch.cuda.synchronize()
    for _ in range(8):
        tick()
    st.synchronize()
    ec = eng.episode_config(min_up=-1.0, min_height=-1e9)   # (nobody ends)
    count = [0]

    def update():
        count[0] += 1
        eng.episode_update_device(n, count[0], episode, state, 12, R, d_root_pos=d["root_pos"], d_root_lin_vel=d["root_lin_vel"], d_root_lin_vel_d=d["root_lin_vel_d"],
                                  d_root_pos_d_z=d["root_pos_d_z"], d_grf_body=d["grf"], d_contacts=d["contacts"], d_status=d["status"], config=ec, stream=s)
    nobody = eng.respawn_config(codes=0xE, max_ticks=0)
    decide = lambda: eng.respawn_device(n, episode, life, mask_out, d_finished=finished, config=nobody, stream=s)
    report("decision", timed(dict(episode_update=update, respawn_nobody=decide), st), "episode_update")
    carry = 72 * H + 14
    block_bytes = dict(ekf=343 * 8, contact=384 + (960 + 100) * 8, sensor=6 * (WINDOW + 2) * 8 + 8, warm=(12 * H + 20 * H + 1 + carry) * 8)
    fills = [torch.empty(n * b, dtype=torch.uint8, device=dev) for b in block_bytes.values()]

    def fill():
        with torch.cuda.stream(st):
            for f in fills:
                f.zero_()
    calls = {"fill of the same bytes": fill}
    calls.update({"reset, " + k: (lambda m=m: eng.respawn_reset_device(n, m, 15, stream=s)) for k, m in masks.items()})
    per_robot = sum(block_bytes.values())
    extra = {"reset, " + k: dict(bytes=int(m.sum().item()) * per_robot + n) for k, m in masks.items()}
    extra["fill of the same bytes"] = dict(bytes=n * per_robot)
    report("reset", timed(calls, st, launches=max(launches // 10, 10)), "fill of the same bytes", extra)
    st.synchronize()
    for _ in range(8):   # (every robot's state was cleared: a few ticks bring the handle back to a running loop)
        tick()
    st.synchronize()

    def rows(m):
        eng.respawn_rows_device(n, m, plant, stream=s); eng.respawn_rows_device(n, m, carried, stream=s)
    calls = {"rows, " + k: (lambda m=m: rows(m)) for k, m in masks.items()}
    extra = {"rows, " + k: dict(bytes=2 * int(m.sum().item()) * row_bytes + 2 * n, calls=2, entries=len(plant) + len(carried)) for k, m in masks.items()}
    report("rows (two calls: a table of 6 + 14 entries)", timed(calls, st, launches=max(launches // 4, 10)), "rows, nobody", extra)
    none = masks["nobody"]

    def tick_behind(what):
        eng.respawn_reset_device(n, none, what, stream=s); tick()
    report("ekf init", timed({"tick": tick, "reset (warm, nobody) + tick": lambda: tick_behind(8), "reset (ekf, nobody) + tick: the init kernel runs": lambda: tick_behind(1)}, st,
                             launches=max(launches // 10, 10)), "tick")

    def loop(respawn):
        tick(); update()
        if respawn:
            decide(); rows(mask_out)
    report("tick", timed({"tick + episode_update": lambda: loop(False), "tick + episode_update + respawn + rows": lambda: loop(True)}, st, launches=max(launches // 10, 10)),
           "tick + episode_update")
    print(json.dumps(dict(alive=float((episode[:, 2] == 0).float().mean().item()), respawned=int(life[:, 1].sum().item()), solved=float((d["status"] == 1).float().mean().item()))))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
