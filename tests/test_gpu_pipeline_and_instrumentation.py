"""GPU, through the C ABI: batches in flight (a1mpc_pipeline_*), streams, the sharded handle, the dense-QP formation entry, stage counters, scheduling switches -- bit-identity between the ways through a batch."""
import ctypes as C

import numpy as np
import pytest

from gpu_common import *  # noqa: F401,F403  (_engine, _strided_inputs, tick_inputs, TICK_STATE, _oracle_update_ticks, SETTINGS_CASES)
from gpu_common import _engine, _oracle_update_ticks, _strided_inputs  # noqa: F401
from helpers import TOL_FORCE_BALANCE_N, TOL_FORCE_N, compare, exact_resolver, noise_band, oracle_batch, oracle_params, take  # noqa: F401

pytestmark = pytest.mark.gpu


def test_queue_order_does_not_change_results(pkg, scen):
    """a1mpc_set_schedule: longest-first by the previous solve's cost vs index order -- same QPs, bit-identical results, any order"""
    sc = scen.config3_random_flat(nb=3000)
    cfg = pkg.make_config(sc["params"], 10, warm_start=0)
    args = (sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"])
    with pkg.Engine(cfg, 3000, 0) as eng:
        first = eng.solve(*args)            # no history yet: index order
        again = eng.solve(*args)            # ordered by the first solve's costs
        eng.set_schedule(False)
        plain = eng.solve(*args)
    for k in ("grf", "iters", "status"):
        assert np.array_equal(first[k], again[k]) and np.array_equal(first[k], plain[k]), k


def test_calls_on_different_streams_are_ordered(pkg, scen):
    """two device-pointer solves of one handle issued on two different streams must not overlap on the handle's
    scratch (prepared-state records, queue counter): results equal the same two solves issued on one stream."""
    import torch
    n = 4096
    sc = scen.config3_random_flat(nb=n); sc2 = scen.config3_random_flat(nb=n, seed=77)
    dev = torch.device("cuda:0")
    t = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dt)
    ins = [[t(s["x0"]), t(s["xref"]), t(s["R"]), t(s["foot"]), t(s["contact"], torch.uint8)] for s in (sc, sc2)]
    with _engine(pkg, sc, n, warm_start=0) as eng:
        ref = []
        for k in range(2):
            g = torch.zeros(n, 12, dtype=torch.float64, device=dev)
            eng.solve_device(n, *ins[k], g); torch.cuda.synchronize(); ref.append(g.cpu().numpy())
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        for rep in range(3):
            g1 = torch.zeros(n, 12, dtype=torch.float64, device=dev); g2 = torch.zeros(n, 12, dtype=torch.float64, device=dev)
            eng.solve_device(n, *ins[0], g1, stream=s1.cuda_stream)
            eng.solve_device(n, *ins[1], g2, stream=s2.cuda_stream)
            torch.cuda.synchronize()
            assert np.array_equal(g1.cpu().numpy(), ref[0]) and np.array_equal(g2.cpu().numpy(), ref[1]), rep


@pytest.mark.parametrize("h", [10, 16, 20])
def test_gpu_formed_dense_qp_equals_reference_ConvexMpc(pkg, oracle, scen, h):
    """a1mpc_form_qp_batch (the GPU's implicit Hessian written out entry by entry) vs S/ConvexMpc.cpp compiled verbatim (oracle/_ref), and
    vs the
    oracle: P, g, l, u for broadcast and per-step feet / contacts.  This compares the engine's formation with the REFERENCE directly,
    not through iterates."""
    import ref as REF
    if not REF.build():
        pytest.skip("oracle/_ref not available")
    rng = np.random.default_rng(h)
    nb = 6
    sc, foot, fs, contact, cs = _strided_inputs(scen, rng, h, nb, True, True)
    p = sc["params"]
    pr = oracle.mpc_params(h, p["dt"], p["mu"], p["fz_min"], p["fz_max"], p["q"], p["r"], p["mass"], p["inertia"])
    with _engine(pkg, sc, nb, warm_start=0) as eng:
        bc = eng.form_qp(sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"])
        ps = eng.form_qp(sc["x0"], sc["xref"], sc["R"], foot, sc["contact"], foot_stride=12)
        pc = eng.form_qp(sc["x0"], sc["xref"], sc["R"], foot, contact, foot_stride=12, contact_stride=4)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    for b in range(nb):
        for out, f, fstr in ((bc, sc["foot"][b], 0), (ps, foot[b], 12)):
            r = REF.convex_mpc_form(h, p["q"], p["r"], sc["x0"][b][:3], p["mass"], p["inertia"], sc["R"][b], f, sc["contact"][b],
                    sc["x0"][b], sc["xref"][b], p["dt"],
                                    foot_stride=fstr)
            assert rel(out["P"][b], r["P"]) <= 1e-12 and rel(out["g"][b], r["g"]) <= 1e-10, (b, fstr, rel(out["P"][b], r["P"]),
                    rel(out["g"][b], r["g"]))
            assert np.array_equal(out["l"][b], r["l"]) and np.array_equal(out["u"][b], r["u"])
        P, g, A, l, u, _ = oracle.mpc_form(pr, sc["x0"][b], sc["xref"][b], sc["R"][b], foot[b], contact[b], foot_stride=12,
                contact_stride=4)
        assert rel(pc["P"][b], P) <= 1e-12 and rel(pc["g"][b], g) <= 1e-10 and np.array_equal(pc["l"][b],
                l) and np.array_equal(pc["u"][b], u)


def test_native_sharded_handle_two_shards_on_one_gpu(pkg, scen):
    """a1mpc_sharded_* (SURVEY 8b device = -1, 8e): the batch cut into contiguous shards behind one handle.  The test box has one GPU, so
    the
    pinned-copy transport runs two (three) shards on device 0 -- results must equal the single-handle solve bit for bit, ragged sizes
    included;
    the RCCL transport is created on the one device (communicator set-up, root staging; no peer to talk to)."""
    sc = scen.config3_random_flat(nb=4097)
    cfg = pkg.make_config(sc["params"], 10, warm_start=0)
    with pkg.Engine(cfg, 4097, 0) as eng:
        ref = eng.solve(sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"])
    for devs in ([0, 0], [0, 0, 0]):
        with pkg.ShardedEngine(cfg, 4097, devices=devs, transport=0) as sh:
            assert sh.info()["n_shards"] == len(devs)
            for n in (4097, 5, 1):
                out = sh.solve(sc["x0"][:n], sc["xref"][:n], sc["R"][:n], sc["foot"][:n], sc["contact"][:n])
                assert np.array_equal(out["grf"], ref["grf"][:n]) and np.array_equal(out["iters"],
                        ref["iters"][:n]) and np.array_equal(out["status"], ref["status"][:n]), (devs, n)
    with pkg.ShardedEngine(cfg, 512, devices=None, transport=0) as sh:   # "all visible devices"
        out = sh.solve(sc["x0"][:512], sc["xref"][:512], sc["R"][:512], sc["foot"][:512], sc["contact"][:512])
        assert np.array_equal(out["grf"], ref["grf"][:512])
    with pkg.ShardedEngine(cfg, 512, devices=[0], transport=1) as sh:    # RCCL transport, one rank
        out = sh.solve(sc["x0"][:512], sc["xref"][:512], sc["R"][:512], sc["foot"][:512], sc["contact"][:512])
        assert np.array_equal(out["grf"], ref["grf"][:512]) and sh.info()["transport"] == 1
    with pytest.raises(pkg.A1MpcError):
        pkg.ShardedEngine(cfg, 512, devices=[0, 0], transport=1)       # RCCL needs distinct devices


def test_stage_split_instrumentation(pkg, scen):
    """SURVEY 5 "tracing": form | solve split of the last launch (the reference's t1..t6 stopwatches, S/A1RobotControl.cpp:491-553)"""
    sc = scen.config3_random_flat(nb=8192)
    with _engine(pkg, sc, 8192, warm_start=0) as eng:
        eng.solve(sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"])
        form, solve = eng.last_stage_ms(); total = eng.last_kernel_ms()
        assert form > 0.05 and solve > form and abs(form + solve - total) < 0.05 * total, (form, solve, total)
        eng.solve(sc["x0"][:64], sc["xref"][:64], sc["R"][:64], sc["foot"][:64], sc["contact"][:64])   # fused kernel: not separable
        form, solve = eng.last_stage_ms()
        assert form == 0.0 and solve > 0.0


def test_batch_pipeline_overlaps_batches_and_changes_no_bit(pkg, oracle, scen):
    """a1mpc_pipeline_*: consecutive batches in flight on `depth` handles / HIP streams.  Every batch comes back bit-identical to a lone
    handle's
    solve (and the first one is oracle-checked), slots go round-robin, a fixed slot keeps its warm start, wait / join deliver the outputs,
    and at
    4096 x h10 two batches in flight are faster per batch than one (the next batch runs in the tail of the one before)."""
    import time
    import torch
    n, NB = 4096, 4
    dev = torch.device("cuda:0")
    scs = [scen.config3_random_flat(nb=n, seed=500 + k) for k in range(NB)]
    t = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dt)
    ins = [[t(s["x0"]), t(s["xref"]), t(s["R"]), t(s["foot"]), t(s["contact"], torch.uint8)] for s in scs]
    cfg = pkg.make_config(scs[0]["params"], 10, warm_start=0)
    ref = []
    with pkg.Engine(cfg, n, 0) as eng:
        for k in range(NB):
            g = torch.zeros(n, 12, dtype=torch.float64, device=dev); it = torch.zeros(n, dtype=torch.int32, device=dev)
            eng.set_schedule(True)
            eng.solve_device(n, *ins[k], g, None, it); torch.cuda.synchronize()
            ref.append((g.cpu().numpy(), it.cpu().numpy()))
    o = oracle_batch(oracle, scs[0])
    assert np.abs(ref[0][0] - o["grf"]).max() <= TOL_FORCE_N and (ref[0][1] == o["iters"]).all()

    def run(depth, steps):
        outs = [(torch.zeros(n, 12, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)) for _ in range(NB)]
        with pkg.Pipeline(cfg, n, 0, depth=depth) as pipe:
            assert pipe.depth == depth
            slots = [pipe.submit_device(n, *ins[k % NB], outs[k % NB][0], None, outs[k % NB][1]) for k in range(NB)]
            assert slots == [k % depth for k in range(NB)]
            pipe.wait()
            for k in range(NB):
                assert np.array_equal(outs[k][0].cpu().numpy(), ref[k][0]) and np.array_equal(outs[k][1].cpu().numpy(),
                        ref[k][1]), (depth, k)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for k in range(steps):
                pipe.submit_device(n, *ins[k % NB], outs[k % NB][0], None, outs[k % NB][1])
            pipe.wait()
            ms = (time.perf_counter() - t0) / steps * 1e3
            # join: a caller's stream sees the outputs of a submit that waited for that stream's inputs
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                x0 = ins[1][0].clone()
            g = torch.zeros(n, 12, dtype=torch.float64, device=dev)
            k = pipe.submit_device(n, x0, *ins[1][1:], g, after_stream=s.cuda_stream)
            pipe.join(s.cuda_stream, k)
            with torch.cuda.stream(s):
                gsum = g.clone()
            s.synchronize()
            assert np.array_equal(gsum.cpu().numpy(), ref[1][0])
        return ms
    # Timing: a run's figure depends on WHEN it runs (the part's clocks ramp around every synchronisation: +-20 % between identical runs, profiles/r06_control_tick_timeline.md),
    # so the two depths alternate (1 2 2 1 1 2) and the best of three counts.  Two batches in flight are normally 20-25 % faster per batch at this size (0.61 vs 0.80 ms); the
    # gate only refuses "slower" -- bit-identity above is what this test is about, bench.py reports the rates
    tms = {1: [], 2: []}
    for depth in (1, 2, 2, 1, 1, 2):
        tms[depth].append(run(depth, 32))
    ms1, ms2 = min(tms[1]), min(tms[2])
    print(f"4096 x h10 first solves: {ms1:.3f} ms per batch alone, {ms2:.3f} ms with two in flight ({tms})")
    assert ms2 < 1.02 * ms1, (ms1, ms2, tms)

    # a warm-started population stays on its slot: slot 1 alone carries its own OSQP workspace from tick to tick
    sc = scen.config3_random_flat(nb=256, seed=9)
    cfgw = pkg.make_config(sc["params"], 10, warm_start=1)
    a = [t(sc["x0"]), t(sc["xref"]), t(sc["R"]), t(sc["foot"]), t(sc["contact"], torch.uint8)]
    with pkg.Engine(cfgw, 256, 0) as eng, pkg.Pipeline(cfgw, 256, 0, depth=2) as pipe:
        for tick in range(3):
            g0 = torch.zeros(256, 12, dtype=torch.float64, device=dev); i0 = torch.zeros(256, dtype=torch.int32, device=dev)
            g1 = torch.zeros(256, 12, dtype=torch.float64, device=dev); i1 = torch.zeros(256, dtype=torch.int32, device=dev)
            eng.solve_device(256, *a, g0, None, i0)
            assert pipe.submit_device(256, *a, g1, None, i1, slot=1, fresh=False) == 1
            pipe.wait(1); torch.cuda.synchronize()
            assert np.array_equal(g0.cpu().numpy(), g1.cpu().numpy()) and np.array_equal(i0.cpu().numpy(), i1.cpu().numpy()), tick
        assert i1.float().mean().item() < 40   # warm: 25 iterations for nearly every QP


def test_batch_pipeline_argument_errors(pkg, scen):
    import ctypes as C
    sc = scen.config3_random_flat(nb=8)
    cfg = pkg.make_config(sc["params"], 10, warm_start=0)
    lib = pkg.load_library()
    p = C.c_void_p()
    assert lib.a1mpc_pipeline_create(C.byref(cfg), 8, 0, 9, C.byref(p)) != 0 and not p          # depth > 8
    assert lib.a1mpc_pipeline_create(C.byref(cfg), 0, 0, 2, C.byref(p)) != 0
    bad = pkg.make_config(sc["params"], 7)
    assert lib.a1mpc_pipeline_create(C.byref(bad), 8, 0, 2, C.byref(p)) != 0 and not p          # unsupported horizon, nothing leaked
    with pkg.Pipeline(cfg, 8, 0, depth=0) as pipe:
        assert pipe.depth == 2   # default: two batches in flight at every size
        with pkg.Pipeline(cfg, 4096, 0, depth=0) as big:
            assert big.depth == 2
        with pytest.raises(pkg.A1MpcError):
            pipe.submit_device(8, None, None, None, None, None, None)
        with pytest.raises(pkg.A1MpcError):
            pipe.wait(5)
        pipe.wait()   # nothing submitted yet: returns at once
        assert lib.a1mpc_pipeline_wait(None, -1) != 0
    lib.a1mpc_pipeline_destroy(None)


def test_host_pointer_pipeline_matches_the_synchronous_entry(pkg, scen):
    """a1mpc_pipeline_submit / _wait: host arrays in, host arrays out (the reference's side of the boundary, S/A1RobotControl.h:44), two or
    three batches in flight.
    The inputs are snapshotted before submit returns (they are overwritten right behind it here); every batch comes back bit-identical to
    a1mpc_solve_batch,
    u_full / iters / status included; a slot that is resubmitted first delivers its previous batch; n = 0 and ragged sizes work."""
    n, NB = 3000, 5   # beyond the resident rows: the split pipeline
    scs = [scen.config3_random_flat(nb=n, seed=800 + k) for k in range(NB)]
    cfg = pkg.make_config(scs[0]["params"], 10, warm_start=0)
    ref = []
    with pkg.Engine(cfg, n, 0) as eng:
        for s in scs:
            eng.set_schedule(True)
            ref.append(eng.solve(s["x0"], s["xref"], s["R"], s["foot"], s["contact"], want_u=True))
    for depth in (2, 3):
        with pkg.Pipeline(cfg, n, 0, depth=depth) as pipe:
            outs = [dict(grf=np.full((n, 12), np.nan), u=np.full((n, 120), np.nan), iters=np.full(n, -1, np.int32),
                    status=np.full(n, -99, np.int32)) for _ in range(NB)]
            for k, s in enumerate(scs):
                ins = [np.array(s[f]) for f in ("x0", "xref", "R", "foot", "contact")]
                slot = pipe.submit(*ins, outs[k], fresh=True)   # round-robin: a slot that still holds batch k - depth delivers it first
                assert slot == k % depth
                for a in ins:
                    a[...] = 0            # the caller's arrays are free again as soon as submit returns
                if k >= depth:            # batch k - depth was delivered by this submit
                    j = k - depth
                    assert np.array_equal(outs[j]["grf"], ref[j]["grf"]) and np.array_equal(outs[j]["iters"], ref[j]["iters"]), (depth, j)
            pipe.wait()
            for k in range(NB):
                assert np.array_equal(outs[k]["grf"], ref[k]["grf"]) and np.array_equal(outs[k]["u"], ref[k]["u"]), (depth, k)
                assert np.array_equal(outs[k]["iters"], ref[k]["iters"]) and np.array_equal(outs[k]["status"], ref[k]["status"]), (depth, k)
            # ragged: fewer QPs than max_batch, outputs optional, and an empty batch
            m = 37
            o = dict(grf=np.zeros((m, 12)))
            pipe.submit(scs[1]["x0"][:m], scs[1]["xref"][:m], scs[1]["R"][:m], scs[1]["foot"][:m], scs[1]["contact"][:m], o, slot=0)
            pipe.wait(0)
            with pkg.Engine(cfg, m, 0) as small:
                r = small.solve(scs[1]["x0"][:m], scs[1]["xref"][:m], scs[1]["R"][:m], scs[1]["foot"][:m], scs[1]["contact"][:m])
            assert np.array_equal(o["grf"], r["grf"])
            # m <= A1MPC_ZERO_COPY_MAX: the kernel writes the in-flight slot's pinned mirror itself, pipeline_wait delivers it
            m = 5
            o = dict(grf=np.zeros((m, 12)), u=np.zeros((m, 120)), iters=np.full(m, -1, np.int32), status=np.full(m, -99, np.int32))
            pipe.submit(scs[2]["x0"][:m], scs[2]["xref"][:m], scs[2]["R"][:m], scs[2]["foot"][:m], scs[2]["contact"][:m], o, slot=1)
            pipe.wait(1)
            with pkg.Engine(cfg, m, 0) as small:
                r = small.solve(scs[2]["x0"][:m], scs[2]["xref"][:m], scs[2]["R"][:m], scs[2]["foot"][:m], scs[2]["contact"][:m], want_u=True)
            assert np.array_equal(o["grf"], r["grf"]) and np.array_equal(o["u"], r["u"]), depth
            assert np.array_equal(o["iters"], r["iters"]) and np.array_equal(o["status"], r["status"]), depth
            e = dict(grf=np.zeros((0, 12)))
            pipe.submit(scs[1]["x0"][:0], scs[1]["xref"][:0], scs[1]["R"][:0], scs[1]["foot"][:0], scs[1]["contact"][:0], e, slot=1)
            pipe.wait()
            with pytest.raises(pkg.A1MpcError):
                pipe.submit(np.zeros((n + 1, 13)), np.zeros((n + 1, 130)), np.zeros((n + 1, 9)), np.zeros((n + 1, 12)),
                        np.zeros((n + 1, 4), np.uint8), dict(grf=np.zeros((n + 1, 12))))


@pytest.mark.parametrize("gen,n", [("config3_random_flat", 4096), ("config4_random_h16", 2560), ("config5_divergent", 2048)])
def test_stage_cycles_through_the_abi(pkg, scen, gen, n):
    """VERDICT r3 item 9 / SURVEY 5 (the reference's t1..t6 stopwatches, S/A1RobotControl.cpp:491-553): a1mpc_set_profiling runs the
    clock-stamped instantiation of the
    persistent ADMM kernel -- bit-identical results -- and a1mpc_last_stage_cycles splits the solve stage into factor passes | iterations |
    residual checks."""
    sc = getattr(scen, gen)(nb=n)
    with _engine(pkg, sc, n, warm_start=0) as eng:
        a = eng.solve(sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"], want_u=True)
        assert eng.last_stage_cycles()["qps"] == 0          # not profiled
        eng.set_profiling(True)
        b = eng.solve(sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"], want_u=True)
        cyc = eng.last_stage_cycles(); nf = eng.last_nfact(n)
        eng.set_profiling(False)
        c = eng.solve(sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"], want_u=True)
        assert eng.last_stage_cycles()["qps"] == 0
    for k in ("grf", "u", "iters", "status"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    assert cyc["qps"] == n and min(cyc["factor"], cyc["iterate"], cyc["check"]) > 0
    tot = cyc["factor"] + cyc["iterate"] + cyc["check"]
    per_it = cyc["iterate"] / float(a["iters"].sum()); per_f = cyc["factor"] / float(nf.sum())
    print(f"{gen} x {n}: factor {cyc['factor'] / tot:.3f} | iterate {cyc['iterate'] / tot:.3f} | "
          f"check {cyc['check'] / tot:.3f} of the solve stage; "
          f"{per_it:.0f} cycles per iteration, {per_f:.0f} per factor pass (wave-mates' stalls included)")
    assert 0.5 < cyc["iterate"] / tot < 0.95 and 0.03 < cyc["factor"] / tot < 0.45


@pytest.mark.parametrize("n,mode", [(4096, 1), (4096, 2), (1, 1), (1, 2), (200, 2)])
def test_tick_stage_cycles_of_the_fused_and_latency_kernels(pkg, scen, n, mode):
    """a1mpc_set_profiling + a1mpc_last_tick_stage_cycles on the ticks the reference actually runs -- warm-started ticks through the fused kernel
    (4096 robots) and the latency kernel (1 and 200 robots), both warm-start semantics: the clock-stamped instantiation gives the same bits as the plain one, every
    stage is filled, the stages add up to the whole tick, and a tick that is not profiled (or runs the split pipeline) reports qps = 0."""
    sc = scen.config3_random_flat(nb=max(n, 8))
    take_n = lambda k: sc[k][:n]
    rng = np.random.default_rng(31 + n)
    with _engine(pkg, sc, n, warm_start=mode) as eng:
        outs = []
        for t in range(5):
            x0 = take_n("x0").copy(); x0[:, :12] += rng.normal(0, 0.002, (n, 12)) * (t > 0)
            prof = t == 3
            eng.set_profiling(prof)
            o = eng.solve(x0, take_n("xref"), take_n("R"), take_n("foot"), take_n("contact"), want_u=True)
            cyc = eng.last_tick_stage_cycles()
            if prof:
                assert cyc["qps"] == n, cyc
                parts = sum(cyc[k] for k in eng.TICK_STAGES[:-1])
                assert all(cyc[k] > 0 for k in eng.TICK_STAGES) and abs(parts - cyc["total"]) <= 1e-9 * cyc["total"], cyc
                assert 0.15 < cyc["iterate"] / cyc["total"] < 0.8 and 0.1 < cyc["ruiz"] / cyc["total"] < 0.5, cyc
                print(f"{n} robots, mode {mode}:", {k: round(cyc[k] / cyc["total"], 3) for k in eng.TICK_STAGES[:-1]}, "cycles per QP", round(cyc["total"] / n))
            else:
                assert cyc["qps"] == 0, (t, cyc)     # tick 0 of 4096 robots runs the split pipeline (its stage record is a1mpc_last_stage_cycles'), the others are not profiled
            outs.append(o)
    # the same five ticks without ever touching the profiler: bit for bit
    rng = np.random.default_rng(31 + n)
    with _engine(pkg, sc, n, warm_start=mode) as eng:
        for t in range(5):
            x0 = take_n("x0").copy(); x0[:, :12] += rng.normal(0, 0.002, (n, 12)) * (t > 0)
            o = eng.solve(x0, take_n("xref"), take_n("R"), take_n("foot"), take_n("contact"), want_u=True)
            for k in ("grf", "u", "iters", "status"):
                assert np.array_equal(o[k], outs[t][k]), (t, k)


@pytest.mark.parametrize("var,n,ticks,warm,values", [("A1MPC_FUSED_QUEUE", 4096, 2, 0, "0,1"), ("A1MPC_WARM_ORDER", 4096, 4, 1, "0,1"), ("A1MPC_WARM_ORDER", 4096, 4, 2, "0,1"),
                                                    ("A1MPC_ZERO_COPY_MAX", 1, 4, 2, "0,8"), ("A1MPC_ZERO_COPY_MAX", 8, 3, 1, "0,8"), ("A1MPC_ZERO_COPY_MAX", 8, 2, 0, "0,8")])
def test_opt_in_scheduling_switches_change_nothing_but_the_schedule(pkg, var, n, ticks, warm, values):
    """Round 5's two measured-and-not-adopted trials stay in the library behind environment switches: A1MPC_FUSED_QUEUE=1 (the fused kernel as persistent wavefronts on
    the work queue, profiles/r05_fused_queue_trial.txt) and A1MPC_WARM_ORDER=1 (warm ticks launched in the order of the previous tick's costs,
    profiles/r05_warm_tick_order.txt).  Both only reorder independent QPs: forces, full solutions, iteration counts and statuses of every tick are bit-identical
    with the switch on and off (children of tools/env_ab.py).  Round 6: the same for the small-batch host path -- A1MPC_ZERO_COPY_MAX = 0 (inputs / outputs
    staged through device memory) against the default 8 (the kernels read and write the handle's pinned block over PCIe): batch 1 and batch 8, full solutions included,
    cold and both warm-start semantics; the batch-1 latency figures of bench.py and tests/cpp/latency_harness.cpp are measured on the zero-copy path."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "env_ab.py"), var, str(n), str(ticks), str(warm), values], capture_output=True, text=True, timeout=600)
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 2 and all("digest" in x for x in rows), (r.stdout[-500:], r.stderr[-500:])
    assert rows[0]["digest"] == rows[1]["digest"] and rows[0]["solved"] == 1.0, rows
    print(var, [x["kernel_ms"] for x in rows])


def test_timing_events_can_be_turned_off(pkg, scen):
    """a1mpc_set_timing(h, 0): no HIP timing events around the launches (a 400 Hz loop does not read them) -- the same results, and the calls that read the events say so"""
    sc = scen.config3_random_flat(nb=64)
    with _engine(pkg, sc, 64, warm_start=0) as eng:
        a = eng.solve(sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"])
        assert eng.last_kernel_ms() > 0
        eng.set_timing(False)
        b = eng.solve(sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"])
        with pytest.raises(pkg.A1MpcError):
            eng.last_kernel_ms()
        eng.set_timing(True)
        c = eng.solve(sc["x0"], sc["xref"], sc["R"], sc["foot"], sc["contact"])
        assert eng.last_kernel_ms() > 0
    assert np.array_equal(a["grf"], b["grf"]) and np.array_equal(a["grf"], c["grf"]) and np.array_equal(a["iters"], b["iters"])


@pytest.mark.parametrize("h,n", [(20, 2100), (16, 2600)])
def test_quad_of_rows_kernels_leave_the_twin_pairs_bits(pkg, h, n):
    """h = 20 (one QP per wavefront) and waves 1-3 of the CU-wide kernel at h = 16 run the four rows of a wavefront as a QUAD on one QP
    (RowSolver<.., QUAD>): the per-lane state
    split four ways, the chains untouched.  Against the twin-pair kernels of the same library (A1MPC_QUAD=0 in a child process): forces,
    the full solution, iteration counts and
    statuses of first solves, solves in history order and three warm-started ticks -- the same bits."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "ab_quad.py"), pkg.build.LIB_PATH, str(h), str(n), "1"],
            capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["bit_identical"] is True, r.stdout[-800:]


# (QPs, threads, dynamic LDS bytes) per workgroup of the persistent ADMM kernel.  The LDS byte counts are what a1mpc_kernel_info of the library returned on an MI355X at
# the commit before the launch layer took these numbers from the launch code's own geometry (they equal 8 x QPs x Layout<H>::ROW_STRIDE).
KERNEL_INFO = {1: (2, 32, 5280), 10: (2, 64, 40704), 12: (2, 64, 48576), 16: (5, 256, 160880), 20: (1, 64, 40064)}
KERNEL_INFO_H16_ONE_WAVE = (1, 64, 32176)   # A1MPC_CU_WIDE=0: the one-wave kernel, one QP (a main / twin pair of rows) per wavefront


def test_kernel_info_matches_the_launched_geometry(pkg, scen):
    """a1mpc_kernel_info reports the geometry the split pipeline's persistent kernel is launched with (one source: admm_geometry, csrc/a1mpc_common.hpp): every kernel
    layout there is -- h = 1 (no twin rows), two QPs per wavefront, the CU-wide workgroup of h = 16, one QP per wavefront -- and, in a child process, h = 16 without the
    CU-wide kernel.  No solve is needed."""
    import json, os, subprocess, sys
    def info(horizon):
        sc = scen.config3_random_flat(nb=8, horizon=horizon)
        with _engine(pkg, sc, 8) as eng:
            k = eng.kernel_info()
        return (k["qps_per_workgroup"], k["threads_per_workgroup"], k["lds_bytes_per_workgroup"])
    for horizon, want in KERNEL_INFO.items():
        assert info(horizon) == want, horizon
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = ("import json, sys; sys.path.insert(0, sys.argv[1]); import __graft_entry__ as g; pkg = g.load_package(); sc = pkg.scenarios.config3_random_flat(nb=8, horizon=16)\n"
             "with pkg.Engine(pkg.make_config(sc['params'], 16), max_batch=8, device=0) as eng: print(json.dumps(eng.kernel_info()))")
    r = subprocess.run([sys.executable, "-c", child, root], capture_output=True, text=True, timeout=300, env=dict(os.environ, A1MPC_CU_WIDE="0"))
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-500:]
    k = json.loads(r.stdout.strip().splitlines()[-1])
    assert (k["qps_per_workgroup"], k["threads_per_workgroup"], k["lds_bytes_per_workgroup"]) == KERNEL_INFO_H16_ONE_WAVE
