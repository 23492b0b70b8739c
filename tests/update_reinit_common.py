"""Shared by tests/test_gpu_update_reinit.py and tests/test_update_reinit_host.py: robot fleets whose Hessian pattern changes on a planned timetable.

warm_start = 2 re-initialises the solver when the zero pattern of the reference's dense Hessian changes between two ticks (RowSolver::setup, "pattern change";
oracle/a1mpc_oracle.c `reinit`).  The fleets here change it the way a robot can: a coordinate of one foot is set to exactly 0.0, which removes entries of the omega
rows of B~ and with them entries of B_qp' Q B_qp.  Which leg and axis is zero on which tick is a timetable per robot CLASS (index % 4, so every pair, quad and
workgroup of rows holds robots of every class on the same tick):

    class 0   never changes (every other one of them is rolled / pitched / yawed: a dense inverse inertia, no exact zeros at all)
    class 1   changes on tick 2 (general path: the zero holds from horizon step LATE_STEP on only, so the per-step flags differ)
    class 2   changes on ticks 2 and 4 -- the second change MOVES the zero from one leg to another: the same number of zeros, another pattern
    class 3   changes on every tick from 2 on, through a cycle of four distinct patterns that then repeats

The PLAN (which robot re-initialises on which tick) follows from the timetable alone: a tick re-initialises exactly when the robot's zero set differs from the tick
before.  The tests assert that the oracle's info.reinit equals the plan before they look at a kernel's output."""
import numpy as np

LATE_STEP = 3
# zero sets: tuples of (leg, axis)
NONE = ()
CYCLE = (((3, 2),), ((1, 0),), ((3, 1),), ((0, 2),))


def zero_set(cls, t):
    """the (leg, axis) pairs that are exactly 0.0 for a robot of class `cls` on tick t"""
    if cls == 0 or t < 2:
        return NONE
    if cls == 1:
        return ((2, 1),)
    if cls == 2:
        return ((0, 1),) if t < 4 else ((1, 1),)
    return CYCLE[(t - 2) % 4]


def plan(classes, ticks, zero_of=zero_set):
    """plan[t][b]: robot b re-initialises on tick t"""
    return np.array([[t > 0 and zero_of(c, t) != zero_of(c, t - 1) for c in classes] for t in range(ticks)], dtype=bool)


def followed(n, classes, most=64):
    """the robots chained through the oracle: the first 16, the last 16 and an even sample of the rest that covers all four classes -- at most `most`"""
    if n <= most:
        return np.arange(n)
    k = most - 32
    mid = np.linspace(16, n - 17, k).astype(int)
    mid = np.clip(mid - mid % 4 + np.arange(k) % 4, 16, n - 17)
    idx = np.unique(np.concatenate([np.arange(16), mid, np.arange(n - 16, n)]))
    assert len(idx) <= most and set(np.asarray(classes)[idx]) == {0, 1, 2, 3}
    return idx


class Fleet:
    """n robots at horizon h with constants `params` (a scenarios.PARAM_SETS entry + MPC_CONSTANTS): inputs of tick t from tick(t, general)"""

    def __init__(self, scen, params, n, h, seed, class_offset=0, zero_of=zero_set, late=True):
        rng = np.random.default_rng(seed)
        self.scen, self.p, self.n, self.h, self.zero_of, self.late = scen, params, n, h, zero_of, late
        self.classes = (np.arange(n) + class_offset) % 4
        self.tilted = (self.classes == 0) & ((np.arange(n) // 4) % 2 == 1)
        eul = np.zeros((n, 3))
        eul[self.tilted] = rng.uniform(-0.15, 0.15, (int(self.tilted.sum()), 3))
        self.euler = eul
        self.R = scen.rot_zyx(eul[:, 0], eul[:, 1], eul[:, 2])
        self.pos = np.c_[rng.normal(0, 1.0, (n, 2)), rng.uniform(0.26, 0.31, n)]
        self.ang_vel = rng.normal(0, 0.2, (n, 3)); self.lin_vel = rng.normal(0, 0.2, (n, 3))
        self.vd = np.c_[rng.uniform(-0.5, 0.5, n), rng.uniform(-0.2, 0.2, n), np.zeros(n)]
        self.foot_body = np.array(params["foot"], dtype=float)[None] + rng.uniform(-0.03, 0.03, (n, 4, 3))
        self.vx = rng.uniform(0.2, 0.6, n) * rng.choice([-1.0, 1.0], n)      # the general path's per-step drift of the feet: in x only, so a zero y or z holds over the horizon
        # all feet down: with swing legs (rows held at 0, rho 1e3 times larger) every re-initialised solve amplifies rounding differences ~30x, and after five in a row
        # the ORACLE's own two linear-system back ends are 1e-6 N apart -- no yardstick for a kernel
        self.contact = np.ones((n, 4), np.uint8)

    def tick(self, t, general=False):
        """inputs of tick t: dict(x0, xref, R, foot, contact, foot_stride); the state moves a little from tick to tick"""
        n, h, p = self.n, self.h, self.p
        rng = np.random.default_rng(1000 * t + 17)
        pos = self.pos + np.c_[np.zeros((n, 2)), 1e-3 * t * np.ones(n)]
        w = self.ang_vel + rng.normal(0, 2e-3, (n, 3)); v = self.lin_vel + rng.normal(0, 2e-3, (n, 3))
        x0 = self.scen.pack_x0(self.euler, pos, w, v)
        xref = self.scen.build_reference(h, p["dt"], self.euler, pos, self.R, np.zeros((n, 3)), self.vd, np.zeros((n, 3)), np.full(n, 0.3))
        foot = np.einsum("bij,blj->bli", self.R, self.foot_body + 1e-3 * t)           # (n, 4, 3)
        if general:
            steps = np.arange(h).reshape(1, h, 1, 1)
            drift = np.zeros((n, 1, 1, 3)); drift[:, 0, 0, 0] = self.vx
            foot = foot[:, None] - drift * p["dt"] * 40.0 * steps                        # (n, h, 4, 3)
        else:
            foot = foot[:, None].copy()                                                  # (n, 1, 4, 3)
        for b in range(n):
            first = LATE_STEP if (general and self.late and self.classes[b] == 1) else 0
            for leg, ax in self.zero_of(int(self.classes[b]), t):
                foot[b, first:, leg, ax] = 0.0
        foot = np.ascontiguousarray(foot.reshape(n, -1))
        return dict(x0=x0, xref=xref, R=np.ascontiguousarray(self.R.reshape(n, 9)), foot=foot, contact=self.contact, foot_stride=12 if general else 0)

    def plan(self, ticks):
        return plan(self.classes, ticks, self.zero_of)


def oracle_tick(oracle, pr, st, q, b, carry):
    """robot b of the tick inputs q on the oracle's update path"""
    return oracle.mpc_solve_update(pr, st, q["x0"][b], q["xref"][b], q["R"][b], q["foot"][b], q["contact"][b], carry, foot_stride=q["foot_stride"])


def hardware(scen):
    """the main constant set of these tests: on it the oracle's two linear-system back ends stay within 1e-9 N of each other through every sequence here
    (tests/test_update_reinit_host.py asserts it), so a distance to the oracle measures the kernel"""
    return dict(scen.PARAM_SETS["hardware"], **scen.MPC_CONSTANTS)


# path switches: F = the fast path (step-invariant feet), G = the general path (per-step feet).  Switches F->G at ticks 2 and 6, G->F at ticks 4 and 7.
SWITCH_PATHS = "FFGGFFGF"


def switch_sets(cls, t):
    """class 1: changes WITH the F->G switch (2) and on the tick after a G->F switch (5); class 2: on the tick after an F->G switch (3), WITH the G->F switch (4) and
    WITH the second F->G switch (6); class 0 never (every switch without a change), class 3 on every tick from 2 on"""
    if cls == 0 or t < 2:
        return NONE
    if cls == 1:
        return ((2, 1),) if t < 5 else ((0, 0),)
    if cls == 2:
        return NONE if t < 3 else (((1, 2),) if t == 3 else (((3, 1),) if t < 6 else ((1, 0),)))
    return CYCLE[(t - 2) % 4]


def unweighted(scen):
    """the `hardware` constants with roll, pitch and their rates unweighted: a foot's z coordinate then reaches no stored entry of the Hessian"""
    p = dict(scen.PARAM_SETS["hardware"], **scen.MPC_CONSTANTS)
    p["q"] = [0, 0, 1, 0, 0, 50, 0, 0, 1, 1, 1, 1, 0]
    return p


def zero_weight_sets(cls, t):
    """timetable of the zero-weight cases: classes 1 and 3 toggle a foot's z (under the unweighted set no stored entry changes), class 2 a foot's y.  Two changes per
    robot, no more: on the ill-conditioned `test_mpc` constants (r = 1e-6) every further re-initialised solve takes the oracle's own back ends 30x further apart"""
    if cls == 0 or t < 2:
        return NONE
    if cls == 1:
        return ((1, 2),) if t == 2 else NONE
    if cls == 2:
        return ((2, 1),) if t in (2, 3) else NONE
    return NONE if t < 3 else (((0, 2),) if t < 5 else ((3, 2),))


def weighted_part(cls, t):
    """what the unweighted set sees of zero_weight_sets: the zeros that are no z coordinate"""
    return tuple(z for z in zero_weight_sets(cls, t) if z[1] != 2)


def constants(scen, weights):
    return hardware(scen) if weights == "hardware" else (unweighted(scen) if weights == "unweighted" else dict(scen.PARAM_SETS["test_mpc"], **scen.MPC_CONSTANTS))


class Seq:
    """one sequence of tests/test_gpu_update_reinit.py: a fleet, the path of every tick ('F' fast / 'G' general) and the plan of its re-initialisations.  staged: the warm
    ticks have a set-up stage of their own (True: the split pipeline / False), or a tuple with the expectation of every tick, the first included"""

    def __init__(self, name, n, h, paths, seed, weights="hardware", off=0, zero_of=zero_set, plan_of=None, late=True, staged=None, settings=None):
        self.name, self.n, self.h, self.paths, self.seed, self.weights, self.off = name, n, h, paths, seed, weights, off
        self.zero_of, self.plan_of, self.late, self.staged, self.settings = zero_of, plan_of or zero_of, late, staged, settings or {}

    def fleet(self, scen):
        return Fleet(scen, constants(scen, self.weights), self.n, self.h, self.seed, class_offset=self.off, zero_of=self.zero_of, late=self.late)

    def plan(self, classes):
        return plan(classes, len(self.paths), self.plan_of)


def _family(name, general, n, h, ticks, staged, off=0):
    return Seq(name, n, h, ("G" if general else "F") * ticks, 8100 + n + h, off=off, staged=staged)


# the kernel families, reached by batch size (n = 3 holds three classes at a time: it runs with the classes rotated once more)
FAMILIES = [_family("fast-latency", False, 3, 10, 7, False), _family("fast-latency+1", False, 3, 10, 7, False, off=1), _family("fast-fused-pairs", False, 301, 10, 7, False),
            _family("fast-fused-quads-h16", False, 301, 16, 6, False), _family("fast-split-h10", False, 8300, 10, 6, True), _family("fast-cu-wide-h16", False, 1300, 16, 6, True),
            _family("fast-quads-h20", False, 1100, 20, 6, (True,) + (False,) * 5), _family("fast-extended-h6", False, 301, 6, 7, False),
            _family("general-latency", True, 3, 10, 7, False), _family("general-latency+1", True, 3, 10, 7, False, off=1), _family("general-fused-pairs", True, 301, 10, 7, False),
            _family("general-quads-h16-n5", True, 5, 16, 6, False), _family("general-quads-h16", True, 301, 16, 6, False), _family("general-rounds-h10", True, 4001, 10, 6, False)]
SWITCHES = [Seq(f"switches-h{h}-n{n}-class+{off}", n, h, SWITCH_PATHS, 8200 + n + h, off=off, zero_of=switch_sets, late=False)
            for h, n, off in ((10, 1, 1), (10, 1, 2), (10, 1, 3), (10, 41, 0), (16, 5, 0))]
ZERO_WEIGHTS = [Seq(f"{w}-{path}", 41, 10, path * 6, 8300, weights=w, zero_of=zero_weight_sets, plan_of=weighted_part if w == "unweighted" else None, late=False)
                for w in ("unweighted", "test_mpc") for path in "FG"]
SETTINGS = [Seq("settings-" + ",".join(f"{k}={v}" for k, v in over.items()) + "-" + path, 41, 10, path * 6, 8700, settings=over)
            for over in (dict(rho=1.0), dict(rho=0.01, adaptive_rho=0), dict(scaling=0)) for path in "FG"]
# the fleets of the interplay tests (a failed tick, an injected warm start, a reset, two pipeline slots, both paths on one sequence)
INTERPLAY = {k: Seq(k, n, 10, "F" * 6, seed, off=off) for k, n, seed, off in (("failed", 41, 8400, 0), ("injected", 24, 8500, 0), ("reset", 41, 8600, 0), ("slot0", 41, 8800, 0),
                                                                              ("slot1", 41, 8801, 1), ("both-paths", 41, 8900, 0))}
ALL_SEQUENCES = FAMILIES + SWITCHES + ZERO_WEIGHTS + SETTINGS + list(INTERPLAY.values())
