"""Episode record and batch summary on the CPU: the product's kernel text compiled for the host (tests/emu/episode_host.py: 64 host threads in lock step are one
wavefront) against the numpy restatement of tests/episode_ref.py, bit for bit -- neither kernel calls a library function, so there is no bar anywhere in this file --
and what must hold structurally: a robot alone, a split batch, frozen records, each way an episode ends, the tie of the summary's row, and the rows nobody may read."""
import numpy as np
import pytest

import episode_host as host
import episode_ref as ER

SIZES = (1, 15, 16, 17, 65)
STRIDES = (12, 13, 22)
TICKS = 30
SUMMARY_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097)
POISON = 0x7FF8DEADBEEF0001
_SHARED = {}


def _inputs(stride=12):
    """30 ticks of inputs for 68 robots (65 and a tail of three), per stride: computed once, never changed"""
    if stride not in _SHARED:
        _SHARED[stride] = ER.random_inputs(max(SIZES) + 3, seed=9100 + stride, stride=stride, ticks=TICKS)
    return _SHARED[stride]


def _records(n=130, ticks=6):
    """130 records after six accumulated ticks (all alive), the starting point of the structural checks"""
    key = ("rec", n, ticks)
    if key not in _SHARED:
        ep = np.zeros((n, ER.WORDS))
        for t, d in enumerate(ER.random_inputs(n, seed=9300, ticks=ticks)):
            ep = ER.update(ep, t, **d)
        assert (ep[:, 0] == ticks).all() and (ep[:, 2] == 0).all()
        ep.setflags(write=False)
        _SHARED[key] = ep
    return _SHARED[key]


def _rows(d, sl):
    return {k: (None if v is None else v[sl]) for k, v in d.items()}


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("n", SIZES)
def test_update_on_the_host_is_the_restatement(n, stride):
    """a lone robot, either side of a wavefront edge, several workgroups with a partly filled last one; the three state strides; 30 consecutive ticks on random finite
    inputs from the all-zero record, every input given: every word of every record after every tick, and the three rows beyond n keep their poison"""
    ins = _inputs(stride)
    ref = np.zeros((n, ER.WORDS))
    out = np.zeros((n + 3, ER.WORDS)); out[n:].view(np.uint64)[:] = POISON
    for t, d in enumerate(ins):
        ref = ER.update(ref, 1000 + t, **_rows(d, slice(0, n)))
        out = host.update(out, 1000 + t, n=n, **d)
        assert ER.bits_equal(out[:n], ref), (t, np.argwhere(out[:n].view(np.uint64) != ref.view(np.uint64))[:4])
        assert (out[n:].view(np.uint64) == POISON).all(), t
    assert (ref[:, 0] == TICKS).all() and (ref[:, 3:13] > 0).any(0).all() and (ref[:, 15] > 0).all()   # (the inputs do reach every word)


@pytest.mark.parametrize("key", ER.OPTIONAL)
def test_a_null_input_leaves_its_words_alone(key):
    """each optional input NULL in turn, on records whose every word of that input holds a NaN payload: those words keep the payload, every other word is the
    restatement's, and (the ground aside) equals the all-inputs run"""
    n = 17
    d = _rows(_inputs()[0], slice(0, n))
    start = np.array(_records()[:n])
    start.view(np.uint64)[:, list(ER.WORDS_OF[key])] = POISON
    less = ER.without(d, key)
    out = host.update(start, 6, **less)
    assert ER.bits_equal(out, ER.update(start, 6, **less))
    full = host.update(_records()[:n], 6, **d)   # (from the records without the payload: a NaN would pass through the sums)
    words = list(ER.WORDS_OF[key])
    assert (out[:, words].view(np.uint64) == POISON).all()
    rest = [k for k in range(ER.WORDS) if k not in words and not (key == "ground" and k == 4)]
    assert ER.bits_equal(out[:, rest], full[:, rest]) and (out[:, 0] == 7).all()
    if words:
        assert not (full[:, words].view(np.uint64) == POISON).any()


@pytest.mark.parametrize("n", SUMMARY_SIZES)
def test_summary_on_the_host_is_the_restatement(n):
    """one row, a pair, either side of one and of two wavefronts, either side of 64 wavefronts (one, two and three launch levels): all 20 words, with row n poisoned"""
    ep = np.vstack([ER.random_records(n, seed=9200 + n), np.full((1, ER.WORDS), np.nan)])
    out, launches = host.summary(ep, n)
    ref = ER.summary(ep[:n])
    assert ER.bits_equal(out, ref), (out, ref)
    assert launches == (1 if n <= 64 else (2 if n <= 4096 else 3))
    assert out[0] == n and out[1:5].sum() == n and (out[5] >= 0) == (out[1] < n)


def test_a_robot_alone_and_a_split_batch():
    """robot g alone (n = 1) gives its row of the batch of 130; the batch split at 100 gives the whole; the summary of the 130 does not depend on how the records were made"""
    n = 130
    d = ER.random_inputs(n, seed=9400)[0]
    start = _records(n)
    whole = host.update(start, 6, **d)
    assert ER.bits_equal(whole, ER.update(start, 6, **d))
    for g in (0, 15, 16, 63, 64, 129):
        one = host.update(start[g:g + 1], 6, **_rows(d, slice(g, g + 1)))
        assert ER.bits_equal(one, whole[g:g + 1]), g
    lo, hi = host.update(start[:100], 6, **_rows(d, slice(0, 100))), host.update(start[100:], 6, **_rows(d, slice(100, n)))
    assert ER.bits_equal(np.vstack([lo, hi]), whole)
    assert ER.bits_equal(host.summary(whole)[0], host.summary(np.vstack([lo, hi]))[0])


def test_a_frozen_record_keeps_every_bit():
    """records ended with each code, then further updates with any inputs -- finite, NaN everywhere, and inputs that would end the episode otherwise: not a bit changes,
    a NaN payload in an unused word included; the alive rows between them go on"""
    n = 20
    start = np.array(_records()[:n])
    frozen = [2, 3, 16, 19]
    for i, g in enumerate(frozen):
        start[g, 2] = 1 + i % 3; start[g, 1] = 5
        start.view(np.uint64)[g, 13] = POISON
    d = _rows(ER.random_inputs(n, seed=9500)[0], slice(0, n))
    nan = {k: (np.full(v.shape, np.nan) if v.dtype == np.float64 else v) for k, v in d.items()}
    low = dict(d, state=np.array(d["state"])); low["state"][:, 5] = 0.0
    for ins in (d, nan, low):
        out = host.update(start, 9, **ins)
        assert ER.bits_equal(out[frozen], start[frozen])
        assert ER.bits_equal(out, ER.update(start, 9, **ins))
    alive = [g for g in range(n) if g not in frozen]
    assert (host.update(start, 9, **d)[alive, 0] == 7).all() and (host.update(start, 9, **nan)[alive, 2] == 1).all()


@pytest.mark.parametrize("where", ["pos", "v", "R", "estimate", "command", "height command", "ground", "stance force", "inf in pos"])
def test_a_non_finite_input_ends_the_episode_and_stays_with_its_robot(where):
    """a NaN (or an infinity) in one robot's row of one input: end_code 1 and end_tick_p1 = tick + 1 in that record and nothing else changed in it; the neighbouring
    rows are what they are without the NaN"""
    n, g, tick = 33, 17, 41
    d = {k: np.array(v) for k, v in _rows(ER.random_inputs(n, seed=9600)[0], slice(0, n)).items()}
    start = _records()[:n]
    clean = host.update(start, tick, **d)
    d["contacts"][g] = (1, 0, 1, 0)
    bad = float("inf") if where.startswith("inf") else float("nan")
    if where in ("pos", "inf in pos"): d["state"][g, 4] = bad
    elif where == "v": d["state"][g, 11] = bad
    elif where == "R": d["R"][g, 3] = bad
    elif where == "estimate": d["root_lin_vel"][g, 1] = bad
    elif where == "command": d["root_lin_vel_d"][g, 0] = bad
    elif where == "height command": d["root_pos_d_z"][g] = bad
    elif where == "ground": d["ground"][g, 2] = bad
    else: d["grf_body"][g, 7] = bad   # (leg 2: a stance leg)
    out = host.update(start, tick, **d)
    assert ER.bits_equal(out, ER.update(start, tick, **d))
    want = np.array(start[g]); want[1] = tick + 1; want[2] = 1
    assert ER.bits_equal(out[g], want)
    keep = np.arange(n) != g
    assert ER.bits_equal(out[keep], clean[keep]) and (out[keep, 2] == 0).all()


def test_a_nan_in_a_swing_legs_force_changes_nothing():
    n, g = 33, 17
    d = {k: np.array(v) for k, v in _rows(ER.random_inputs(n, seed=9600)[0], slice(0, n)).items()}
    d["contacts"][g] = (1, 0, 1, 0)
    start = _records()[:n]
    clean = host.update(start, 41, **d)
    d["grf_body"][g, 3:6] = np.nan; d["grf_body"][g, 9:12] = np.inf   # (legs 1 and 3 swing)
    out = host.update(start, 41, **d)
    assert ER.bits_equal(out, clean) and out[g, 2] == 0 and out[g, 0] == 7


def test_the_ways_an_episode_ends():
    """tilt takes precedence over height when both hold; each alone gives its code; the comparisons are strict; the ending update accumulates nothing; a sloped
    ground moves the height test with the robot; x0 / y0 are taken once"""
    n = 8
    d = {k: np.array(v) for k, v in _rows(ER.random_inputs(n, seed=9700)[0], slice(0, n)).items()}
    start = _records()[:n]
    cfg = dict(min_up=0.5, min_height=0.12)
    d["ground"][:] = 0.0
    d["R"][0, 8] = 0.4; d["state"][0, 5] = 0.05             # both: tilt
    d["R"][1, 8] = 0.4                                       # tilt alone
    d["state"][2, 5] = 0.05                                  # height alone
    d["R"][3, 8] = 0.5; d["state"][3, 5] = 0.12              # on both thresholds: alive
    d["ground"][4] = (0.1, 0.5, 0.0); d["state"][4, 3] = 0.2; d["state"][4, 5] = 0.3   # 0.3 above z = 0, 0.1 above its own plane: height
    d["R"][5, 8] = np.nextafter(0.5, 0)                      # one ulp under: tilt
    out = host.update(start, 77, cfg=cfg, **d)
    assert ER.bits_equal(out, ER.update(start, 77, cfg=cfg, **d))
    assert list(out[:8, 2]) == [2, 2, 3, 0, 3, 2, 0, 0]
    for g in (0, 1, 2, 4, 5):
        want = np.array(start[g]); want[1] = 78; want[2] = out[g, 2]
        assert ER.bits_equal(out[g], want), g
    assert out[3, 0] == 7 and out[3, 5] >= 0.5
    # x0 / y0: the update that finds ticks == 0 takes them, no later one does
    zero = np.zeros((n, ER.WORDS))
    ins = [_rows(x, slice(0, n)) for x in ER.random_inputs(n, seed=9800, ticks=3)]
    a = host.update(zero, 0, **ins[0])
    assert ER.bits_equal(a[:, 13], ins[0]["state"][:, 3]) and ER.bits_equal(a[:, 14], ins[0]["state"][:, 4]) and (a[:, 15] == 0).all()
    b = host.update(host.update(a, 1, **ins[1]), 2, **ins[2])
    assert ER.bits_equal(b[:, 13:15], a[:, 13:15]) and (b[:, 15] > 0).all()
    dx, dy = ins[2]["state"][:, 3] - a[:, 13], ins[2]["state"][:, 4] - a[:, 14]
    assert ER.bits_equal(b[:, 15], dx * dx + dy * dy)


def test_the_summary_row_is_the_lowest_on_a_tie_and_nothing_reads_row_n():
    """the largest tilt_max three times, in two wavefronts and two workgroups of the second level: word 10 is the lowest of the three rows; no ended record: word 5 is -1;
    the first ended tick is found wherever it is; row n may hold anything"""
    n = 4200
    ep = ER.random_records(n + 1, seed=9900)
    ep[:, 5] = np.minimum(ep[:, 5], 0.4)
    for g in (4150, 77, 2000):
        ep[g, 5] = 0.45
    ep[n] = np.nan
    out, _ = host.summary(ep, n)
    assert ER.bits_equal(out, ER.summary(ep[:n])) and out[9] == 0.45 and out[10] == 77
    some = np.array(ep[:131]); some[130] = np.nan
    o = host.summary(some, 130)[0]
    some[130] = 1e300; some[130, 2] = 2; some[130, 1] = 1   # (a row that would change eleven words, were it read)
    assert ER.bits_equal(host.summary(some, 130)[0], o) and ER.bits_equal(o, ER.summary(some[:130]))
    few = np.array(ep[:130]); few[:, 1:3] = 0
    o = host.summary(few)[0]
    assert o[5] == -1 and o[1] == 130 and o[2:5].sum() == 0 and ER.bits_equal(o, ER.summary(few))
    few[129, 1:3] = (300, 3); few[3, 1:3] = (12, 1); few[64, 1:3] = (12, 2)
    o = host.summary(few)[0]
    assert o[5] == 11 and list(o[1:5]) == [127, 1, 1, 1] and ER.bits_equal(o, ER.summary(few))


def test_the_tree_is_not_the_running_sum():
    """the restatement's tree against a left-to-right sum of the same column: they differ in the last bits on random data (so the bit-for-bit comparisons above do hold
    the kernel to the tree), and agree on integers"""
    ep = ER.random_records(4097, seed=9200 + 4097)
    run = 0.0
    for x in ep[:, 3]:
        run = run + x
    assert ER.tree_sum(ep[:, 3]) != run and abs(ER.tree_sum(ep[:, 3]) - run) <= 1e-9 * run
    assert ER.tree_sum(ep[:, 0]) == ep[:, 0].sum()
