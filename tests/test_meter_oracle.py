"""CPU: the numpy restatement of the level meter and squelch (tests/meter_oracle.py) against arm_power_f32 of the reference and a C division by
(float)n, recorded in tests/golden/meter.npz (tests/golden/make_meter_golden.py), bit for bit; then the properties of the law on hand-built
sequences of block powers: hysteresis, hang, non-finite blocks, the two senses, the counters, and the scalar form against the array form."""
import os

import numpy as np
import pytest

import meter_oracle as mo
import rxcommon as rc

GOLD = np.load(os.path.join(rc.GOLDEN_DIR, "meter.npz"))
NAMES = [str(n) for n in GOLD["names"]]
LENGTHS = [int(n) for n in GOLD["lengths"]]
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, what):
    """bit for bit where the reference's value is finite; elsewhere the same SET of NaN / Inf positions (not the payloads)"""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), what + ": NaN / Inf positions"
    ok = np.isfinite(want)
    assert np.array_equal(bits(got)[ok], bits(want)[ok]), what


def test_fixture_is_the_one_the_issue_asks_for():
    assert LENGTHS == [1, 3, 24, 64, 128]
    assert NAMES[-2:] == ["nan_sample", "inf_sample"]
    for k in ("noise_full_scale", "level_1e-22", "int16_slot_values", "ascending_magnitudes"):
        assert k in NAMES
    assert os.path.getsize(os.path.join(rc.GOLDEN_DIR, "meter.npz")) < 64 * 1024


@pytest.mark.parametrize("n", LENGTHS)
def test_power_and_mean_square_equal_the_reference_bit_for_bit(n):
    bl, pw, ms = GOLD["n%d/blocks" % n], GOLD["n%d/pw" % n], GOLD["n%d/ms" % n]
    assert bl.shape == (len(NAMES), n)
    assert np.isfinite(pw[:-2]).all() and np.isnan(pw[-2]) and np.isinf(pw[-1])
    same(mo.power(bl), pw, "arm_power_f32")
    same(mo.mean_square(bl), ms, "pw / (float)n")
    q = bl[NAMES.index("level_1e-22")]
    assert pw[NAMES.index("level_1e-22")] > 0 and pw[NAMES.index("level_1e-22")] < np.finfo(np.float32).tiny      # denormals are kept
    assert np.array_equal(np.trunc(bl[NAMES.index("int16_slot_values")] * 32768.0), bl[NAMES.index("int16_slot_values")] * 32768.0)
    assert q.any()


@pytest.mark.parametrize("n", [24, 64, 128])
def test_fixture_catches_another_summation_order(n):
    def pairwise(v):
        return v[0] if len(v) == 1 else np.float32(pairwise(v[:len(v) // 2]) + pairwise(v[len(v) // 2:]))
    a = GOLD["n%d/blocks" % n][NAMES.index("ascending_magnitudes")]
    assert pairwise(a * a) != GOLD["n%d/pw" % n][NAMES.index("ascending_magnitudes")]
    assert mo.power(a) == GOLD["n%d/pw" % n][NAMES.index("ascending_magnitudes")]


def blocks_of_power(ms, n=4):
    """audio [1][len(ms) * n] whose blocks have exactly the mean squares `ms` (each a float32 whose root is exact: powers of four)"""
    x = np.repeat(np.sqrt(np.asarray(ms, np.float64)), n).astype(np.float32)[None, :]
    assert np.array_equal(mo.mean_square(x.reshape(1, -1, n))[0], np.asarray(ms, np.float32))
    return x


def run(ms, **par):
    par.setdefault("attack", 1.0); par.setdefault("decay", 1.0)         # the level is the block's mean square
    m = mo.Meter(1, 4, **par)
    bitsv = m.process(blocks_of_power(ms))
    return m, bitsv[0]


HI, MID, LO = 1.0, 0.25, 0.0625


def test_hysteresis_holds_between_the_levels():
    # open above 0.5, close below 0.125: MID neither opens a closed gate nor closes an open one
    m, g = run([MID, MID, HI, MID, MID, LO, MID, MID, HI, LO], open_level=0.5, close_level=0.125)
    assert g.tolist() == [0, 0, 1, 1, 1, 0, 0, 0, 1, 0]
    assert m.opens[0] == 2 and m.open_blocks[0] == 4 and m.open[0] == 0
    # at the levels themselves: the comparisons are strict
    _, g = run([MID, HI, LO, LO / 4], open_level=MID, close_level=LO)
    assert g.tolist() == [0, 1, 1, 0]


@pytest.mark.parametrize("k", [0, 1, 3])
def test_hang_keeps_the_gate_open_exactly_k_closing_blocks(k):
    m, g = run([HI] + [LO] * (k + 3), open_level=0.5, close_level=0.125, hang=k)
    assert g.tolist() == [1] + [1] * k + [0] * 3
    assert m.trace["kept"][0].sum() == k and m.hold[0] == 0
    # a block that does not want to close re-arms the hang
    if k:
        _, g = run([HI] + [LO] * k + [MID] + [LO] * (k + 1), open_level=0.5, close_level=0.125, hang=k)
        assert g.tolist() == [1] + [1] * k + [1] + [1] * k + [0]


def test_a_nan_or_inf_block_leaves_the_level():
    m = mo.Meter(3, 4, attack=0.5, decay=0.25, open_level=0.5, close_level=0.125)
    x = np.tile(blocks_of_power([HI, HI, HI, LO]), (3, 1))
    x[1, 9] = np.nan
    x[2, 10] = np.inf
    g = m.process(x)
    lv = m.trace["level"]
    assert lv[1, 2] == lv[1, 1] and lv[2, 2] == lv[2, 1] and lv[0, 2] != lv[0, 1]
    assert np.isfinite(m.level).all() and g[1, 2] == g[1, 1]
    assert m.level[0] != m.level[1] and m.level[1] == m.level[2]


def test_attack_and_decay_are_the_agc_form():
    m = mo.Meter(1, 4, attack=0.5, decay=0.125, level_init=0.25)
    m.process(blocks_of_power([HI]))
    assert m.level[0] == F32(F32(0.25) + F32(F32(0.5) * F32(F32(1.0) - F32(0.25))))
    m.process(blocks_of_power([LO]))
    assert m.level[0] == F32(F32(0.625) + F32(F32(0.125) * F32(F32(0.0625) - F32(0.625))))


def test_below_mirrors_above():
    seq = [MID, MID, HI, MID, MID, LO, MID, MID, HI, LO, LO, HI]
    _, up = run(seq, sense=mo.ABOVE, open_level=0.5, close_level=0.125, hang=1)
    inv = [HI * LO / v for v in seq]                                  # HI <-> LO, MID stays
    m, dn = run(inv, sense=mo.BELOW, open_level=0.125, close_level=0.5, hang=1)
    assert up.tolist() == dn.tolist() and 0 < up.sum() < len(seq)
    assert m.opens[0] == 2


def test_counters_and_state_across_calls():
    seq = [HI, LO, LO, HI, LO, LO, MID, HI, LO, LO]
    par = dict(open_level=0.5, close_level=0.125, hang=1, attack=1.0, decay=1.0)
    one, many = mo.Meter(1, 4, **par), mo.Meter(1, 4, **par)
    g1 = one.process(blocks_of_power(seq))
    g2 = np.concatenate([many.process(blocks_of_power(seq[a:b])) for a, b in ((0, 1), (1, 4), (4, 10))], axis=1)
    assert np.array_equal(g1, g2)
    for k, v in one.state().items():
        assert np.array_equal(v, many.state()[k]), k
    assert one.opens[0] == 3 and one.open_blocks[0] == g1.sum() and one.opens.dtype == np.uint64
    one.reset()
    assert one.level[0] == 0 and not one.open[0] and not one.opens[0] and not one.open_blocks[0]


def test_scalar_step_equals_the_array_form():
    rng = np.random.default_rng(7)
    ch, n, nblk = 5, 3, 60
    x = (rng.uniform(-1, 1, (ch, nblk * n)) * np.repeat(rng.choice([1e-3, 1.0], (ch, nblk)), n, axis=1)).astype(np.float32)
    x[2, 17] = np.inf
    for sense, op, cl in ((mo.ABOVE, 0.05, 0.01), (mo.BELOW, 0.01, 0.05)):
        par = dict(sense=sense, hang=2, attack=0.5, decay=0.25, open_level=op, close_level=cl, level_init=0.02)
        m = mo.Meter(ch, n, **par)
        g = m.process(x)
        ms = mo.mean_square(x.reshape(ch, nblk, n))
        for c in range(ch):
            level, is_open, hold, opens = F32(0.02), 0, 0, 0
            for b in range(nblk):
                level, is_open, hold, opened, kept = mo.step(ms[c, b], level, is_open, hold, m.par)
                opens += opened
                assert is_open == g[c, b] and kept == m.trace["kept"][c, b]
            assert bits(level) == bits(m.level[c]) and hold == m.hold[c] and opens == m.opens[c]
        assert 0 < g.sum() < g.size


def test_gate_zeroes_closed_blocks_only():
    m = mo.Meter(2, 4, gate=1)
    y = np.arange(1, 17, dtype=np.float32).reshape(2, 8)
    out = m.gate_audio(y, np.array([[1, 0], [0, 1]], np.uint8))
    assert out.tolist() == [[1, 2, 3, 4, 0, 0, 0, 0], [0, 0, 0, 0, 13, 14, 15, 16]]
    assert mo.Meter(2, 4, gate=0).gate_audio(y, np.zeros((2, 2), np.uint8)) is y
