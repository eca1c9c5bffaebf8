"""CPU: the numpy restatement of the tone-detector bank (tests/tones_oracle.py) against the reference's own arm_biquad_cascade_df1_f32,
arm_power_f32, arm_cmplx_mag_squared_f32 and arm_max_f32 (tests/golden/tones.npz, written by tests/golden/make_tones_golden.py), the two
documented exceptions of the three-operation recurrence, the decision law on hand-written sequences, the design helpers, and what the bank
is for: the 50 CTCSS tones under noise."""
import os

import numpy as np
import pytest

import afilt_oracle as afo
import rxcommon as rc
import selenite_rx as sr
import tones_oracle as to

F = np.float32
NONE = to.NONE


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(rc.GOLDEN_DIR, "tones.npz")) as z:
        return {k: z[k] for k in z.files}


def test_fixture_covers_the_issue_cases(gold):
    cases = [tuple(int(v) for v in c) for c in gold["cases"]]
    assert {k for k, _ in cases} == {1, 5, 50, 64} and {n for _, n in cases} == {12, 24, 64, 200}
    for K, N in cases:
        x, lens = gold["k%d_n%d/x" % (K, N)], gold["k%d_n%d/lens" % (K, N)]
        assert np.isfinite(x).all() and not (np.signbit(x) & (x == 0)).any()
        assert (x[1] == 0).any() and ((x[1] != 0) & (np.abs(x[1]) < np.finfo(np.float32).tiny)).any()      # +0.0f and denormals
        ends = np.cumsum(lens)
        assert ends[-1] == x.shape[1] and any(e % N for e in ends[:-1])
        # a call ends a frame in its middle
        assert any((e - n) // N != (e - 1) // N and e % N for e, n in zip(ends, lens))


@pytest.mark.parametrize("case", range(7))
def test_restatement_equals_the_reference_on_bits(gold, case):
    K, N = (int(v) for v in gold["cases"][case])
    g = {k: gold["k%d_n%d/%s" % (K, N, k)] for k in ("coeffs", "x", "lens", "call_s", "call_e", "p", "fe", "pbest", "best")}
    t = to.Tones(2, 1, g["coeffs"], frame_blocks=N)
    at, frames = 0, 0
    for i, n in enumerate(int(v) for v in g["lens"]):
        before = (at // N)
        # one call: the restatement ends every frame inside it; the rows of the frames a call ends are checked sample by sample below
        for j in range(n):
            t.process(g["x"][:, at + j:at + j + 1])
            if (at + j + 1) % N == 0:
                f = (at + j + 1) // N - 1
                assert t.power.tobytes() == g["p"][:, f].tobytes(), ("p", K, N, f)
                assert t.frame_energy.tobytes() == g["fe"][:, f].tobytes(), ("E", K, N, f)
                assert (t.last_best == g["best"][:, f]).all(), ("best", K, N, f)
                pb, bi = to.arm_max(t.power)
                assert pb.tobytes() == g["pbest"][:, f].tobytes() and (bi == g["best"][:, f]).all()
                frames += 1
        at += n
        assert t.s.tobytes() == g["call_s"][:, i].tobytes(), ("state", K, N, i)
        assert t.energy.tobytes() == g["call_e"][:, i].tobytes(), ("running energy", K, N, i)
        assert at // N >= before
    assert frames == g["p"].shape[1] == 2 and t.position == at


def test_calls_of_any_cut_give_the_same_rows(gold):
    K, N = 5, 24
    g = {k: gold["k%d_n%d/%s" % (K, N, k)] for k in ("coeffs", "x")}
    x = g["x"][:, :48]
    a, b = to.Tones(2, 12, g["coeffs"], frame_blocks=2), to.Tones(2, 12, g["coeffs"], frame_blocks=2)
    a.process(x)
    for i in range(0, 48, 12):
        b.process(x[:, i:i + 12])
    for k, v in a.state().items():
        assert v.tobytes() == b.state()[k].tobytes(), k
    assert a.position == 4 and a.power.tobytes() == gold["k5_n24/p"][:, 1].tobytes()


def section_step(c, x, st):
    """one sample of arm_biquad_cascade_df1_f32 with the section {1, 0, 0, c, -1}, every product and sum kept (afilt_oracle.Afilt)"""
    f = afo.Afilt(1, np.array([[1, 0, 0, c, -1]], np.float32))
    f.state[0, 0] = st
    y = f.process(np.array([[x]], np.float32))
    return y[0, 0], f.state[0, 0].copy()


def test_the_two_exceptions_of_the_three_operation_form():
    """a -0.0f sample can give a zero of the other sign, and an Inf sample becomes NaN one step later than in the section"""
    c = F(-1.5)
    t = to.Tones(1, 1, np.array([[c, c / 2, 0.5]], np.float32), frame_blocks=100)
    t.process(np.array([[-0.0]], np.float32))
    y, _ = section_step(c, F(-0.0), np.zeros(4, np.float32))
    assert t.s[0, 0, 0] == 0 and np.signbit(t.s[0, 0, 0])           # c * +0 = -0; -0 + -0 = -0; -0 - +0 = -0
    assert y == 0 and not np.signbit(y)                             # 1 * -0 + 0 * +0 = +0 ...
    # Inf: the section's 0 * x1 is NaN at the step behind the Inf sample; the recurrence carries Inf one step more
    t = to.Tones(1, 1, np.array([[F(0.5), F(0.25), F(0.9)]], np.float32), frame_blocks=100)
    st = np.zeros(4, np.float32)
    y0, st = section_step(F(0.5), F(np.inf), st)
    t.process(np.array([[np.inf]], np.float32))
    assert np.isinf(y0) and np.isinf(t.s[0, 0, 0])
    y1, st = section_step(F(0.5), F(1.0), st)
    t.process(np.array([[1.0]], np.float32))
    assert np.isnan(y1) and np.isinf(t.s[0, 0, 0])                  # 0 * Inf there; 1 + 0.5 * Inf - 0 here
    t.process(np.array([[1.0]], np.float32))
    assert np.isnan(t.s[0, 0, 0])                                   # Inf - Inf, one step later


def test_finite_input_without_negative_zero_equals_the_section(gold):
    g = {k: gold["k5_n24/%s" % k] for k in ("coeffs", "x")}
    t = to.Tones(2, 1, g["coeffs"], frame_blocks=1000)
    x = g["x"][:, :40]
    t.process(x)
    for k in range(5):
        f = afo.Afilt(2, np.array([[1, 0, 0, g["coeffs"][k, 0], -1]], np.float32))
        f.process(x)
        assert f.state[:, 0, 2].tobytes() == t.s[:, k, 0].tobytes() and f.state[:, 0, 3].tobytes() == t.s[:, k, 1].tobytes()


def run_law(hits, confirm, release):
    """drives Tones.decide with frames whose best tone and hit are given: hits = list of tone index or None"""
    t = to.Tones(1, 1, to.design([0.1, 0.2, 0.3, 0.4]), confirm=confirm, release=release, ratio=0.0, min_power=1.0)
    rows = []
    for h in hits:
        pb = np.array([0.5 if h is None else 2.0], np.float32)
        t.decide(pb, np.array([0 if h is None else h], np.uint32), np.array([1.0], np.float32))
        rows.append((int(t.tone[0]), int(t.cand[0]), int(t.run[0]), int(t.changes[0])))
    return rows


def test_decision_law_confirm_release_and_a_candidate_change_mid_run():
    rows = run_law([2, 2, 2, None, 2, None, None, None], confirm=3, release=2)
    assert rows == [(NONE, 2, 1, 0), (NONE, 2, 2, 0), (2, 2, 3, 1), (2, NONE, 1, 1), (2, 2, 1, 1), (2, NONE, 1, 1), (NONE, NONE, 2, 2),
                    (NONE, NONE, 3, 2)]
    # a candidate change mid-run starts the count again; the reported tone moves from 1 to 3 without passing NONE
    rows = run_law([1, 1, 3, 1, 1, 3, 3], confirm=2, release=5)
    assert rows == [(NONE, 1, 1, 0), (1, 1, 2, 1), (1, 3, 1, 1), (1, 1, 1, 1), (1, 1, 2, 1), (1, 3, 1, 1), (3, 3, 2, 2)]
    # the first frames without a hit: cand == NONE from the start, tone == NONE: nothing changes, run counts and saturates
    t = to.Tones(1, 1, to.design([0.1]), confirm=1, release=1, min_power=1.0)
    t.run[:] = 65534
    for want in (65535, 65535):
        t.decide(np.array([0.0], np.float32), np.array([0], np.uint32), np.array([1.0], np.float32))
        assert (int(t.tone[0]), int(t.cand[0]), int(t.run[0]), int(t.changes[0])) == (NONE, NONE, want, 0)


def test_thresholds_of_a_hit():
    t = to.Tones(1, 12, to.design([0.1, 0.2]), frame_blocks=2, ratio=0.25, min_power=3.0)
    for pb, E, hit in ((7.0, 1.0, True), (6.0, 1.0, False), (3.0, 0.0, False), (3.5, 0.0, True), (np.inf, 0.0, False), (np.nan, 0.0, False)):
        t.reset()
        t.decide(np.array([pb], np.float32), np.array([1], np.uint32), np.array([E], np.float32))       # t = 0.25 * E * 24
        assert int(t.cand[0]) == (1 if hit else NONE), (pb, E)


def test_nan_at_index_0_wins_and_elsewhere_is_skipped():
    p = np.array([[np.nan, 1, 5, 2, 5], [1, 2, 7, np.nan, 3], [4, 4, 1, 0, 4]], np.float32)
    v, i = to.arm_max(p)
    assert np.isnan(v[0]) and list(i) == [0, 2, 0] and v[1] == 7 and v[2] == 4
    t = to.Tones(3, 1, to.design([0.1, 0.2, 0.3, 0.4, 0.45]), min_power=0.5)
    t.decide(v, i, np.zeros(3, np.float32))
    assert list(t.cand) == [NONE, 2, 0]                           # the NaN frame is no hit


def test_design_tones_matches_double_rounded_once():
    f = np.array([67.0 / 12000, 0.1, 0.25, 0.4999, 1e-6])
    c = sr.design_tones(f)
    w = 2 * np.pi * f
    assert c.tobytes() == np.stack([2 * np.cos(w), np.cos(w), np.sin(w)], axis=1).astype(np.float32).tobytes()
    assert c.tobytes() == to.design(f).tobytes()
    for bad in ([0.0], [0.5], [-0.1], [np.nan], [0.1, 0.6]):
        with pytest.raises(ValueError):
            sr.design_tones(bad)


def test_ctcss_hz_is_the_standard_table():
    hz = sr.ctcss_hz()
    assert hz.shape == (50,) and (np.diff(hz) > 0).all() and hz[0] == 67.0 and hz[-1] == 254.1
    assert {100.0, 123.0, 88.5, 151.4, 203.5} <= set(hz.tolist())
    assert np.allclose(hz * 10, np.round(hz * 10), atol=1e-9)


# ---- what the bank is for --------------------------------------------------------------------------------------------------------------
FS = 12000.0
# (the margins measured with these seeds: profiles/tones/README.md)


@pytest.mark.parametrize("N", [2400, 4800, 6000])
def test_the_50_ctcss_tones_under_noise(N):
    """12 kHz audio, each of the 50 CTCSS tones at amplitude 0.1 under uniform noise of +-0.3, ratio 0.02: the f32 bank picks the right tone
    50 of 50, the smallest p_best / (E N) is over the threshold and the largest for noise alone under it; the f32 powers against a double
    DFT; best against second best"""
    hz = sr.ctcss_hz()
    coeffs = sr.design_tones(hz / FS)
    rng = np.random.default_rng(0xC7C55 + N)
    t = np.arange(N)
    x = rng.uniform(-0.3, 0.3, (51, N))
    x[:50] += 0.1 * np.cos(2 * np.pi * (hz / FS)[:, None] * t[None, :] + rng.uniform(0, 2 * np.pi, (50, 1)))
    x = x.astype(np.float32)
    bank = to.Tones(51, N, coeffs, frame_blocks=1, confirm=1, release=1, ratio=0.02, min_power=0.0)
    bank.process(x)
    assert list(bank.tone[:50]) == list(range(50)), "50 of 50"
    assert bank.tone[50] == NONE and bank.changes[50] == 0, "noise alone"
    q = bank.power.astype(np.float64).max(axis=1) / (bank.frame_energy.astype(np.float64) * N)
    # |sum x e^{-jwn}|^2 in double: what the recurrence computes
    w = 2 * np.pi * hz / FS
    dft = np.abs(x.astype(np.float64) @ np.exp(-1j * np.outer(t, w))) ** 2
    err = np.abs(bank.power.astype(np.float64) - dft).max(axis=1) / dft.max(axis=1)
    srt = np.sort(bank.power[:50].astype(np.float64), axis=1)
    print("N=%d: min p_best/(E N) with a tone %.4f, noise alone %.5f, f32 error / peak %.2e, best / second >= %.2f"
          % (N, q[:50].min(), q[50], err.max(), (srt[:, -1] / srt[:, -2]).min()))
    assert q[:50].min() > 0.02 > q[50]
    assert err.max() <= 5.2e-4 * 4          # the issue measured 5.2e-4 on its inputs; the error grows with sqrt(N) eps: a factor of 4 of room for other seeds
    assert (srt[:, -1] / srt[:, -2]).min() > 1.0
