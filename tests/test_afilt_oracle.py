"""CPU: the numpy restatement of the audio filter stage (tests/afilt_oracle.py) against the reference's own arm_biquad_cascade_df1_f32
(tests/golden/afilt.npz, recorded through ref_biquad; live where oracle/_ref is built) and against the oracle's
orc_biquad_cascade_df1_f32; and the design helpers selenite_rx_design_biquad / selenite_rx_design_deemphasis (the library loads without a
device)."""
import ctypes as C
import os

import numpy as np
import pytest

import afilt_oracle as afo
import rxcommon as rc
import selenite_rx as sr

GOLDEN = os.path.join(rc.GOLDEN_DIR, "afilt.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def cut(lengths):
    a = 0
    for n in lengths:
        yield a, int(n)
        a += int(n)


@pytest.mark.parametrize("ns", range(1, 9))
def test_restatement_equals_the_reference_fixture(gold, ns):
    assert os.path.getsize(GOLDEN) < 150 * 1024
    assert list(gold["lengths"]) == [1, 3, 4, 12, 24, 96, 256]
    coeffs, x, y, states = (gold["ns%d/%s" % (ns, k)] for k in ("coeffs", "x", "y", "state"))
    assert coeffs.shape == (3, ns, 5) and x.shape == y.shape == (3, 396) and states.shape == (7, 3, ns, 4)
    # the inputs hold what they are there for
    assert (np.signbit(x[1]) & (x[1] == 0)).sum() >= 30 and ((np.abs(x[1]) < np.finfo(np.float32).tiny) & (x[1] != 0)).sum() >= 30
    assert (np.abs(x[2]) == np.finfo(np.float32).max).sum() == 2 and np.isinf(x[2]).sum() == 2 and np.isnan(y[2, -1])
    f = afo.Afilt(3, coeffs, per_channel=True)
    for i, (a, n) in enumerate(cut(gold["lengths"])):
        got = f.process(x[:, a:a + n])
        assert afo.same_bits(got, y[:, a:a + n]), ("audio", ns, a, n)
        assert afo.same_bits(f.state, states[i]), ("state", ns, a, n)
    # the finite streams: plain bits, no NaN rule needed
    assert afo.Afilt(2, coeffs[:2], True).process(x[:2]).tobytes() == y[:2].tobytes()


@pytest.mark.parametrize("ns", [1, 3, 8])
def test_restatement_equals_oracle_and_live_reference(gold, ns):
    coeffs, x = gold["ns%d/coeffs" % ns], gold["ns%d/x" % ns]
    L = rc.oracle_lib()
    ref = rc.RefLib() if rc.ref_available() else None
    f = afo.Afilt(3, coeffs, per_channel=True)
    so, sr_ = np.zeros((3, ns * 4), np.float32), np.zeros((3, ns * 4), np.float32)
    for a, n in cut(gold["lengths"]):
        want = f.process(x[:, a:a + n])
        for c in range(3):
            k5, xi, yo = np.ascontiguousarray(coeffs[c].reshape(-1)), np.ascontiguousarray(x[c, a:a + n]), np.empty(n, np.float32)
            L.orc_biquad_cascade_df1_f32(rc.fptr(k5), ns, rc.fptr(so[c]), rc.fptr(xi), rc.fptr(yo), n, rc.ARITH_CMSIS)
            assert afo.same_bits(yo, want[c]), ("orc", ns, c, a)
            assert afo.same_bits(so[c].reshape(ns, 4), f.state[c])
            if ref is not None:
                yr = ref.biquad(k5, ns, sr_[c], xi, n)
                assert afo.same_bits(yr, want[c]), ("ref", ns, c, a)
                assert afo.same_bits(sr_[c].reshape(ns, 4), f.state[c])


def test_one_call_of_2048_equals_eight_calls_of_256(gold):
    rng = np.random.default_rng(5)
    coeffs = gold["ns5/coeffs"][:2]
    x = rng.uniform(-0.5, 0.5, (2, 2048)).astype(np.float32)
    one, many = afo.Afilt(2, coeffs, True), afo.Afilt(2, coeffs, True)
    whole = one.process(x)
    parts = np.concatenate([many.process(x[:, a:a + 256]) for a in range(0, 2048, 256)], axis=1)
    assert whole.tobytes() == parts.tobytes() and one.state.tobytes() == many.state.tobytes()
    assert np.abs(whole).max() > 1e-3


def test_identity_section_is_not_a_pass_through():
    """why the kernel must not pad unused stage lanes with {1, 0, 0, 0, 0}: -0.0f + 0.0f is +0.0f, and 0 * Inf is NaN"""
    f = afo.Afilt(1, [[1, 0, 0, 0, 0]])
    y = f.process(np.array([[-0.0, 0.25]], np.float32))
    assert y[0, 0] == 0 and not np.signbit(y[0, 0]) and y[0, 1] == np.float32(0.25)
    y = afo.Afilt(1, [[1, 0, 0, 0, 0]]).process(np.array([[np.inf, 1.0]], np.float32))
    assert np.isinf(y[0, 0]) and np.isnan(y[0, 1])


# ---- the design helpers -------------------------------------------------------------------------
def rbj(kind, f0, q, gain_db=0.0):
    w, A = 2.0 * np.pi * f0, 10.0 ** (gain_db / 40.0)
    cw, al = np.cos(w), np.sin(w) / (2.0 * q)
    if kind == sr.BIQUAD_NOTCH:
        b, a = (1.0, -2.0 * cw, 1.0), (1.0 + al, -2.0 * cw, 1.0 - al)
    elif kind == sr.BIQUAD_PEAKING:
        b, a = (1.0 + al * A, -2.0 * cw, 1.0 - al * A), (1.0 + al / A, -2.0 * cw, 1.0 - al / A)
    elif kind == sr.BIQUAD_LOWPASS:
        b, a = ((1.0 - cw) / 2.0, 1.0 - cw, (1.0 - cw) / 2.0), (1.0 + al, -2.0 * cw, 1.0 - al)
    else:
        b, a = ((1.0 + cw) / 2.0, -(1.0 + cw), (1.0 + cw) / 2.0), (1.0 + al, -2.0 * cw, 1.0 - al)
    return np.array([b[0] / a[0], b[1] / a[0], b[2] / a[0], -a[1] / a[0], -a[2] / a[0]]).astype(np.float32)


def within_one_ulp(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return bool(np.all((got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))))


@pytest.mark.parametrize("kind", [sr.BIQUAD_NOTCH, sr.BIQUAD_PEAKING, sr.BIQUAD_LOWPASS, sr.BIQUAD_HIGHPASS])
def test_design_biquad_equals_the_cookbook_in_double(kind):
    for f0, q, g in ((1000.0 / 12000.0, 10.0, 6.0), (0.2, 0.7071, -12.0), (0.01, 30.0, 3.0), (0.49, 1.0, 0.5)):
        got = sr.design_biquad(kind, f0, q, g)
        assert got.dtype == np.float32 and within_one_ulp(got, rbj(kind, f0, q, g)), (kind, f0, q, g, got, rbj(kind, f0, q, g))


def test_design_deemphasis_and_refused_arguments():
    for tau in (0.9, 0.6, 3.6, 50.0):
        p = np.exp(-1.0 / tau)
        got = sr.design_deemphasis(tau)
        assert within_one_ulp(got, np.array([1.0 - p, 0, 0, p, 0]).astype(np.float32))
        assert got[1] == 0 and got[2] == 0 and got[4] == 0 and not np.signbit(got[1:3]).any()
    L, c = sr.lib(), np.full(5, 7.0, np.float32)
    p5 = c.ctypes.data_as(sr.f32p)
    for args in ((p5, 9, 0.1, 1.0, 0.0), (p5, -1, 0.1, 1.0, 0.0), (p5, 0, 0.0, 1.0, 0.0), (p5, 0, 0.5, 1.0, 0.0), (p5, 0, float("nan"), 1.0, 0.0),
                 (p5, 0, 0.1, 0.0, 0.0), (p5, 0, 0.1, float("nan"), 0.0), (p5, 1, 0.1, 1.0, float("inf")), (None, 0, 0.1, 1.0, 0.0)):
        assert L.selenite_rx_design_biquad(*args) == sr.ARGUMENT_ERROR, args
    for args in ((p5, 0.0), (p5, -1.0), (p5, float("nan")), (p5, float("inf")), (None, 0.9)):
        assert L.selenite_rx_design_deemphasis(*args) == sr.ARGUMENT_ERROR, args
    assert (c == 7.0).all()
    with pytest.raises(ValueError):
        sr.design_biquad(sr.BIQUAD_NOTCH, 0.6, 1.0)


FS = 12000.0


def level_db(coeffs, f):
    """level of a 0.5-amplitude tone of 8192 samples at f Hz behind the section, over the last 4096 samples, against the tone's own"""
    x = (0.5 * np.cos(2.0 * np.pi * f / FS * np.arange(8192))).astype(np.float32)[None, :]
    y = afo.Afilt(1, coeffs.reshape(1, 5)).process(x)
    rms = lambda v: np.sqrt(np.mean(v[0, 4096:].astype(np.float64) ** 2))  # noqa: E731
    return 20.0 * np.log10(max(rms(y), 1e-300) / rms(x))


@pytest.mark.parametrize("f0,q", [(1000.0, 10.0), (1000.0, 30.0), (2300.0, 10.0), (400.0, 5.0)])
def test_notch_removes_its_tone_and_leaves_the_neighbours(f0, q):
    """measured with the helper's own floats, float32 arithmetic: the tone at f0 falls by 111.0, 99.7, 134.4 and 105.4 dB; a tone 300 Hz
    below / above moves by (1000 Hz, Q 10) -0.08 / -0.13 dB, (1000, 30) -0.01 / -0.01, (2300, 10) -0.34 / -0.38, (400, 5) -0.01 / -0.12:
    at most 0.38 dB"""
    c = sr.design_biquad(sr.BIQUAD_NOTCH, f0 / FS, q)
    depth = -level_db(c, f0)
    near = [level_db(c, f0 - 300.0), level_db(c, f0 + 300.0)]
    print("notch f0 %g Q %g: %.1f dB at f0, %.2f / %.2f dB 300 Hz away" % (f0, q, depth, near[0], near[1]))
    assert depth >= 80.0
    assert max(abs(v) for v in near) < 1.0


def test_deemphasis_follows_the_one_pole_response():
    """tau = 75 us at 12 kHz (tau_samples = 0.9); measured: -0.0082, -0.7780, -3.9149 and -5.7172 dB at 100, 1000, 3000 and 5000
    Hz against |(1 - p) / (1 - p e^{-jw})| = -0.0087, -0.7774, -3.9149, -5.7174 dB: within 0.0006 dB"""
    c = sr.design_deemphasis(0.9)
    p = np.exp(-1.0 / 0.9)
    for f in (100.0, 1000.0, 3000.0, 5000.0):
        w = 2.0 * np.pi * f / FS
        want = 20.0 * np.log10(abs((1.0 - p) / (1.0 - p * np.exp(-1j * w))))
        got = level_db(c, f)
        print("de-emphasis %g Hz: %.4f dB, one pole %.4f dB" % (f, got, want))
        assert abs(got - want) < 0.01
