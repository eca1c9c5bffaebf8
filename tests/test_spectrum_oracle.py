"""CPU: the numpy restatement of the spectrum tap (tests/spectrum_oracle.py) against arm_cmplx_mult_real_f32 -> arm_cfft_f32 ->
arm_cmplx_mag_squared_f32 of the reference, recorded in tests/golden/spectrum.npz (tests/golden/make_spectrum_golden.py), bit for bit; the
library's twiddle generator against the reference's two tables, bit for bit; the restatement against numpy's double FFT; the framing."""
import os

import numpy as np
import pytest

import rxcommon as rc
import selenite_rx as sr
import spectrum_oracle as so

GOLD = np.load(os.path.join(rc.GOLDEN_DIR, "spectrum.npz"))
NAMES = [str(n) for n in GOLD["names"]]
LENS = (64, 512)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("tag", ["plain", "windowed"])
@pytest.mark.parametrize("n", LENS)
def test_restatement_equals_the_reference_bit_for_bit(n, tag):
    fr, win = GOLD["n%d/frames" % n], GOLD["n%d/window" % n] if tag == "windowed" else None
    assert fr.shape == (len(NAMES), n, 2) and NAMES[-1] == "inf_sample"
    y, p = so.power(fr, win)
    wy, wp = GOLD["n%d/%s/fft" % (n, tag)], GOLD["n%d/%s/power" % (n, tag)]
    fin = slice(0, len(NAMES) - 1)
    assert np.isfinite(wy[fin]).all() and not np.isnan(wp[fin]).any()     # (at 1e18 the power of 512 points overflows to +Inf: one bit pattern)
    assert np.array_equal(bits(y[fin]), bits(wy[fin])), "transform"
    assert np.array_equal(bits(p[fin]), bits(wp[fin])), "power"
    # the frame with an Inf sample: the SET of NaN / Inf values, not their payloads
    assert not np.isfinite(wp[-1]).all()
    for got, want in ((y[-1], wy[-1]), (p[-1], wp[-1])):
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
        ok = np.isfinite(want)
        assert np.array_equal(bits(got)[ok], bits(want)[ok])


def test_fixture_holds_what_it_should():
    for n in LENS:
        fr = GOLD["n%d/frames" % n]
        i = NAMES.index
        assert not fr[i("silent")].any() and not np.signbit(fr[i("silent")]).any()
        assert np.signbit(fr[i("minus_zero")]).any() and not fr[i("minus_zero")].any()
        assert 0 < np.abs(fr[i("level_1e-22")]).max() < 1.1e-22 and np.abs(fr[i("level_1e18")]).max() > 5e17
        # level 1e-22: every product of the power is a denormal (or zero) -- a flushed multiply shows
        p = GOLD["n%d/plain/power" % n][i("level_1e-22")]
        assert (p < np.finfo(np.float32).tiny).all() and (p > 0).any()
        assert np.isinf(fr[i("inf_sample")]).sum() == 1
    assert os.path.getsize(os.path.join(rc.GOLDEN_DIR, "spectrum.npz")) < 1 << 20


@pytest.mark.parametrize("n", LENS)
def test_library_twiddles_equal_the_reference_tables(n):
    want = GOLD["twiddle%d" % n]
    got = sr.spectrum_twiddles(n)
    assert got.shape == want.shape == (n, 2)
    assert np.array_equal(bits(got), bits(want))               # signs of the zeros included
    assert np.array_equal(bits(so.twiddles(n)), bits(want))
    # ... and the plain (float)cos / sin is NOT that table
    a = 2.0 * np.pi * np.arange(n) / n
    plain = np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)
    assert (bits(plain) != bits(want)).any()


def test_twiddles_refuse_other_lengths():
    L = sr.lib()
    buf = np.zeros(2 * 4096, np.float32)
    for n in (0, 16, 32, 128, 256, 1024, 2048, 4096, 100):
        assert L.selenite_rx_spectrum_twiddles(buf.ctypes.data_as(sr.f32p), n) == sr.LENGTH_ERROR
    assert L.selenite_rx_spectrum_twiddles(None, 64) == sr.ARGUMENT_ERROR


@pytest.mark.parametrize("tag", ["plain", "windowed"])
@pytest.mark.parametrize("n", LENS)
def test_restatement_against_numpy_double_fft(n, tag):
    """the project's bar: 1e-5 of the row maximum (the reference itself is at 2.3e-7 here: a factor of 40 below)"""
    fr = GOLD["n%d/frames" % n][:-1].astype(np.float64)
    if tag == "windowed":
        fr = fr * GOLD["n%d/window" % n].astype(np.float32).astype(np.float64)[None, :, None]
    ref = np.fft.fft(fr[..., 0] + 1j * fr[..., 1], axis=1)
    y, p = so.power(GOLD["n%d/frames" % n][:-1], GOLD["n%d/window" % n] if tag == "windowed" else None)
    for f in range(fr.shape[0]):
        top = np.abs(ref[f]).max()
        if top == 0:
            assert not y[f].any() and not p[f].any()
            continue
        err = np.abs((y[f, :, 0].astype(np.float64) + 1j * y[f, :, 1]) - ref[f]).max() / top
        assert err < 1e-5, (NAMES[f], err)
        if NAMES[f] in ("level_1e-22", "level_1e18"):
            continue                                           # (the power of these leaves the float32 normal range)
        perr = np.abs(p[f].astype(np.float64) - np.abs(ref[f]) ** 2).max() / (top * top)
        assert perr < 1e-5, (NAMES[f], perr)


@pytest.mark.parametrize("n", LENS)
def test_tone_at_bin_k_peaks_at_its_display_index(n):
    t = np.arange(n)
    for k in (0, 1, 5, n // 2 - 1, n // 2, n - 3, n - 1):
        iq = np.stack([np.cos(2 * np.pi * k * t / n), np.sin(2 * np.pi * k * t / n)], axis=1).astype(np.float32)[None]
        st = so.Spectrum(1, n)
        row = st.process(iq)
        assert int(np.argmax(row[0])) == (k + n // 2) % n, k
        assert st.frames == 1


@pytest.mark.parametrize("n", LENS)
def test_rows_and_state_do_not_depend_on_the_call_cuts(n):
    rng = np.random.default_rng(n)
    ch, total = 3, 4096
    x = rng.uniform(-1, 1, (ch, total, 2)).astype(np.float32)
    win = GOLD["n%d/window" % n]
    for stride, average in ((1, 0), (1, 1), (3, 1), (8, 0)):
        one = so.Spectrum(ch, n, stride, average, 0.25, win)
        one.process(x)
        for cuts in ([256] * 16, [768, 256, 3072], [96] * 40 + [256], [1, 4095], [63, 1, 64, 448, 3520]):
            assert sum(cuts) == total
            many, at = so.Spectrum(ch, n, stride, average, 0.25, win), 0
            for c in cuts:
                many.process(x[:, at:at + c])
                at += c
            assert np.array_equal(bits(many.rows), bits(one.rows)), (stride, average, cuts)
            assert many.position == one.position == total and many.frames == one.frames == -(-(total // n) // stride)


def test_stride_larger_than_the_stream_transforms_frame_zero_only():
    x = np.random.default_rng(5).uniform(-1, 1, (2, 2048, 2)).astype(np.float32)
    st = so.Spectrum(2, 512, stride=1000)
    st.process(x[:, :1024])
    row = st.rows.copy()
    assert st.frames == 1 and row.any()
    st.process(x[:, 1024:])
    assert st.frames == 1 and np.array_equal(bits(st.rows), bits(row))


def test_averaging_form_is_the_agcs():
    x = np.random.default_rng(6).uniform(-1, 1, (1, 3 * 64, 2)).astype(np.float32)
    st = so.Spectrum(1, 64, average=1, alpha=0.3)
    st.process(x)
    row = np.zeros(64, np.float32)
    for f in range(3):
        _, p = so.power(x[0, 64 * f:64 * f + 64])
        p = np.roll(p, 32)
        row = row + np.float32(0.3) * (p - row)
    assert np.array_equal(bits(st.rows[0]), bits(row))


@pytest.mark.parametrize("kind", [sr.WINDOW_HANN, sr.WINDOW_BLACKMAN_HARRIS])
def test_design_window(kind):
    for n in LENS:
        w = sr.design_window(n, kind)
        a = 2.0 * np.pi * np.arange(n) / n
        want = 0.5 - 0.5 * np.cos(a) if kind == sr.WINDOW_HANN else \
            0.35875 - 0.48829 * np.cos(a) + 0.14128 * np.cos(2 * a) - 0.01168 * np.cos(3 * a)
        assert w.dtype == np.float32 and np.abs(w.astype(np.float64) - want).max() < 1e-7
        assert np.isfinite(w).all() and int(np.argmax(w)) == n // 2
    L = sr.lib()
    buf = np.zeros(64, np.float32)
    assert L.selenite_rx_design_window(None, 64, kind) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_design_window(buf.ctypes.data_as(sr.f32p), 1, kind) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_design_window(buf.ctypes.data_as(sr.f32p), 64, 2) == sr.ARGUMENT_ERROR
