"""CPU: the numpy restatement of the I/Q correction stage (tests/iqc_oracle.py) against arm_mean_f32, arm_offset_f32, arm_scale_f32,
arm_sub_f32, arm_power_f32, arm_dot_prod_f32, arm_sqrt_f32, a C division and arm_q15_to_float of the reference, recorded in
tests/golden/iqc.npz (tests/golden/make_iqc_golden.py), bit for bit; then every branch of the stage on hand-built frames, and what the stage
is for: the image of an impaired two-tone input."""
import os

import numpy as np
import pytest

import iqc_oracle as io
import rxcommon as rc

GOLD = np.load(os.path.join(rc.GOLDEN_DIR, "iqc.npz"))
NAMES = [str(n) for n in GOLD["names"]]
FRAMES = (32, 64, 128)
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


def gold(n):
    return {k: GOLD["f%d/%s" % (n, k)] for k in ("frames", "coef", "mean", "rails", "t", "u", "qout", "sums", "est")}


@pytest.mark.parametrize("n", FRAMES)
def test_primitives_equal_the_reference_bit_for_bit(n):
    g = gold(n)
    fr, co = g["frames"], g["coef"]
    assert fr.shape == (len(NAMES), n, 2) and NAMES[-2:] == ["nan_sample", "inf_sample"]
    fin = slice(0, len(NAMES) - 2)
    for k in ("mean", "rails", "t", "u", "qout", "sums"):
        assert np.isfinite(g[k][fin]).all(), k
    I, Q = fr[..., 0], fr[..., 1]
    same(np.stack([io.mean(I), io.mean(Q)], axis=1), g["mean"], "arm_mean_f32")
    i, q = io.offset(I, -co[:, 0:1]), io.offset(Q, -co[:, 1:2])
    same(np.stack([i, q], axis=1), g["rails"], "arm_offset_f32")
    assert np.array_equal(bits(io.sub(I, co[:, 0:1]))[fin], bits(i)[fin])         # x - dc is x + (-dc): the same bits
    t = io.scale(i, co[:, 2:3])
    u = io.sub(q, t)
    same(t, g["t"], "arm_scale_f32"); same(u, g["u"], "arm_sub_f32"); same(io.scale(u, co[:, 3:4]), g["qout"], "arm_scale_f32 (g)")
    pii, pqq, piq, a, r, b = io.estimate(i, q)
    same(np.stack([pii, pqq, piq], axis=1), g["sums"], "arm_power_f32 / arm_dot_prod_f32")
    same(a, g["est"][:, 0], "quotient"); same(r, g["est"][:, 1], "r")
    d = io.quotient(pii, r)
    same(d, g["est"][:, 2], "pii / r")
    pos = g["est"][:, 2] >= 0                                      # (arm_sqrt_f32 refuses the rest and leaves 0: the stage never uses those)
    assert pos[fin].sum() >= 6
    same(b[pos], g["est"][pos, 3], "arm_sqrt_f32")
    assert not g["est"][~pos, 3].any()


def test_fixture_holds_what_it_should():
    i = NAMES.index
    tiny = np.finfo(np.float32).tiny
    for n in FRAMES:
        g = gold(n)
        fr, sums, est = g["frames"], g["sums"], g["est"]
        assert np.abs(fr[i("noise_full_scale")]).max() > 0.9
        # level 1e-22 with dc = 0: every product is a denormal (or zero) -- a flushed multiply shows; so are the three sums and r
        assert not g["coef"][i("level_1e-22"), :2].any()
        assert (0 < sums[i("level_1e-22"), :2]).all() and (sums[i("level_1e-22"), :2] < tiny).all() and 0 < est[i("level_1e-22"), 1] < tiny
        assert np.isfinite(est[i("level_1e-22")]).all() and est[i("level_1e-22"), 3] > 0
        q = fr[i("int16_slot_values")] * 32768.0
        assert np.array_equal(q, np.trunc(q)) and np.abs(q).max() > 30000
        assert np.isnan(fr[i("nan_sample")]).sum() == 1 and np.isinf(fr[i("inf_sample")]).sum() == 1
        assert np.isnan(g["mean"][i("nan_sample"), 0]) and np.isinf(g["mean"][i("inf_sample"), 1])
        assert not fr[i("q_zero"), :, 1].any() and sums[i("q_zero"), 1] == 0 and est[i("q_zero"), 1] == 0
        # the summation order shows: summing the ascending rail backwards gives another mean and another power
        asc = fr[i("ascending_magnitudes"), :, 0]
        assert asc.max() / asc.min() > 2.0 ** 22
        back, backp = F32(0), F32(0)
        ii = g["rails"][i("ascending_magnitudes"), 0]
        for v, w in zip(asc[::-1], ii[::-1]):
            back, backp = back + v, backp + w * w
        assert bits(back / F32(n)) != bits(g["mean"][i("ascending_magnitudes"), 0])
        assert bits(backp) != bits(sums[i("ascending_magnitudes"), 0])
    assert os.path.getsize(os.path.join(rc.GOLDEN_DIR, "iqc.npz")) < 1000000


def test_q15_to_float_equals_the_reference_on_every_value():
    q = np.arange(-32768, 32768, dtype=np.int16)
    assert np.array_equal(bits(io.q15_to_float(q)), bits(GOLD["q15_to_float"]))


def test_contraction_in_the_power_or_in_the_subtraction_would_show():
    """q - i * p fused is another float on 7 of the 128 samples of the full-scale noise frame (|p| is small: the product's own rounding is
    small against q); sum + in * in with the product fused into the sum changes a partial
    sum now and then, and what is left of that in the frame's pii shows on 3 of the fixture's 24 finite frames"""
    differ, total = 0, 0
    for n in FRAMES:
        g = gold(n)
        for k in range(len(NAMES) - 2):
            s = F32(0)
            for v in g["rails"][k, 0].astype(np.float64):
                s = F32(np.float64(s) + v * v)                     # one rounding instead of two (the double product is exact)
            differ, total = differ + int(bits(s)[0] != bits(g["sums"][k, 0])[0]), total + 1
    assert total == 24 and differ >= 2, (differ, total)
    g = gold(128)
    k = NAMES.index("noise_full_scale")
    i, q = g["rails"][k, 0].astype(np.float64), g["rails"][k, 1].astype(np.float64)
    fused = (q - i * np.float64(g["coef"][k, 2])).astype(F32)
    assert (bits(fused) != bits(g["u"][k])).sum() >= 4


# ---- the branches, on hand-built frames --------------------------------------------------------------------------------------------
def tone_frame(F, amp=0.5, gain=1.0, phase_deg=0.0, cycles=3):
    """one channel, one frame: a whole number of cycles, so that the rails' means are (nearly) zero and piq / pii is g sin(phase)"""
    w = 2 * np.pi * cycles * np.arange(F) / F
    x = np.zeros((1, F, 2), F32)
    x[0, :, 0] = amp * np.cos(w)
    x[0, :, 1] = gain * amp * np.sin(w + np.deg2rad(phase_deg))
    return x


def raw_estimate(x, dc=(0.0, 0.0)):
    i, q = io.sub(x[:, :, 0], F32(dc[0])), io.sub(x[:, :, 1], F32(dc[1]))
    return io.estimate(i, q)


@pytest.mark.parametrize("F", FRAMES)
def test_valid_estimate_moves_p_and_g_and_corrects_with_the_coefficients_in_front_of_the_frame(F):
    c = io.Corrector(1, F, alpha=0.25, dc_alpha=0.0, p_init=0.05, g_init=1.1, dc_i_init=0.01, dc_q_init=-0.02)
    x = tone_frame(F, gain=1.08, phase_deg=4.0)
    y = c.process(x)
    i, q = x[0, :, 0] - F32(0.01), x[0, :, 1] - F32(-0.02)
    assert np.array_equal(bits(y[0, :, 0]), bits(i))
    assert np.array_equal(bits(y[0, :, 1]), bits((q - i * F32(0.05)) * F32(1.1)))
    _, _, _, a, _, b = raw_estimate(x, (0.01, -0.02))
    assert abs(a[0] - 1.08 * np.sin(np.deg2rad(4.0))) < 0.02 and abs(b[0] - 1 / (1.08 * np.cos(np.deg2rad(4.0)))) < 0.02
    assert bits(c.p)[0] == bits(F32(0.05) + F32(0.25) * (a[0] - F32(0.05))) and bits(c.g)[0] == bits(F32(1.1) + F32(0.25) * (b[0] - F32(1.1)))
    assert c.held[0] == 0 and c.dc_i[0] == F32(0.01) and c.dc_q[0] == F32(-0.02)


@pytest.mark.parametrize("F", FRAMES)
def test_estimate_held_by_low_power_by_a_zero_rail_and_by_a_nan(F):
    x = tone_frame(F, gain=2.0)                                   # (r is about 4 pii: pii alone decides here)
    pii = raw_estimate(x)[0][0]
    # pii <= min_power: held, at equality too; just under it: taken
    for mp, held in ((pii, 1), (np.nextafter(pii, F32(0)), 0)):
        c = io.Corrector(1, F, alpha=0.5, dc_alpha=0.0, min_power=mp, p_init=0.1, g_init=1.2, g_max=4.0)
        c.process(x)
        assert c.held[0] == held and (c.p[0] == F32(0.1)) == bool(held) and (c.g[0] == F32(1.2)) == bool(held)
    # Q = 0: r = 0 is not > min_power = 0 (b would be +Inf); I = 0: pii = 0
    for rail in (1, 0):
        z = x.copy()
        z[:, :, rail] = 0
        c = io.Corrector(1, F, alpha=0.5, dc_alpha=0.0, min_power=0.0, p_init=0.1, g_init=1.2)
        c.process(z)
        assert c.held[0] == 1 and c.p[0] == F32(0.1) and c.g[0] == F32(1.2)
    # a NaN on either rail, an Inf on either rail: every comparison with a NaN is false, Inf is not <= FLT_MAX
    for rail in (0, 1):
        for v in (np.nan, np.inf):
            z = x.copy()
            z[0, 5, rail] = v
            c = io.Corrector(1, F, alpha=0.5, dc_alpha=0.0, min_power=0.0, p_init=0.1, g_init=1.2)
            y = c.process(z)
            assert c.held[0] == 1 and c.p[0] == F32(0.1) and c.g[0] == F32(1.2)
            assert np.isfinite(y[0, :5]).all() and np.isfinite(y[0, 6:]).all()      # (the sample itself is the chain's business)
    # silence with min_power = 0
    c = io.Corrector(1, F, alpha=0.5, min_power=0.0)
    c.process(np.zeros((1, 3 * F, 2), F32))
    assert c.held[0] == 3 and c.p[0] == 0 and c.g[0] == 1 and c.dc_i[0] == 0


@pytest.mark.parametrize("F", FRAMES)
def test_clamps_of_a_and_b(F):
    # 30 degrees: a = sin 30 = 0.5 > p_max = 0.25, and the other sign
    for deg, want in ((30.0, 0.25), (-30.0, -0.25)):
        x = tone_frame(F, phase_deg=deg)
        assert abs(raw_estimate(x)[3][0]) > 0.4
        c = io.Corrector(1, F, alpha=1.0, dc_alpha=0.0, p_max=0.25)
        c.process(x)
        assert c.p[0] == F32(want) and c.held[0] == 0
    # Q twice I: b = 0.5 < 1 / g_max; Q half of I: b = 2 > g_max
    for gain, want in ((2.0, F32(1.0) / F32(1.5)), (0.5, F32(1.5))):
        x = tone_frame(F, gain=gain)
        b = raw_estimate(x)[5][0]
        assert abs(b - 1 / gain) < 0.01
        c = io.Corrector(1, F, alpha=1.0, dc_alpha=0.0, g_max=1.5)
        c.process(x)
        assert bits(c.g)[0] == bits(want) and c.held[0] == 0


@pytest.mark.parametrize("F", FRAMES)
def test_dc_follows_the_frame_means_and_a_non_finite_mean_leaves_it(F):
    x = tone_frame(F)
    x[0, :, 0] += F32(0.125)
    x[0, :, 1] -= F32(0.0625)
    c = io.Corrector(1, F, alpha=0.0, dc_alpha=0.25, dc_i_init=0.01, dc_q_init=0.02)
    c.process(x)
    mi, mq = io.mean(x[0, :, 0]), io.mean(x[0, :, 1])
    assert abs(mi - 0.125) < 1e-6 and abs(mq + 0.0625) < 1e-6
    assert bits(c.dc_i)[0] == bits(F32(0.01) + F32(0.25) * (mi - F32(0.01))) and bits(c.dc_q)[0] == bits(F32(0.02) + F32(0.25) * (mq - F32(0.02)))
    # a NaN on I: dc_i stays, dc_q moves; an Inf on Q: the other way round
    for rail, v in ((0, np.nan), (1, np.inf), (1, -np.inf)):
        z = x.copy()
        z[0, 9, rail] = v
        c = io.Corrector(1, F, alpha=0.0, dc_alpha=0.25, dc_i_init=0.01, dc_q_init=0.02)
        c.process(z)
        moved = (c.dc_i[0] != F32(0.01), c.dc_q[0] != F32(0.02))
        assert moved == ((False, True) if rail == 0 else (True, False)) and np.isfinite([c.dc_i[0], c.dc_q[0]]).all()


@pytest.mark.parametrize("F", FRAMES)
def test_alpha_zero_and_dc_alpha_zero(F):
    x = tone_frame(F, gain=1.08, phase_deg=4.0)
    x[0, :, 0] += F32(0.1)
    z = np.concatenate([x, np.zeros_like(x)], axis=1)             # (the silent frame would be held)
    c = io.Corrector(1, F, alpha=0.0, dc_alpha=0.5, p_init=0.07, g_init=0.9, min_power=0.0)
    y = c.process(z)
    assert c.p[0] == F32(0.07) and c.g[0] == F32(0.9) and c.held[0] == 0 and c.dc_i[0] != 0
    assert np.array_equal(bits(y[0, :F, 1]), bits((x[0, :, 1] - x[0, :, 0] * F32(0.07)) * F32(0.9)))      # manual calibration is applied
    c = io.Corrector(1, F, alpha=0.5, dc_alpha=0.0, dc_i_init=0.03, dc_q_init=-0.04, min_power=0.0)
    c.process(x)
    assert c.dc_i[0] == F32(0.03) and c.dc_q[0] == F32(-0.04) and c.p[0] != 0 and c.held[0] == 0


def test_int16_slots_are_seen_through_q15_to_float_and_the_copy_is_f32():
    rng = np.random.default_rng(7)
    q = rng.integers(-32768, 32768, (2, 256, 2)).astype(np.int16)
    q[0, 3] = (-32768, 32767)
    a, b = io.Corrector(2, 64, alpha=0.25, dc_alpha=0.25), io.Corrector(2, 64, alpha=0.25, dc_alpha=0.25)
    ya, yb = a.process(q), b.process(q.astype(F32) / F32(32768.0))
    assert ya.dtype == np.float32 and np.array_equal(bits(ya), bits(yb))
    for k in ("dc_i", "dc_q", "p", "g", "held"):
        assert a.state()[k].tobytes() == b.state()[k].tobytes()


@pytest.mark.parametrize("F", FRAMES)
def test_stream_does_not_depend_on_the_call_cuts(F):
    x = impaired(3, 4096, seed=F)
    one = io.Corrector(3, F)
    want = one.process(x)
    for cuts in ([256] * 16, [768, 256, 3072], [128] * 32):
        many, at, parts = io.Corrector(3, F), 0, []
        for c in cuts:
            parts.append(many.process(x[:, at:at + c]))
            at += c
        assert np.array_equal(bits(np.concatenate(parts, axis=1)), bits(want))
        for k in ("dc_i", "dc_q", "p", "g", "held"):
            assert many.state()[k].tobytes() == one.state()[k].tobytes(), (k, cuts)


def test_state_round_trip_and_reset():
    x = impaired(2, 1024, seed=3)
    a = io.Corrector(2, 64, p_init=0.01, g_init=1.01, dc_i_init=0.001, dc_q_init=-0.001)
    a.process(x[:, :512])
    b = io.Corrector(2, 64)
    b.set_state(a.state())
    assert np.array_equal(bits(a.process(x[:, 512:])), bits(b.process(x[:, 512:])))
    a.reset()
    assert (a.p == F32(0.01)).all() and (a.g == F32(1.01)).all() and (a.dc_i == F32(0.001)).all() and (a.dc_q == F32(-0.001)).all() and not a.held.any()


# ---- what the stage is for ---------------------------------------------------------------------------------------------------------
K1, K2, NFFT = 301, -517, 4096                                    # the tones, in bins of the last 4096 samples


def impaired(channels, nsamp, seed=1, gain=1.08, phase_deg=4.0, dc=(-0.03, 0.02)):
    """a 0.5-amplitude tone, a second one 14 dB down on the other side, noise at -34 dB; then 8 % gain error, 4 degrees of phase error and a
    DC offset on each rail"""
    rng = np.random.default_rng(seed)
    n = np.arange(nsamp)
    s = 0.5 * np.exp(2j * np.pi * K1 * n / NFFT) + 0.5 * 10 ** (-14 / 20) * np.exp(2j * np.pi * K2 * n / NFFT)
    s = s[None, :] + 10 ** (-34 / 20) * (rng.standard_normal((channels, nsamp)) + 1j * rng.standard_normal((channels, nsamp))) / np.sqrt(2)
    ph = np.deg2rad(phase_deg)
    x = np.empty((channels, nsamp, 2), F32)
    x[:, :, 0] = s.real + dc[0]
    x[:, :, 1] = gain * (s.imag * np.cos(ph) + s.real * np.sin(ph)) + dc[1]
    return x


def image_db(y):
    """the image of the first tone over the last 4096 samples: the bin at -K1 over the bin at +K1, dB"""
    z = y[:, -NFFT:, 0].astype(np.float64) + 1j * y[:, -NFFT:, 1]
    X = np.fft.fft(z, axis=1)
    return 20 * np.log10(np.abs(X[:, -K1 % NFFT]) / np.abs(X[:, K1]))


@pytest.mark.parametrize("alpha", [1.0 / 16, 1.0 / 64], ids=["a16", "a64"])
@pytest.mark.parametrize("F", FRAMES)
def test_image_of_an_impaired_two_tone_input_drops_by_25_db(F, alpha):
    """32 768 samples; raw image -25.6 dB in that simulation.  The bar: 25 dB of improvement, 8 dB under the worst case (33 dB) of an independent float32
    simulation of the law.  The restatement's own improvement, dB (corrected image in brackets):
        F = 32:  alpha 1/16: 29.5 (-55.1)   alpha 1/64: 30.2 (-55.8)
        F = 64:  alpha 1/16: 40.2 (-65.9)   alpha 1/64: 42.2 (-67.8)
        F = 128: alpha 1/16: 54.2 (-79.8)   alpha 1/64: 32.7 (-58.4)
    (raw image of this input: -25.7 dB)"""
    x = impaired(1, 32768)
    raw = image_db(x)[0]
    assert -26.5 < raw < -25.0
    c = io.Corrector(1, F, alpha=alpha, dc_alpha=1.0 / 16)
    got = image_db(c.process(x))[0]
    print("F = %d alpha = %g: raw %.1f dB, corrected %.1f dB, improvement %.1f dB" % (F, alpha, raw, got, raw - got))
    assert raw - got >= 25.0
    assert c.held[0] == 0 and abs(c.dc_i[0] + 0.03) < 0.01 and abs(c.dc_q[0] - 0.02) < 0.01
