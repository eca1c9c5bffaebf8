"""CPU: the numpy restatement of the noise blanker (tests/nb_oracle.py) against arm_cmplx_mag_squared_f32, arm_mean_f32 and arm_q15_to_float
of the reference, recorded in tests/golden/nb.npz (tests/golden/make_nb_golden.py), bit for bit; then every decision branch of the stage on
hand-built frames."""
import os

import numpy as np
import pytest

import nb_oracle as no
import rxcommon as rc

GOLD = np.load(os.path.join(rc.GOLDEN_DIR, "nb.npz"))
NAMES = [str(n) for n in GOLD["names"]]
FRAMES = (32, 64, 128)
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("n", FRAMES)
def test_power_and_mean_equal_the_reference_bit_for_bit(n):
    fr, wp, wm = GOLD["f%d/frames" % n], GOLD["f%d/power" % n], GOLD["f%d/mean" % n]
    assert fr.shape == (len(NAMES), n, 2) and NAMES[-2:] == ["nan_sample", "inf_sample"]
    p = no.power(fr)
    m = no.mean(p)
    fin = slice(0, len(NAMES) - 2)
    assert not np.isnan(wp[fin]).any() and not np.isnan(wm[fin]).any()       # (at 1e18 the power overflows to +Inf: one bit pattern)
    assert np.array_equal(bits(p[fin]), bits(wp[fin])), "power"
    assert np.array_equal(bits(m[fin]), bits(wm[fin])), "mean"
    # the frames with a NaN / an Inf sample: the SET of NaN / Inf values, not their payloads
    for f in (-2, -1):
        assert not np.isfinite(wp[f]).all() and not np.isfinite(wm[f])
        for got, want in ((p[f], wp[f]), (m[f:][:1], wm[f:][:1])):
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
            ok = np.isfinite(want)
            assert np.array_equal(bits(got)[ok], bits(want)[ok])


def test_fixture_holds_what_it_should():
    i = NAMES.index
    for n in FRAMES:
        fr, pw, mn = GOLD["f%d/frames" % n], GOLD["f%d/power" % n], GOLD["f%d/mean" % n]
        assert not fr[i("silent")].any() and mn[i("silent")] == 0 and not np.signbit(mn[i("silent")])
        assert np.signbit(fr[i("minus_zero")]).any() and not pw[i("minus_zero")].any() and not np.signbit(pw[i("minus_zero")]).any()
        # level 1e-22: every product is a denormal (or zero) -- a flushed multiply shows; so is the mean
        assert (pw[i("level_1e-22")] < np.finfo(np.float32).tiny).all() and (pw[i("level_1e-22")] > 0).any()
        assert 0 < mn[i("level_1e-22")] < np.finfo(np.float32).tiny
        assert np.isnan(fr[i("nan_sample")]).sum() == 1 and np.isinf(fr[i("inf_sample")]).sum() == 1
        assert pw[i("noise_with_impulse"), n // 2] == 32.0
        # the summation order shows: summing the ascending frame backwards, or pairwise, gives another float
        p = pw[i("ascending_magnitudes")]
        back = F32(0)
        for v in p[::-1]:
            back = back + v
        assert bits(back / F32(n)) != bits(mn[i("ascending_magnitudes")])
    assert os.path.getsize(os.path.join(rc.GOLDEN_DIR, "nb.npz")) < 1 << 20


def test_q15_to_float_equals_the_reference_on_every_value():
    q = np.arange(-32768, 32768, dtype=np.int16)
    assert np.array_equal(bits(no.q15_to_float(q)), bits(GOLD["q15_to_float"]))


def test_contraction_in_the_power_would_show():
    """re * re + im * im with the second product fused into the sum is another float on a good share of random samples"""
    x = GOLD["f128/frames"][NAMES.index("noise_full_scale")].astype(np.float64)
    fused = (x[:, 0] * x[:, 0] + (x[:, 1].astype(F32) * x[:, 1].astype(F32)).astype(np.float64)).astype(F32)      # one rounding fewer
    assert (bits(fused) != bits(GOLD["f128/power"][NAMES.index("noise_full_scale")])).any()


# ---- the decisions, on hand-built frames ---------------------------------------------------------------------------------------------
def frame(F, base=0.25, at=(), amp=4.0):
    """one channel, one frame: I = base, Q = 0 (power base^2 exactly for the bases used here), `amp` on I and Q at the positions `at`"""
    x = np.zeros((1, F, 2), F32)
    x[0, :, 0] = base
    for n in at:
        x[0, n] = amp
    return x


def primed(F, level=0.0625, **kw):
    b = no.Blanker(1, F, **kw)
    b.level[:] = level
    return b


@pytest.mark.parametrize("F", FRAMES)
def test_unprimed_level_blanks_nothing_and_takes_the_mean(F):
    for lv in (0.0, -0.0, -1.0, np.nan):
        b = primed(F, lv)
        x = frame(F, at=(3, 4))
        y = b.process(x)
        assert np.array_equal(bits(y), bits(x)) and b.blanked[0] == 0 and b.bursts[0] == 0
        assert bits(b.level)[0] == bits(no.mean(no.power(x)))[0] and b.level[0] > 0
    # ... and a silent frame leaves it unprimed
    b = no.Blanker(1, F)
    b.process(np.zeros((1, 2 * F, 2), F32))
    assert bits(b.level)[0] == 0


@pytest.mark.parametrize("F", FRAMES)
def test_max_hits_blanks_and_one_more_is_a_burst(F):
    mh = F // 4
    at = list(range(5, 5 + 2 * mh, 2))                            # mh hits, one sample apart: guard 0 blanks exactly them
    b = primed(F, guard=0, max_hits=mh)
    y = b.process(frame(F, at=at))
    assert b.blanked[0] == mh and b.bursts[0] == 0
    assert not y[0, at].any() and (y[0, [n for n in range(F) if n not in at], 0] == 0.25).all()
    b = primed(F, guard=0, max_hits=mh)
    x = frame(F, at=at + [5 + 2 * mh])
    y = b.process(x)
    assert b.blanked[0] == 0 and b.bursts[0] == 1 and np.array_equal(bits(y), bits(x))
    # the level moves the same way in both: it does not depend on what was blanked
    assert b.level[0] == F32(0.0625) + F32(0.125) * (F32(2.0) * F32(0.0625) - F32(0.0625))


@pytest.mark.parametrize("F", FRAMES)
@pytest.mark.parametrize("guard", [0, 1, 3, 8])
def test_guard_is_clipped_at_both_edges_of_the_frame(F, guard):
    """two frames, a hit in the last sample of the first and one in the first sample of the second: neither reaches across"""
    b = primed(F, guard=guard, max_hits=2)
    x = np.concatenate([frame(F, at=(0, F - 1)), frame(F, at=(0,))], axis=1)
    y = b.process(x)
    gone = np.zeros(2 * F, bool)
    gone[:guard + 1] = gone[F - 1 - guard:F] = gone[F:F + guard + 1] = True
    assert np.array_equal(~y[0].any(axis=1), gone)
    assert b.blanked[0] == gone.sum() and np.array_equal(bits(y[0, ~gone]), bits(x[0, ~gone]))
    # mid-frame, for comparison: guard samples on either side
    b = primed(F, guard=guard, max_hits=2)
    y = b.process(frame(F, at=(F // 2,)))
    assert b.blanked[0] == 2 * guard + 1 and not y[0, F // 2 - guard:F // 2 + guard + 1].any() and y[0, F // 2 - guard - 1, 0] == 0.25


@pytest.mark.parametrize("F", FRAMES)
def test_power_equal_to_the_threshold_is_not_a_hit(F):
    # level 0.0625, threshold 8: thr = 0.5; (0.5, 0.5) has power 0.5 exactly; the next float up on I is a hit
    b = primed(F, guard=0)
    x = frame(F, at=(7, 9), amp=0.5)
    x[0, 9, 0] = np.nextafter(F32(0.5), F32(1))
    y = b.process(x)
    assert b.blanked[0] == 1 and y[0, 7, 0] == 0.5 and not y[0, 9].any()


@pytest.mark.parametrize("F", FRAMES)
def test_clamp_binding_and_not_binding(F):
    lv, a = F32(0.0625), F32(0.125)
    # mean 0.0625 * 1.5 < clamp * level: the mean itself
    b = primed(F)
    x = frame(F, base=np.sqrt(F32(0.09375)))
    b.process(x)
    m = no.mean(no.power(x))[0]
    assert m < F32(2) * lv and bits(b.level)[0] == bits(lv + a * (m - lv))
    # mean far above: the clamp; the same level whatever the mean
    for base in (1.0, 30.0):
        b = primed(F, max_hits=1)
        b.process(frame(F, base=base))
        assert bits(b.level)[0] == bits(lv + a * (F32(2) * lv - lv)) and b.bursts[0] == 1
    # clamp 1: the level never rises
    b = primed(F, clamp=1.0)
    b.process(frame(F, base=1.0))
    assert bits(b.level)[0] == bits(lv)


@pytest.mark.parametrize("F", FRAMES)
def test_nan_and_inf_samples(F):
    # a NaN sample is not a hit and passes with its payload; the frame's mean is NaN: m < c is false, the clamp binds
    b = primed(F, guard=1)
    x = frame(F, at=(5,))
    x.view(np.uint32)[0, 11, 0] = 0x7FC12345
    y = b.process(x)
    assert b.blanked[0] == 3 and y.view(np.uint32)[0, 11, 0] == 0x7FC12345 and y[0, 10, 0] == 0.25
    assert bits(b.level)[0] == bits(F32(0.0625) + F32(0.125) * (F32(0.125) - F32(0.0625)))
    # an Inf sample is a hit; unprimed, its frame's mean becomes the level: Inf, then NaN (Inf - Inf), then the next mean
    b = primed(F, guard=0)
    x = frame(F)
    x[0, 6, 1] = np.inf
    y = b.process(x)
    assert b.blanked[0] == 1 and not y[0, 6].any()
    b = no.Blanker(1, F)
    quiet = frame(F)
    b.process(x)
    assert np.isinf(b.level[0])
    b.process(quiet)
    assert np.isnan(b.level[0]) and b.blanked[0] == 0
    b.process(quiet)
    assert b.level[0] == F32(0.0625)


def test_int16_slots_keep_their_words_and_minus_32768():
    b = primed(64, level=2.0 ** -12, guard=1)
    x = np.full((1, 64, 2), 256, np.int16)                        # power 2^-14 + 2^-14
    x[0, 20] = (-32768, 32767)
    x[0, 40] = (-32768, 0)                                        # power 1.0 > 8 * 2^-12: a hit
    x[0, 50, 0] = -32768
    b.threshold = F32(1024.0)                                     # thr = 0.25: 20, 40 and 50 are hits
    y = b.process(x)
    assert y.dtype == np.int16 and b.blanked[0] == 9
    assert not y[0, 19:22].any() and (y[0, 22] == 256).all() and (y[0, 18] == 256).all()
    b = primed(64, level=0.5)
    y = b.process(x)                                              # thr = 4: nothing is a hit; -32768 survives
    assert np.array_equal(y, x) and y[0, 20, 0] == -32768


@pytest.mark.parametrize("F", FRAMES)
def test_stream_does_not_depend_on_the_call_cuts(F):
    rng = np.random.default_rng(F)
    x = rng.uniform(-0.1, 0.1, (3, 4096, 2)).astype(F32)             # (peak power 3 times the mean: no hit without an impulse)
    x[1, [100, 1023, 1024, 3000, 3001, 3002]] = 4.0
    one = no.Blanker(3, F)
    want = one.process(x)
    assert one.blanked[1] > 0 and one.blanked[0] == 0
    for cuts in ([256] * 16, [768, 256, 3072], [128] * 32):
        many, at, parts = no.Blanker(3, F), 0, []
        for c in cuts:
            parts.append(many.process(x[:, at:at + c]))
            at += c
        assert np.array_equal(bits(np.concatenate(parts, axis=1)), bits(want))
        for k in ("level", "blanked", "bursts"):
            assert many.state()[k].tobytes() == one.state()[k].tobytes(), (k, cuts)
