"""CPU: the numpy restatement of the polyphase combiner (tests/comb_oracle.py) equals the composition of the reference's own functions bit for
bit (tests/golden/comb.npz: arm_cfft_f32 inverse + arm_dot_prod_f32 + both builds of arm_float_to_q15, outputs and history), does not depend
on how the stream is cut into calls, is the float64 direct form (zero-stuff, filter, mix up, sum, / K) to the project's 1e-5 bar, turns a
constant on one channel into that bin's tone, and comes back out of the channeliser as what went in."""
import os

import numpy as np
import pytest

import chan_oracle as co
import comb_oracle as bo
import rxcommon as rc
import selenite_rx as sr

GOLD = np.load(os.path.join(rc.ROOT, "tests", "golden", "comb.npz"))
TAGS = [str(t) for t in GOLD["names"]]
Q15_TAG = "k64_p8_o2"


def case(tag):
    k, p, o = [int(s[1:]) for s in tag.split("_")]
    bins = GOLD[tag + "/bins"].astype(np.int64)
    return k, p, o, GOLD[tag + "/coeffs"], GOLD[tag + "/rows"], (None if len(bins) == k else bins), GOLD[tag + "/out"], int(GOLD[tag + "/cut"])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def to_c(y):
    return y[..., 0].astype(np.float64) + 1j * y[..., 1].astype(np.float64)


def run_cuts(cb, x, cuts, q15=False):
    outs, at = [], 0
    for n in cuts:
        outs.append((cb.process_q15 if q15 else cb.process)(x[:, at:at + n]))
        at += n
    assert at == x.shape[1]
    return np.concatenate(outs, axis=1)


def test_fixture_holds_the_cases_the_kernel_needs():
    assert TAGS == ["k64_p4_o1", "k64_p8_o2", "k512_p4_o2"]
    for tag in TAGS:
        k, p, o, g, x, bins, want, cut = case(tag)
        nb = k if bins is None else len(bins)
        assert g.shape == (k * p,) and x.shape[0] == nb and want.shape == (x.shape[1] * (k // o), 2) and 0 < cut < x.shape[1]
        ax = np.abs(x)
        assert ax.max() == 1.0 and ((ax > 0) & (ax < 1e-21)).any() and (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any()
        assert np.isfinite(want).all()
    bins = case("k512_p4_o2")[5]
    assert len(bins) == 64 and len(set(bins.tolist())) == 64 and {0, 255, 256, 511} <= set(bins.tolist()) and (np.diff(bins) < 0).any()
    for name in ("trunc", "round"):
        z = GOLD[Q15_TAG + "/q15_" + name]
        assert z.dtype == np.int16 and (z == 32767).any() and (z == -32768).any() and (np.abs(z.astype(np.int32)) < 32767).mean() > 0.75
    assert os.path.getsize(os.path.join(rc.ROOT, "tests", "golden", "comb.npz")) < 200 * 1024


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_equals_the_reference_composition_bit_for_bit(tag):
    k, p, o, g, x, bins, want, cut = case(tag)
    cb = bo.Combiner(1, k, o, p, g, bins)
    got = run_cuts(cb, x, [cut, x.shape[1] - cut])
    assert np.array_equal(bits(got[0]), bits(want))
    st = cb.state()
    assert np.array_equal(bits(st["history"]), bits(GOLD[tag + "/history"])) and int(st["position"][0]) == x.shape[1] * (k // o)


@pytest.mark.parametrize("tag", TAGS)
def test_cutting_the_stream_differently_gives_the_same_bits(tag):
    k, p, o, g, x, bins, want, _ = case(tag)
    nf = x.shape[1]
    for cuts in ([nf], [1] * nf, [1, 2, nf - 8, 5], [nf - 1, 1]):
        cb = bo.Combiner(1, k, o, p, g, bins)
        assert np.array_equal(bits(run_cuts(cb, x, cuts)[0]), bits(want)), cuts
        assert np.array_equal(bits(cb.history), bits(GOLD[tag + "/history"])), cuts


@pytest.mark.parametrize("rounding,name", [(0, "trunc"), (1, "round")])
def test_int16_output_equals_both_builds_of_float_to_q15(rounding, name):
    k, p, o, g, _, bins, _, cut = case(Q15_TAG)
    x, want = GOLD[Q15_TAG + "/q15_rows"], GOLD[Q15_TAG + "/q15_" + name]
    for cuts in ([cut, x.shape[1] - cut], [x.shape[1]]):
        got = run_cuts(bo.Combiner(1, k, o, p, g, bins, rounding), x, cuts, q15=True)
        assert got.dtype == np.int16 and np.array_equal(got[0], want)


def test_bands_are_independent_and_rows_follow_the_bin_table():
    k, p, o, g, x, bins, want, cut = case("k512_p4_o2")
    two = np.concatenate([x, x[::-1]])
    order = np.argsort(bins)
    cb = bo.Combiner(2, k, o, p, g, bins)
    got = cb.process(two)
    assert np.array_equal(bits(got[0]), bits(want))
    # band 1 has the rows reversed: the same as feeding the reversed bin table with the rows as they were
    assert np.array_equal(bits(got[1]), bits(bo.Combiner(1, k, o, p, g, bins[::-1]).process(x)[0]))
    assert np.array_equal(bits(bo.Combiner(1, k, o, p, g, bins[order]).process(x[order])[0]), bits(want))


@pytest.mark.parametrize("tag", TAGS)
def test_composition_is_the_float64_direct_form_to_1e_5(tag):
    """zero-stuff by D, filter by h, mix up by e^(+2 pi i k n / K), sum, / K: first the reference composition itself (the fixture), then the
    restatement, within 1e-5 of the output's maximum (measured on these rows: 9.5e-8 at worst)"""
    k, p, o, g, x, bins, want, cut = case(tag)
    ref = bo.direct64(x, g, k, o, bins)
    top = np.abs(ref).max()
    assert np.abs(to_c(want) - ref).max() <= 1e-5 * top
    got = bo.Combiner(1, k, o, p, g, bins).process(x)[0]
    assert np.abs(to_c(got) - ref).max() <= 1e-5 * top


# A constant 0.5 e^(0.3 i) on bin 5 alone, through selenite_comb_design_prototype's taps: once Q frames have passed the stream is the tone
# 0.5 e^(i (0.3 + 2 pi 5 n / K)).  The float64 direct form's own largest deviation from that tone, relative to 0.5 (the images of the
# zero-stuffed constant at multiples of fs / D, which the Hamming prototype leaves):
#   K 64, P 8, oversample 1, width 1.0: -52.35 dB      K 64, P 8, oversample 2, width 1.0: -62.52 dB      K 64, P 4, oversample 2, width 1.0: -58.33 dB
# The f32 composition may be 3 dB above that (measured: within 0.01 dB of the float64 form).
@pytest.mark.parametrize("p,ovs,dev_db", [(8, 1, -52.35), (8, 2, -62.52), (4, 2, -58.33)])
def test_constant_on_one_channel_leaves_as_that_bins_tone(p, ovs, dev_db):
    k, kb = 64, 5
    d, q = k // ovs, p * ovs
    g = sr.design_comb_prototype(k, p, 1.0, ovs)
    frames = q + 12
    x = np.empty((1, frames, 2), np.float32)
    x[0, :, 0], x[0, :, 1] = 0.5 * np.cos(0.3), 0.5 * np.sin(0.3)
    c0 = complex(x[0, 0, 0], x[0, 0, 1])
    n = np.arange(frames * d)
    ideal = c0 * np.exp(2j * np.pi * kb * n / k)
    s = q * d
    ref = bo.direct64(x, g, k, ovs, [kb])
    ref_db = 20 * np.log10(np.abs(ref[s:] - ideal[s:]).max() / 0.5)
    assert abs(ref_db - dev_db) <= 0.05, ref_db                  # the stated figure is the float64 form's
    cb = bo.Combiner(1, k, ovs, p, g, [kb])
    y = to_c(run_cuts(cb, x, [5, frames - 5]))[0]                # (with oversample 2 the second call starts on the upper half)
    assert 20 * np.log10(np.abs(y[s:] - ideal[s:]).max() / 0.5) <= dev_db + 3.0


# Combiner into channeliser, K 64, P 8, oversample 2, prototypes of width 1.0 on both sides, three slow complex tones of amplitude 0.3 on bins
# 3, 9 and 40.  The float64 direct forms (comb_oracle.direct64 into chan_oracle.direct64), behind the settling of both filters:
#   the three channels come back delayed by 2 P - 1 = 15 samples, within 2.23e-4 absolute (the Hamming prototype's pass-band droop);
#   at most 1.99e-4 in any of the other 61 bins.
# (A delay of 14 or 16 samples leaves 2.07e-2.)  The f32 compositions get the project's 1e-5 of the signal's amplitude on top of those.
def test_loop_back_through_the_channeliser():
    k, p, ovs, amp, frames = 64, 8, 2, 0.3, 200
    delay, fed = 2 * p - 1, [3, 9, 40]
    err64, leak64 = 2.23e-4, 1.99e-4
    others = [b for b in range(k) if b not in fed]
    gc, ga = sr.design_comb_prototype(k, p, 1.0, ovs), sr.design_chan_prototype(k, p, 1.0)
    m = np.arange(frames)
    c = np.zeros((k, frames), np.complex128)
    for b, f, ph in ((3, 0.004, 0.1), (9, -0.007, 1.0), (40, 0.011, 2.0)):
        c[b] = amp * np.exp(2j * np.pi * f * m + 1j * ph)
    rows = np.stack([c.real, c.imag], axis=-1).astype(np.float32)
    c = to_c(rows)
    s = delay + 2 * p * ovs                                      # both filters hold nothing but the tones

    def figures(back):
        return np.abs(back[fed][:, s:] - c[fed][:, s - delay:frames - delay]).max(), np.abs(back[others][:, s:]).max()

    wide = bo.direct64(rows, gc, k, ovs)
    e64, l64 = figures(co.direct64(np.stack([wide.real, wide.imag], axis=-1), ga, k, ovs))
    assert abs(e64 - err64) <= 0.01 * err64 and abs(l64 - leak64) <= 0.01 * leak64, (e64, l64)      # the stated figures are the float64 forms'
    cb, ch = bo.Combiner(1, k, ovs, p, gc), co.Channelizer(1, k, ovs, p, ga)
    w32 = run_cuts(cb, rows, [77, frames - 77])
    e32, l32 = figures(to_c(ch.process(w32)))
    assert e32 <= err64 * 1.01 + 1e-5 * amp and l32 <= leak64 * 1.01 + 1e-5 * amp, (e32, l32)
