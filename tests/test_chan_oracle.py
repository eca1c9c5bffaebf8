"""CPU: the numpy restatement of the polyphase channeliser (tests/chan_oracle.py) equals the composition of the reference's own functions
bit for bit (tests/golden/chan.npz: arm_dot_prod_f32 + arm_cfft_f32, outputs and history), does not depend on how the stream is cut into
calls, is the float64 direct form (mix, filter, decimate) to the project's 1e-5 bar, and does to a bin-centred tone what a channeliser must."""
import os

import numpy as np
import pytest

import chan_oracle as co
import rxcommon as rc
import selenite_rx as sr

GOLD = np.load(os.path.join(rc.ROOT, "tests", "golden", "chan.npz"))
TAGS = [str(t) for t in GOLD["names"]]


def case(tag):
    k, p, o = [int(s[1:]) for s in tag.split("_")]
    return k, p, o, GOLD[tag + "/coeffs"], GOLD[tag + "/stream"], GOLD[tag + "/out"], int(GOLD[tag + "/cut"])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def to_c(y):
    return y[..., 0].astype(np.float64) + 1j * y[..., 1].astype(np.float64)


def test_fixture_holds_the_cases_the_kernel_needs():
    assert TAGS == ["k64_p4_o1", "k64_p4_o2", "k512_p4_o2"]
    for tag in TAGS:
        k, p, o, g, x, want, cut = case(tag)
        assert g.shape == (k * p,) and x.shape[0] == want.shape[1] * (k // o) and 0 < cut < x.shape[0] and cut % (k // o) == 0
        ax = np.abs(x)
        assert ax.max() == 1.0 and ((ax > 0) & (ax < 1e-21)).any() and (np.signbit(x) & (x == 0)).any()      # full scale, 1e-22, -0.0f
        assert np.isfinite(want).all()
    assert os.path.getsize(os.path.join(rc.ROOT, "tests", "golden", "chan.npz")) <= os.path.getsize(os.path.join(rc.ROOT, "tests", "golden", "spectrum.npz"))


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_equals_the_reference_composition_bit_for_bit(tag):
    k, p, o, g, x, want, cut = case(tag)
    ch = co.Channelizer(1, k, o, p, g)
    got = np.concatenate([ch.process(x[None, :cut]), ch.process(x[None, cut:])], axis=1)
    assert np.array_equal(bits(got), bits(want))
    st = ch.state()
    assert np.array_equal(bits(st["history"][0]), bits(GOLD[tag + "/history"])) and int(st["position"][0]) == x.shape[0]


@pytest.mark.parametrize("tag", TAGS)
def test_cutting_the_stream_differently_gives_the_same_bits(tag):
    k, p, o, g, x, want, _ = case(tag)
    d, nout = k // o, want.shape[1]
    for cuts in ([nout], [1] * nout, [1, 2, nout - 8, 5], [nout - 1, 1]):
        ch = co.Channelizer(1, k, o, p, g)
        outs, at = [], 0
        for n in cuts:
            outs.append(ch.process(x[None, at * d:(at + n) * d]))
            at += n
        assert at == nout
        assert np.array_equal(bits(np.concatenate(outs, axis=1)), bits(want)), cuts
        assert np.array_equal(bits(ch.history[0]), bits(GOLD[tag + "/history"])), cuts


def test_int16_input_goes_through_q15_to_float_and_bands_and_bins_are_rows():
    k, p, o, g, x, want, cut = case("k64_p4_o2")
    q = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    xf = (q.astype(np.float32) / np.float32(32768.0))
    both = np.stack([q, q[::-1].copy()])
    bins = [7, 63, 7, 0]
    ch, ref0, ref1 = co.Channelizer(2, k, o, p, g, bins), co.Channelizer(1, k, o, p, g), co.Channelizer(1, k, o, p, g)
    got = ch.process(both)
    w0, w1 = ref0.process(xf[None]), ref1.process(xf[None, ::-1])
    assert got.shape == (8, x.shape[0] // (k // o), 2)
    assert np.array_equal(bits(got[:4]), bits(w0[bins])) and np.array_equal(bits(got[4:]), bits(w1[bins]))
    assert np.array_equal(bits(ch.history[0]), bits(xf[-ch.hlen:]))


@pytest.mark.parametrize("tag", TAGS)
def test_composition_is_the_float64_direct_form_to_1e_5(tag):
    """mix by e^(-2 pi i k n / K), filter by h, keep every D-th: first the reference composition itself (the fixture), then the restatement,
    every channel within 1e-5 of its own maximum (measured on these streams: 5.0e-7 at worst)"""
    k, p, o, g, x, want, cut = case(tag)
    ref = co.direct64(x, g, k, o)
    top = np.abs(ref).max(axis=1)
    assert (np.abs(to_c(want) - ref).max(axis=1) <= 1e-5 * top).all()
    got = co.Channelizer(1, k, o, p, g).process(x[None])
    assert (np.abs(to_c(got) - ref).max(axis=1) <= 1e-5 * top).all()


# The far-off-bin level of the float64 direct form with selenite_chan_design_prototype's taps, the largest |channel| over the bins two or
# more away from the tone relative to the tone's amplitude, once P * oversample outputs have passed (the window holds nothing but the tone):
#   K 64, P 8, oversample 1, width 1.0: -72.09 dB        K 64, P 8, oversample 2, width 2.0: -64.65 dB
# (the Hamming prototype's side lobes).  The f32 composition may be 3 dB above that.
@pytest.mark.parametrize("ovs,width,far_db", [(1, 1.0, -72.09), (2, 2.0, -64.65)])
def test_bin_centred_tone_leaves_its_channel_as_a_constant(ovs, width, far_db):
    k, p, kb = 64, 8, 5
    g = sr.design_chan_prototype(k, p, width)
    d, settle = k // ovs, p * ovs
    nout = settle + 12
    t = np.arange(nout * d)
    x = (0.5 * np.stack([np.cos(2 * np.pi * kb * t / k + 0.3), np.sin(2 * np.pi * kb * t / k + 0.3)], axis=1)).astype(np.float32)
    ch = co.Channelizer(1, k, ovs, p, g)
    y = to_c(np.concatenate([ch.process(x[None, :5 * d]), ch.process(x[None, 5 * d:])], axis=1))[:, settle:]      # (the second call starts rotated)
    # the prototype has unity DC gain: the tone's own channel is 0.5 e^(i 0.3), the same value at every output
    assert np.abs(np.abs(y[kb]) - 0.5).max() <= 1e-5 * 0.5
    assert np.abs(y[kb] - 0.5 * np.exp(0.3j)).max() <= 1e-5 * 0.5
    dist = np.minimum((np.arange(k) - kb) % k, (kb - np.arange(k)) % k)
    far = dist >= 2
    ref = co.direct64(x, g, k, ovs)[:, settle:]
    ref_db = 20 * np.log10(np.abs(ref[far]).max() / 0.5)
    assert abs(ref_db - far_db) <= 0.05, ref_db                  # the stated figure is the float64 form's
    assert 20 * np.log10(np.abs(y[far]).max() / 0.5) <= far_db + 3.0
