"""GPU: the polyphase channeliser (csrc/chan.hip) away from its first workgroup -- more bands than one K = 64 wave packs, bands and runs
together, the tile (16) and run (64) edges hit exactly, bin tables across a packed wave, state set on either history buffer, a position
past 2^32, the headline geometry (128 bands x 512 bins), more bands than a grid's y holds, and the hand-over into an Rx with a bin table and
oversample 2.  Every comparison is tests/test_gpu_chan.py's: output, history and position as bits against tests/chan_oracle.py, the
sentinel behind dst's end; the only tolerance is the project's own AUTO bar in the last test."""
import ctypes as C
import os

import numpy as np
import pytest

import chan_oracle as co
import rxcommon as rc
import selenite_rx as sr
from test_gpu_chan import Pair, assert_bits, stream

pytestmark = pytest.mark.gpu


# P rotates through 4 / 8 / 12 / 16 in both columns
PACKED = [(8, 1, 4), (8, 2, 16), (9, 1, 8), (9, 2, 4), (17, 1, 12), (17, 2, 8), (1024, 1, 16), (1024, 2, 12)]


@pytest.mark.parametrize("bands,ovs,p", PACKED)
def test_k64_band_packing_across_workgroups(bands, ovs, p):
    """K 64 packs eight bands into a wave: a full wave (8), a second workgroup with one live slot (9), a third (17), and 1024 bands x 64 bins,
    the K 64 way to 65 536 channels; every band has its own stream, so a band read or stored in another one's place shows"""
    k = 64
    nout = 3 if bands == 1024 else 19
    pr = Pair(bands, k, ovs, p)
    pr.call(stream(bands, nout * (k // ovs), 21), "%d bands o%d p%d" % (bands, ovs, p))
    pr.close()


def test_headline_geometry_k512():
    """128 bands x 512 bins = 65 536 rows, oversample 2, P 8, 5 outputs; then a table of 3 bins, one of them twice"""
    bands, k, ovs, p, nout = 128, 512, 2, 8, 5
    x = stream(bands, nout * (k // ovs), 22)
    full = Pair(bands, k, ovs, p)
    assert full.gpu.out_channels() == 65536
    whole = full.call(x, "all bins").reshape(bands, k, nout, 2)
    full.close()
    bins = [509, 2, 509]
    pr = Pair(bands, k, ovs, p, bins)
    got = pr.call(x, "3 bins").reshape(bands, len(bins), nout, 2)
    assert_bits(got, whole[:, bins], "rows of the all-bins run")
    pr.close()


def test_bands_and_runs_together_on_the_rotated_step():
    """K 64, oversample 2, 20 bands: one output (position mod K = K / 2), then 129: three workgroups in x by three runs in y; the 130 outputs
    equal those of one call on a second object"""
    bands, k, ovs, p = 20, 64, 2, 12
    d = k // ovs
    x = stream(bands, 130 * d, 23)
    pr = Pair(bands, k, ovs, p)
    first = pr.call(x[:, :d], "1 output")
    assert int(pr.gpu.state()["position"][0]) % k == k // 2
    rest = pr.call(x[:, d:], "129 outputs")
    pr.close()
    one = Pair(bands, k, ovs, p)
    whole = one.call(x, "130 outputs")
    one.close()
    assert_bits(np.concatenate([first, rest], axis=1), whole, "1 + 129 against one call")


@pytest.mark.parametrize("nout", [15, 16, 17, 63, 64, 65])
@pytest.mark.parametrize("bands,k,ovs,p", [(9, 64, 2, 4), (1, 512, 1, 4)])
def test_tile_and_run_edges(bands, k, ovs, p, nout):
    """a call that ends one output short of, on, and one past the tile of 16 and the run of 64; the second call starts from a history (and,
    with oversample 2 behind an odd length, on the rotated step)"""
    d = k // ovs
    x = stream(bands, 2 * nout * d, 24)
    pr = Pair(bands, k, ovs, p)
    pr.call(x[:, :nout * d], "first of %d" % nout)
    pr.call(x[:, nout * d:], "second of %d" % nout)
    pr.close()


def test_bin_tables_across_a_packed_wave():
    """K 64, 11 bands (the store loop leaves the second wave at slot 3), int16 input, two calls: tables of 1, 3 and 5 bins (fewer than, and no
    multiple of, the four rows a store instruction covers) and of 35 with a duplicate"""
    bands, k, ovs, p = 11, 64, 1, 8
    d, n1, n2 = k // ovs, 9, 12
    x = stream(bands, (n1 + n2) * d, 25, q15=True)
    full = Pair(bands, k, ovs, p)
    whole = np.concatenate([full.call(x[:, :n1 * d], "all bins, first"), full.call(x[:, n1 * d:], "all bins, second")], axis=1)
    whole = whole.reshape(bands, k, n1 + n2, 2)
    full.close()
    rng = np.random.default_rng(6)
    long = [int(v) for v in rng.permutation(k)[:35]]
    long[20] = long[2]                                           # a duplicate
    for bins in ([k - 1], [5, 0, 62], [7, 63, 1, 32, 31], long):
        pr = Pair(bands, k, ovs, p, bins)
        got = np.concatenate([pr.call(x[:, :n1 * d], "%d bins, first" % len(bins)), pr.call(x[:, n1 * d:], "%d bins, second" % len(bins))], axis=1)
        assert_bits(got.reshape(bands, len(bins), n1 + n2, 2), whole[:, bins], "%d bins: rows of the all-bins run" % len(bins))
        pr.close()


def test_set_state_replays_on_the_same_object():
    """the state lives in one of two buffers that swap per call: after three calls it is the second one.  state(), two more calls,
    set_state(saved) on the SAME object, the two calls again: same outputs, same final state"""
    bands, k, ovs, p = 3, 64, 2, 8
    d = k // ovs
    x = stream(bands, 20 * d, 26)
    pr = Pair(bands, k, ovs, p)
    at = 0
    for n in (3, 4, 2):                                          # 9 outputs: the rest runs on the rotated step
        pr.call(x[:, at * d:(at + n) * d], "call at %d" % at)
        at += n
    saved = pr.gpu.state()
    assert int(saved["position"][0]) == 9 * d
    a1, a2 = pr.call(x[:, 9 * d:14 * d], "fourth"), pr.call(x[:, 14 * d:], "fifth")
    end = pr.gpu.state()
    pr.gpu.set_state(saved)
    pr.orc.set_state(saved)
    pr.check_state("behind set_state")
    b1, b2 = pr.call(x[:, 9 * d:14 * d], "fourth again"), pr.call(x[:, 14 * d:], "fifth again")
    assert_bits(b1, a1, "fourth call replayed")
    assert_bits(b2, a2, "fifth call replayed")
    again = pr.gpu.state()
    assert_bits(again["history"], end["history"], "final history replayed")
    assert int(again["position"][0]) == int(end["position"][0]) == 20 * d
    pr.close()


def test_set_state_into_an_object_that_has_run():
    """A's state behind one call goes into B, which has made one call of another stream and length: both continue identically"""
    bands, k, ovs, p = 3, 64, 2, 8
    d = k // ovs
    x, y = stream(bands, 12 * d, 27), stream(bands, 4 * d, 28)
    a, b = Pair(bands, k, ovs, p), Pair(bands, k, ovs, p)
    a.call(x[:, :3 * d], "A first")
    b.call(y, "B first")
    st = a.gpu.state()
    b.gpu.set_state(st)
    b.orc.set_state(st)
    b.check_state("B behind set_state")
    for lo, hi in ((3, 8), (8, 12)):
        ga, gb = a.call(x[:, lo * d:hi * d], "A at %d" % lo), b.call(x[:, lo * d:hi * d], "B at %d" % lo)
        assert_bits(gb, ga, "B against A at %d" % lo)
    sa, sb = a.gpu.state(), b.gpu.state()
    assert_bits(sb["history"], sa["history"], "B's history against A's")
    assert int(sb["position"][0]) == int(sa["position"][0]) == 12 * d
    a.close(); b.close()


def test_position_past_32_bits():
    """K divides 2^32, so a position cut to 32 bits gives the same step; it shows in the position that is reported back"""
    bands, k, ovs, p = 3, 64, 2, 8
    d = k // ovs
    pr = Pair(bands, k, ovs, p)
    rng = np.random.default_rng(29)
    st = {"history": rng.uniform(-1, 1, (bands, k * p - d, 2)).astype(np.float32), "position": np.array([2 ** 32 + 3 * d], np.uint64)}
    pr.gpu.set_state(st)
    pr.orc.set_state(st)
    pr.check_state("behind set_state")
    x = stream(bands, 9 * d, 30)
    pr.call(x[:, :5 * d], "5 outputs")
    pr.call(x[:, 5 * d:], "4 outputs")
    assert int(pr.gpu.state()["position"][0]) == 2 ** 32 + 12 * d
    pr.close()


def test_more_bands_than_a_grid_has_rows():
    """65 539 bands x K 64 (P 4, oversample 1): the history kernel has the bands in its grid's y, which ends at 65 535, and is launched per
    slab of 32 768 bands.  Two calls (2 outputs, 1 output): status, output, the history of every band -- what that kernel writes -- and the
    position.  Every band has its own stream: stream()'s recipe, vectorised over the bands"""
    bands, k, ovs, p = 65539, 64, 1, 4
    rng = np.random.default_rng(31)
    L = 3 * k
    x = 0.3 * rng.uniform(-1, 1, (bands, L, 2))
    b = np.arange(bands)[:, None]
    ph = 2 * np.pi * ((3 + 7 * b) % 64) / 64.0 * np.arange(L)[None, :] + b
    x[:, :, 0] += 0.4 * np.cos(ph)
    x[:, :, 1] += 0.4 * np.sin(ph)
    x = x.astype(np.float32)
    pr = Pair(bands, k, ovs, p)
    pr.call(x[:, :2 * k], "2 outputs")
    assert pr.gpu.status() == sr.SUCCESS
    pr.call(x[:, 2 * k:], "1 output")
    assert pr.gpu.status() == sr.SUCCESS
    st = pr.gpu.state()
    assert int(st["position"][0]) == 3 * k
    assert_bits(st["history"], x[:, -(k * p - k):], "the history is the newest K P - D samples of every band")
    pr.close()


def test_into_the_rx_chain_with_a_bin_table_and_oversample_2():
    """2 bands x K 512 x oversample 2 x P 8, 40 bins per band -> 80 channels x 1024 samples as two calls of 512 -> an Rx of 80 channels (256-tap
    decimator by 4, 63-tap USB, AGC, DSP block 256), int16 wideband input, all four launches on one stream with no synchronisation between
    them: I/Q, audio and chain state equal chan_oracle -> rc.CpuChain bit for bit in SELENITE_ARITH_CMSIS, and AUTO is within its bar: per DSP
    block max |gpu - ref| <= 1e-5 max |ref|"""
    bands, k, ovs, p, nout, ncall = 2, 512, 2, 8, 512, 2
    d = k // ovs
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    st = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(st)) == 0
    rng = np.random.default_rng(32)
    bins = [int(v) for v in rng.permutation(k)[:40]]
    nch = bands * len(bins)
    L = ncall * nout * d
    t = np.arange(L)
    x = 0.02 * rng.uniform(-1, 1, (bands, L, 2))
    for c in range(nch):                                        # the recipe of test_into_the_rx_chain_on_one_stream; the channel rate is 2 fs / K
        bd, i = divmod(c, len(bins))
        f = (bins[i] + 2.0 * (0.05 + 0.1 * ((c * 7) % 10) / 10.0)) / k
        a = 0.01 * 10.0 ** (-2.0 * ((c * 5) % 8) / 8.0) * (8.0 if c % 9 == 0 else 1.0)
        x[bd, :, 0] += a * np.cos(2 * np.pi * f * t + c)
        x[bd, :, 1] += a * np.sin(2 * np.pi * f * t + c)
    assert np.abs(x).max() < 1.0
    x = np.trunc(x * 32768.0).astype(np.int16)
    calls = [np.ascontiguousarray(x[:, j * nout * d:(j + 1) * nout * d]) for j in range(ncall)]
    g = sr.design_chan_prototype(k, p, 2.0)
    och = co.Channelizer(bands, k, ovs, p, g, bins)
    want_iq = [och.process(xc) for xc in calls]
    for arith in (rc.ARITH_CMSIS, rc.ARITH_AUTO):
        spec = rc.ChainSpec(nch, 256, 4, 256, 63, 0, rc.MODE_USB, arith)
        orc = rc.CpuChain(rc.ChainSpec(nch, 256, 4, 256, 63, 0, rc.MODE_USB, rc.ARITH_CMSIS), "orc")
        want = [orc.process(w) for w in want_iq]
        ch, rx = sr.Channelizer(bands, k, ovs, p, g, bins), sr.Rx(spec.config())
        assert ch.out_channels() == nch and ch.out_len(nout * d) == nout
        assert ch.set_stream(st) == 0 and rx.set_stream(st) == 0
        d_x = [sr.DeviceBuffer(xc.nbytes) for xc in calls]
        d_iq = [sr.DeviceBuffer(nch * nout * 8) for _ in calls]
        d_audio = [sr.DeviceBuffer(nch * (nout // 4) * 4) for _ in calls]
        for j, xc in enumerate(calls):
            d_x[j].upload(xc)
        for j in range(ncall):
            ch.process_q15_device(d_x[j].ptr, d_iq[j].ptr, nout * d)
            rx.process_device(d_iq[j].ptr, d_audio[j].ptr, nout)
        rx.sync(); ch.sync()
        for j in range(ncall):
            got = d_audio[j].download((nch, nout // 4), np.float32)
            if arith == rc.ARITH_CMSIS:
                assert rc.bits_equal(d_iq[j].download((nch, nout, 2), np.float32), want_iq[j]), "I/Q of call %d" % j
                assert rc.bits_equal(got, want[j]), "audio of call %d off the oracle chain by %g" % (j, rc.rel_err(got, want[j]))
            else:
                dg = np.abs(got.astype(np.float64) - want[j]).reshape(nch, -1, 64).max(axis=2)
                m = np.abs(want[j].astype(np.float64)).reshape(nch, -1, 64).max(axis=2)
                assert (dg <= 1e-5 * m).all(), "AUTO off the CMSIS chain by %g of a block maximum in call %d" % ((dg / np.maximum(m, 1e-30)).max(), j)
        if arith == rc.ARITH_CMSIS:
            sg, so_ = rx.state(), orc.state()
            for name in so_:
                assert np.array_equal(sg[name], so_[name]) or rc.bits_equal(sg[name], so_[name]), name
            sc, sco = ch.state(), och.state()
            assert_bits(sc["history"], sco["history"], "channeliser history")
            assert int(sc["position"][0]) == int(sco["position"][0]) == L
        rx.close(); ch.close()
        for bf in d_x + d_iq + d_audio:
            bf.free()
    hip.hipStreamDestroy(st)
