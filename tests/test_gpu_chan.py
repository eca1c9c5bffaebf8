"""GPU: the polyphase channeliser (include/selenite_chan.h, csrc/chan.hip) against the numpy restatement (tests/chan_oracle.py, pinned to
the reference's arm_dot_prod_f32 + arm_cfft_f32 by tests/test_chan_oracle.py): outputs, history and position as bits; where the restatement
is not finite, the same NaN / Inf positions.  Every compiled k_chan<K, P, OVS, TIn> runs at least once: the 16 (K, P, OVS) in
test_every_instantiation_f32 and again in test_int16_input.  Band counts past the first workgroup, the tile and run edges, state on either
buffer and the headline geometry are in tests/test_gpu_chan_scale.py."""
import ctypes as C
import os

import numpy as np
import pytest

import chan_oracle as co
import rxcommon as rc
import selenite_rx as sr

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25)
TAIL = 64                      # sentinel floats behind dst's end


def assert_bits(got, want, what=""):
    """bit for bit where `want` is finite; elsewhere the same NaN / Inf positions"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), what + ": NaN / Inf positions"
    ne = (got.view(np.uint32) != want.view(np.uint32)) & np.isfinite(want)
    bad = np.argwhere(ne)
    if len(bad):
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


_TAPS = {}


def taps(k, p, ovs):
    """the library's own design, two channel spacings wide with oversample 2, with 1 % of noise on top: no symmetry hides an index error"""
    if (k, p, ovs) not in _TAPS:
        rng = np.random.default_rng(1000 * k + 10 * p + ovs)
        _TAPS[(k, p, ovs)] = (sr.design_chan_prototype(k, p, float(ovs)) * (1.0 + 0.01 * rng.standard_normal(k * p))).astype(np.float32)
    return _TAPS[(k, p, ovs)]


def stream(bands, length, seed, q15=False):
    """per band a tone on its own bin over noise, a few dB under full scale"""
    rng = np.random.default_rng(seed)
    t = np.arange(length)
    x = 0.3 * rng.uniform(-1, 1, (bands, length, 2))
    for b in range(bands):
        f = (3 + 7 * b) / 64.0
        x[b, :, 0] += 0.4 * np.cos(2 * np.pi * f * t + b)
        x[b, :, 1] += 0.4 * np.sin(2 * np.pi * f * t + b)
    if q15:
        return np.clip(np.trunc(x * 32768.0), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)


class Pair:
    """the object and its restatement, fed the same calls"""

    def __init__(self, bands, k, ovs, p, bins=None):
        g = taps(k, p, ovs)
        self.gpu, self.orc = sr.Channelizer(bands, k, ovs, p, g, bins), co.Channelizer(bands, k, ovs, p, g, bins)
        self.bands, self.d = bands, k // ovs
        self.rows = bands * (k if bins is None else len(bins))

    def gpu_call(self, x):
        """one call on the GPU alone; checks the sentinel behind dst's end"""
        q15 = x.dtype == np.int16
        L = x.shape[1]
        nout = self.gpu.out_len(L)
        assert nout == L // self.d and self.gpu.out_channels() == self.rows
        d_src, d_dst = sr.DeviceBuffer(x.nbytes), sr.DeviceBuffer(self.rows * nout * 8 + TAIL * 4)
        d_src.upload(x)
        d_dst.upload(np.full(self.rows * nout * 2 + TAIL, SENTINEL, np.float32))
        (self.gpu.process_q15_device if q15 else self.gpu.process_device)(d_src.ptr, d_dst.ptr, L)
        self.gpu.sync()
        flat = d_dst.download((self.rows * nout * 2 + TAIL,), np.float32)
        d_src.free(); d_dst.free()
        assert (flat[-TAIL:] == SENTINEL).all(), "the sentinel behind dst's end was overwritten"
        return flat[:-TAIL].reshape(self.rows, nout, 2)

    def call(self, x, what=""):
        got, want = self.gpu_call(x), self.orc.process(x)
        assert_bits(got, want, what + " output")
        self.check_state(what)
        return got

    def check_state(self, what=""):
        sg, so_ = self.gpu.state(), self.orc.state()
        assert_bits(sg["history"], so_["history"], what + " history")
        assert int(sg["position"][0]) == int(so_["position"][0]), what + " position"

    def close(self):
        self.gpu.close()


KS, PS, OVS = (64, 512), (4, 8, 12, 16), (1, 2)


@pytest.mark.parametrize("ovs", OVS)
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("k", KS)
def test_every_instantiation_f32(k, p, ovs):
    """3 bands at K 64 (a wave of eight transforms is left partly empty), 2 at K 512; one call of 37 outputs (no multiple of the tile of 16)"""
    bands = 3 if k == 64 else 2
    pr = Pair(bands, k, ovs, p)
    pr.call(stream(bands, 37 * (k // ovs), 11), "k%d p%d o%d" % (k, p, ovs))
    pr.close()


def int16_case(bands, k, ovs, p):
    pr = Pair(bands, k, ovs, p)
    x = stream(bands, 37 * (k // ovs), 12, q15=True)
    x[0, 5], x[bands - 1, -1] = (-32768, 32767), (-32768, -32768)
    pr.call(x[:, :20 * (k // ovs)], "first")
    pr.call(x[:, 20 * (k // ovs):], "second")                   # (the history holds converted samples)
    pr.close()


@pytest.mark.parametrize("k,ovs,p", [(k, ovs, p) for k in KS for ovs in OVS for p in PS])
def test_int16_input(k, ovs, p):
    """every k_chan<K, P, OVS, int16_t>: two full-scale samples, two calls"""
    int16_case(3 if k == 64 else 2, k, ovs, p)


def test_int16_input_nine_bands():
    """K 64: a full wave of eight bands and a second workgroup with one live slot"""
    int16_case(9, 64, 2, 12)


@pytest.mark.parametrize("ovs", OVS)
@pytest.mark.parametrize("k,p", [(64, 16), (512, 4)])
def test_call_cuts_give_the_bits_of_one_call(k, p, ovs):
    """104 outputs as one call and as 1 + 5 + 31 + 67 (with oversample 2 the odd lengths start the next call on the rotated step), then with the
    call that is shorter than the history last instead of first"""
    bands, d = 2, k // ovs
    x = stream(bands, 104 * d, 13)
    one = Pair(bands, k, ovs, p)
    whole = one.call(x, "one call")
    one.close()
    for cuts in ([1, 5, 31, 67], [67, 31, 5, 1]):
        assert d < k * p - d                                    # a call of one output is shorter than the history
        pr, at, outs = Pair(bands, k, ovs, p), 0, []
        for n in cuts:
            outs.append(pr.call(x[:, at * d:(at + n) * d], "cuts %s at %d" % (cuts, at)))
            at += n
        assert_bits(np.concatenate(outs, axis=1), whole, "cuts %s against one call" % cuts)
        pr.close()


@pytest.mark.parametrize("k,ovs,p", [(64, 2, 4), (512, 1, 8)])
def test_selected_bins_are_the_rows_of_the_all_bins_run(k, ovs, p):
    bands, d = 2, k // ovs
    x = stream(bands, 21 * d, 14)
    full = Pair(bands, k, ovs, p)
    whole = full.call(x).reshape(bands, k, 21, 2)
    full.close()
    rng = np.random.default_rng(5)
    some = [int(v) for v in rng.permutation(k)[:k // 2 + 3]]
    some[4] = some[1]                                            # a duplicate
    for bins in (some, [k - 1]):
        pr = Pair(bands, k, ovs, p, bins)
        got = pr.call(x, "bins").reshape(bands, len(bins), 21, 2)          # (gpu_call checks the sentinel behind the shorter dst)
        assert_bits(got, whole[:, bins], "rows of the all-bins run")
        pr.close()


def test_state_moves_to_a_fresh_object_and_reset_equals_fresh():
    k, ovs, p, bands = 64, 2, 8, 3
    d = k // ovs
    x = stream(bands, 30 * d, 15)
    a = Pair(bands, k, ovs, p)
    a.call(x[:, :7 * d]); a.call(x[:, 7 * d:18 * d])
    st = a.gpu.state()
    assert int(st["position"][0]) == 18 * d
    third = a.call(x[:, 18 * d:])
    b = sr.Channelizer(bands, k, ovs, p, taps(k, p, ovs))
    b.set_state(st)
    pb = Pair.__new__(Pair)
    pb.gpu, pb.bands, pb.d, pb.rows = b, bands, d, bands * k
    assert_bits(pb.gpu_call(x[:, 18 * d:]), third, "third call behind set_state")
    with pytest.raises(sr.RxError):
        b.set_state({"history": None, "position": np.array([d + 1], np.uint64)})      # not a multiple of D
    b.close()
    assert a.gpu.reset() == sr.SUCCESS
    a.orc.reset()
    a.check_state("after reset")
    a.call(x[:, :9 * d], "after reset")
    a.close()


@pytest.mark.parametrize("k,ovs,p", [(64, 1, 4), (512, 2, 8)])
def test_edge_values(k, ovs, p):
    """-0.0f, 1e-22 (denormal products with taps of 1e-3 and less), 1e18 and one Inf sample, a band each"""
    bands, d = 5, k // ovs
    L = 20 * d
    x = stream(bands, L, 16)
    x[0] = -0.0
    x[0, ::7, 1] = 0.0
    x[1] *= np.float32(1e-22)
    x[2] *= np.float32(1e18)
    x[3, L // 2 + 3, 0] = np.inf
    pr = Pair(bands, k, ovs, p)
    want = pr.orc.process(x[:, :11 * d].copy())
    pr.orc.reset()
    assert not np.isfinite(want[3 * k:4 * k]).all() and np.isfinite(want[:3 * k]).all()
    assert (np.signbit(want[:k]) & (want[:k] == 0)).any() or (want[:k] == 0).all()
    pr.call(x[:, :11 * d], "first")
    pr.call(x[:, 11 * d:], "second")
    pr.close()


def test_int16_minus_full_scale():
    k, ovs, p, bands = 64, 2, 16, 1
    x = np.full((bands, 40 * 32, 2), -32768, np.int16)
    x[0, ::3, 1] = 32767
    pr = Pair(bands, k, ovs, p)
    pr.call(x, "-32768")
    pr.close()


def test_several_units_of_work_per_band_and_launch():
    """5 bands x K 512 x 130 outputs: nine runs of the tile per band, the last one of two outputs"""
    pr = Pair(5, 512, 2, 8)
    pr.call(stream(5, 130 * 256, 17), "130 outputs")
    pr.close()


@pytest.mark.parametrize("k,ovs", [(64, 2), (512, 1)])
def test_bad_block_size_is_a_sticky_length_error_and_writes_nothing(k, ovs):
    d, p, bands = k // ovs, 4, 1
    ch = sr.Channelizer(bands, k, ovs, p, taps(k, p, ovs))
    n = 4 * k * 2 + TAIL
    d_src, d_dst = sr.DeviceBuffer(bands * 4 * d * 8), sr.DeviceBuffer(n * 4)
    d_src.upload(stream(bands, 4 * d, 18))
    d_dst.upload(np.full(n, SENTINEL, np.float32))
    for bad in (0, d - 1, d + 1, 3 * d + d // 2):
        assert ch.out_len(bad) == 0
        ch.L.selenite_chan_process_f32_device(ch.h, d_src.ptr, d_dst.ptr, bad)
        assert ch.status() == sr.LENGTH_ERROR
    with pytest.raises(sr.RxError) as e:
        ch.process_device(d_src.ptr, d_dst.ptr, 4 * d)          # sticky: a good call still reports it
    assert e.value.code == sr.LENGTH_ERROR
    ch.L.selenite_chan_sync(ch.h)
    st = ch.state()
    # the refused calls wrote nothing and moved nothing; the good call behind them ran (the status is a report, not a lock)
    assert int(st["position"][0]) == 4 * d
    ch2 = sr.Channelizer(bands, k, ovs, p, taps(k, p, ovs))
    d_dst2 = sr.DeviceBuffer(n * 4)
    d_dst2.upload(np.full(n, SENTINEL, np.float32))
    for bad in (d - 1, 3 * d + 1):
        ch2.L.selenite_chan_process_f32_device(ch2.h, d_src.ptr, d_dst2.ptr, bad)
    ch2.L.selenite_chan_sync(ch2.h)
    assert (d_dst2.download((n,), np.float32) == SENTINEL).all(), "a refused call wrote to dst"
    st2 = ch2.state()
    assert int(st2["position"][0]) == 0 and not st2["history"].any()
    for o in (ch, ch2):
        o.close()
    for b in (d_src, d_dst, d_dst2):
        b.free()


def test_into_the_rx_chain_on_one_stream():
    """one band -> 64 channels x 1024 samples -> an Rx of 64 channels (256-tap decimator by 4, 63-tap USB, AGC, DSP block 256), both on one
    stream with no synchronisation between them: audio and chain state equal chan_oracle -> rc.CpuChain bit for bit in SELENITE_ARITH_CMSIS,
    and AUTO is within its bar: per DSP block max |gpu - ref| <= 1e-5 max |ref|"""
    k, p, nout = 64, 8, 1024
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    st = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(st)) == 0
    rng = np.random.default_rng(19)
    t = np.arange(nout * k)
    x = 0.02 * rng.uniform(-1, 1, (1, nout * k, 2))
    for c in range(64):                                         # a carrier 300 .. 900 Hz-equivalents off every channel's centre, levels over 40 dB
        f = (c + (0.05 + 0.1 * ((c * 7) % 10) / 10.0)) / k
        a = 0.01 * 10.0 ** (-2.0 * ((c * 5) % 8) / 8.0) * (8.0 if c % 9 == 0 else 1.0)
        x[0, :, 0] += a * np.cos(2 * np.pi * f * t + c)
        x[0, :, 1] += a * np.sin(2 * np.pi * f * t + c)
    x = x.astype(np.float32)
    g = sr.design_chan_prototype(k, p, 1.0)
    want_iq = co.Channelizer(1, k, 1, p, g).process(x)
    for arith in (rc.ARITH_CMSIS, rc.ARITH_AUTO):
        spec = rc.ChainSpec(64, 256, 4, 256, 63, 0, rc.MODE_USB, arith)
        orc = rc.CpuChain(rc.ChainSpec(64, 256, 4, 256, 63, 0, rc.MODE_USB, rc.ARITH_CMSIS), "orc")
        want = orc.process(want_iq)
        ch, rx = sr.Channelizer(1, k, 1, p, g), sr.Rx(spec.config())
        assert ch.set_stream(st) == 0 and rx.set_stream(st) == 0
        d_x, d_iq, d_audio = sr.DeviceBuffer(x.nbytes), sr.DeviceBuffer(64 * nout * 8), sr.DeviceBuffer(64 * (nout // 4) * 4)
        d_x.upload(x)
        ch.process_device(d_x.ptr, d_iq.ptr, nout * k)
        rx.process_device(d_iq.ptr, d_audio.ptr, nout)
        rx.sync(); ch.sync()
        got = d_audio.download((64, nout // 4), np.float32)
        if arith == rc.ARITH_CMSIS:
            assert rc.bits_equal(d_iq.download((64, nout, 2), np.float32), want_iq)
            assert rc.bits_equal(got, want), "audio off the oracle chain by %g" % rc.rel_err(got, want)
            sg, so_ = rx.state(), orc.state()
            for name in so_:
                assert np.array_equal(sg[name], so_[name]) or rc.bits_equal(sg[name], so_[name]), name
        else:
            dg = np.abs(got.astype(np.float64) - want).reshape(64, -1, 64).max(axis=2)
            m = np.abs(want.astype(np.float64)).reshape(64, -1, 64).max(axis=2)
            assert (dg <= 1e-5 * m).all(), "AUTO off the CMSIS chain by %g of a block maximum" % (dg / np.maximum(m, 1e-30)).max()
        rx.close(); ch.close()
        for b in (d_x, d_iq, d_audio):
            b.free()
    hip.hipStreamDestroy(st)
