"""GPU: the polyphase combiner (include/selenite_comb.h, csrc/comb.hip) at its edges, bit for bit against tests/comb_oracle.py: edge values
(full scale with the int16 output saturating both ways in both roundings, denormals, -0.0f, Inf and NaN), refused calls, the chains
Tx -> Combiner and Combiner -> Channelizer on one stream with no host synchronisation between the launches, and the headline geometry with
sampled bands.  The instantiations, call cuts, bin subsets and the state are in tests/test_gpu_comb.py."""
import ctypes as C
import os

import numpy as np
import pytest

import chan_oracle as co
import comb_oracle as bo
import rxcommon as rc
import selenite_rx as sr
from test_gpu_comb import RUN, SENTINEL, TAIL, Pair, assert_bits, rows_in, taps

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k,p,ovs", [(64, 4, 1), (512, 4, 2)])
def test_edge_values(k, p, ovs):
    """a band each: -0.0f with a few +0.0f; 1e-38 (denormal inputs, transforms and products); +-1.0 on all K rows; an Inf and a NaN on one
    row; they pass through as the arithmetic gives them"""
    bands, frames = 5, 24
    x = rows_in(bands * k, frames, 31).reshape(bands, k, frames, 2)
    x[0] = -0.0
    x[0, ::3, ::7, 1] = 0.0
    x[1] *= np.float32(1e-38)
    x[2] = np.where(np.random.default_rng(32).random((k, frames, 2)) < 0.5, np.float32(-1.0), np.float32(1.0))
    x[3, 5, 7, 0] = np.inf
    x[3, 5, 15, 1] = np.nan
    x = x.reshape(bands * k, frames, 2)
    pr = Pair(bands, k, ovs, p)
    want = pr.orc.process(x[:, :11].copy())
    pr.orc.reset()
    assert not np.isfinite(want[3]).all() and np.isfinite(want[[0, 1, 2, 4]]).all()
    assert (want[0] == 0).all()
    tiny = np.abs(want[1])
    assert ((tiny > 0) & (tiny < np.finfo(np.float32).tiny)).any(), "no denormal output in the restatement"
    pr.call(x[:, :11], "first")
    pr.call(x[:, 11:], "second")
    pr.close()


@pytest.mark.parametrize("rounding", [0, 1])
@pytest.mark.parametrize("k,p,ovs", [(64, 8, 2), (512, 4, 1)])
def test_full_scale_on_every_row_saturates_int16_both_ways(k, p, ovs, rounding):
    """+1.0 on all K rows (K at every K-th output sample), -1.0 on all, random signs: arm_float_to_q15 saturates to 32767 and -32768"""
    bands, frames = 3, 20
    x = np.ones((bands, k, frames, 2), np.float32)
    x[1] = -1.0
    x[2] = np.where(np.random.default_rng(33).random((k, frames, 2)) < 0.5, np.float32(-1.0), np.float32(1.0))
    pr = Pair(bands, k, ovs, p, None, rounding)
    got = pr.call(x.reshape(bands * k, frames, 2), "full scale", q15=True)
    assert (got[0] == 32767).any() and (got[1] == -32768).any() and (got[2] == 32767).any() and (got[2] == -32768).any()
    pr.close()


@pytest.mark.parametrize("k,ovs", [(64, 2), (512, 1)])
def test_refused_calls_are_sticky_and_write_nothing(k, ovs):
    """blockSize 0, a blockSize past the launch's grid, NULL buffers: nothing launched, dst and state untouched, the first code stays"""
    p, bands, d, nin = 4, 1, k // ovs, 4
    n = bands * nin * d * 2 + TAIL
    d_src, d_dst = sr.DeviceBuffer(bands * k * nin * 8), sr.DeviceBuffer(n * 4)
    d_src.upload(rows_in(bands * k, nin, 34))
    d_dst.upload(np.full(n, SENTINEL, np.float32))
    a = sr.Combiner(bands, k, ovs, p, taps(k, p, ovs))
    for bad in (0, RUN * 65535 + 1, 0xFFFFFFFF):
        assert a.out_len(bad) == 0
        a.L.selenite_comb_process_f32_device(a.h, d_src.ptr, d_dst.ptr, bad)
        assert a.status() == sr.LENGTH_ERROR
        a.L.selenite_comb_process_q15_device(a.h, d_src.ptr, d_dst.ptr, bad)
    assert a.out_len(RUN * 65535) == (RUN * 65535 * d if RUN * 65535 * d < 2 ** 32 else 0)
    b = sr.Combiner(bands, k, ovs, p, taps(k, p, ovs))
    b.L.selenite_comb_process_f32_device(b.h, None, d_dst.ptr, nin)
    assert b.status() == sr.ARGUMENT_ERROR
    b.L.selenite_comb_process_q15_device(b.h, d_src.ptr, None, nin)
    b.L.selenite_comb_process_f32_device(b.h, d_src.ptr, d_dst.ptr, 0)
    assert b.status() == sr.ARGUMENT_ERROR                       # the first code stays
    for o in (a, b):
        o.L.selenite_comb_sync(o.h)
        st = o.state()
        assert int(st["position"][0]) == 0 and not st["history"].any()
    assert (d_dst.download((n,), np.float32) == SENTINEL).all(), "a refused call wrote to dst"
    with pytest.raises(sr.RxError) as e:
        a.process_device(d_src.ptr, d_dst.ptr, nin)             # sticky: a good call still reports it ...
    assert e.value.code == sr.LENGTH_ERROR
    a.L.selenite_comb_sync(a.h)
    assert int(a.state()["position"][0]) == nin * d             # ... and ran (the status is a report, not a lock)
    flat = d_dst.download((n,), np.float32)
    assert (flat[-TAIL:] == SENTINEL).all() and (flat[:-TAIL] != SENTINEL).all()
    for o in (a, b):
        o.close()
    for bf in (d_src, d_dst):
        bf.free()


def hip_stream():
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    st = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(st)) == 0
    return hip, st


def test_tx_into_the_combiner_on_one_stream():
    """an sr.Tx of 64 channels (block 64, interpolation by 4: 256 I/Q samples per channel and call) -> a Combiner of one band x K 64, oversample
    2, P 8, two calls, all four launches on one stream with no synchronisation between: the wideband stream equals the tx oracle into
    comb_oracle bit for bit"""
    k, p, ovs, nch, bs = 64, 8, 2, 64, 64
    hip, st = hip_stream()
    spec = rc.TxSpec(nch)
    tx, otx = sr.Tx(spec.config()), rc.TxCpuChain(spec, "orc")
    g = sr.design_comb_prototype(k, p, 1.0, ovs)
    cb, ocb = sr.Combiner(1, k, ovs, p, g), bo.Combiner(1, k, ovs, p, g)
    assert tx.L.selenite_tx_set_stream(tx.h, st) == 0 and cb.set_stream(st) == 0
    nin = bs * spec.interp
    audio = [rc.synth_audio(0, nch, j * bs, bs) for j in range(2)]
    d_a = [sr.DeviceBuffer(a.nbytes) for a in audio]
    d_iq = [sr.DeviceBuffer(nch * nin * 8) for _ in audio]
    d_w = [sr.DeviceBuffer(cb.out_len(nin) * 8) for _ in audio]
    for j, a in enumerate(audio):
        d_a[j].upload(a)
    for j in range(2):
        tx.process_device(d_a[j].ptr, d_iq[j].ptr, bs)
        cb.process_device(d_iq[j].ptr, d_w[j].ptr, nin)
    cb.sync(); tx.sync(); tx.check()
    for j in range(2):
        iq = otx.process(audio[j])
        assert rc.bits_equal(d_iq[j].download((nch, nin, 2), np.float32), iq), "Tx I/Q of call %d" % j
        assert_bits(d_w[j].download((1, nin * (k // ovs), 2), np.float32), ocb.process(iq), "wideband stream of call %d" % j)
    assert_bits(cb.state()["history"], ocb.state()["history"], "combiner history")
    tx.close(); cb.close()
    for bf in d_a + d_iq + d_w:
        bf.free()
    hip.hipStreamDestroy(st)


def test_combiner_into_the_channeliser_on_one_stream():
    """3 bands x K 64, P 8, oversample 2 on both sides: 192 rows -> 3 wideband streams -> 192 rows, two calls of 37 and 28 frames, on one stream
    with no synchronisation between: equals comb_oracle into chan_oracle bit for bit"""
    bands, k, p, ovs = 3, 64, 8, 2
    d = k // ovs
    hip, st = hip_stream()
    gc, ga = sr.design_comb_prototype(k, p, 1.0, ovs), sr.design_chan_prototype(k, p, 1.0)
    cb, ocb = sr.Combiner(bands, k, ovs, p, gc), bo.Combiner(bands, k, ovs, p, gc)
    ch, och = sr.Channelizer(bands, k, ovs, p, ga), co.Channelizer(bands, k, ovs, p, ga)
    assert cb.set_stream(st) == 0 and ch.set_stream(st) == 0
    x = rows_in(bands * k, 65, 35, 0.2)
    calls = [np.ascontiguousarray(x[:, :37]), np.ascontiguousarray(x[:, 37:])]
    d_x = [sr.DeviceBuffer(c.nbytes) for c in calls]
    d_w = [sr.DeviceBuffer(bands * c.shape[1] * d * 8) for c in calls]
    d_y = [sr.DeviceBuffer(c.nbytes) for c in calls]
    for j, c in enumerate(calls):
        d_x[j].upload(c)
    for j, c in enumerate(calls):
        cb.process_device(d_x[j].ptr, d_w[j].ptr, c.shape[1])
        ch.process_device(d_w[j].ptr, d_y[j].ptr, c.shape[1] * d)
    ch.sync(); cb.sync()
    for j, c in enumerate(calls):
        w = ocb.process(c)
        assert_bits(d_w[j].download(w.shape, np.float32), w, "wideband streams of call %d" % j)
        assert_bits(d_y[j].download(c.shape, np.float32), och.process(w), "channels of call %d" % j)
    cb.close(); ch.close()
    for bf in d_x + d_w + d_y:
        bf.free()
    hip.hipStreamDestroy(st)


def test_1024_bands_of_64_channels():
    """1024 bands x K 64 (128 workgroups of eight band slots), P 4, oversample 2, two calls of 9 and 4 frames: every band against the oracle"""
    bands, k, p, ovs = 1024, 64, 4, 2
    x = rows_in(bands * k, 13, 36)
    pr = Pair(bands, k, ovs, p)
    pr.call(x[:, :9], "9 frames")
    pr.call(x[:, 9:], "4 frames")
    pr.close()


def test_history_of_more_samples_than_the_history_kernels_grid_has_threads():
    """1024 bands x K 64 x Q 16: 65 536 rows x 15 = 983 040 history samples against k_comb_hist's grid of at most 2048 x 256 = 524 288 threads,
    so every thread forms two samples.  Calls of 20 and 3 frames (the second shorter than the history): the history of EVERY row is the newest
    15 input samples, and the output of the first and the last band equals the oracle's"""
    bands, k, p, ovs = 1024, 64, 8, 2
    q1 = p * ovs - 1
    assert bands * k * q1 > 2048 * 256
    x = rows_in(bands * k, 23, 38)
    g = taps(k, p, ovs)
    cb = sr.Combiner(bands, k, ovs, p, g)
    pr = Pair(bands, k, ovs, p, gpu=cb)
    got = [pr.gpu_call(x[:, :20]), pr.gpu_call(x[:, 20:])]
    st = cb.state()
    assert_bits(st["history"], x[:, 23 - q1:], "the history is the newest Q - 1 samples of every row")
    assert int(st["position"][0]) == 23 * (k // ovs)
    for b in (0, bands - 1):
        orc = bo.Combiner(1, k, ovs, p, g)
        want = [orc.process(x[b * k:(b + 1) * k, :20]), orc.process(x[b * k:(b + 1) * k, 20:])]
        for j in range(2):
            assert_bits(got[j][b:b + 1], want[j], "band %d call %d" % (b, j))
    cb.close()


def test_headline_geometry_with_sampled_bands():
    """128 bands x 512 bins (65 536 channel rows) x 2 RUN frames, P 8, oversample 2 (Q 16): the first, a middle and the last band against the
    oracle, f32 out; the history of the sampled bands"""
    bands, k, p, ovs, frames = 128, 512, 8, 2, 2 * RUN
    d, some = k // ovs, [0, 77, 127]
    rng = np.random.default_rng(37)
    x = rng.random((bands * k, frames, 2), np.float32)
    x -= np.float32(0.5)
    g = taps(k, p, ovs)
    cb = sr.Combiner(bands, k, ovs, p, g)
    n = bands * frames * d * 2
    d_src, d_dst = sr.DeviceBuffer(x.nbytes), sr.DeviceBuffer(n * 4 + TAIL * 4)
    d_src.upload(x)
    tail = np.full(TAIL, SENTINEL, np.float32)                  # (only the tail is checked: dst itself is written whole)
    assert sr.lib().selenite_rx_memcpy_h2d(d_dst.ptr + n * 4, tail.ctypes.data, tail.nbytes) == 0
    cb.process_device(d_src.ptr, d_dst.ptr, frames)
    cb.sync()
    flat = d_dst.download((n + TAIL,), np.float32)
    assert (flat[-TAIL:] == SENTINEL).all(), "the sentinel behind dst's end was overwritten"
    got = flat[:-TAIL].reshape(bands, frames * d, 2)
    hist = cb.state()["history"].reshape(bands, k, p * ovs - 1, 2)
    rows = x.reshape(bands, k, frames, 2)
    for b in some:
        orc = bo.Combiner(1, k, ovs, p, g)
        assert_bits(got[b:b + 1], orc.process(rows[b]), "band %d" % b)
        assert_bits(hist[b], orc.history, "history of band %d" % b)
    cb.close()
    d_src.free(); d_dst.free()
