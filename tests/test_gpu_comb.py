"""GPU: the polyphase combiner (include/selenite_comb.h, csrc/comb.hip) against the numpy restatement (tests/comb_oracle.py, pinned to the
reference's arm_cfft_f32 + arm_dot_prod_f32 + arm_float_to_q15 by tests/test_comb_oracle.py): outputs and history as bits, position as a
number; where the restatement is not finite, the same NaN / Inf positions.  Every compiled k_comb<K, Q, OVS, TOut> runs in
test_every_instantiation.  Edge values, errors, the chains with Tx and the channeliser and the headline geometry are in
tests/test_gpu_comb_edges.py."""
import numpy as np
import pytest

import comb_oracle as bo
import selenite_rx as sr

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25)
TAIL = 64                      # sentinel floats behind dst's end
RUN = 64                       # kCombRun: frames per workgroup
SHAPES = [(4, 1), (8, 1), (12, 1), (16, 1), (4, 2), (8, 2)]     # (P, oversample): Q = P * oversample <= 16


def assert_bits(got, want, what=""):
    """bit for bit where `want` is finite; elsewhere the same NaN / Inf positions"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() == want.tobytes():
        return
    assert got.dtype == np.float32, what + ": int16 output differs at %s" % np.argwhere(got != want)[0]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), what + ": NaN / Inf positions"
    ne = (got.view(np.uint32) != want.view(np.uint32)) & np.isfinite(want)
    bad = np.argwhere(ne)
    if len(bad):
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


_TAPS = {}


def taps(k, p, ovs):
    """the library's own design, one channel spacing wide, with 1 % of noise on top: no symmetry hides an index error"""
    if (k, p, ovs) not in _TAPS:
        rng = np.random.default_rng(1000 * k + 10 * p + ovs)
        _TAPS[(k, p, ovs)] = (sr.design_comb_prototype(k, p, 1.0, ovs) * (1.0 + 0.01 * rng.standard_normal(k * p))).astype(np.float32)
    return _TAPS[(k, p, ovs)]


def rows_in(nrows, frames, seed, level=1.0):
    """per row a slow tone of its own over noise, a few dB under full scale"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)
    x = 0.3 * rng.uniform(-1, 1, (nrows, frames, 2))
    f = ((np.arange(nrows) * 7) % 23 - 11)[:, None] / 230.0
    x[:, :, 0] += 0.4 * np.cos(2 * np.pi * f * t + np.arange(nrows)[:, None])
    x[:, :, 1] += 0.4 * np.sin(2 * np.pi * f * t + np.arange(nrows)[:, None])
    return (level * x).astype(np.float32)


class Pair:
    """the object and its restatement, fed the same calls"""

    def __init__(self, bands, k, ovs, p, bins=None, rounding=0, gpu=None):
        g = taps(k, p, ovs)
        self.gpu = gpu if gpu is not None else sr.Combiner(bands, k, ovs, p, g, bins, rounding)
        self.orc = bo.Combiner(bands, k, ovs, p, g, bins, rounding)
        self.bands, self.d = bands, k // ovs
        self.rows = bands * (k if bins is None else len(bins))

    def gpu_call(self, x, q15=False):
        """one call on the GPU alone; checks the sentinel behind dst's end"""
        nin = x.shape[1]
        n = self.gpu.out_len(nin)
        assert n == nin * self.d and self.gpu.in_channels() == self.rows == x.shape[0]
        vals = self.bands * n * 2
        dt = np.int16 if q15 else np.float32
        host = np.empty(vals * dt().itemsize + TAIL * 4, np.uint8)
        host[:vals * dt().itemsize].view(dt)[:] = 0x5A5A if q15 else SENTINEL
        host[vals * dt().itemsize:].view(np.float32)[:] = SENTINEL
        d_src, d_dst = sr.DeviceBuffer(x.nbytes), sr.DeviceBuffer(host.nbytes)
        d_src.upload(x)
        d_dst.upload(host)
        (self.gpu.process_q15_device if q15 else self.gpu.process_device)(d_src.ptr, d_dst.ptr, nin)
        self.gpu.sync()
        flat = d_dst.download((host.nbytes,), np.uint8)
        d_src.free(); d_dst.free()
        assert (flat[vals * dt().itemsize:].view(np.float32) == SENTINEL).all(), "the sentinel behind dst's end was overwritten"
        return flat[:vals * dt().itemsize].view(dt).reshape(self.bands, n, 2).copy()

    def call(self, x, what="", q15=False):
        got = self.gpu_call(x, q15)
        want = self.orc.process_q15(x) if q15 else self.orc.process(x)
        assert_bits(got, want, what + " output")
        self.check_state(what)
        return got

    def check_state(self, what=""):
        sg, so_ = self.gpu.state(), self.orc.state()
        assert_bits(sg["history"], so_["history"], what + " history")
        assert int(sg["position"][0]) == int(so_["position"][0]), what + " position"

    def close(self):
        self.gpu.close()


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("p,ovs", SHAPES)
@pytest.mark.parametrize("k", (64, 512))
def test_every_instantiation(k, p, ovs, q15):
    """K 64: 9 bands (a second workgroup with one live slot), K 512: 2 bands; one call of RUN + 16 + 1 frames: a full run, then a run of a full
    tile and a single-frame tile.  int16: both roundings, at a level where some samples saturate and most do not"""
    bands, frames = (9 if k == 64 else 2), RUN + 16 + 1
    x = rows_in(bands * k, frames, 21, 1.5 / np.sqrt(k) if q15 else 1.0)
    for rounding in ((0, 1) if q15 else (0,)):
        pr = Pair(bands, k, ovs, p, None, rounding)
        got = pr.call(x, "k%d p%d o%d r%d" % (k, p, ovs, rounding), q15)
        if q15:
            sat = (np.abs(got.astype(np.int32)) >= 32767).mean()
            assert 0 < sat < 0.25 and (got == 32767).any() and (got == -32768).any()
        pr.close()


@pytest.mark.parametrize("k,p,ovs", [(64, 8, 2), (512, 4, 2), (64, 12, 1), (512, 8, 2)])
def test_call_cuts_give_the_bits_of_one_call(k, p, ovs):
    """calls of [1, 2, RUN - 1, 17, 1] frames against one call (the odd totals start a later call on the other half-frame parity with oversample
    2), then [20, 3, 5, 56]: calls of 3 and 5 frames are shorter than the history of Q - 1 = 7 .. 15 and leave old samples mixed with new"""
    bands = 2
    total = 1 + 2 + (RUN - 1) + 17 + 1
    x = rows_in(bands * k, total, 22)
    one = Pair(bands, k, ovs, p)
    whole = one.call(x, "one call")
    one.close()
    for cuts in ([1, 2, RUN - 1, 17, 1], [20, 3, 5, 56]):
        assert sum(cuts) == total
        pr, at, outs = Pair(bands, k, ovs, p), 0, []
        for n in cuts:
            outs.append(pr.call(x[:, at:at + n], "cuts %s at %d" % (cuts, at)))
            at += n
        assert_bits(np.concatenate(outs, axis=1), whole, "cuts %s against one call" % cuts)
        pr.close()


@pytest.mark.parametrize("k,p,ovs,bands", [(64, 4, 2, 11), (512, 8, 1, 2), (64, 16, 1, 3)])
def test_bin_subsets_equal_the_all_bins_run_with_zero_rows(k, p, ovs, bands):
    """scattered bins, a single bin, bins in descending order; K 64 with 11 and 3 bands: waves with eight and with three live slots.  Bins
    nobody feeds contribute exactly nothing: the bits of the all-bins run whose other rows are +0.0f"""
    frames = 21
    rng = np.random.default_rng(6)
    subsets = ([int(v) for v in rng.permutation(k)[:k // 2 + 3]], [k - 3], list(range(k - 1, -1, -2)))
    for bins in subsets:
        x = rows_in(bands * len(bins), frames, 23 + len(bins))
        pr = Pair(bands, k, ovs, p, bins)
        got = pr.call(x[:, :9], "bins first")
        got = np.concatenate([got, pr.call(x[:, 9:], "bins second")], axis=1)
        pr.close()
        full = np.zeros((bands, k, frames, 2), np.float32)
        full[:, bins] = x.reshape(bands, len(bins), frames, 2)
        fp = Pair(bands, k, ovs, p)
        assert_bits(got, fp.gpu_call(full.reshape(bands * k, frames, 2)), "the all-bins run with zero rows")
        fp.close()


def test_state_moves_to_a_fresh_object_from_either_buffer_and_reset_equals_fresh():
    k, ovs, p, bands = 64, 2, 8, 3
    d = k // ovs
    x = rows_in(bands * k, 30, 24)
    a = Pair(bands, k, ovs, p)
    a.call(x[:, :7])
    cuts = [7, 18, 30]
    for i in (1, 2):                                            # behind one call and behind two: the state sits in either of the two buffers
        st = a.gpu.state()
        assert int(st["position"][0]) == cuts[i - 1] * d
        nxt = a.call(x[:, cuts[i - 1]:cuts[i]])
        b = sr.Combiner(bands, k, ovs, p, taps(k, p, ovs))
        b.set_state(st)
        pb = Pair(bands, k, ovs, p, gpu=b)
        assert_bits(pb.gpu_call(x[:, cuts[i - 1]:cuts[i]]), nxt, "the call behind set_state (%d)" % i)
        assert_bits(b.state()["history"], a.gpu.state()["history"], "history behind set_state")
        with pytest.raises(sr.RxError):
            b.set_state({"history": None, "position": np.array([d + 1], np.uint64)})      # not a multiple of D
        b.close()
    assert a.gpu.reset() == sr.SUCCESS
    a.orc.reset()
    a.check_state("after reset")
    a.call(x[:, :9], "after reset")
    a.close()


@pytest.mark.parametrize("k,p,ovs", [(64, 8, 2), (512, 4, 1)])
def test_set_state_with_a_position_past_2_to_the_32(k, p, ovs):
    """an odd frame index past 2^32 samples: with oversample 2 the call starts on the upper half"""
    bands, d = 2, k // ovs
    x = rows_in(bands * k, 19, 25)
    pr = Pair(bands, k, ovs, p)
    st = {"history": rows_in(bands * k, p * ovs - 1, 26), "position": np.array([(1 << 32) + 5 * d], np.uint64)}
    pr.gpu.set_state(st)
    pr.orc.set_state(st)
    pr.check_state("set_state")
    pr.call(x[:, :6], "first")
    pr.call(x[:, 6:], "second")
    assert int(pr.gpu.state()["position"][0]) == (1 << 32) + 24 * d
    pr.close()
