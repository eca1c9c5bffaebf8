"""GPU: the signal-level meter and squelch (selenite_rx_set_meter, csrc/rx_meter.hip) against the numpy restatement of its law
(tests/meter_oracle.py, pinned to the reference's arm_power_f32 by tests/test_meter_oracle.py), by the twin method of tests/test_gpu_nr.py.

Three instances per case.  `rx` has the stage.  The stage's input is the un-scaled audio of a twin with stage and AGC off: the oracle chain
(SELENITE_ARITH_CMSIS / _FMA: bit-exact end to end) or a GPU instance (_SPLIT16 / _AUTO: the stage is bit-exact given its input); the
restatement runs on that and gives level, open, hold, opens, open_blocks and the gate of every block.  The expected output is the audio of a
twin with the AGC on and no stage, with the restatement's closed blocks zeroed.  After EVERY call the five state rows are compared as bits;
the audio is compared as bits; at the end the chain state, agc_gain with it, is compared as bits against the AGC-on twin.

int16 slots: both twins have f32 slots and are fed arm_q15_to_float of the words (the stage's route converts the input up front), the
expected words are nr_oracle.float_to_q15 of the AGC-on twin's audio with the closed blocks zeroed: equal as bits in _CMSIS and _FMA; in
_SPLIT16 and _AUTO within the project's int16 bar, 1 LSB + 1e-5 x the float block maximum x 32768 (the bar tests/test_gpu_iqc.py applies to
this route).  The stage state is compared as bits in every mode.

The input is bursts: low noise (1e-3) everywhere and, for 3 DSP blocks of every 7 (shifted from channel to channel), a tone of amplitude 0.5
inside the passband; FM: the tone ON the LO, which quiets the discriminator (SELENITE_RX_SQ_BELOW).  Where the calls are device calls
channel 1 gets one Inf sample; non-finite input is outside the parity contract of the chain (the kernels skip structural zeros, which changes
how NaN spreads), so that one channel's stage input is the GPU's own audio in every arith mode; and the AGC inside the fused kernels and
k_agc_generic, which finishes a call with the stage, part ways on non-finite audio (measured: the fused AGC's gain becomes NaN and stays, the
generic kernel's block maximum skips the NaN and its gain stays finite -- the NLMS route has had that difference all along), so that one
channel's expected audio and chain state come from a twin on the stage's own route (a meter with gate = 0), gated by the restatement.  Its
stage state is compared as bits like every other channel's: a NaN / Inf block leaves the level.  Every case asserts on the restatement's
trace that the run was neither all open nor all closed: at least one closed and one open block, two opens on some channel and a block kept
open by `hang`.  Levels and burst lengths were chosen with the restatement on the oracle chain's audio: a burst is a mean square of 0.1 to
0.5, the noise 1e-7, and with a decay of 15/16 the level falls below close_level (4e-3) in the second block behind a burst, is kept open one
block by hang = 1, and closes in the third."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import meter_oracle as mo
import nr_oracle as nro
import out_oracle as oo
import rxcommon as rc
import selenite_rx as sr

pytestmark = pytest.mark.gpu

EXACT = (rc.ARITH_CMSIS, rc.ARITH_FMA)
ARITHS = (rc.ARITH_CMSIS, rc.ARITH_FMA, rc.ARITH_SPLIT16, rc.ARITH_AUTO)
ARITH_IDS = ["cmsis", "fma", "split16", "auto"]
PAR = dict(sense=sr.SQ_ABOVE, gate=1, hang=1, attack=0.5, decay=0.9375, open_level=2e-2, close_level=4e-3, level_init=0.0)
FM_PAR = dict(sense=sr.SQ_BELOW, gate=1, hang=1, attack=0.5, decay=0.9375, open_level=1e-2, close_level=1e-1, level_init=1.0)
FIELDS = ("level", "open", "hold", "opens", "open_blocks")
INF_CH = 1


def spec_of(name, channels, arith, mode=None, **kw):
    s = rc.baseline_spec(name, channels, arith, **kw)
    if mode is not None:
        s.mode = mode
    return s


def to_q15(iq):
    return np.clip(np.trunc(iq * 32768.0), -32768, 32767).astype(np.int16)


def assert_bits(got, want, what=""):
    """bit for bit where `want` is finite (all of it, for integers); elsewhere the same NaN / Inf positions"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    u = {4: np.uint32, 2: np.uint16, 8: np.uint64, 1: np.uint8}[got.dtype.itemsize]
    ne = got.view(u) != want.view(u)
    if got.dtype.kind == "f":
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), what + ": NaN / Inf positions"
        ne &= np.isfinite(want)
    bad = np.argwhere(ne)
    if len(bad):
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def tone_of(spec):
    """cycles per input sample of the burst tone: inside the passband of the chain's mode"""
    lo = (spec.nco_step_all / 2.0 ** 32) if spec.nco else 0.0
    if spec.mode == sr.MODE_FM:
        return lo                                                      # on the LO: a quieted discriminator
    if spec.n_biquad:
        return lo + 500.0 / 48000.0                                     # the CW filter's centre
    off = 0.05 / spec.decim
    return lo - off if spec.mode in (sr.MODE_LSB, sr.MODE_CWR, sr.MODE_PKT) else lo + off


def bursts(spec, total, q15=False, inf=False, tone=None, seed=11):
    """[channels][total][2]: noise of 1e-3 and, in DSP blocks b with (b + 2 c) % 7 < 3, a tone of amplitude 0.5; inf: one Inf sample in channel 1"""
    ch = spec.channels
    rng = np.random.default_rng(seed)
    f = tone_of(spec) if tone is None else tone
    t = np.arange(total)
    on = ((t[None, :] // spec.block + 2 * np.arange(ch)[:, None]) % 7) < 3
    ph = 2.0 * np.pi * (f * t[None, :] + 0.37 * np.arange(ch)[:, None])
    x = rng.uniform(-1e-3, 1e-3, (ch, total, 2))
    x[..., 0] += 0.5 * on * np.cos(ph)
    x[..., 1] += 0.5 * on * np.sin(ph)
    x = x.astype(np.float32)
    if inf:
        assert not q15 and ch > INF_CH
        x[INF_CH, total // 2 + 5, 0] = np.inf
    return to_q15(x) if q15 else x


def run(rx, data, device=False, naninf_ok=False):
    """one process call on `data` (f32 or int16 I/Q, by its dtype) through the host-pointer or the device-pointer entry point"""
    q15 = data.dtype == np.int16
    if not device:
        assert not naninf_ok
        return rx.process_q15(data) if q15 else rx.process(data)
    ch, bs = data.shape[0], data.shape[1]
    vals = rx.out_len(bs)
    d_in, d_out = sr.DeviceBuffer(data.nbytes), sr.DeviceBuffer(ch * vals * data.dtype.itemsize)
    d_in.upload(np.ascontiguousarray(data))
    (rx.process_q15_device if q15 else rx.process_device)(d_in.ptr, d_out.ptr, bs)
    code = rx.L.selenite_rx_sync(rx.h)
    assert code == 0 or (naninf_ok and code == sr.NANINF), (code, rx.error())      # (an Inf input sample is NaN audio: that status is the chain's)
    out = d_out.download((ch, vals), data.dtype)
    d_in.free(); d_out.free()
    return out


def chain_state_equal(a, b, what=""):
    sa, sb = a.state(), b.state()
    for k in sa:
        assert_bits(sa[k], sb[k], what + " chain state." + k)


class Twins:
    """`rx` with the stage, the twin that gives the stage's input, the twin that gives the expected audio, and the restatement"""

    def __init__(self, spec, par=None, prepare=None, nlms=None, out=None, gpu_pre=False, inf=False):
        self.spec, self.par = spec, dict(PAR if par is None else par)
        self.na = spec.block // spec.decim
        self.rx, self.ref = sr.Rx(spec.config()), sr.Rx(spec.config())
        off = copy.copy(spec)
        off.agc, off.agc_global = False, False
        self.exact = spec.arith in EXACT and not gpu_pre
        self.pre = rc.CpuChain(off, "orc") if self.exact else sr.Rx(off.config())
        self.pre_inf = sr.Rx(off.config()) if self.exact and inf else None      # the Inf channel's stage input (INF_CH)
        self.ref_inf = sr.Rx(spec.config()) if inf else None                    # the Inf channel's audio and chain state: a meter alone, gate = 0
        self.nlms = None
        for r in (self.rx, self.ref) + (() if self.exact else (self.pre,)):
            if prepare:
                prepare(r)
            if nlms:
                r.set_nr(*nlms[:1], **nlms[1])
        if nlms and self.exact:
            self.nlms = (nro.Nlms(spec.channels, nlms[1]["num_taps"], nlms[1]["mu"], delay=nlms[1]["delay"]), nlms[0])
        self.out = None
        if out:                                                        # (interp, coeffs, frames): on rx alone; the expected frames come from out_oracle
            self.rx.set_out(*out)
            self.out = oo.OutStage(spec.channels, *out)
        self.rx.set_meter(**self.par)
        if self.ref_inf:
            self.ref_inf.set_meter(**dict(self.par, gate=0))
        self.orc = mo.Meter(spec.channels, self.na, **self.par)
        self.seen = dict(open=0, closed=0, kept=0)

    def stage_input(self, xf, device, naninf_ok=False):
        """the un-scaled audio in front of the AGC for the f32 input xf"""
        if self.exact:
            y = self.pre.process(xf)
            if self.pre_inf:
                y[INF_CH] = run(self.pre_inf, xf, True, True)[INF_CH]
            return self.nlms[0].process(y, self.nlms[1]) if self.nlms else y
        return run(self.pre, xf, device, naninf_ok)

    def note(self):
        tr = self.orc.trace
        self.seen["open"] += int(tr["open"].sum()); self.seen["closed"] += int((tr["open"] == 0).sum()); self.seen["kept"] += int(tr["kept"].sum())

    def expected(self, ref_audio, bits, q15):
        y = self.orc.gate_audio(ref_audio, bits)
        if self.out:
            return self.out.process(y, q15=q15, rounding=self.spec.q15_rounding)
        return nro.float_to_q15(y, self.spec.q15_rounding) if q15 else y

    def check_state(self, what=""):
        st, want = self.rx.meter_state(), self.orc.state()
        for k in FIELDS:
            assert_bits(st[k], want[k], "%s %s" % (what, k))

    def check_audio(self, got, want, ref_audio, what=""):
        if got.dtype == np.float32 or self.spec.arith in EXACT or self.out:      # (an output stage: the chain runs as an f32 call in both)
            return assert_bits(got, want, what)
        # _SPLIT16 / _AUTO, int16 words: the int16 bar, per DSP block
        ch = got.shape[0]
        mf = np.abs(ref_audio.astype(np.float64)).reshape(ch, -1, self.na).max(axis=2)
        allow = 1 + np.ceil(1e-5 * mf * 32768.0).astype(np.int64)
        dd = np.abs(got.astype(np.int32) - want.astype(np.int32)).reshape(ch, -1, self.na).max(axis=2)
        if (dd > allow).any():
            c, b = np.argwhere(dd > allow)[0]
            raise AssertionError("%s: channel %d block %d: %d LSB, %d allowed (float block maximum %.4g)" % (what, c, b, dd[c, b], allow[c, b], mf[c, b]))

    def call(self, data, device=False, naninf_ok=False, what=""):
        q15 = data.dtype == np.int16
        xf = data.astype(np.float32) / np.float32(32768.0) if q15 else data
        bits = self.orc.process(self.stage_input(xf, device or naninf_ok, naninf_ok))
        self.note()
        ref_audio = run(self.ref, xf, device or naninf_ok, naninf_ok)
        if self.ref_inf:
            ref_audio[INF_CH] = run(self.ref_inf, xf, True, True)[INF_CH]
        got = run(self.rx, data, device, naninf_ok)
        self.check_audio(got, self.expected(ref_audio, bits, q15), ref_audio, what + " audio")
        self.check_state(what)
        return got

    def finish(self, min_opens=2):
        if self.ref_inf:
            sa, sb, sc = self.rx.state(), self.ref.state(), self.ref_inf.state()
            for k in sa:
                sb[k][INF_CH] = sc[k][INF_CH]
                assert_bits(sa[k], sb[k], "chain state." + k)
        else:
            chain_state_equal(self.rx, self.ref)
        if self.out:
            assert_bits(self.rx.out_state(), self.out.state, "interpolator state")
        assert self.seen["open"] >= 1 and self.seen["closed"] >= 1 and self.seen["kept"] >= 1, self.seen
        assert self.orc.opens.max() >= min_opens, self.orc.opens


def stream(spec, cuts, par=None, q15=False, device=False, inf=False, **kw):
    tw = Twins(spec, par, inf=inf, **kw)
    x = bursts(spec, sum(cuts), q15, inf)
    at, audio = 0, []
    for i, bs in enumerate(cuts):
        dev = device if isinstance(device, bool) else device[i % len(device)]
        audio.append(tw.call(np.ascontiguousarray(x[:, at:at + bs]), dev or inf, inf, "call %d at %d" % (i, at)))
        at += bs
    tw.finish()
    return tw, np.concatenate(audio, axis=1)


# ---- the kernel's shapes: calls of 1, 2 and 16 blocks; 3 and 67 channels; every arith mode; both slot formats -------------------------------
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
@pytest.mark.parametrize("channels", [3, 67])
def test_cfg3_calls_of_1_2_and_16_blocks(channels, arith, q15):
    """cfg3's chain, block 256 / 4: k_meter<1>, <2> and <16> (64, 32 and 4 channels per wave: 67 channels leave a partial wave in each)"""
    spec = rc.baseline_spec("cfg3", channels, arith)
    stream(spec, [256, 512, 4096, 256, 512, 256], q15=q15, inf=not q15)


@pytest.mark.parametrize("calls", [[768, 96, 1536], [384, 2304]], ids=["8-1-16", "4-24"])
@pytest.mark.parametrize("arith", [rc.ARITH_CMSIS, rc.ARITH_AUTO], ids=["cmsis", "auto"])
def test_block_96_by_4_blocks_of_24_samples(arith, calls):
    """n = 24: not a power of two, the division by (float)n is a real one; calls of 8, 1, 16, 4 and 24 blocks (k_meter<8>, <1>, <16>, <4>, <32>)"""
    spec = rc.ChainSpec(67, 96, 4, 256, 63, 0, sr.MODE_USB, arith, nco=True, nco_step_all=0x01000000)
    stream(spec, calls, device=[True, False], inf=False)


@pytest.mark.parametrize("arith", [rc.ARITH_FMA, rc.ARITH_AUTO], ids=["fma", "auto"])
def test_cfg2_call_of_375_blocks(arith):
    """the no-decimator cfg2 chain, block 128 (n = 128: four passes of 32 samples per tile), one second per call at 2 channels: one channel per
    wave, five tiles of 64 blocks and one of 55"""
    spec = rc.baseline_spec("cfg2_48k128", 2, arith)
    stream(spec, [48000, 128 * 3], inf=True)


def test_call_cut_in_two_under_split16():
    """a call the dispatcher cuts (a whole pass and a tail): each part is a launch of its own with its own gate bytes, rows `out_stride` apart"""
    spec = rc.ChainSpec(35, 128, 4, 256, 63, 0, sr.MODE_USB, rc.ARITH_SPLIT16, nco=True, nco_step_all=0x01000000)
    for q15 in (False, True):
        stream(spec, [1152, 1408, 2176, 128], q15=q15, device=[True, False])


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("case", ["cw", "am", "fm", "generic"])
def test_cw_am_fm_and_the_generic_kernels(case, q15):
    if case == "cw":
        stream(rc.baseline_spec("cfg4", 35, rc.ARITH_CMSIS), [1024, 256, 2048], q15=q15, device=[False, True])
    elif case == "am":
        stream(spec_of("cfg3", 35, rc.ARITH_FMA, sr.MODE_AM), [1024, 256, 2048], q15=q15, device=[True, False])
    elif case == "fm":
        stream(spec_of("cfg3", 35, rc.ARITH_AUTO, sr.MODE_FM), [1024, 256, 2048, 2048], FM_PAR, q15=q15, device=[True, False])
    else:
        with sr.plan_option(sr.OPT_FORCE_GENERIC):
            stream(rc.baseline_spec("cfg3", 35, rc.ARITH_CMSIS), [1024, 256, 2048], q15=q15, device=[False, True])


# ---- combinations ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("arith", [rc.ARITH_CMSIS, rc.ARITH_AUTO], ids=["cmsis", "auto"])
def test_with_nlms(arith, q15):
    """the stage reads the audio behind NLMS"""
    spec = rc.baseline_spec("cfg3", 35, arith)
    stream(spec, [1024, 256, 2048, 1024], q15=q15, device=[False, True], nlms=(sr.NR_DENOISE, dict(num_taps=16, delay=8, mu=0.05)))


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("arith", [rc.ARITH_CMSIS, rc.ARITH_AUTO], ids=["cmsis", "auto"])
def test_with_the_output_stage(arith, q15):
    """the gate sits in front of the interpolator: the expected frames are out_oracle's on the gated audio of the twin without an output stage"""
    spec = rc.baseline_spec("cfg3", 35, arith)
    stream(spec, [1024, 256, 2048, 1024], q15=q15, device=[True, False], out=(4, sr.design_interp(32, 4, 0.1), sr.OUT_STEREO))


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_with_iqc_and_nb_in_front(q15):
    """I/Q correction and the blanker in front of the chain (each bit-exact by its own tests): the twins carry them too, on the GPU"""
    spec = rc.baseline_spec("cfg3", 35, rc.ARITH_AUTO)

    def prepare(r):
        r.set_iqc(64)
        r.set_nb(64)
    tw, _ = stream(spec, [1024, 256, 2048, 1024], q15=q15, device=[True, False], prepare=prepare)
    for k, v in tw.rx.iqc_state().items():
        assert_bits(v, tw.ref.iqc_state()[k], "iqc " + k)
    for k, v in tw.rx.nb_state().items():
        assert_bits(v, tw.ref.nb_state()[k], "nb " + k)


def test_gate_0_is_a_meter_only():
    spec = rc.baseline_spec("cfg3", 35, rc.ARITH_AUTO)
    for q15 in (False, True):
        tw, audio = stream(spec, [1024, 256, 2048], dict(PAR, gate=0), q15=q15, device=[True, False])
        assert tw.orc.open_blocks.sum() < 35 * 13 and np.count_nonzero(audio) > audio.size // 2      # closed blocks there were, and they left as they are


# ---- global gain: the one-call entries, selenite_rx_global_process_f32_device, the split pair -------------------------------------------
@pytest.mark.parametrize("arith", [rc.ARITH_CMSIS, rc.ARITH_AUTO], ids=["cmsis", "auto"])
def test_global_gain_every_entry(arith):
    ch, bs = 35, 1024
    spec = rc.baseline_spec("cfg3", ch, arith, agc_global=True)
    # the one-call entries on an agc_global instance, both slot formats
    stream(spec, [bs, 256, 2048], device=[True, False])
    stream(spec, [bs, 256, 2048], q15=True, device=[False, True])
    # phase 1 + phase 2 (the gate bytes live from one to the other), and selenite_rx_global_process_f32_device
    a, b = Twins(spec), Twins(spec)
    nout = bs // 4
    x = bursts(spec, 4 * bs)
    d_in, d_out, d_env = sr.DeviceBuffer(ch * bs * 8), sr.DeviceBuffer(ch * nout * 4), sr.DeviceBuffer(4 * (bs // 256))
    a.rx.L.selenite_rx_global_process_f32_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    for call in range(4):
        iq = np.ascontiguousarray(x[:, call * bs:(call + 1) * bs])
        for tw in (a, b):
            bits = tw.orc.process(tw.stage_input(iq, False))
            tw.note()
            want = tw.expected(tw.ref.process(iq), bits, False)
        d_in.upload(iq)
        a.rx.global_phase1(d_in.ptr, d_out.ptr, d_env.ptr, bs)
        a.rx.sync()
        a.check_state("behind phase 1 of call %d" % call)
        a.rx.global_phase2(d_out.ptr, d_env.ptr, bs)
        a.rx.sync()
        assert_bits(d_out.download((ch, nout), np.float32), want, "split calls, audio %d" % call)
        a.check_state("behind phase 2 of call %d" % call)
        assert b.rx.L.selenite_rx_global_process_f32_device(b.rx.h, d_in.ptr, d_out.ptr, bs, None) == 0
        b.rx.sync()
        assert_bits(d_out.download((ch, nout), np.float32), want, "one entry, audio %d" % call)
        b.check_state("one entry, call %d" % call)
    a.finish(); b.finish()
    d_in.free(); d_out.free(); d_env.free()


# ---- pointer kinds ----------------------------------------------------------------------------------------------------------------------
def host_chunks_body(q15):
    """300 channels x 2048 samples with a 1 MiB chunk: 64-channel chunks for f32 slots, 128-channel chunks for int16 slots, a ragged last one;
    the state rows and the gate bytes follow each chunk's first channel"""
    spec = rc.baseline_spec("cfg3", 300, rc.ARITH_AUTO)
    tw, _ = stream(spec, [2048, 2048, 256], q15=bool(q15), device=False)
    assert tw.orc.opens[299] >= 1 and tw.orc.opens[64] >= 1 and tw.orc.open_blocks[257] >= 1
    print("OK")


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_host_call_cut_into_channel_chunks(q15):
    """(a subprocess: the library reads SELENITE_RX_HOST_CHUNK_MB once)"""
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_meter as t; t.host_chunks_body(%d)" % (
        os.path.join(rc.ROOT, "tests"), rc.PKG_DIR, int(q15))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, SELENITE_RX_HOST_CHUNK_MB="1"))
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), (out.stdout[-1000:], out.stderr[-3000:])


def test_timing_calls_run_the_stage():
    ch, bs = 16, 1024
    spec = rc.baseline_spec("cfg3", ch, rc.ARITH_AUTO)
    tw = Twins(spec)
    iq, qi = bursts(spec, bs), bursts(spec, bs, q15=True, seed=12)
    d_in, d_q, d_out = sr.DeviceBuffer(iq.nbytes), sr.DeviceBuffer(qi.nbytes), sr.DeviceBuffer(ch * bs)
    d_in.upload(iq); d_q.upload(qi)
    tw.rx.time_process(d_in.ptr, d_out.ptr, bs, 3)
    tw.rx.time_process_each(d_in.ptr, d_out.ptr, bs, 2)
    tw.rx.sync()
    got = d_out.download((ch, bs // 4), np.float32)
    for _ in range(5):
        bits = tw.orc.process(tw.stage_input(iq, False))
        tw.note()
        want = tw.expected(tw.ref.process(iq), bits, False)
    assert_bits(got, want, "audio of the fifth run")
    tw.check_state("f32 timing calls")
    tw.rx.time_process_q15(d_q.ptr, d_out.ptr, bs, 2)
    tw.rx.time_process_each(d_q.ptr, d_out.ptr, bs, 1, q15=True)
    tw.rx.sync()
    qf = qi.astype(np.float32) / np.float32(32768.0)
    for _ in range(3):
        tw.orc.process(tw.stage_input(qf, False))
        tw.note()
        tw.ref.process(qf)
    tw.check_state("int16 timing calls")
    tw.finish()
    d_in.free(); d_q.free(); d_out.free()


# ---- state calls ------------------------------------------------------------------------------------------------------------------------
def test_state_round_trip_reset_and_set_mode():
    spec = rc.baseline_spec("cfg3", 35, rc.ARITH_CMSIS)
    cuts = [1024, 512, 1024, 768]
    x = bursts(spec, sum(cuts))
    a = Twins(spec)
    a.call(np.ascontiguousarray(x[:, :1024])); a.call(np.ascontiguousarray(x[:, 1024:1536]))
    st = a.rx.meter_state()
    assert st["level"].any() and st["opens"].any() and st["open"].any() and not st["open"].all()
    # a second instance continues the stream from the state rows
    b = sr.Rx(spec.config())
    b.set_meter(**PAR)
    b.set_meter_state(st)
    b.set_state(a.rx.state())
    iq = np.ascontiguousarray(x[:, 1536:2560])
    assert_bits(b.process(iq), a.call(iq), "after set_meter_state")
    for k, v in b.meter_state().items():
        assert_bits(v, a.orc.state()[k], "b " + k)
    # a partial view: hold alone
    hv = np.full(35, 3, np.uint32)
    b.set_meter_state(dict(hold=hv))
    st2 = b.meter_state()
    assert_bits(st2["hold"], hv); assert_bits(st2["level"], a.orc.level); assert_bits(st2["opens"], a.orc.opens)
    # set_mode keeps the state (and the stage goes on in the new mode)
    assert a.rx.set_mode(sr.MODE_LSB) == 0 and a.ref.set_mode(sr.MODE_LSB) == 0 and a.pre.set_mode(sr.MODE_LSB) == 0
    a.check_state("behind set_mode")
    a.call(np.ascontiguousarray(x[:, 2560:]), what="LSB")
    # the device rows are the state rows
    lv, op = np.empty(35, np.float32), np.empty(35, np.uint32)
    assert a.rx.meter_level_device() and a.rx.meter_open_device()
    a.rx.L.selenite_rx_memcpy_d2h(lv.ctypes.data_as(C.c_void_p), a.rx.meter_level_device(), lv.nbytes)
    a.rx.L.selenite_rx_memcpy_d2h(op.ctypes.data_as(C.c_void_p), a.rx.meter_open_device(), op.nbytes)
    assert_bits(lv, a.orc.level); assert_bits(op, a.orc.open)
    a.finish()
    # reset: back to the state set_meter left, the same stream gives the same audio again
    first = a.rx.meter_state()
    assert a.rx.reset() == 0
    s0 = a.rx.meter_state()
    assert (s0["level"] == np.float32(PAR["level_init"])).all() and not any(s0[k].any() for k in FIELDS[1:]) and first["opens"].any()
    c = Twins(spec)
    c.rx.set_mode(sr.MODE_LSB); c.ref.set_mode(sr.MODE_LSB); c.pre.set_mode(sr.MODE_LSB)
    iq = np.ascontiguousarray(x[:, :1024])
    assert_bits(a.rx.process(iq), c.call(iq), "behind reset")


GOOD = dict(sense=sr.SQ_ABOVE, gate=1, hang=3, attack=0.25, decay=0.125, open_level=1e-2, close_level=1e-3, level_init=0.5)
NAN, INF = float("nan"), float("inf")
BAD = [("struct_size", 32), ("sense", 2), ("gate", 2), ("hang", 65536), ("attack", 0.0), ("attack", 1.5), ("attack", -0.5), ("attack", NAN),
       ("decay", 0.0), ("decay", 1.0001), ("decay", NAN), ("open_level", -1.0), ("open_level", INF), ("open_level", NAN), ("close_level", -1.0),
       ("close_level", INF), ("close_level", NAN), ("close_level", 2e-2), ("level_init", -1.0), ("level_init", INF), ("level_init", NAN)]


def test_bad_fields_leave_a_working_stage_as_it_was():
    spec = rc.baseline_spec("cfg3", 20, rc.ARITH_CMSIS)
    x = bursts(spec, 3072)
    tw = Twins(spec)
    tw.call(np.ascontiguousarray(x[:, :1024]))
    for field, value in BAD + [("close_below", None)]:
        g = sr.MeterConfig()
        g.struct_size = C.sizeof(sr.MeterConfig)
        for k, v in GOOD.items():
            setattr(g, k, v)
        if field == "close_below":                                     # SELENITE_RX_SQ_BELOW: close_level below open_level
            g.sense, g.open_level, g.close_level = sr.SQ_BELOW, 1e-2, 1e-3
        else:
            setattr(g, field, value)
        assert tw.rx.L.selenite_rx_set_meter(tw.rx.h, C.byref(g)) == sr.ARGUMENT_ERROR, (field, value)
        assert tw.rx.status() == 0 and tw.rx.L.selenite_rx_error_string(None)
    tw.check_state("behind the refused calls")
    tw.call(np.ascontiguousarray(x[:, 1024:]), what="the call behind them")
    tw.finish()
    # the Python face keeps the stage on a refusal
    with pytest.raises(sr.RxError) as ei:
        tw.rx.set_meter(**dict(PAR, attack=2.0))
    assert ei.value.code == sr.ARGUMENT_ERROR
    tw.check_state("behind the Python face's refusal")
    # ... and the good one is taken, the edges of the ranges too
    tw.rx.set_meter(**GOOD)
    st = tw.rx.meter_state()
    assert (st["level"] == np.float32(0.5)).all() and not any(st[k].any() for k in FIELDS[1:])
    tw.rx.set_meter(sr.SQ_BELOW, gate=0, hang=65535, attack=1.0, decay=1.0, open_level=0.0, close_level=0.0, level_init=0.0)
    tw.rx.set_meter(sr.SQ_ABOVE, gate=1, hang=0, attack=1e-6, decay=1e-6, open_level=1.0, close_level=1.0, level_init=0.0)


@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
def test_set_meter_null_returns_the_call_to_the_parents_bits(arith):
    """an instance that had the stage, used it for a call, and dropped it, against one that never had it: audio and chain state.  (int16 slots
    in _SPLIT16 / _AUTO: the stage's call takes another route than the twin's, inside the int16 bar but not bit for bit, so there the stage is
    dropped before the first call.)"""
    for name, q15 in (("cfg3", False), ("cfg3", True), ("cfg4", True)):
        spec = rc.baseline_spec(name, 19, arith)
        a, b = sr.Rx(spec.config()), sr.Rx(spec.config())
        a.set_meter(**dict(PAR, gate=0))
        cuts, at = [1024, 256, 768], 0
        x = bursts(spec, sum(cuts), q15)
        for i, bs in enumerate(cuts):
            data = np.ascontiguousarray(x[:, at:at + bs])
            at += bs
            if i == 0 and (not q15 or arith in EXACT):
                assert_bits(run(a, data), run(b, data), "%s: a meter alone leaves the audio the twin's" % name)
                assert a.meter_state()["open_blocks"].any()
                a.set_meter(None)
                continue
            if i == 0:
                a.set_meter(None)
            if i <= 1:
                with pytest.raises(sr.RxError):
                    a.meter_state()
                v = sr.MeterStateView(None, None, None, None, None)
                assert a.L.selenite_rx_get_meter_state(a.h, C.byref(v)) == sr.ARGUMENT_ERROR
                assert a.L.selenite_rx_set_meter_state(a.h, C.byref(v)) == sr.ARGUMENT_ERROR
                assert a.meter_level_device() is None and a.meter_open_device() is None
            assert_bits(run(a, data, i % 2 == 1), run(b, data, i % 2 == 1), "%s call %d" % (name, i))
        chain_state_equal(a, b)


def test_other_setters_leave_the_stage_alone():
    spec = rc.baseline_spec("cfg3", 23, rc.ARITH_AUTO)
    tw = Twins(spec)
    h = sr.design_interp(16, 2, 0.2)
    steps = [lambda r: None, lambda r: r.set_spectrum(64), lambda r: r.set_nb(32), lambda r: r.set_iqc(64),
             lambda r: r.set_nr(sr.NR_NOTCH, num_taps=8, delay=4, mu=0.1), lambda r: r.set_mode(sr.MODE_LSB)]
    x = bursts(spec, 1024 * len(steps))
    for i, step in enumerate(steps):
        for r in (tw.rx, tw.ref, tw.pre):
            step(r)
        tw.check_state("behind step %d" % i)
        tw.call(np.ascontiguousarray(x[:, 1024 * i:1024 * (i + 1)]), device=i % 2 == 1, what="step %d" % i)
    tw.finish()
    before = tw.rx.meter_state()
    tw.rx.set_out(2, h, sr.OUT_MONO)
    for k, v in tw.rx.meter_state().items():
        assert_bits(v, before[k], "behind set_out " + k)
