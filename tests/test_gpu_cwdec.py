"""GPU: the Morse decoder (selenite_rx_set_cwdec, csrc/rx_cwdec.hip: k_cwdec<B>) against the reference's arm_power_f32 and the second
statement of the law (tests/golden/cwdec.npz) and against the numpy restatement (tests/cwdec_oracle.py, pinned to that fixture by
tests/test_cwdec_oracle.py).  The stage is a tap: the restatement is fed the un-scaled audio -- the oracle chain's with its AGC off in
_CMSIS / _FMA (which the call's own audio must equal on bits), the library's own audio of the same call without the stage in _SPLIT16 /
_AUTO -- and every row of the state is compared on bits behind every call.  The input is the suite's synthetic I/Q under a per-channel
on / off envelope with edges off the block grid, so that marks, spaces, characters, blanks and the ring's wrap all happen."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import cwdec_oracle as co
import nr_oracle as nro
import rxcommon as rc
import selenite_rx as sr

pytestmark = pytest.mark.gpu

ARITHS = (rc.ARITH_CMSIS, rc.ARITH_FMA, rc.ARITH_SPLIT16, rc.ARITH_AUTO)
ARITH_IDS = ["cmsis", "fma", "split16", "auto"]
# fast timing for short streams: dits of 2 blocks from a unit of 2, a ring that wraps within a test
PAR = dict(peak_attack=0.5, peak_decay=0.01, floor_attack=0.25, floor_decay=0.01, on_frac=0.4, off_frac=0.25, snr=4.0, min_power=1e-12,
           debounce=1, adapt=1, track=1, unit_min=256, unit_init=2 * 256, unit_max=16 * 256, ring=16)
BLOCKS = (1, 3, 16, 64, 65, 130)          # per call: B = 1, 4, 16, 64, then two and three tiles


def to_q15(iq):
    return np.clip(np.trunc(iq * 32768.0), -32768, 32767).astype(np.int16)


def q15_to_f32(q):
    return q.astype(np.float32) / np.float32(32768.0)


def assert_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.itemsize]
        bad = np.argwhere(got.view(u) != want.view(u))
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def assert_state(rx, exp, what=""):
    got, want = rx.cwdec_state(), exp.state() if hasattr(exp, "state") else exp
    assert set(got) == set(want) == set(co.ROWS)
    for k in want:
        assert_bits(got[k], want[k], "%s: %s" % (what, k))


def run_device(rx, data, naninf_ok=False):
    q15 = data.dtype == np.int16
    ch, bs = data.shape[0], data.shape[1]
    vals = rx.out_len(bs)
    d_in, d_out = sr.DeviceBuffer(data.nbytes), sr.DeviceBuffer(ch * vals * data.dtype.itemsize)
    d_in.upload(np.ascontiguousarray(data))
    (rx.process_q15_device if q15 else rx.process_device)(d_in.ptr, d_out.ptr, bs)
    if naninf_ok:                            # (the stage itself never raises the flag; the chain may)
        assert rx.L.selenite_rx_sync(rx.h) in (sr.SUCCESS, sr.NANINF)
    else:
        rx.sync()
    out = d_out.download((ch, vals), data.dtype)
    d_in.free(); d_out.free()
    return out


def run(rx, data, device=False):
    if device:
        return run_device(rx, data)
    return rx.process_q15(data) if data.dtype == np.int16 else rx.process(data)


def no_agc(spec):
    s = copy.copy(spec)
    s.agc = False
    return s


def envelope(channels, first, count, block, seed=5):
    """the keying of `count` input samples from sample `first`: per channel marks of about 2 or 6 DSP blocks and spaces of about 2, 6 or 14,
    each a few per cent off and so with its edges off the block grid; 0.03 up, 1 down.  A pure function of (channel, sample)."""
    env = np.empty((channels, count), np.float32)
    for c in range(channels):
        rng = np.random.default_rng(1000 * seed + c)
        runs, total, down = [], 0, False
        while total < first + count:
            blocks = rng.choice([2, 6]) if down else rng.choice([2, 2, 6, 6, 14])
            n = max(1, int(blocks * block * rng.uniform(0.9, 1.1)))
            runs.append(np.full(n, 1.0 if down else 0.03, np.float32))
            total += n
            down = not down
        env[c] = np.concatenate(runs)[first:first + count]
    return env


def keyed_iq(channels, first, count, block, seed=5):
    return rc.synth_iq(0, channels, first, count) * envelope(channels, first, count, block, seed)[:, :, None]


class Tap:
    """An instance of `spec` (AGC off) with the decoder, an instance without it, the restatement, and in _CMSIS / _FMA the oracle chain:
    call() runs one call everywhere and compares the audio and every row of the stage's state on bits."""

    def __init__(self, spec, par=PAR):
        assert not spec.agc
        self.spec = spec
        self.a, self.b = sr.Rx(spec.config()), sr.Rx(spec.config())
        self.a.set_cwdec(**par)
        self.exp = co.CwDec(spec.channels, spec.block // spec.decim, **par)
        self.orc = rc.CpuChain(spec, "orc") if spec.arith in (rc.ARITH_CMSIS, rc.ARITH_FMA) else None
        self.at = 0

    def call(self, bs, device=False, q15=False):
        iq = keyed_iq(self.spec.channels, self.at, bs, self.spec.block)
        what = "call at %d" % self.at
        if q15:
            qi = to_q15(iq)
            pre = run(self.b, q15_to_f32(qi), device)             # the un-scaled f32 audio of the int16 slot
            assert_bits(run(self.a, qi, device), nro.float_to_q15(pre, self.spec.q15_rounding), what + ": int16 audio")
            iq = q15_to_f32(qi)
        else:
            pre = run(self.b, iq, device)
            assert_bits(run(self.a, iq, device), pre, what + ": the tap changes no audio")
        if self.orc is not None:
            assert_bits(pre, self.orc.process(iq), what + ": oracle chain")
        self.exp.process(pre)
        self.at += bs
        assert_state(self.a, self.exp, what)
        return pre


def generic_spec(ch, n, arith=rc.ARITH_CMSIS):
    """a chain on the generic kernels whose DSP block is n audio samples"""
    if n in (24, 32):
        return rc.ChainSpec(ch, 4 * n, 4, 64, 31, 0, sr.MODE_USB, arith, nco=True, nco_step_all=0x01000000, agc=False)
    return rc.ChainSpec(ch, n, 1, 0, 31, 0, sr.MODE_USB, arith, agc=False)


# ---- 4. the fixture's vectors through the library ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(rc.GOLDEN_DIR, "cwdec.npz")) as z:
        return {k: z[k] for k in z.files}


def gold_par(g):
    return {k[4:]: (float(g[k]) if g[k].dtype == np.float32 else int(g[k])) for k in g if k.startswith("par/")}


def test_golden_vectors_through_the_library(gold):
    """an instance whose chain passes the I rail through (no NCO, no decimator, no FIR pair, AGC off, DSP block n): the fixture's streams go
    in as I, in the fixture's calls; behind every call every row equals the fixture's -- the NaN and the Inf block of channel 2 included"""
    n = int(gold["n"])
    spec = rc.ChainSpec(3, n, 1, 0, 0, 0, sr.MODE_USB, rc.ARITH_CMSIS, agc=False)
    rx = sr.Rx(spec.config())
    rx.set_cwdec(table=gold["table"], **gold_par(gold))
    at = 0
    for i, nb in enumerate(int(v) for v in gold["lens"]):
        x = gold["x"][:, at * n:(at + nb) * n]
        iq = np.zeros((3, nb * n, 2), np.float32)
        iq[..., 0] = x
        got = run_device(rx, iq, naninf_ok=True)
        assert got.view(np.uint32).tobytes() == x.view(np.uint32).tobytes(), "the chain does not pass the I rail through as it is"
        at += nb
        st = rx.cwdec_state()
        for k in st:
            assert_bits(st[k], gold["call/" + k][i], "%s behind call %d" % (k, i))
    assert [rx.cw_text(c).rstrip() for c in range(2)] == [str(s) for s in gold["sent"]]
    assert rx.cw_text() == [rx.cw_text(c) for c in range(3)]


# ---- 5. lane-plan shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 5, 17, 67])
@pytest.mark.parametrize("n", [24, 32, 33, 64, 128])
def test_blocks_per_call_by_block_length_by_channels(n, ch):
    """calls of 1, 3, 16, 64, 65 and 130 DSP blocks (B = 1, 4, 16, 64, two tiles, three tiles with the integers carried in registers) of
    n = 24 (no power of two), 32 (one full LDS pass), 33 (a second pass of one sample), 64 and 128 samples, over 1, 5, 17 and 67 channels
    (partial groups at every B, a partial last wave); device and host entries alternate"""
    t = Tap(generic_spec(ch, n))
    for i, blocks in enumerate(BLOCKS):
        t.call(t.spec.block * blocks, device=i % 2 == 0)
    st = t.exp.state()
    if ch >= 5:
        assert st["count"].max() > PAR["ring"] and (st["unit"] != PAR["unit_init"]).any() and st["text"].any()


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
@pytest.mark.parametrize("name", ["cfg3", "cfg4"])
def test_fused_shapes_arith_modes_and_slot_formats(name, arith, q15):
    """the fused SSB and CW kernels with their own AGC off in front of the stage: n = 64 and 256, calls of 4, 1, 16 and 5 blocks"""
    spec = no_agc(rc.baseline_spec(name, 70, arith))
    t = Tap(spec)
    for i, blocks in enumerate((4, 1, 16, 5)):
        t.call(spec.block * blocks, device=i % 2 == 1, q15=q15)
    assert (t.exp.unit != PAR["unit_init"]).any()                            # marks have ended


def test_modes_am_and_fm():
    for mode in (sr.MODE_AM, sr.MODE_FM):
        spec = no_agc(rc.baseline_spec("cfg1", 33, rc.ARITH_CMSIS))
        spec.mode = mode
        t = Tap(spec)
        for bs in (512, 256, 768):
            t.call(bs)


# ---- 6. cut invariance --------------------------------------------------------------------------------------------------------------------------
def test_one_call_equals_calls_of_1_7_and_64_blocks():
    ch, n, total = 19, 24, 130
    spec = generic_spec(ch, n)
    iq = keyed_iq(ch, 0, total * spec.block, spec.block)
    one = sr.Rx(spec.config())
    one.set_cwdec(**PAR)
    whole = run_device(one, iq)
    want = one.cwdec_state()
    assert want["count"].max() > 4 and want["text"].any()
    for cut in (1, 7, 64):
        rx = sr.Rx(spec.config())
        rx.set_cwdec(**PAR)
        for a in range(0, total, cut):
            b = min(a + cut, total)
            part = run_device(rx, np.ascontiguousarray(iq[:, a * spec.block:b * spec.block]))
            assert_bits(part, whole[:, a * n:b * n], "audio of blocks %d .. %d" % (a, b))
        assert_state(rx, want, "calls of %d blocks" % cut)


# ---- 7. life cycle ------------------------------------------------------------------------------------------------------------------------------
def test_state_round_trip_mid_character_reset_and_the_other_setters():
    ch = 33
    spec = generic_spec(ch, 64)
    rx, fresh = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (rx, fresh):
        r.set_cwdec(**PAR)
    exp = co.CwDec(ch, 64, **PAR)
    assert_state(rx, exp, "behind set_cwdec")
    s0 = rx.cwdec_state()
    assert not np.signbit(s0["peak"]).any() and (s0["code"] == 1).all() and (s0["unit"] == PAR["unit_init"]).all() and not s0["text"].any()
    first = keyed_iq(ch, 0, 41 * 64, 64)
    rx.process(first)
    st, g = rx.cwdec_state(), rx.state()
    assert (st["code"] > 1).any() and st["key"].any()      # some channel stands inside a character
    nxt = keyed_iq(ch, 41 * 64, 50 * 64, 64)
    rx.process(nxt)
    fresh.set_state(g)
    fresh.set_cwdec_state(st)
    fresh.process(nxt)
    a = rx.cwdec_state()
    assert_state(fresh, a, "after set_cwdec_state")
    assert a["count"].any()
    # set_mode and the other setters keep the state, the parameters and the table
    assert rx.set_mode(sr.MODE_LSB) == 0
    rx.set_nr(sr.NR_NOTCH, num_taps=16, delay=4, mu=0.1); rx.set_nr(sr.NR_OFF)
    rx.set_meter(); rx.set_meter(sense=None)
    rx.set_afilt(sr.design_deemphasis(0.9)); rx.set_afilt(None)
    rx.set_tones(sr.design_tones([0.1])); rx.set_tones(None)
    rx.set_out(4, sr.design_interp(32, 4, 0.1), sr.OUT_STEREO); rx.set_out(None)
    rx.set_spectrum(64); rx.set_spectrum(None)
    rx.set_nb(); rx.set_nb(None)
    rx.set_iqc(); rx.set_iqc(None)
    assert_state(rx, a, "behind the other setters")
    # reset: back to the state set_cwdec left; the same stream gives the same rows again
    assert rx.reset() == 0
    assert_state(rx, exp, "behind reset")
    rx.set_mode(sr.MODE_USB)
    rx.process(first)
    assert_state(rx, st, "the same stream behind reset")


BAD = [("struct_size", 68), ("peak_attack", 0.0), ("peak_attack", 1.5), ("peak_decay", float("nan")), ("peak_decay", -0.1),
       ("floor_attack", float("inf")), ("floor_attack", 0.0), ("floor_decay", 0.0), ("floor_decay", 2.0), ("on_frac", 1.0), ("on_frac", 0.2),
       ("on_frac", float("nan")), ("off_frac", 0.0), ("off_frac", 0.5), ("off_frac", float("nan")), ("snr", 0.5), ("snr", float("nan")),
       ("snr", float("inf")), ("min_power", -1.0), ("min_power", float("inf")), ("min_power", float("nan")), ("debounce", 0), ("debounce", 256),
       ("adapt", 2), ("track", 9), ("unit_min", 255), ("unit_min", 11 * 256), ("unit_init", 65 * 256), ("unit_max", 256),
       ("unit_max", 8192 * 256 + 1), ("ring", 8), ("ring", 24), ("ring", 0), ("ring", 131072)]


@pytest.mark.parametrize("field,value", BAD, ids=["%s=%s" % b for b in BAD])
def test_bad_field_is_argument_error_and_the_stage_stays(field, value):
    ch = 16
    spec = generic_spec(ch, 64)
    rx, ref = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (rx, ref):
        r.set_cwdec(**PAR)
    iq = keyed_iq(ch, 0, 20 * 64, 64)
    rx.process(iq); ref.process(iq)
    g = sr.CwdecConfig()
    g.struct_size = C.sizeof(sr.CwdecConfig)
    for k, v in dict(sr.CWDEC_DEFAULTS, ring=64).items():                    # another, valid configuration ...
        setattr(g, k, v)
    assert g.off_frac == np.float32(0.25) and g.on_frac == np.float32(0.4) and g.unit_min == 512 and g.unit_init == 2560 and g.unit_max == 16384
    setattr(g, field, value)                                                 # ... with one bad field
    assert rx.L.selenite_rx_set_cwdec(rx.h, C.byref(g)) == sr.ARGUMENT_ERROR
    assert rx.status() == 0 and rx.L.selenite_rx_error_string(None).decode().startswith("selenite_rx_set_cwdec: ")
    iq = keyed_iq(ch, 20 * 64, 30 * 64, 64)
    rx.process(iq); ref.process(iq)
    assert_state(rx, ref.cwdec_state(), "after the refused set_cwdec")
    assert ref.cwdec_state()["count"].any()
    with pytest.raises(sr.RxError):
        rx.set_cwdec(**{field: value} if field != "struct_size" else {"ring": 3})
    assert_state(rx, ref.cwdec_state(), "after the refused Rx.set_cwdec")


@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
def test_stage_removed_is_no_stage(arith):
    spec = rc.baseline_spec("cfg3", 70, arith)
    a, b = sr.Rx(spec.config()), sr.Rx(spec.config())
    a.set_cwdec(**PAR)
    assert a.cwdec_text_device() and a.cwdec_count_device() and a.cwdec_unit_device()
    a.set_cwdec(None)
    for call in range(2):
        iq = rc.synth_iq(0, 70, call * 2048, 2048)
        assert_bits(a.process(iq), b.process(iq), "call %d" % call)
    with pytest.raises(sr.RxError):
        a.cwdec_state()
    with pytest.raises(sr.RxError):
        a.cw_text(0)
    assert a.L.selenite_rx_get_cwdec_state(a.h, C.byref(sr.CwdecStateView())) == sr.ARGUMENT_ERROR
    assert a.L.selenite_rx_set_cwdec_state(a.h, C.byref(sr.CwdecStateView())) == sr.ARGUMENT_ERROR
    assert a.L.selenite_rx_get_cwdec(a.h, None, None, None, None) == sr.ARGUMENT_ERROR
    assert a.cwdec_text_device() is None and a.cwdec_count_device() is None and a.cwdec_unit_device() is None


# ---- 8. with the other stages on ----------------------------------------------------------------------------------------------------------------
def neighbours(r):
    r.set_tones(sr.design_tones([0.05, 0.11, 0.2]), frame_blocks=3, confirm=2, release=2, ratio=0.02, min_power=1e-6)
    r.set_afilt(sr.design_biquad(sr.BIQUAD_HIGHPASS, 300.0 / 12000.0, 0.7071).reshape(1, 5))
    r.set_nr(sr.NR_DENOISE, num_taps=16, delay=8, mu=0.05)
    r.set_meter(sense=sr.SQ_ABOVE, gate=1, hang=1, attack=0.5, decay=0.9375, open_level=2e-2, close_level=4e-3, level_init=0.0)


def neighbour_states(r):
    return (("chain", r.state()), ("tones", r.tones_state()), ("afilt", r.afilt_state()), ("nr", r.nr_state()), ("meter", r.meter_state()))


def test_with_tones_afilt_nlms_and_the_gated_meter_on():
    """the decoder's rows are those of the decoder alone (and of the restatement fed the audio in front of the filter); audio, chain state and
    the four other stages' rows are those of the same calls without it"""
    ch = 35
    spec = rc.baseline_spec("cfg3", ch, rc.ARITH_CMSIS)
    a, b, alone = sr.Rx(spec.config()), sr.Rx(spec.config()), sr.Rx(spec.config())
    neighbours(a); neighbours(b)
    a.set_cwdec(**PAR); alone.set_cwdec(**PAR)
    orc, exp = rc.CpuChain(no_agc(spec), "orc"), co.CwDec(ch, 64, **PAR)
    at = 0
    for i, bs in enumerate((1024, 256, 4096, 2048)):
        iq = keyed_iq(ch, at, bs, spec.block)
        assert_bits(run(a, iq, device=i == 1), run(b, iq, device=i == 1), "call %d" % i)
        run(alone, iq)
        exp.process(orc.process(iq))
        assert_state(a, exp, "call %d" % i)
        assert_state(alone, exp, "call %d, the decoder alone" % i)
        at += bs
    assert exp.count.any()
    for (name, sa), (_, sb) in zip(neighbour_states(a), neighbour_states(b)):
        for k in sa:
            assert_bits(np.asarray(sa[k]), np.asarray(sb[k]), "%s state: %s" % (name, k))


def test_global_gain_one_call_and_the_two_phases():
    """phase 1 runs the stage, phase 2 does not; the one-call forms run it once; the neighbours' rows do not notice it"""
    ch, bs = 35, 2048
    sa = rc.baseline_spec("cfg3", ch, rc.ARITH_CMSIS, agc_global=True)
    nout = bs // 4
    d_in, d_out, d_env = sr.DeviceBuffer(ch * bs * 8), sr.DeviceBuffer(ch * nout * 4), sr.DeviceBuffer(4 * (bs // 256))

    def one_call(rx, iq, check):
        return rx.process(iq)

    def split(rx, iq, check):
        d_in.upload(iq)
        rx.global_phase1(d_in.ptr, d_out.ptr, d_env.ptr, bs)
        rx.sync()
        mid = rx.cwdec_state() if check else None
        rx.global_phase2(d_out.ptr, d_env.ptr, bs)
        rx.sync()
        if check:
            assert_state(rx, mid, "phase 2 moved the decoder")
        return d_out.download((ch, nout), np.float32), mid

    def process_entry(rx, iq, check):
        rx.L.selenite_rx_global_process_f32_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        d_in.upload(iq)
        assert rx.L.selenite_rx_global_process_f32_device(rx.h, d_in.ptr, d_out.ptr, bs, None) == 0
        rx.sync()
        return d_out.download((ch, nout), np.float32)

    for entry in (one_call, split, process_entry):
        a, b = sr.Rx(sa.config()), sr.Rx(sa.config())
        neighbours(a); neighbours(b)
        a.set_cwdec(**PAR)
        orc, exp = rc.CpuChain(no_agc(rc.baseline_spec("cfg3", ch, rc.ARITH_CMSIS)), "orc"), co.CwDec(ch, 64, **PAR)
        for call in range(2):
            iq = keyed_iq(ch, call * bs, bs, 256)
            ya, yb = entry(a, iq, True), entry(b, iq, False)
            exp.process(orc.process(iq))
            if entry is split:
                assert_bits(ya[0], yb[0], "split, call %d" % call)
                assert_state(a, ya[1], "split, call %d: behind phase 2" % call)
                for k, v in exp.state().items():
                    assert_bits(ya[1][k], v, "split, call %d: behind phase 1: %s" % (call, k))
            else:
                assert_bits(ya, yb, "%s, call %d" % (entry.__name__, call))
            assert_state(a, exp, "%s, call %d" % (entry.__name__, call))
        for (name, s1), (_, s2) in zip(neighbour_states(a), neighbour_states(b)):
            for k in s1:
                assert_bits(np.asarray(s1[k]), np.asarray(s2[k]), "%s: %s state: %s" % (entry.__name__, name, k))
        assert exp.count.any()
    d_in.free(); d_out.free(); d_env.free()


# ---- 9. loop-back ---------------------------------------------------------------------------------------------------------------------------------
def test_a_keyed_transmitter_is_read_back_as_text():
    """four Tx channels in CW mode keyed with sr.morse_key, each its own text and speed (15, 20, 25 and 30 WPM at 12 kHz of audio, blocks of
    64: units of 15, 11.25, 9 and 7.5 blocks from unit_init 10), pitch 703 Hz; the receiver of tests/test_gpu_txcw.py's read-back with the
    decoder at its defaults.  Behind the last character come 3.5 units of key-up for the slowest channel, more for the others: a faster
    channel may have its blank out, nothing else."""
    import test_txcw_oracle as tco
    L, fs = tco.L_RF, 12000
    sent = [("CQ DE K1ABC", 15), ("5NN TU 73", 20), ("PSE K = QRZ?", 25), ("W1AW/3 @ 7.030", 30)]
    keys = [sr.morse_key(t, int(round(1.2 / w * fs))) for t, w in sent]
    lead = 40 * 64
    total = max(lead + len(k) + (7 * int(round(1.2 / w * fs))) // 2 for k, (_, w) in zip(keys, sent))
    total = -(-total // 64) * 64
    key = np.zeros((4, total), np.uint8)
    for c, k in enumerate(keys):
        key[c, lead:lead + len(k)] = k
    tx = sr.Tx(rc.TxSpec(4, block=64, interp=L, ni_taps=256, nh_taps=63, mode=rc.MODE_CW, alc=False, nco_step_all=tco.LOOP_STEP).config())
    assert tco.loop_cw(tx) == 0
    rx = sr.Rx(rc.ChainSpec(4, 64 * L, L, 256, 63, 0, rc.MODE_CW, rc.ARITH_CMSIS, nco=True, nco_step_all=tco.LOOP_STEP, agc=False).config())
    rx.set_cwdec()
    d_k, d_iq, d_y = sr.DeviceBuffer(key.nbytes), sr.DeviceBuffer(4 * total * L * 8), sr.DeviceBuffer(4 * total * 4)
    d_k.upload(key)
    assert tx.process_key(d_k.ptr, d_iq.ptr, None, total) == 0
    assert tx.sync() == 0
    rx.process_device(d_iq.ptr, d_y.ptr, total * L)
    rx.sync()
    rx.check()
    audio = d_y.download((4, total), np.float32)
    exp = co.CwDec(4, 64)
    exp.process(audio)
    assert_state(rx, exp, "the receiver's rows")
    got, unit = rx.cw_text(), rx.cw_unit()
    print("read back: %r, units %s blocks" % (got, unit))
    for c, (text, wpm) in enumerate(sent):
        assert rx.cw_text(c) == got[c] and got[c].rstrip(" ") == text, (c, got[c], text)
        assert abs(unit[c] - 1.2 / wpm * fs / 64) < 1.0
    d_k.free(); d_iq.free(); d_y.free()
    tx.close(); rx.close()


# ---- 10. device accessors ---------------------------------------------------------------------------------------------------------------------
def test_device_rows_are_the_host_copies():
    ch = 21
    spec = generic_spec(ch, 24)
    rx = sr.Rx(spec.config())
    rx.set_cwdec(**PAR)
    run_device(rx, keyed_iq(ch, 0, 300 * spec.block, spec.block))                # five tiles: the rings wrap
    text, count, unit = np.zeros((ch, PAR["ring"]), np.uint8), np.zeros(ch, np.uint64), np.zeros(ch, np.uint32)
    for arr, ptr in ((text, rx.cwdec_text_device()), (count, rx.cwdec_count_device()), (unit, rx.cwdec_unit_device())):
        assert ptr
        assert rx.L.selenite_rx_memcpy_d2h(arr.ctypes.data_as(C.c_void_p), ptr, arr.nbytes) == 0
    t2, c2, u2, k2 = rx.cwdec()
    st = rx.cwdec_state()
    assert_bits(text, t2); assert_bits(count, c2); assert_bits(unit, u2)
    assert_bits(t2, st["text"]); assert_bits(c2, st["count"]); assert_bits(u2, st["unit"]); assert_bits(k2, st["key"])
    assert count.max() > PAR["ring"] and text.any()
    assert_bits(rx.cw_unit(), unit.astype(np.float64) / 256.0)
    for c in range(ch):
        assert rx.cw_text(c) == sr.ring_text(text[c], int(count[c])) and len(rx.cw_text(c)) == min(int(count[c]), PAR["ring"])
    # NULLs are skipped
    only = np.zeros(ch, np.uint64)
    assert rx.L.selenite_rx_get_cwdec(rx.h, None, only.ctypes.data_as(sr.u64p), None, None) == 0
    assert_bits(only, count)
