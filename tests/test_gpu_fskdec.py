"""GPU: the FSK teleprinter decoder (selenite_rx_set_fskdec, csrc/rx_fskdec.hip: k_fskdec) against the reference's
arm_biquad_cascade_df1_f32 / arm_power_f32 and the second statement of the law (tests/golden/fskdec.npz) and against the numpy restatement
(tests/fskdec_oracle.py, pinned to that fixture by tests/test_fskdec_oracle.py).  The stage is a tap: the restatement is fed the call's own
un-scaled audio -- the audio of the same call on an instance without the stage, which in _CMSIS / _FMA must equal the oracle chain's with its
AGC off on bits -- and every row of the state is compared on bits behind every call.  The shape tests run a chain that passes the I rail
through, so the audio is what the test wrote: a random FSK keying per channel at the decoder's own bit length, which makes start edges,
characters, framing errors and the ring's wrap all happen within a few hundred ticks."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fskdec_oracle as fo
import nr_oracle as nro
import rxcommon as rc
import selenite_rx as sr

pytestmark = pytest.mark.gpu

ARITHS = (rc.ARITH_CMSIS, rc.ARITH_FMA, rc.ARITH_SPLIT16, rc.ARITH_AUTO)
ARITH_IDS = ["cmsis", "fma", "split16", "auto"]
F_MARK, F_SPACE = 0.11, 0.19                       # cycles per audio sample, for the shape tests
MARK, SPACE = fo.design(F_MARK, F_SPACE, 0.06)
# fast timing for short streams: bits of 8 ticks, followers that settle within a bit, a ring that wraps within a test
FAST = dict(bit_q8=8 * 256, reverse=0, usos=1, ring=16, alpha=0.5, hyst=0.05, frac=0.2)
LOOSE = dict(hyst=0.0, frac=0.0, min_power=0.0)    # any audio moves the level and the clock (the suite's synthetic I/Q is no FSK signal)


def par(tick, **over):
    """min_power: a tick of the keyed signal sums to 0.045 T, a tick of the noise-only channels' filter outputs to about 2e-4 T"""
    return dict(FAST, tick=tick, min_power=0.005 * tick, **over)


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
    got, want = rx.fskdec_state(), exp.state() if hasattr(exp, "state") else exp
    assert set(got) == set(want) == set(fo.ROWS)
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


def keyed(channels, first, count, per_bit, seed=5, f_mark=F_MARK, f_space=F_SPACE):
    """`count` samples from sample `first` of a random, phase-continuous FSK keying per channel: a new bit every per_bit samples (a few
    per cent off per channel, so that the edges leave the tick grid), amplitude 0.3 in noise of sigma 0.02; channel 3 mod 7 is noise alone.
    A pure function of (channel, sample)."""
    out = np.empty((channels, count), np.float32)
    for c in range(channels):
        rng = np.random.default_rng(1000 * seed + c)
        pb = per_bit * rng.uniform(0.97, 1.03)
        nbits = int((first + count) / pb) + 2
        bits = rng.integers(0, 2, nbits)
        bits[::9] = 1                                    # now and then two marks in a row: room for a stop bit
        idx = (np.arange(first + count) / pb).astype(np.int64)
        f = np.where(bits[idx] == 1, f_mark, f_space)
        x = (0.3 if c % 7 != 3 else 0.0) * np.sin(2.0 * np.pi * np.cumsum(f)) + rng.normal(0.0, 0.02, first + count)
        out[c] = x[first:]
    return out


def i_rail(x):
    iq = np.zeros(x.shape + (2,), np.float32)
    iq[..., 0] = x
    return iq


def through_spec(ch, n, arith=rc.ARITH_CMSIS):
    """a chain that passes the I rail through: no NCO, no decimator, no FIR pair, AGC off, DSP blocks of n samples"""
    return rc.ChainSpec(ch, n, 1, 0, 0, 0, sr.MODE_USB, arith, agc=False)


class Tap:
    """An instance of `spec` (AGC off) with the decoder, an instance without it, the restatement, and in _CMSIS / _FMA the oracle chain:
    call() runs one call everywhere and compares the audio and every row of the stage's state on bits."""

    def __init__(self, spec, p, mark=MARK, space=SPACE):
        assert not spec.agc
        self.spec = spec
        self.a, self.b = sr.Rx(spec.config()), sr.Rx(spec.config())
        self.a.set_fskdec(mark, space, **p)
        self.exp = fo.FskDec(spec.channels, mark, space, **p)
        self.orc = rc.CpuChain(spec, "orc") if spec.arith in (rc.ARITH_CMSIS, rc.ARITH_FMA) else None
        self.at = 0

    def call(self, iq, device=False, q15=False):
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
        self.at += iq.shape[1]
        assert_state(self.a, self.exp, what)
        return pre


# ---- 1. the fixture's vectors through the library ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(rc.GOLDEN_DIR, "fskdec.npz")) as z:
        return {k: z[k] for k in z.files}


def gold_par(g):
    return {k[4:]: (float(g[k]) if g[k].dtype == np.float32 else int(g[k])) for k in g if k.startswith("par/")}


def test_golden_vectors_through_the_library(gold):
    """DSP blocks of n = T = 8 samples, the fixture's streams in as I, in the fixture's calls of 1 ... 300 ticks, each channel at its own `bit`
    through the state; behind every call every row equals the fixture's -- the NaN of channel 2 and the Inf of channel 3 included"""
    T = int(gold["par/tick"])
    rx = sr.Rx(through_spec(4, T).config())
    rx.set_fskdec(gold["mark"], gold["space"], table=gold["table"], **gold_par(gold))
    rx.set_fskdec_state({"bit": gold["bit"]})
    at = 0
    for i, nt in enumerate(int(v) for v in gold["lens"]):
        x = gold["x"][:, at * T:(at + nt) * T]
        got = run_device(rx, i_rail(x), naninf_ok=True)
        assert got.view(np.uint32).tobytes() == x.view(np.uint32).tobytes(), "the chain does not pass the I rail through as it is"
        at += nt
        st = rx.fskdec_state()
        for k in st:
            assert_bits(st[k], gold["call/" + k][i], "%s behind call %d" % (k, i))
    assert [rx.fsk_text(c) for c in range(2)] == [str(s) for s in gold["sent"][:2]]
    assert rx.fsk_text() == [rx.fsk_text(c) for c in range(4)] and rx.fsk_text(3) == ""


# ---- 2. lane-plan shapes ------------------------------------------------------------------------------------------------------------------------
SHAPES = [(T, n) for T in (4, 8, 16, 32) for n in (T, 2 * T, 96)]


@pytest.mark.parametrize("ch", [1, 63, 65, 130])
@pytest.mark.parametrize("T,n", SHAPES, ids=["T%d-n%d" % s for s in SHAPES])
def test_blocks_per_call_by_tick_by_block_length_by_channels(T, n, ch):
    """calls of 1, 3 and 17 DSP blocks of n = T, 2 T and 96 samples (a tile of 32 samples holds several ticks, one tick, a part of one; a
    last tile of 4 ... 32 samples) over 1, 63, 65 and 130 channels (the wave edges of one lane per channel: a lone lane, one short of a wave,
    one past it, two waves and two lanes); device and host entries alternate"""
    t = Tap(through_spec(ch, n), par(T))
    for i, blocks in enumerate((1, 3, 17)):
        t.call(i_rail(keyed(ch, t.at, blocks * n, 8 * T)), device=i % 2 == 0)
    if n == 96:
        st = t.exp.state()
        assert (st["em"] != 0).all()
        if ch > 1:                                       # (a lone channel may stand idle behind its last character)
            assert (st["k"] != 0).any() and (T != 4 or st["count"].any())


def test_uneven_cuts_of_one_stream_and_a_ring_that_wraps():
    """130 DSP blocks of 96 samples, T = 4: one call against calls of 1, 7 and 64 blocks; the rings of 16 wrap"""
    ch, n, T, total = 67, 96, 4, 130
    spec = through_spec(ch, n)
    iq = i_rail(keyed(ch, 0, total * n, 8 * T))
    one = sr.Rx(spec.config())
    one.set_fskdec(MARK, SPACE, **par(T))
    whole = run_device(one, iq)
    want = one.fskdec_state()
    exp = fo.FskDec(ch, MARK, SPACE, **par(T))
    exp.process(whole)
    assert_state(one, exp, "one call")
    assert want["count"].max() > 16 and want["ferr"].any() and want["figs"].any() and want["count"][3] == 0
    for cut in (1, 7, 64):
        rx = sr.Rx(spec.config())
        rx.set_fskdec(MARK, SPACE, **par(T))
        for a in range(0, total, cut):
            b = min(a + cut, total)
            part = run_device(rx, np.ascontiguousarray(iq[:, a * n:b * n]))
            assert_bits(part, whole[:, a * n:b * n], "audio of blocks %d .. %d" % (a, b))
        assert_state(rx, want, "calls of %d blocks" % cut)
    for c in (0, 1, 66):
        assert one.fsk_text(c) == exp.fsk_text(c) and len(one.fsk_text(c)) == min(int(want["count"][c]), 16)


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
@pytest.mark.parametrize("name", ["cfg3", "cfg4"])
def test_fused_shapes_arith_modes_and_slot_formats(name, arith, q15):
    """the fused SSB and CW kernels with their own AGC off in front of the stage: n = 64 and 256, T = 16, calls of 4, 1, 17 and 3 blocks (the two
    forms of _AUTO: test_auto_in_one_launch_and_in_three)"""
    spec = no_agc(rc.baseline_spec(name, 70, arith))
    t = Tap(spec, dict(par(16), **LOOSE))
    for i, blocks in enumerate((4, 1, 17, 3)):
        bs = spec.block * blocks
        t.call(rc.synth_iq(0, 70, t.at, bs), device=i % 2 == 1, q15=q15)
    assert (t.exp.em != 0).all()


@pytest.mark.parametrize("form", [1, 3])
def test_auto_in_one_launch_and_in_three(form):
    """SELENITE_ARITH_AUTO on a no-decimator shape (k_hilb_split16), where selenite_rx_set_auto_launches chooses between the workgroup that
    guarded a channel recomputing it itself and the two launches behind the matrix kernel; channels that change level between calls, so that
    some are rerun exactly.  The audio given to the restatement is the call's own."""
    ch = 70
    spec = rc.ChainSpec(ch, 256, 1, 0, 63, 0, sr.MODE_USB, rc.ARITH_AUTO, nco=True, nco_steps=np.full(ch, 0x0B000000, np.uint32), agc=False)
    t = Tap(spec, dict(par(32), **LOOSE))
    for r in (t.a, t.b):
        assert r.set_auto_launches(form) == 0
    for call, bs in enumerate((3072, 1536, 1536, 3072)):
        iq = rc.synth_iq(0, ch, t.at, bs)
        if call % 2 == 1:
            iq[np.arange(ch) % 3 == 1] *= np.float32(0.01)
        iq[5] = 0.0
        t.call(iq, device=call % 2 == 0)
        assert t.b.auto_launches_last() == form
        print("form %d, call %d: with the stage on the call took form %d" % (form, call, t.a.auto_launches_last()))
    print("form %d: %d channel-calls rerun exactly" % (form, t.b.guard_stats()["rerun_channel_calls"]))
    assert (t.exp.em[np.arange(ch) != 5] != 0).all() and t.exp.em[5] == 0


def test_modes_am_and_fm():
    for mode in (sr.MODE_AM, sr.MODE_FM):
        spec = no_agc(rc.baseline_spec("cfg1", 33, rc.ARITH_CMSIS))
        spec.mode = mode
        t = Tap(spec, dict(par(32), **LOOSE))
        for bs in (512, 256, 768):
            t.call(rc.synth_iq(0, 33, t.at, bs))


# ---- 3. a host-pointer call cut into channel chunks ---------------------------------------------------------------------------------------------
def host_chunks_body(q15):
    """cfg3, 300 channels x 2048 samples with a 1 MiB chunk: 64-channel chunks for f32 slots, 128-channel chunks for int16 slots, a ragged last
    one; the state rows and the rings follow each chunk's first channel"""
    spec = no_agc(rc.baseline_spec("cfg3", 300, rc.ARITH_AUTO))
    t = Tap(spec, dict(par(16), **LOOSE))
    for bs in (2048, 2048, 256):
        t.call(rc.synth_iq(0, 300, t.at, bs), device=False, q15=bool(q15))
    st = t.exp.state()
    assert len(set(st["em"].view(np.uint32).tolist())) > 250 and (st["em"] != 0).all()
    print("OK")


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_host_call_cut_into_channel_chunks(q15):
    """(a subprocess: the library reads SELENITE_RX_HOST_CHUNK_MB once)"""
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_fskdec as t; t.host_chunks_body(%d)" % (
        os.path.join(rc.ROOT, "tests"), rc.PKG_DIR, int(q15))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, SELENITE_RX_HOST_CHUNK_MB="1"))
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), (out.stdout[-1000:], out.stderr[-3000:])


# ---- 4. life cycle ------------------------------------------------------------------------------------------------------------------------------
def test_state_round_trip_mid_character_reset_and_the_other_setters():
    ch, n, T = 33, 64, 4
    spec = through_spec(ch, n)
    rx, fresh = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (rx, fresh):
        r.set_fskdec(MARK, SPACE, **par(T))
    exp = fo.FskDec(ch, MARK, SPACE, **par(T))
    assert_state(rx, exp, "behind set_fskdec")
    s0 = rx.fskdec_state()
    assert not np.signbit(s0["filt"]).any() and (s0["lvl"] == 1).all() and (s0["bit"] == 8 * 256).all() and not s0["text"].any()
    first = i_rail(keyed(ch, 0, 41 * n, 8 * T))
    rx.process(first)
    st = rx.fskdec_state()
    assert (st["k"] > 1).any() and (st["lvl"] == 0).any()      # some channel stands inside a character
    nxt = i_rail(keyed(ch, 41 * n, 50 * n, 8 * T))
    rx.process(nxt)
    fresh.set_fskdec_state(st)
    fresh.process(nxt)
    a = rx.fskdec_state()
    assert_state(fresh, a, "after set_fskdec_state")
    assert a["count"].any()
    # a `bit` per channel goes in through the state and stays
    bits = (8 * 256 + 37 * np.arange(ch)).astype(np.uint32)
    fresh.set_fskdec_state({"bit": bits})
    exp2 = fo.FskDec(ch, MARK, SPACE, **par(T))
    exp2.set_state(dict(a, bit=bits))
    more = keyed(ch, 91 * n, 30 * n, 8 * T)
    exp2.process(fresh.process(i_rail(more)))
    assert_state(fresh, exp2, "a bit per channel")
    # set_mode and the other setters keep the state, the parameters and the table
    assert rx.set_mode(sr.MODE_LSB) == 0
    rx.set_nr(sr.NR_NOTCH, num_taps=16, delay=4, mu=0.1); rx.set_nr(sr.NR_OFF)
    rx.set_meter(); rx.set_meter(sense=None)
    rx.set_afilt(sr.design_deemphasis(0.9)); rx.set_afilt(None)
    rx.set_tones(sr.design_tones([0.1])); rx.set_tones(None)
    rx.set_cwdec(); rx.set_cwdec(None)
    rx.set_spectrum(64); rx.set_spectrum(None)
    rx.set_nb(); rx.set_nb(None)
    rx.set_iqc(); rx.set_iqc(None)
    assert_state(rx, a, "behind the other setters")
    # reset: back to the state set_fskdec left; the same stream gives the same rows again
    assert rx.reset() == 0
    assert_state(rx, exp, "behind reset")
    rx.set_mode(sr.MODE_USB)
    rx.process(first)
    assert_state(rx, st, "the same stream behind reset")


BAD = [("struct_size", 84), ("tick", 3), ("tick", 257), ("tick", 0), ("bit_q8", 8 * 256 - 1), ("bit_q8", 1024 * 256 + 1), ("bit_q8", 0),
       ("reverse", 2), ("usos", 2), ("ring", 8), ("ring", 24), ("ring", 0), ("ring", 131072), ("mark", float("nan")), ("mark", float("inf")),
       ("space", float("nan")), ("space", float("-inf")), ("alpha", 0.0), ("alpha", 1.5), ("alpha", float("nan")), ("alpha", -0.1),
       ("hyst", 1.0), ("hyst", -0.1), ("hyst", float("nan")), ("frac", 1.5), ("frac", -0.1), ("frac", float("nan")), ("min_power", -1.0),
       ("min_power", float("inf")), ("min_power", float("nan"))]
LENGTH = [("tick", 5), ("tick", 24), ("tick", 128)]              # in range, but no divisor of n = 64


@pytest.mark.parametrize("field,value", BAD + LENGTH, ids=["%s=%s" % b for b in BAD + LENGTH])
def test_bad_field_is_refused_and_the_stage_stays(field, value):
    ch, n, T = 16, 64, 4
    spec = through_spec(ch, n)
    rx, ref = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (rx, ref):
        r.set_fskdec(MARK, SPACE, **par(T))
    iq = i_rail(keyed(ch, 0, 20 * n, 8 * T))
    rx.process(iq); ref.process(iq)
    g = sr.FskdecConfig()
    g.struct_size = C.sizeof(sr.FskdecConfig)
    for k, v in dict(sr.FSKDEC_DEFAULTS, ring=64).items():                   # another, valid configuration ...
        setattr(g, k, v)
    g.mark[:], g.space[:] = SPACE.tolist(), MARK.tolist()
    if field in ("mark", "space"):                                           # ... with one bad field
        getattr(g, field)[3] = value
    else:
        setattr(g, field, value)
    code = sr.LENGTH_ERROR if (field, value) in LENGTH else sr.ARGUMENT_ERROR
    assert rx.L.selenite_rx_set_fskdec(rx.h, C.byref(g)) == code
    assert rx.status() == 0 and rx.L.selenite_rx_error_string(None).decode().startswith("selenite_rx_set_fskdec: ")
    iq = i_rail(keyed(ch, 20 * n, 30 * n, 8 * T))
    rx.process(iq); ref.process(iq)
    assert_state(rx, ref.fskdec_state(), "after the refused set_fskdec")
    assert ref.fskdec_state()["count"].any()
    with pytest.raises(sr.RxError) as e:
        if field == "struct_size":
            rx.set_fskdec(MARK, SPACE, ring=3)
        elif field in ("mark", "space"):
            rx.set_fskdec(**{"mark": MARK, "space": SPACE, field: np.array([1, 0, 0, value, 0], np.float32)})
        else:
            rx.set_fskdec(MARK, SPACE, **{field: value})
    assert e.value.code == (code if field != "struct_size" else sr.ARGUMENT_ERROR)
    assert_state(rx, ref.fskdec_state(), "after the refused Rx.set_fskdec")


@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
def test_stage_removed_is_no_stage(arith):
    spec = rc.baseline_spec("cfg3", 70, arith)
    a, b = sr.Rx(spec.config()), sr.Rx(spec.config())
    a.set_fskdec(MARK, SPACE, **par(16))
    assert a.fskdec_text_device() and a.fskdec_count_device() and a.fskdec_lvl_device()
    a.set_fskdec(None)
    for call in range(2):
        iq = rc.synth_iq(0, 70, call * 2048, 2048)
        assert_bits(a.process(iq), b.process(iq), "call %d" % call)
    with pytest.raises(sr.RxError):
        a.fskdec_state()
    with pytest.raises(sr.RxError):
        a.fsk_text(0)
    assert a.L.selenite_rx_get_fskdec_state(a.h, C.byref(sr.FskdecStateView())) == sr.ARGUMENT_ERROR
    assert a.L.selenite_rx_set_fskdec_state(a.h, C.byref(sr.FskdecStateView())) == sr.ARGUMENT_ERROR
    assert a.L.selenite_rx_get_fskdec(a.h, None, None, None, None) == sr.ARGUMENT_ERROR
    assert a.fskdec_text_device() is None and a.fskdec_count_device() is None and a.fskdec_lvl_device() is None


# ---- 5. with the other stages on ----------------------------------------------------------------------------------------------------------------
def neighbour(r, which):
    if which == "tones":
        r.set_tones(sr.design_tones([0.05, 0.11, 0.2]), frame_blocks=3, confirm=2, release=2, ratio=0.02, min_power=1e-6)
    elif which == "cwdec":
        r.set_cwdec(ring=16, unit_init=2 * 256, unit_min=256, debounce=1)
    elif which == "afilt":
        r.set_afilt(sr.design_biquad(sr.BIQUAD_HIGHPASS, 300.0 / 12000.0, 0.7071).reshape(1, 5))
    elif which == "nr":
        r.set_nr(sr.NR_DENOISE, num_taps=16, delay=8, mu=0.05)
    else:
        r.set_meter(sense=sr.SQ_ABOVE, gate=1, hang=1, attack=0.5, decay=0.9375, open_level=2e-2, close_level=4e-3, level_init=0.0)


def neighbour_state(r, which):
    return dict(r.state(), **{"stage/" + k: v for k, v in getattr(r, {"meter+gate": "meter"}.get(which, which) + "_state")().items()})


@pytest.mark.parametrize("which", ["tones", "cwdec", "afilt", "nr", "meter+gate"])
def test_with_each_other_stage_on(which):
    """the decoder's rows are those of the decoder alone and of the restatement fed the audio in front of the filters (afilt and NLMS do not
    reach the tap; the taps see the same audio); audio, chain state and the other stage's rows are those of the same calls without it"""
    ch = 35
    spec = rc.baseline_spec("cfg3", ch, rc.ARITH_CMSIS)
    a, b, alone = sr.Rx(spec.config()), sr.Rx(spec.config()), sr.Rx(spec.config())
    neighbour(a, which); neighbour(b, which)
    p = dict(par(16), **LOOSE)
    a.set_fskdec(MARK, SPACE, **p); alone.set_fskdec(MARK, SPACE, **p)
    orc, exp = rc.CpuChain(no_agc(spec), "orc"), fo.FskDec(ch, MARK, SPACE, **p)
    at = 0
    for i, bs in enumerate((1024, 256, 4096)):
        iq = rc.synth_iq(0, ch, at, bs)
        assert_bits(run(a, iq, device=i == 1), run(b, iq, device=i == 1), "call %d" % i)
        run(alone, iq)
        exp.process(orc.process(iq))
        assert_state(a, exp, "call %d" % i)
        assert_state(alone, exp, "call %d, the decoder alone" % i)
        at += bs
    assert (exp.em != 0).all() and exp.t_q8.any()
    sa, sb = neighbour_state(a, which), neighbour_state(b, which)
    for k in sa:
        assert_bits(np.asarray(sa[k]), np.asarray(sb[k]), "%s state: %s" % (which, k))


def test_global_gain_one_call_and_the_two_phases():
    """phase 1 runs the stage, phase 2 does not; the one-call forms run it once"""
    ch, bs = 35, 2048
    sa = rc.baseline_spec("cfg3", ch, rc.ARITH_CMSIS, agc_global=True)
    nout = bs // 4
    d_in, d_out, d_env = sr.DeviceBuffer(ch * bs * 8), sr.DeviceBuffer(ch * nout * 4), sr.DeviceBuffer(4 * (bs // 256))
    p = dict(par(16), **LOOSE)

    def one_call(rx, iq, check):
        return rx.process(iq)

    def split(rx, iq, check):
        d_in.upload(iq)
        rx.global_phase1(d_in.ptr, d_out.ptr, d_env.ptr, bs)
        rx.sync()
        mid = rx.fskdec_state() if check else None
        rx.global_phase2(d_out.ptr, d_env.ptr, bs)
        rx.sync()
        if check:
            assert_state(rx, mid, "phase 2 moved the decoder")
        return d_out.download((ch, nout), np.float32), mid

    def process_entry(rx, iq, check):
        d_in.upload(iq)
        assert rx.L.selenite_rx_global_process_f32_device(rx.h, d_in.ptr, d_out.ptr, bs, None) == 0
        rx.sync()
        return d_out.download((ch, nout), np.float32)

    for entry in (one_call, split, process_entry):
        a, b = sr.Rx(sa.config()), sr.Rx(sa.config())
        a.set_fskdec(MARK, SPACE, **p)
        orc, exp = rc.CpuChain(no_agc(rc.baseline_spec("cfg3", ch, rc.ARITH_CMSIS)), "orc"), fo.FskDec(ch, MARK, SPACE, **p)
        for call in range(2):
            iq = rc.synth_iq(0, ch, call * bs, bs)
            ya, yb = entry(a, iq, True), entry(b, iq, False)
            exp.process(orc.process(iq))
            if entry is split:
                assert_bits(ya[0], yb[0], "split, call %d" % call)
                for k, v in exp.state().items():
                    assert_bits(ya[1][k], v, "split, call %d: behind phase 1: %s" % (call, k))
            else:
                assert_bits(ya, yb, "%s, call %d" % (entry.__name__, call))
            assert_state(a, exp, "%s, call %d" % (entry.__name__, call))
        assert (exp.em != 0).all()
    d_in.free(); d_out.free(); d_env.free()


# ---- 6. loop-back ---------------------------------------------------------------------------------------------------------------------------------
FS, RTTY_MARK, RTTY_SPACE = 12000.0, 2125.0, 2295.0
SENT = [("CQ CQ DE K1ABC K1ABC PSE K", 45.45), ("UR 599 599 NR 001 TU", 50.0), ("W1AW (3) $5.00 #2 OK?", 75.0), ("RYRYRY DE N0CALL", 75.0)]
STEP = 0x01000000


@pytest.mark.parametrize("mode", ["dig", "pkt_reverse"])
def test_a_transmitter_fed_afsk_is_read_back_as_text(mode):
    """four Tx channels in USB fed fo.afsk() audio of amplitude 0.3 in noise of sigma 0.1, each its own text, at 45.45, 50, 75 and 75 baud
    (the speeds on different channels through the `bit` row), a channel of noise alone and a channel of zeros; the chain's own Rx reads them:
    in DIG (= USB) on the transmitters' carrier; in PKT (= LSB) tuned mark + space above it, where the tones come out swapped, with
    reverse = 1.  T = 16, mark 2125 Hz, space 2295 Hz, 140 Hz of bandwidth (one coefficient pair serves every speed), alpha 0.25, hyst 0.1,
    frac 0.35, min_power 1e-6.  Every text is read back whole; the noise and the zeros stay silent."""
    L, ch = 4, len(SENT) + 2
    audio = [0.3 * fo.afsk(fo.encode(t), FS, baud, RTTY_MARK, RTTY_SPACE, 1.5, lead=12, tail=6) for t, baud in SENT]
    total = -(-max(a.size for a in audio) // 64) * 64
    x = np.zeros((ch, total), np.float32)
    for c, a in enumerate(audio):
        x[c, :a.size] = a
        x[c, a.size:] = 0.3 * np.sin(2.0 * np.pi * RTTY_MARK / FS * np.arange(a.size, total))        # (an idle mark to the end)
    x[:ch - 1] += np.random.default_rng(17).normal(0.0, 0.1, (ch - 1, total)).astype(np.float32)
    tx = sr.Tx(rc.TxSpec(ch, alc=False, nco_step_all=STEP).config())
    rev = mode == "pkt_reverse"
    step = (STEP + int(round((RTTY_MARK + RTTY_SPACE) / (FS * L) * 2.0 ** 32))) & 0xFFFFFFFF if rev else STEP
    rspec = rc.ChainSpec(ch, 64 * L, L, 256, 63, 0, sr.MODE_PKT if rev else sr.MODE_DIG, rc.ARITH_CMSIS, nco=True, nco_step_all=step, agc=False)
    rx = sr.Rx(rspec.config())
    mark, space = sr.fsk_bandpass(RTTY_MARK / FS, RTTY_SPACE / FS, 140.0 / FS)
    rx.set_fskdec(mark, space, reverse=int(rev))
    bits = np.array([fo.bit_q8(FS, baud, 16) for _, baud in SENT] + [4224, 4224], np.uint32)
    rx.set_fskdec_state({"bit": bits})
    d_a, d_iq, d_y = sr.DeviceBuffer(x.nbytes), sr.DeviceBuffer(ch * total * L * 8), sr.DeviceBuffer(ch * total * 4)
    d_a.upload(x)
    tx.process_device(d_a.ptr, d_iq.ptr, total)
    tx.sync(); tx.check()
    rx.process_device(d_iq.ptr, d_y.ptr, total * L)
    rx.sync(); rx.check()
    y = d_y.download((ch, total), np.float32)
    exp = fo.FskDec(ch, mark, space, reverse=int(rev))
    exp.set_state({"bit": bits})
    exp.process(y)
    assert_state(rx, exp, "the receiver's rows")
    got, (_, count, ferr, _) = rx.fsk_text(), rx.fskdec()
    print("read back: %r, ferr %s" % (got, ferr.tolist()))
    for c, (text, _) in enumerate(SENT):
        assert got[c] == text, (c, got[c], text)
    assert count[ch - 2] == 0 and count[ch - 1] == 0
    d_a.free(); d_iq.free(); d_y.free()
    tx.close(); rx.close()


# ---- 7. device accessors ---------------------------------------------------------------------------------------------------------------------
def test_device_rows_are_the_host_copies():
    ch, n, T = 21, 96, 4
    rx = sr.Rx(through_spec(ch, n).config())
    rx.set_fskdec(MARK, SPACE, **par(T))
    run_device(rx, i_rail(keyed(ch, 0, 130 * n, 8 * T)))
    text, count, lvl = np.zeros((ch, 16), np.uint8), np.zeros(ch, np.uint64), np.zeros(ch, np.uint32)
    for arr, ptr in ((text, rx.fskdec_text_device()), (count, rx.fskdec_count_device()), (lvl, rx.fskdec_lvl_device())):
        assert ptr
        assert rx.L.selenite_rx_memcpy_d2h(arr.ctypes.data_as(C.c_void_p), ptr, arr.nbytes) == 0
    t2, c2, f2, l2 = rx.fskdec()
    st = rx.fskdec_state()
    assert_bits(text, t2); assert_bits(count, c2); assert_bits(lvl, l2)
    assert_bits(t2, st["text"]); assert_bits(c2, st["count"]); assert_bits(f2, st["ferr"]); assert_bits(l2, st["lvl"])
    assert count.max() > 16 and text.any()
    assert_bits(rx.fsk_lvl(), lvl)
    for c in range(ch):
        assert rx.fsk_text(c) == sr.ring_text(text[c], int(count[c])) and len(rx.fsk_text(c)) == min(int(count[c]), 16)
    only = np.zeros(ch, np.uint64)                       # NULLs are skipped
    assert rx.L.selenite_rx_get_fskdec(rx.h, None, only.ctypes.data_as(sr.u64p), None, None) == 0
    assert_bits(only, count)
