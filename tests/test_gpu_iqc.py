"""GPU: the I/Q correction stage (selenite_rx_set_iqc, csrc/rx_iqc.hip) against the numpy restatement of the stage (tests/iqc_oracle.py, pinned
to the reference by tests/test_iqc_oracle.py).  The stage's output is observed through the chain: an instance with the stage, fed X, must
give the same audio bits and the same chain state as an instance without it fed iqc_oracle(X) as f32; dc_i, dc_q, p and g must equal the
restatement's after every call (as bits where finite, elsewhere as the set of NaN / Inf positions), and held must equal its counter.

int16 slots: the reference instance has f32 slots (the stage's copy is f32), so the expected words are nr_oracle.float_to_q15 of its f32
audio: equal as bits in CMSIS and FMA; in SPLIT16 and AUTO within the project's int16 bar, 1 LSB + 1e-5 x the float block maximum x 32768
(DESIGN section 3).  The chain state, the AGC gain with it, is compared as bits in every mode and slot format: both instances run the same
fused kernel on the same f32 input, and k_agc_generic's agc_update is the operations of the fused kernels' agc_desired / agc_step in the
same order, on a block maximum that no order of taking it changes.

The input is rc.synth_iq (scaled by 0.25 for int16 slots) with the impairment of each channel's role (ROLES, by c % 17) applied:
I' = I + dc_i, Q' = gain (Q cos(phase) + I sin(phase)) + dc_q.  min_power is 0 throughout, so that the channel at level 1e-20 (denormal
products) estimates and the silent ones are held."""
import ctypes as C

import numpy as np
import pytest

import iqc_oracle as io
import nr_oracle as nro
import rxcommon as rc
import selenite_rx as sr
import spectrum_oracle as so

pytestmark = pytest.mark.gpu

FRAMES = (32, 64, 128)
ARITHS = (rc.ARITH_CMSIS, rc.ARITH_FMA, rc.ARITH_SPLIT16, rc.ARITH_AUTO)
ARITH_IDS = ["cmsis", "fma", "split16", "auto"]
DEFAULTS = dict(alpha=1.0 / 16, dc_alpha=1.0 / 16, p_max=0.25, g_max=1.5, min_power=0.0)
FLOATS = ("dc_i", "dc_q", "p", "g")
# what is done to the channels c with c % PERIOD == role (every other channel is left balanced)
ROLES = ["balanced", "gain_only", "phase_only", "dc_only", "all_three", "silent", "late_start", "q_zero", "i_zero", "p_clamp", "g_clamp_low",
         "g_clamp_high", "level_1e-20", "nan", "inf"]
PERIOD = 17
CH = 2 * PERIOD
R = {r: ROLES.index(r) for r in ROLES}
#          gain, phase (degrees), dc_i, dc_q
IMPAIR = {"gain_only": (1.08, 0.0, 0.0, 0.0), "phase_only": (1.0, 4.0, 0.0, 0.0), "dc_only": (1.0, 0.0, -0.03, 0.02),
          "all_three": (1.08, 4.0, -0.03, 0.02), "p_clamp": (1.0, 30.0, 0.0, 0.0), "g_clamp_low": (2.0, 0.0, 0.0, 0.0),
          "g_clamp_high": (0.5, 0.0, 0.0, 0.0)}


def to_q15(iq):
    return np.clip(np.trunc(iq * 32768.0), -32768, 32767).astype(np.int16)


def assert_bits(got, want, what=""):
    """bit for bit where `want` is finite (all of it, for integers); elsewhere the same NaN / Inf positions"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    u = {4: np.uint32, 2: np.uint16, 8: np.uint64}[got.dtype.itemsize]
    ne = got.view(u) != want.view(u)
    if got.dtype.kind == "f":
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), what + ": NaN / Inf positions"
        ne &= np.isfinite(want)
    bad = np.argwhere(ne)
    if len(bad):
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def role_of(c):
    return ROLES[c % PERIOD] if c % PERIOD < len(ROLES) else "balanced"


def make_stream(channels, total, q15=False, nonfinite=False, ch0=0):
    """the whole stream [channels][total][2] with the impairments of ROLES, in the slot's format"""
    x = rc.synth_iq(ch0, channels, 0, total) * np.float32(0.25 if q15 else 1.0)
    for c in range(channels):
        role = role_of(c)
        if role in IMPAIR:
            gain, deg, di, dq = IMPAIR[role]
            ph = np.deg2rad(deg)
            i, q = x[c, :, 0].copy(), x[c, :, 1].copy()
            x[c, :, 0] = i + np.float32(di)
            x[c, :, 1] = np.float32(gain) * (q * np.float32(np.cos(ph)) + i * np.float32(np.sin(ph))) + np.float32(dq)
        elif role == "silent":
            x[c] = 0
        elif role == "late_start":
            x[c, :total // 3] = 0
        elif role == "q_zero":
            x[c, :, 1] = 0
        elif role == "i_zero":
            x[c, :, 0] = 0
        elif role == "level_1e-20":
            x[c] *= np.float32(1e-20)
        elif role == "nan" and nonfinite:
            x[c, 5 * 128 + 7, 1] = np.nan
        elif role == "inf" and nonfinite:
            x[c, 5 * 128 + 9, 0] = np.inf
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
    assert code == 0 or (naninf_ok and code == sr.NANINF), (code, rx.error())      # (a NaN input sample is NaN audio: that status is the chain's)
    out = d_out.download((ch, vals), data.dtype)
    d_in.free(); d_out.free()
    return out


def check(rx, orc, what=""):
    st = rx.iqc_state()
    for k in FLOATS:
        assert_bits(st[k], getattr(orc, k), "%s %s" % (what, k))
    assert_bits(st["held"], orc.held, what + " held")


def exact_q15(arith):
    return arith in (rc.ARITH_CMSIS, rc.ARITH_FMA)


def assert_audio(got, ref_f32, arith, na, what=""):
    """`got` against the reference instance's f32 audio: as bits, or -- int16 words -- as this file's docstring says"""
    if got.dtype == np.float32:
        return assert_bits(got, ref_f32, what)
    want = nro.float_to_q15(ref_f32)
    if exact_q15(arith):
        return assert_bits(got, want, what)
    ch = got.shape[0]
    mf = np.abs(ref_f32.astype(np.float64)).reshape(ch, -1, na).max(axis=2)
    allow = 1 + np.ceil(1e-5 * mf * 32768.0).astype(np.int64)
    dd = np.abs(got.astype(np.int32) - want.astype(np.int32)).reshape(ch, -1, na).max(axis=2)
    if (dd > allow).any():
        c, b = np.argwhere(dd > allow)[0]
        raise AssertionError("%s: channel %d block %d: %d LSB, %d allowed (float block maximum %.4g)" % (what, c, b, dd[c, b], allow[c, b], mf[c, b]))


def chain_state_equal(a, b, what=""):
    sa, sb = a.state(), b.state()
    for k in sa:
        assert_bits(sa[k], sb[k], what + " chain state." + k)


def stream(spec, cuts, F, q15=False, device=False, prepare=None, nonfinite=False, par=None, x=None, na=None):
    """the stream cut into `cuts` through an instance with the stage fed X, the restatement, and an instance without it fed iqc_oracle(X)"""
    par = dict(DEFAULTS, **(par or {}))
    rx, ref = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (rx, ref):
        if prepare:
            prepare(r)
    rx.set_iqc(F, **par)
    orc = io.Corrector(spec.channels, F, **par)
    if x is None:
        x = make_stream(spec.channels, sum(cuts), q15, nonfinite)
    na = na or spec.block // spec.decim
    at, audio = 0, []
    for i, bs in enumerate(cuts):
        data = np.ascontiguousarray(x[:, at:at + bs])
        dev = device if isinstance(device, bool) else device[i % len(device)]
        got = run(rx, data, dev, nonfinite)
        want = run(ref, orc.process(data), dev, nonfinite)
        assert_audio(got, want, spec.arith, na, "audio of call %d" % i)
        audio.append(got)
        check(rx, orc, "call %d at %d" % (i, at))
        at += bs
    chain_state_equal(rx, ref)
    return rx, orc, ref, np.concatenate(audio, axis=1)


def roles_did_their_work(orc, frames, q15=False):
    """on the restatement, which the instance has just been shown to equal; `frames`: frames per channel so far (at least 24)"""
    assert frames >= 24
    assert orc.held[R["silent"]] == frames and orc.held[R["q_zero"]] == frames and orc.held[R["i_zero"]] == frames
    assert 0 < orc.held[R["late_start"]] < frames
    for r in ("balanced", "gain_only", "phase_only", "dc_only", "all_three", "p_clamp", "g_clamp_low", "g_clamp_high"):
        assert orc.held[R[r]] == 0, r
    assert 0.1 < orc.p[R["p_clamp"]] <= 0.25 and orc.g[R["g_clamp_low"]] < 0.8 and orc.g[R["g_clamp_high"]] > 1.3
    assert orc.dc_i[R["dc_only"]] < -0.004 and orc.dc_q[R["dc_only"]] > 0.002 and orc.p[R["phase_only"]] > 0.03
    assert orc.g[R["gain_only"]] < 0.97 and abs(orc.g[R["balanced"]] - 1) < 0.15 and abs(orc.p[R["balanced"]]) < 0.1
    if not q15:                                                    # (int16 slots: 1e-20 is silence)
        assert orc.held[R["level_1e-20"]] == 0 and orc.g[R["level_1e-20"]] != 1


# ---- the kernel's paths: one tile, the tile loop with a partial tile, masked lanes ---------------------------------------------------------
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("F", FRAMES)
def test_one_tile_then_two_tiles_and_a_half(F, q15):
    spec = rc.baseline_spec("cfg3", CH, rc.ARITH_CMSIS)
    _, orc, _, _ = stream(spec, [1024, 2048 + 512], F, q15=q15, device=[True, False])
    roles_did_their_work(orc, 3584 // F, q15)


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_forty_firmware_slots_of_96(q15):
    """DSP blocks of 96: frames of 32 divide them, three per slot and a half-filled wave load; frames of 64 do not"""
    spec = rc.ChainSpec(CH, 96, 4, 256, 63, 0, sr.MODE_LSB, rc.ARITH_CMSIS, nco=True, nco_step_all=0x01000000)
    rx, orc, _, _ = stream(spec, [96] * 40, 32, q15=q15, device=[False, True, True])
    roles_did_their_work(orc, 120, q15)
    for F in (64, 128):
        with pytest.raises(sr.RxError) as ei:
            rx.set_iqc(F)
        assert ei.value.code == sr.LENGTH_ERROR
    check(rx, orc, "the stage of 32 is still there, with its state")


@pytest.mark.parametrize("F", FRAMES)
def test_call_cuts_give_one_stream(F):
    spec = rc.baseline_spec("cfg3", CH, rc.ARITH_CMSIS)
    x = make_stream(CH, 4096)
    outs = [stream(spec, cuts, F, device=[True, False], x=x) for cuts in ([4096], [256] * 16, [768, 256, 3072])]
    for _, orc, _, audio in outs[1:]:
        assert_bits(audio, outs[0][3], "audio against the uncut stream")
        for k in FLOATS + ("held",):
            assert_bits(orc.state()[k], outs[0][1].state()[k], k)


# ---- chains, arithmetic modes, slot formats --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
@pytest.mark.parametrize("name", ["cfg3", "cfg1"])
def test_chains_and_arith_modes(name, arith, q15):
    """cfg3's chain (NCO, decimator by 4, 63-tap pair) and a USB chain without decimator, DSP blocks of 256"""
    k = ARITHS.index(arith) + (4 if name == "cfg1" else 0) + (1 if q15 else 0)
    _, orc, _, _ = stream(rc.baseline_spec(name, CH, arith), [1024, 256, 2304], FRAMES[k % 3], q15=q15, device=(k // 2) % 2 == 1)
    roles_did_their_work(orc, 3584 // FRAMES[k % 3], q15)


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("name", ["cw", "am"])
def test_cw_and_am(name, q15):
    spec = rc.baseline_spec("cfg4", CH, rc.ARITH_CMSIS) if name == "cw" else rc.baseline_spec("cfg3", CH, rc.ARITH_FMA)
    prepare = None if name == "cw" else (lambda r: r.set_mode(sr.MODE_AM))
    stream(spec, [1024, 768], 64 if name == "cw" else 128, q15=q15, device=[False, True], prepare=prepare)


# ---- pointer kinds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,q15,channels", [(128, False, 1100), (32, True, 2100)])
def test_host_call_cut_into_three_channel_chunks(F, q15, channels):
    """64 KiB of input per channel (32 KiB for int16 slots): the host-pointer pipeline cuts 1100 (2100) channels into chunks of 512 (1024); the
    five state rows follow each chunk's first channel"""
    spec = rc.baseline_spec("cfg1", channels, rc.ARITH_FMA)
    _, orc, _, _ = stream(spec, [8192, 256], F, q15=q15, device=False)
    last = (channels - PERIOD) // PERIOD * PERIOD                   # a whole period of roles in the third chunk
    assert last >= 2 * (1024 if q15 else 512)
    assert orc.held[last + R["silent"]] == 8448 // F and orc.p[last + R["p_clamp"]] > 0.1 and orc.held[last + R["all_three"]] == 0


# ---- combinations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("F", FRAMES)
def test_with_the_blanker_behind_it(F, q15):
    """the blanker reads the corrected f32 copy: its state equals that of the reference instance's blanker, fed the restatement's output"""
    spec = rc.baseline_spec("cfg3", CH, rc.ARITH_AUTO)
    cuts = [1024, 768, 1280]
    x = make_stream(CH, sum(cuts)).copy()
    x[1, 3 * 128 + 40] = 4.0                                       # impulses for the blanker to find
    x[4, 1024 + 5 * 128 + 3] = 4.0
    if q15:
        x = to_q15(x * np.float32(0.25))
    rx, _, ref, _ = stream(spec, cuts, F, device=[True, False], x=x, prepare=lambda r: r.set_nb(64))
    a, b = rx.nb_state(), ref.nb_state()
    for k in a:
        assert_bits(a[k], b[k], "blanker " + k)
    assert a["blanked"][1] > 0 and a["blanked"][4] > 0 and a["level"].any()


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_with_the_spectrum_tap_rows_are_of_the_raw_input(q15):
    spec = rc.baseline_spec("cfg3", CH, rc.ARITH_AUTO)
    cuts = [1024, 768, 2304]
    x = make_stream(CH, sum(cuts), q15)
    rx, orc, _, _ = stream(spec, cuts, 64, device=[True, False], x=x, prepare=lambda r: r.set_spectrum(64, 1, 1, 0.25))
    tap = so.Spectrum(CH, 64, 1, 1, 0.25)
    tap.process(x)
    assert_bits(rx.spectrum()[0], tap.rows, "rows on the raw input")
    corrected = so.Spectrum(CH, 64, 1, 1, 0.25)
    corrected.process(io.Corrector(CH, 64, **DEFAULTS).process(x))
    assert corrected.rows.tobytes() != tap.rows.tobytes()         # (... which the corrected input would not give)


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("arith", [rc.ARITH_CMSIS, rc.ARITH_AUTO], ids=["cmsis", "auto"])
def test_with_the_output_stage(arith, q15):
    """(int16 slots: the stage's own arm_float_to_q15 on the same f32 audio -- as bits in every mode)"""
    spec = rc.baseline_spec("cfg3", CH, arith)
    h = sr.design_interp(32, 4, 0.1)
    rx, ref = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (rx, ref):
        r.set_out(4, h, sr.OUT_STEREO)
    rx.set_iqc(64, **DEFAULTS)
    orc = io.Corrector(CH, 64, **DEFAULTS)
    x = make_stream(CH, 1792, q15)
    for i, (at, bs) in enumerate(((0, 1024), (1024, 768))):
        data = np.ascontiguousarray(x[:, at:at + bs])
        got, want = run(rx, data, i == 0), run(ref, orc.process(data), i == 0)
        assert_bits(got, nro.float_to_q15(want) if q15 else want, "call %d" % i)
        check(rx, orc, "call %d" % i)
    chain_state_equal(rx, ref)
    assert_bits(rx.out_state(), ref.out_state(), "output stage history")


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("arith", [rc.ARITH_FMA, rc.ARITH_AUTO], ids=["fma", "auto"])
def test_with_nlms(arith, q15):
    spec = rc.baseline_spec("cfg3", CH, arith)
    stream(spec, [1024, 768], 128, q15=q15, device=[False, True], prepare=lambda r: r.set_nr(sr.NR_DENOISE, num_taps=16, delay=8, mu=0.05))


@pytest.mark.parametrize("F", FRAMES)
def test_global_gain_one_call_and_split_calls(F):
    ch, bs = CH, 1024
    spec = rc.baseline_spec("cfg3", ch, rc.ARITH_CMSIS, agc_global=True)
    # the one-call entries: process_f32_device / the host call on an agc_global instance
    stream(spec, [bs, 256, bs], F, device=[True, False])
    # phase 1 + phase 2, and selenite_rx_global_process_f32_device: the stage runs in phase 1 (phase 2 has no input)
    a, b, ref = sr.Rx(spec.config()), sr.Rx(spec.config()), sr.Rx(spec.config())
    orc = io.Corrector(ch, F, **DEFAULTS)
    for r in (a, b):
        r.set_iqc(F, **DEFAULTS)
    nout = bs // 4
    x = make_stream(ch, 3 * bs)
    d_in, d_out, d_env = sr.DeviceBuffer(ch * bs * 8), sr.DeviceBuffer(ch * nout * 4), sr.DeviceBuffer(4 * (bs // 256))
    a.L.selenite_rx_global_process_f32_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    for call in range(3):
        iq = np.ascontiguousarray(x[:, call * bs:(call + 1) * bs])
        want = ref.process(orc.process(iq))
        d_in.upload(iq)
        a.global_phase1(d_in.ptr, d_out.ptr, d_env.ptr, bs)
        a.sync()
        check(a, orc, "behind phase 1 of call %d" % call)
        a.global_phase2(d_out.ptr, d_env.ptr, bs)
        a.sync()
        assert_bits(d_out.download((ch, nout), np.float32), want, "split calls, audio %d" % call)
        check(a, orc, "behind phase 2 of call %d" % call)
        assert b.L.selenite_rx_global_process_f32_device(b.h, d_in.ptr, d_out.ptr, bs, None) == 0
        b.sync()
        assert_bits(d_out.download((ch, nout), np.float32), want, "one entry, audio %d" % call)
        check(b, orc, "one entry, call %d" % call)
    chain_state_equal(a, ref); chain_state_equal(b, ref)
    d_in.free(); d_out.free(); d_env.free()


def test_global_gain_on_int16_slots():
    spec = rc.baseline_spec("cfg3", CH, rc.ARITH_FMA, agc_global=True)
    stream(spec, [1024, 512], 64, q15=True, device=[True, False])


def test_timing_calls_run_the_stage():
    ch, bs, F = 16, 1024, 64
    spec = rc.baseline_spec("cfg3", ch, rc.ARITH_AUTO)
    rx = sr.Rx(spec.config())
    rx.set_iqc(F, **DEFAULTS)
    orc = io.Corrector(ch, F, **DEFAULTS)
    iq, qi = make_stream(ch, bs), make_stream(ch, bs, q15=True)
    d_in, d_q, d_out = sr.DeviceBuffer(iq.nbytes), sr.DeviceBuffer(qi.nbytes), sr.DeviceBuffer(ch * bs)
    d_in.upload(iq); d_q.upload(qi)
    rx.time_process(d_in.ptr, d_out.ptr, bs, 3)
    rx.time_process_each(d_in.ptr, d_out.ptr, bs, 2)
    rx.time_process_q15(d_q.ptr, d_out.ptr, bs, 2)
    rx.time_process_each(d_q.ptr, d_out.ptr, bs, 1, q15=True)
    for data in [iq] * 5 + [qi] * 3:
        orc.process(data)
    check(rx, orc)
    d_in.free(); d_q.free(); d_out.free()


# ---- non-finite input -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", FRAMES)
def test_a_nan_sample_and_an_inf_sample(F):
    """each in a channel of its own: the frame's estimate is held and the rail's dc keeps its value; the sample itself goes on to the chain
    (its audio is the chain's business); the stage raises no status of its own"""
    spec = rc.baseline_spec("cfg1", CH, rc.ARITH_CMSIS)
    _, orc, _, _ = stream(spec, [1024, 1024], F, device=True, nonfinite=True)
    assert orc.held[R["nan"]] == 1 and orc.held[R["inf"]] == 1 and orc.held[R["balanced"]] == 0
    for k in FLOATS:
        assert np.isfinite(getattr(orc, k)).all(), k
    # ... and without the NaN and the Inf the status stays clean
    x = make_stream(CH, 1024, nonfinite=False)
    rx2 = sr.Rx(spec.config())
    rx2.set_iqc(F, **DEFAULTS)
    assert np.isfinite(run(rx2, x, device=True)).all() and rx2.status() == 0


# ---- life cycle -------------------------------------------------------------------------------------------------------------------
GOOD = dict(frame=64, alpha=0.5, dc_alpha=0.25, p_max=0.5, g_max=2.0, min_power=1e-9, p_init=0.1, g_init=0.75, dc_i_init=0.01, dc_q_init=-0.01)
BAD = [("frame", 0, sr.LENGTH_ERROR), ("frame", 48, sr.LENGTH_ERROR), ("frame", 256, sr.LENGTH_ERROR), ("alpha", -0.1, sr.ARGUMENT_ERROR),
       ("alpha", 1.5, sr.ARGUMENT_ERROR), ("alpha", float("nan"), sr.ARGUMENT_ERROR), ("dc_alpha", 1.5, sr.ARGUMENT_ERROR),
       ("dc_alpha", float("nan"), sr.ARGUMENT_ERROR), ("p_max", 0.0, sr.ARGUMENT_ERROR), ("p_max", 1.5, sr.ARGUMENT_ERROR),
       ("p_max", float("nan"), sr.ARGUMENT_ERROR), ("g_max", 0.5, sr.ARGUMENT_ERROR), ("g_max", float("inf"), sr.ARGUMENT_ERROR),
       ("min_power", -1.0, sr.ARGUMENT_ERROR), ("min_power", float("inf"), sr.ARGUMENT_ERROR), ("p_init", 0.6, sr.ARGUMENT_ERROR),
       ("p_init", float("nan"), sr.ARGUMENT_ERROR), ("g_init", 0.4, sr.ARGUMENT_ERROR), ("g_init", 2.5, sr.ARGUMENT_ERROR),
       ("dc_i_init", float("inf"), sr.ARGUMENT_ERROR), ("dc_q_init", float("nan"), sr.ARGUMENT_ERROR), ("struct_size", 40, sr.ARGUMENT_ERROR)]


def test_bad_fields_leave_a_working_stage_as_it_was():
    spec = rc.baseline_spec("cfg1", 20, rc.ARITH_CMSIS)
    x = make_stream(20, 1280)
    rx, orc, ref, _ = stream(spec, [768], 32, x=x)
    for field, value, code in BAD:
        g = sr.IqcConfig()
        g.struct_size = C.sizeof(sr.IqcConfig)
        for k, v in GOOD.items():
            setattr(g, k, v)
        setattr(g, field, value)
        assert rx.L.selenite_rx_set_iqc(rx.h, C.byref(g)) == code, (field, value)
        assert rx.status() == 0 and rx.L.selenite_rx_error_string(None)
    check(rx, orc, "behind the refused calls")
    iq = np.ascontiguousarray(x[:, 768:])
    assert_bits(rx.process(iq), ref.process(orc.process(iq)))
    check(rx, orc, "the call behind them")
    # ... and the good one is taken: the inits and the limits at their edges
    rx.set_iqc(**GOOD)
    st = rx.iqc_state()
    assert (st["p"] == np.float32(0.1)).all() and (st["g"] == np.float32(0.75)).all() and (st["dc_i"] == np.float32(0.01)).all() and not st["held"].any()
    rx.set_iqc(64, alpha=0.0, dc_alpha=1.0, p_max=1.0, g_max=1.0, min_power=0.0, p_init=-1.0, g_init=1.0)


def test_python_face_keeps_the_stage_on_a_refusal():
    rx = sr.Rx(rc.baseline_spec("cfg1", 8, rc.ARITH_CMSIS).config())
    with pytest.raises(sr.RxError):
        rx.iqc_state()
    rx.set_iqc(64)
    with pytest.raises(sr.RxError) as ei:
        rx.set_iqc(64, p_max=2.0)
    assert ei.value.code == sr.ARGUMENT_ERROR
    assert rx.iqc_state()["p"].shape == (8,)


@pytest.mark.parametrize("F", FRAMES)
def test_manual_calibration_inits_reset_and_removal(F):
    """alpha = 0 and dc_alpha = 0: the inits are the calibration, applied and never moved; then reset and removal of an estimating stage"""
    spec = rc.baseline_spec("cfg3", CH, rc.ARITH_CMSIS)
    manual = dict(alpha=0.0, dc_alpha=0.0, p_init=0.0697, g_init=0.928, dc_i_init=-0.03, dc_q_init=0.02)
    _, orc, _, _ = stream(spec, [1024, 512], F, par=manual)
    assert not orc.held.any() and (orc.p == np.float32(0.0697)).all() and (orc.dc_q == np.float32(0.02)).all()
    inits = dict(p_init=0.05, g_init=1.1, dc_i_init=0.01, dc_q_init=-0.02)
    cuts = [1024, 512]
    rx, orc, ref, first = stream(spec, cuts, F, par=inits)
    assert orc.held.any() and (orc.p != np.float32(0.05)).any()
    # reset: the four floats back to their inits and held to zero, with the chain's state; the same stream gives the same audio again
    rx.reset(); ref.reset(); orc.reset()
    check(rx, orc, "behind reset")
    st = rx.iqc_state()
    assert (st["p"] == np.float32(0.05)).all() and (st["g"] == np.float32(1.1)).all() and (st["dc_i"] == np.float32(0.01)).all()
    assert (st["dc_q"] == np.float32(-0.02)).all() and not st["held"].any()
    x = make_stream(CH, sum(cuts))
    again = [rx.process(np.ascontiguousarray(x[:, :1024])), rx.process(np.ascontiguousarray(x[:, 1024:]))]
    assert_bits(np.concatenate(again, axis=1), first, "the stream again behind reset")
    for part in (x[:, :1024], x[:, 1024:]):
        ref.process(orc.process(np.ascontiguousarray(part)))
    check(rx, orc, "behind the second run")
    # removal: the next call equals that of the instance that never had the stage; the state calls refuse
    rx.set_iqc(None)
    with pytest.raises(sr.RxError):
        rx.iqc_state()
    v = sr.IqcStateView(None, None, None, None, None)
    assert rx.L.selenite_rx_get_iqc_state(rx.h, C.byref(v)) == sr.ARGUMENT_ERROR
    assert rx.L.selenite_rx_set_iqc_state(rx.h, C.byref(v)) == sr.ARGUMENT_ERROR
    iq = make_stream(CH, 768)
    assert_bits(run(rx, iq, device=True), run(ref, iq, device=True), "behind removal")
    chain_state_equal(rx, ref)
    # set again: state from the inits, the chain's state untouched
    rx.set_iqc(F, **DEFAULTS)
    orc = io.Corrector(CH, F, **DEFAULTS)
    check(rx, orc, "behind the second set_iqc")
    assert_bits(rx.process(iq), ref.process(orc.process(iq)))
    check(rx, orc, "second stage")


def test_an_instance_that_had_the_stage_equals_one_that_never_had():
    for name, q15 in (("cfg3", False), ("cfg3", True), ("cfg4", True)):
        spec = rc.baseline_spec(name, 19, rc.ARITH_AUTO)
        a, b = sr.Rx(spec.config()), sr.Rx(spec.config())
        a.set_iqc(128)
        a.set_iqc(None)
        cuts, at = [1024, 256, 768], 0
        x = make_stream(19, sum(cuts), q15)
        for i, bs in enumerate(cuts):
            data = np.ascontiguousarray(x[:, at:at + bs])
            at += bs
            assert_bits(run(a, data, i % 2 == 1), run(b, data, i % 2 == 1), "%s call %d" % (name, i))
        chain_state_equal(a, b)


def test_set_mode_set_nr_set_out_set_spectrum_set_nb_between_calls_leave_the_stage_alone():
    F = 64
    spec = rc.baseline_spec("cfg3", 23, rc.ARITH_AUTO)
    rx, ref = sr.Rx(spec.config()), sr.Rx(spec.config())
    rx.set_iqc(F, **DEFAULTS)
    orc = io.Corrector(23, F, **DEFAULTS)
    h = sr.design_interp(16, 2, 0.2)
    steps = [lambda r: None, lambda r: r.set_mode(sr.MODE_LSB), lambda r: r.set_nr(sr.NR_NOTCH, num_taps=8, delay=4, mu=0.1),
             lambda r: r.set_spectrum(64), lambda r: r.set_nb(32), lambda r: r.set_mode(sr.MODE_AM), lambda r: r.set_out(2, h, sr.OUT_MONO),
             lambda r: r.set_mode(sr.MODE_FM)]
    x = make_stream(23, 768 * len(steps))
    for i, step in enumerate(steps):
        step(rx); step(ref)
        iq = np.ascontiguousarray(x[:, 768 * i:768 * (i + 1)])
        assert_bits(run(rx, iq, device=i % 2 == 1), run(ref, orc.process(iq), device=i % 2 == 1), "audio %d" % i)
        check(rx, orc, "step %d" % i)
    chain_state_equal(rx, ref)


@pytest.mark.parametrize("F", FRAMES)
def test_state_round_trip_continues_the_stream(F):
    spec = rc.baseline_spec("cfg3", CH, rc.ARITH_CMSIS)
    cuts = [1024, 512, 768, 256]
    x = make_stream(CH, sum(cuts))
    a, orc, _, _ = stream(spec, cuts[:2], F, x=x)
    st = a.iqc_state()
    assert st["p"].any() and st["held"].any()
    b = sr.Rx(spec.config())
    b.set_iqc(F, **DEFAULTS)
    b.set_iqc_state(st)
    b.set_state(a.state())
    for at, bs in ((1536, 768), (2304, 256)):
        iq = np.ascontiguousarray(x[:, at:at + bs])
        assert_bits(b.process(iq), a.process(iq)); orc.process(iq)
        check(a, orc, "a at %d" % at); check(b, orc, "b at %d" % at)
    # a partial view: p alone
    pv = np.full(CH, 0.125, np.float32)
    b.set_iqc_state(dict(p=pv))
    st2 = b.iqc_state()
    assert_bits(st2["p"], pv); assert_bits(st2["g"], orc.g); assert_bits(st2["dc_i"], orc.dc_i); assert_bits(st2["held"], orc.held)
