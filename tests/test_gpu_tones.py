"""GPU: the tone-detector bank (selenite_rx_set_tones, csrc/rx_tones.hip: k_tones<KL>) against the reference's own functions
(tests/golden/tones.npz) and against the numpy restatement (tests/tones_oracle.py, pinned to that fixture by tests/test_tones_oracle.py).
The stage is a tap: the restatement is fed the un-scaled audio -- the oracle chain's with its AGC off in _CMSIS / _FMA (which the call's own
audio must equal on bits), the library's own audio of the same call with agc_enable = 0 and no other audio stage in _SPLIT16 / _AUTO -- and
every row of the state is compared on bits behind every call."""
import copy
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import afilt_oracle as afo
import nr_oracle as nro
import rxcommon as rc
import selenite_rx as sr
import tones_oracle as to

pytestmark = pytest.mark.gpu

KERNEL_TILE = 64          # samples of a channel row per tile of k_tones (csrc/rx_tones.hip: kTnTile)
ARITHS = (rc.ARITH_CMSIS, rc.ARITH_FMA, rc.ARITH_SPLIT16, rc.ARITH_AUTO)
ARITH_IDS = ["cmsis", "fma", "split16", "auto"]
PAR = dict(frame_blocks=3, confirm=2, release=2, ratio=0.02, min_power=1e-6)


def table(K, seed=1):
    rng = np.random.default_rng(7000 * seed + K)
    return sr.design_tones(np.sort(rng.uniform(0.01, 0.49, K)))


def to_q15(iq):
    return np.clip(np.trunc(iq * 32768.0), -32768, 32767).astype(np.int16)


def q15_to_f32(q):
    return q.astype(np.float32) / np.float32(32768.0)


def assert_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.itemsize]
        bad = np.argwhere(got.view(u) != want.view(u))
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def assert_state(rx, exp, what=""):
    got, want = rx.tones_state(), exp.state()
    assert set(got) == set(want)
    for k in want:
        assert_bits(got[k], want[k], "%s: %s" % (what, k))


def run_device(rx, data):
    q15 = data.dtype == np.int16
    ch, bs = data.shape[0], data.shape[1]
    vals = rx.out_len(bs)
    d_in, d_out = sr.DeviceBuffer(data.nbytes), sr.DeviceBuffer(ch * vals * data.dtype.itemsize)
    d_in.upload(np.ascontiguousarray(data))
    (rx.process_q15_device if q15 else rx.process_device)(d_in.ptr, d_out.ptr, bs)
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


class Tap:
    """An instance of `spec` (AGC off) with the bank, an instance without it, the restatement, and in _CMSIS / _FMA the oracle chain: call()
    runs one call everywhere and compares the audio and every row of the stage's state on bits."""

    def __init__(self, spec, K, par=PAR, seed=1):
        assert not spec.agc
        self.spec, self.coeffs = spec, table(K, seed)
        self.a, self.b = sr.Rx(spec.config()), sr.Rx(spec.config())
        self.a.set_tones(self.coeffs, **par)
        self.exp = to.Tones(spec.channels, spec.block // spec.decim, self.coeffs, **par)
        self.orc = rc.CpuChain(spec, "orc") if spec.arith in (rc.ARITH_CMSIS, rc.ARITH_FMA) else None
        self.at = 0

    def call(self, bs, device=False, q15=False):
        iq = rc.synth_iq(0, self.spec.channels, self.at, bs)
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


# ---- 1. the reference's own vectors through the library -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(rc.GOLDEN_DIR, "tones.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", range(7))
def test_golden_vectors_through_the_library(gold, case):
    """an instance whose chain passes the I rail through (no NCO, no decimator, no FIR pair, AGC off, DSP block 1): the fixture's streams go
    in as I, frames of N blocks; behind every call the recurrence state and the running energy equal the fixture's, behind every frame the
    powers, the frame energy and arm_max_f32's index"""
    K, N = (int(v) for v in gold["cases"][case])
    g = {k: gold["k%d_n%d/%s" % (K, N, k)] for k in ("coeffs", "x", "lens", "call_s", "call_e", "p", "fe", "best")}
    spec = rc.ChainSpec(2, 1, 1, 0, 0, 0, sr.MODE_USB, rc.ARITH_CMSIS, agc=False)
    rx = sr.Rx(spec.config())
    rx.set_tones(g["coeffs"], frame_blocks=N)
    at = 0
    for i, n in enumerate(int(v) for v in g["lens"]):
        iq = np.zeros((2, n, 2), np.float32)
        iq[..., 0] = g["x"][:, at:at + n]
        got = run_device(rx, iq)
        assert got.tobytes() == g["x"][:, at:at + n].tobytes(), "the chain does not pass the I rail through as it is"
        at += n
        st = rx.tones_state()
        assert_bits(st["s"], g["call_s"][:, i], "s behind call %d" % i)
        assert_bits(st["energy"], g["call_e"][:, i], "E behind call %d" % i)
        assert st["position"][0] == at
        f = at // N
        if f:
            assert_bits(st["power"], g["p"][:, f - 1], "p of frame %d" % (f - 1))
            assert_bits(st["frame_energy"], g["fe"][:, f - 1], "E of frame %d" % (f - 1))
            assert_bits(st["last_best"], g["best"][:, f - 1], "best of frame %d" % (f - 1))
    assert rx.tones()[2] == 2


# ---- 2. groups, wave remainders, every KL and its edges --------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [1, 3])
@pytest.mark.parametrize("K", [1, 5, 8, 9, 17, 33, 50, 64])
@pytest.mark.parametrize("ch", [1, 3, 65, 130])
def test_channels_by_tones(ch, K, fb):
    """n = 24: calls of 1, 2 and 5 DSP blocks (24, 48 and 120 samples: under a tile, and a tile and a ragged one).  frame_blocks 3: the frames
    straddle the calls; frame_blocks 1: one call ends two and five frames"""
    t = Tap(rc.ChainSpec(ch, 96, 4, 64, 31, 0, sr.MODE_USB, rc.ARITH_CMSIS, nco=True, nco_step_all=0x01000000, agc=False), K, dict(PAR, frame_blocks=fb))
    for i, blocks in enumerate((1, 2, 5)):
        t.call(96 * blocks, device=i == 1)
    assert t.exp.position == 8 and t.a.tones()[2] == 8 // fb


@pytest.mark.parametrize("fb", [1, 3])
@pytest.mark.parametrize("n", [12, 24, 64, 96])
def test_block_lengths_and_tile_edges(n, fb):
    """n = 12 (five blocks are 60 samples: under a tile), 24, 64 (a block is a tile), 96 (a tile and a half)"""
    spec = {12: rc.ChainSpec(35, 96, 8, 64, 31, 0, sr.MODE_USB, rc.ARITH_CMSIS, nco=True, nco_step_all=0x01000000, agc=False),
            24: rc.ChainSpec(35, 96, 4, 64, 31, 0, sr.MODE_USB, rc.ARITH_CMSIS, nco=True, nco_step_all=0x01000000, agc=False),
            64: no_agc(rc.baseline_spec("cfg3", 35, rc.ARITH_CMSIS)),
            96: rc.ChainSpec(35, 96, 1, 0, 31, 0, sr.MODE_USB, rc.ARITH_CMSIS, agc=False)}[n]
    assert spec.block // spec.decim == n
    for K in (5, 50):
        t = Tap(spec, K, dict(PAR, frame_blocks=fb))
        for i, blocks in enumerate((1, 2, 5, 1)):
            t.call(spec.block * blocks, device=i % 2 == 0)


def test_one_call_of_2048_equals_eight_calls_of_256():
    spec = no_agc(rc.baseline_spec("cfg1", 70, rc.ARITH_CMSIS))
    one, many = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (one, many):
        r.set_tones(table(17), **PAR)
    iq = rc.synth_iq(0, 70, 0, 2048)
    run_device(one, iq)
    for a in range(0, 2048, 256):
        run_device(many, np.ascontiguousarray(iq[:, a:a + 256]))
    s1, s2 = one.tones_state(), many.tones_state()
    for k in s1:
        assert_bits(s1[k], s2[k], k)
    assert s1["position"][0] == 8 and s1["power"].any() and s1["s"].any()


# ---- 3. modes and arith modes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
@pytest.mark.parametrize("mode", ["usb", "cw", "am", "fm"])
def test_modes_and_arith_modes(mode, arith):
    if mode == "usb":
        spec, calls = no_agc(rc.baseline_spec("cfg3", 70, arith)), (1024, 2048, 256)
    elif mode == "cw":
        spec, calls = no_agc(rc.baseline_spec("cfg4", 70, arith)), (512, 256, 768)           # behind the CW filter
        assert spec.n_biquad == 4
    else:
        spec, calls = no_agc(rc.baseline_spec("cfg1", 33, arith)), (512, 256, 768)
        spec.mode = sr.MODE_AM if mode == "am" else sr.MODE_FM
    t = Tap(spec, 9)
    for i, bs in enumerate(calls):
        t.call(bs, device=i == 1)
    assert t.exp.power.any()


@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
def test_int16_slots(arith):
    t = Tap(no_agc(rc.baseline_spec("cfg3", 35, arith)), 33)
    for i, bs in enumerate((1024, 256, 1536)):
        t.call(bs, device=i == 1, q15=True)


def test_call_cut_in_two_under_split16():
    """a call the dispatcher cuts (whole passes and a tail): each part is a launch of its own, the second one behind the blocks of the first
    -- frames of 3 blocks against parts of 8 + 1, 8 + 3 and 16 + 1 blocks"""
    spec = rc.ChainSpec(35, 128, 4, 256, 63, 0, sr.MODE_USB, rc.ARITH_SPLIT16, nco=True, nco_step_all=0x01000000, agc=False)
    t = Tap(spec, 17)
    for bs in (1152, 1408, 2176, 128):
        t.call(bs, device=True)
    assert t.exp.position == 38


# ---- 4. the global-gain entries ------------------------------------------------------------------------------------------------------------------
def test_global_gain_every_entry():
    """phase 1 runs the stage, phase 2 does not; the one-call form and the process entry run it once"""
    ch, bs = 35, 1024
    sa, sb = rc.baseline_spec("cfg3", ch, rc.ARITH_CMSIS, agc_global=True), no_agc(rc.baseline_spec("cfg3", ch, rc.ARITH_CMSIS))
    nout = bs // 4
    d_in, d_out, d_env = sr.DeviceBuffer(ch * bs * 8), sr.DeviceBuffer(ch * nout * 4), sr.DeviceBuffer(4 * (bs // 256))

    def one_call(rx, iq):
        return rx.process(iq)

    def split(rx, iq):
        d_in.upload(iq)
        rx.global_phase1(d_in.ptr, d_out.ptr, d_env.ptr, bs)
        rx.sync()
        mid = rx.tones_state()
        rx.global_phase2(d_out.ptr, d_env.ptr, bs)
        rx.sync()
        after = rx.tones_state()
        for k in mid:
            assert_bits(after[k], mid[k], "phase 2 moved " + k)
        return d_out.download((ch, nout), np.float32)

    def process_entry(rx, iq):
        rx.L.selenite_rx_global_process_f32_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        d_in.upload(iq)
        assert rx.L.selenite_rx_global_process_f32_device(rx.h, d_in.ptr, d_out.ptr, bs, None) == 0
        rx.sync()
        return d_out.download((ch, nout), np.float32)

    from test_gpu_nr import GlobalGain
    coeffs = table(9)
    for entry in (one_call, split, process_entry):
        a, b = sr.Rx(sa.config()), sr.Rx(sb.config())
        a.set_tones(coeffs, **PAR)
        exp, gg = to.Tones(ch, 64, coeffs, **PAR), GlobalGain(sa)
        for call in range(2):
            iq = rc.synth_iq(0, ch, call * bs, bs)
            pre = b.process(iq)
            assert_bits(entry(a, iq), gg.process(pre), "%s, call %d" % (entry.__name__, call))
            exp.process(pre)
            assert_state(a, exp, "%s, call %d" % (entry.__name__, call))
        assert exp.position == 8
    d_in.free(); d_out.free(); d_env.free()


# ---- 5. a host-pointer call cut into ragged channel chunks -------------------------------------------------------------------------------
def test_host_pointer_call_across_ragged_channel_chunks():
    """cfg3, 300 channels x 2048 samples with a 1 MiB chunk: 64-channel chunks and a ragged last one of 44: the state rows of a chunk move with
    its first channel and `position` advances once per call, not per chunk.  (A subprocess: the library reads SELENITE_RX_HOST_CHUNK_MB
    once.)"""
    code = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import rxcommon as rc, selenite_rx as sr, test_gpu_tones as t
        nch, bs = 300, 2048
        spec = rc.baseline_spec("cfg3", nch, rc.ARITH_AUTO)
        dev, hst = sr.Rx(spec.config()), sr.Rx(spec.config())
        for r in (dev, hst):
            r.set_tones(t.table(9), **t.PAR)
        for call in range(3):
            iq = rc.synth_iq(0, nch, call * bs, bs)
            t.assert_bits(hst.process(iq), t.run_device(dev, iq), "call %%d" %% call)
            a, b = hst.tones_state(), dev.tones_state()
            for k in a:
                t.assert_bits(a[k], b[k], "call %%d: %%s" %% (call, k))
        assert a["position"][0] == 24 and a["power"][250:].any() and a["frame_energy"][250:].all() and hst.tones()[2] == 8      # (24 blocks are 8 whole frames: s is +0.0f)
        print("OK")
    """ % (os.path.join(rc.ROOT, "tests"), rc.PKG_DIR))
    env = dict(os.environ, SELENITE_RX_HOST_CHUNK_MB="1")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), (out.stdout[-1000:], out.stderr[-3000:])


def test_timing_entry_point_advances_position():
    ch, bs = 35, 1024
    spec = no_agc(rc.baseline_spec("cfg3", ch, rc.ARITH_CMSIS))
    rx, ref = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (rx, ref):
        r.set_tones(table(9), **PAR)
    iq = rc.synth_iq(0, ch, 0, bs)
    d_in, d_out = sr.DeviceBuffer(iq.nbytes), sr.DeviceBuffer(ch * (bs // 4) * 4)
    d_in.upload(iq)
    assert rx.time_process(d_in.ptr, d_out.ptr, bs, 3) > 0          # three calls on the same input: the stream runs on
    rx.sync()
    for _ in range(3):
        ref.process(iq)
    a, b = rx.tones_state(), ref.tones_state()
    for k in a:
        assert_bits(a[k], b[k], k)
    assert a["position"][0] == 12
    d_in.free(); d_out.free()


# ---- 6. the tap changes nothing -----------------------------------------------------------------------------------------------------------------
def test_the_tap_changes_nothing_with_every_neighbour_on():
    """afilt + NLMS + meter (gate 1) + AGC + output stage: audio, chain state and those stages' states equal on bits the same calls without
    the bank; the bank's rows equal the restatement fed the audio in front of the filter"""
    ch = 35
    spec = rc.baseline_spec("cfg3", ch, rc.ARITH_CMSIS)
    k5, h = sr.design_biquad(sr.BIQUAD_HIGHPASS, 300.0 / 12000.0, 0.7071).reshape(1, 5), sr.design_interp(32, 4, 0.1)
    par = dict(sense=sr.SQ_ABOVE, gate=1, hang=1, attack=0.5, decay=0.9375, open_level=2e-2, close_level=4e-3, level_init=0.0)
    a, b = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (a, b):
        r.set_afilt(k5)
        r.set_nr(sr.NR_DENOISE, num_taps=16, delay=8, mu=0.05)
        r.set_meter(**par)
        r.set_out(4, h, sr.OUT_STEREO)
    coeffs = table(50)
    a.set_tones(coeffs, **PAR)
    orc, exp = rc.CpuChain(no_agc(spec), "orc"), to.Tones(ch, 64, coeffs, **PAR)
    at = 0
    for i, bs in enumerate((1024, 256, 2048)):
        iq = rc.synth_iq(0, ch, at, bs)
        assert_bits(run(a, iq, device=i == 1), run(b, iq, device=i == 1), "call %d" % i)
        exp.process(orc.process(iq))
        assert_state(a, exp, "call %d" % i)
        at += bs
    for name, sa, sb in (("chain", a.state(), b.state()), ("afilt", a.afilt_state(), b.afilt_state()), ("nr", a.nr_state(), b.nr_state()),
                         ("meter", a.meter_state(), b.meter_state())):
        for k in sa:
            assert_bits(np.asarray(sa[k]), np.asarray(sb[k]), "%s state: %s" % (name, k))
    assert_bits(a.out_state(), b.out_state(), "output stage state")


# ---- 7. life cycle ------------------------------------------------------------------------------------------------------------------------------
def test_state_round_trip_reset_set_mode_and_the_other_setters():
    ch = 33
    spec = no_agc(rc.baseline_spec("cfg1", ch, rc.ARITH_CMSIS))
    coeffs = table(17)
    rx, fresh = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (rx, fresh):
        r.set_tones(coeffs, **PAR)
    exp = to.Tones(ch, 256, coeffs, **PAR)
    assert_state(rx, exp, "behind set_tones")
    s0 = rx.tones_state()
    assert not any(np.signbit(s0[k]).any() for k in ("s", "energy", "power", "frame_energy")) and (s0["tone"] == sr.TONE_NONE).all()
    rx.process(rc.synth_iq(0, ch, 0, 1024))                         # a frame and a third
    st, g = rx.tones_state(), rx.state()
    assert st["s"].any() and st["power"].any() and st["position"][0] == 4
    nxt = rc.synth_iq(0, ch, 1024, 1280)
    rx.process(nxt)
    fresh.set_state(g)
    fresh.set_tones_state(st)
    fresh.process(nxt)
    a, b = rx.tones_state(), fresh.tones_state()
    for k in a:
        assert_bits(a[k], b[k], "after set_tones_state: " + k)
    assert a["position"][0] == 9
    # set_mode and the other setters keep the state and the table
    assert rx.set_mode(sr.MODE_LSB) == 0
    rx.set_nr(sr.NR_NOTCH, num_taps=16, delay=4, mu=0.1); rx.set_nr(sr.NR_OFF)
    rx.set_meter(); rx.set_meter(sense=None)
    rx.set_afilt(sr.design_deemphasis(0.9)); rx.set_afilt(None)
    rx.set_out(4, sr.design_interp(32, 4, 0.1), sr.OUT_STEREO); rx.set_out(None)
    rx.set_spectrum(64); rx.set_spectrum(None)
    rx.set_nb(); rx.set_nb(None)
    rx.set_iqc(); rx.set_iqc(None)
    b = rx.tones_state()
    for k in a:
        assert_bits(a[k], b[k], "behind the other setters: " + k)
    # the device rows are the host copies
    tone, power = np.empty(ch, np.uint32), np.empty((ch, 17), np.float32)
    assert rx.tones_tone_device() and rx.tones_power_device()
    rx.L.selenite_rx_memcpy_d2h(tone.ctypes.data_as(C.c_void_p), rx.tones_tone_device(), tone.nbytes)
    rx.L.selenite_rx_memcpy_d2h(power.ctypes.data_as(C.c_void_p), rx.tones_power_device(), power.nbytes)
    t2, p2, frames = rx.tones()
    assert_bits(tone, a["tone"]); assert_bits(power, a["power"]); assert_bits(t2, tone); assert_bits(p2, power)
    assert frames == 3
    # reset: back to the state set_tones left, the table kept: the same stream gives the same rows again
    assert rx.reset() == 0
    assert_state(rx, exp, "behind reset")
    rx.set_mode(sr.MODE_USB)
    rx.process(rc.synth_iq(0, ch, 0, 1024))
    b = rx.tones_state()
    for k in st:
        assert_bits(b[k], st[k], "the same stream behind reset: " + k)


BAD = [("n_tones", 0), ("n_tones", 65), ("frame_blocks", 0), ("frame_blocks", 65536), ("confirm", 0), ("confirm", 65536), ("release", 0),
       ("release", 65536), ("reserved", 1), ("struct_size", 36), ("ratio", -0.1), ("ratio", 1.5), ("ratio", float("nan")), ("min_power", -1.0),
       ("min_power", float("inf")), ("coeffs", None), ("nan", None), ("inf", None)]


@pytest.mark.parametrize("field,value", BAD, ids=["%s=%s" % b for b in BAD])
def test_bad_field_is_argument_error_and_the_stage_stays(field, value):
    ch = 16
    spec = no_agc(rc.baseline_spec("cfg1", ch, rc.ARITH_CMSIS))
    rx, ref = sr.Rx(spec.config()), sr.Rx(spec.config())
    for r in (rx, ref):
        r.set_tones(table(5), **PAR)
    iq = rc.synth_iq(0, ch, 0, 512)
    rx.process(iq); ref.process(iq)
    new = table(9, seed=2)
    if field in ("nan", "inf"):
        new[2, 1] = np.nan if field == "nan" else -np.inf
    g = sr.TonesConfig()
    g.struct_size, g.n_tones, g.frame_blocks, g.confirm, g.release, g.reserved = C.sizeof(sr.TonesConfig), 9, 2, 1, 1, 0
    g.ratio, g.min_power, g.coeffs = 0.1, 0.0, new.ctypes.data_as(sr.f32p)
    if field not in ("nan", "inf"):
        setattr(g, field, value)
    assert rx.L.selenite_rx_set_tones(rx.h, C.byref(g)) == sr.ARGUMENT_ERROR
    assert rx.status() == 0
    iq = rc.synth_iq(0, ch, 512, 512)
    rx.process(iq); ref.process(iq)
    a, b = rx.tones_state(), ref.tones_state()
    for k in a:
        assert_bits(a[k], b[k], "after the refused set_tones: " + k)
    assert a["position"][0] == 4


@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
def test_stage_removed_is_no_stage(arith):
    spec = rc.baseline_spec("cfg3", 70, arith)
    a, b = sr.Rx(spec.config()), sr.Rx(spec.config())
    a.set_tones(table(64), **PAR)
    a.set_tones(None)
    for call in range(2):
        iq = rc.synth_iq(0, 70, call * 2048, 2048)
        assert_bits(a.process(iq), b.process(iq), "call %d" % call)
    with pytest.raises(sr.RxError):
        a.tones_state()
    assert a.L.selenite_rx_get_tones_state(a.h, C.byref(sr.TonesStateView())) == sr.ARGUMENT_ERROR
    assert a.L.selenite_rx_set_tones_state(a.h, C.byref(sr.TonesStateView())) == sr.ARGUMENT_ERROR
    assert a.L.selenite_rx_get_tones(a.h, None, None, None) == sr.ARGUMENT_ERROR
    assert a.tones_tone_device() is None and a.tones_power_device() is None


def test_a_frame_with_an_inf_sample_poisons_only_itself(gold):
    """the pass-through chain of the golden test, frames of 24 samples: an Inf in frame 1 makes that frame's powers NaN and no hit; frames 0
    and 2 equal the rows of the same stream without it"""
    coeffs, x = gold["k5_n24/coeffs"], gold["k5_n24/x"][:, :60].copy()
    bad = x.copy()
    bad[0, 30] = np.inf
    spec = rc.ChainSpec(2, 1, 1, 0, 0, 0, sr.MODE_USB, rc.ARITH_CMSIS, agc=False)
    par = dict(frame_blocks=24, confirm=1, release=1, ratio=0.0, min_power=0.0)
    rx, exp, clean = sr.Rx(spec.config()), to.Tones(2, 1, coeffs, **par), to.Tones(2, 1, coeffs, **par)
    rx.set_tones(coeffs, **par)
    rows = []
    for a, n in ((0, 24), (24, 24), (48, 12)):
        iq = np.zeros((2, n, 2), np.float32)
        iq[..., 0] = bad[:, a:a + n]
        assert afo.same_bits(run_device(rx, iq), bad[:, a:a + n])
        exp.process(bad[:, a:a + n])
        clean.process(x[:, a:a + n])
        got, want = rx.tones_state(), exp.state()
        for k in want:
            if want[k].dtype == np.float32:
                assert to.same_bits(got[k], want[k]), (a, k)
                assert_bits(got[k][1], want[k][1], "the stream without the Inf: " + k)
            else:
                assert_bits(got[k], want[k], "%d: %s" % (a, k))
        rows.append(got)
    assert_bits(rows[0]["power"], gold["k5_n24/p"][:, 0])
    assert np.isnan(rows[1]["power"][0]).all() and rows[1]["tone"][0] == sr.TONE_NONE and rows[0]["tone"][0] != sr.TONE_NONE
    assert_bits(rows[2]["s"], clean.s, "the frame behind the poisoned one")
    assert_bits(rows[2]["energy"], clean.energy)
    assert np.isfinite(rows[2]["s"]).all()
