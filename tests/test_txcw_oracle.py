"""CPU: the numpy restatement of the keyed CW path (tests/txcw_oracle.py) against the fixture made from the reference's own CMSIS-DSP
functions (tests/golden/txcw.npz), against a sample-by-sample loop, and what the path is for: the carrier lands where the audio entries in
CW / CWR put a tone of the pitch, the shape lowers the key clicks, and the receiver's tone bank reads the keying back."""
import os

import numpy as np
import pytest

import rxcommon as rc
import selenite_rx as sr
import tones_oracle as to
import txcw_oracle as co
import txfm_oracle as fo

f32 = np.float32
NAMES = ("dits", "hard", "held", "long")


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(rc.GOLDEN_DIR, "txcw.npz")) as z:
        return {k: z[k] for k in z.files}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def fixture_spec(gold, name, arith=rc.ARITH_CMSIS, q15_rounding=False, channels=1):
    """the instance a stream of the fixture describes (tests/test_gpu_txcw.py builds the GPU instance from the same spec)"""
    block, L, nco_step, offset_step, cwr, phase0, side_step, side_phase0 = (int(v) for v in gold[name + "/cfg"])
    ic = gold[name + "/ic"]
    spec = rc.TxSpec(channels, block=block, interp=L, ni_taps=ic.size, nh_taps=0, mode=rc.MODE_CWR if cwr else rc.MODE_CW, arith=arith,
                     nco=nco_step != 0, nco_step_all=nco_step, alc=False, q15_rounding=q15_rounding)
    spec.ic = ic.copy() if ic.size else None
    cw = dict(shape=gold[name + "/shape"], amplitude=float(gold[name + "/par"][0]), offset_step=offset_step, side_level=float(gold[name + "/par"][1]),
              side_step=side_step)
    return spec, cw, phase0, side_phase0


def fixture_oracle(gold, name, side_mix=0, **kw):
    spec, cw, phase0, side_phase0 = fixture_spec(gold, name, **kw)
    o = co.TxCwOracle(spec)
    o.set_cw(side_mix=side_mix, **cw)
    o.set_phase(phase0)
    o.set_cw_state({"side_phase": np.full(spec.channels, side_phase0, np.uint32)})
    return o


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_fixture_f32(gold, name):
    key = gold[name + "/key"][None, :]
    o = fixture_oracle(gold, name)
    out, side = o.process_key(key, side=np.zeros(key.shape, f32))
    assert same_bits(o.last_e[0], gold[name + "/e"])
    assert same_bits(out[0], gold[name + "/out"]) and same_bits(side[0], gold[name + "/y"])
    st = o.state()
    assert st["nco_phase"][0] == gold[name + "/phases"][0] and st["side_phase"][0] == gold[name + "/phases"][1]
    # the pieces: a, u
    a = o.last_e * f32(gold[name + "/par"][0])
    assert same_bits(a[0], gold[name + "/a"])
    u, _ = co.interpolate(o.spec, np.zeros((1, o.p1), f32), a)
    assert same_bits(u[0], gold[name + "/u"])
    # the speaker mix
    o = fixture_oracle(gold, name, side_mix=1)
    _, side = o.process_key(key, side=gold[name + "/side_in"][None, :])
    assert same_bits(side[0], gold[name + "/side_mix"])


@pytest.mark.parametrize("rounding", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_fixture_int16(gold, name, rounding):
    tag = "round" if rounding else "trunc"
    key = gold[name + "/key"][None, :]
    o = fixture_oracle(gold, name, q15_rounding=rounding)
    out, side = o.process_key(key, side=np.zeros(key.shape, np.int16), q15=True)
    assert same_bits(out[0], gold[name + "/q15_" + tag]) and same_bits(side[0], gold[name + "/yq_" + tag])
    o = fixture_oracle(gold, name, side_mix=1, q15_rounding=rounding)
    _, side = o.process_key(key, side=gold[name + "/side_in_q15"][None, :], q15=True)
    assert same_bits(side[0], gold[name + "/side_mix_q_" + tag])


def test_the_int16_builds_differ_and_the_mix_saturates_at_both_ends(gold):
    assert not same_bits(gold["dits/q15_trunc"], gold["dits/q15_round"])
    m = gold["long/side_mix_q_trunc"]
    assert (m == 32767).any() and (m == -32768).any()
    a, b, s = gold["addq15/a"], gold["addq15/b"], gold["addq15/sum"]
    assert (s == 32767).sum() >= 2 and (s == -32768).sum() >= 2
    assert same_bits(co.side_write(a, b.astype(f32) / f32(32768.0), 1), s)      # b / 32768 goes through arm_float_to_q15 unchanged


def test_cut_into_calls_the_oracle_gives_the_same_bits(gold):
    for name in NAMES:
        key = gold[name + "/key"][None, :]
        block = int(gold[name + "/cfg"][0])
        o = fixture_oracle(gold, name)
        parts = [o.process_key(key[:, a:a + block], side=np.zeros((1, block), f32)) for a in range(0, key.shape[1], block)]
        assert same_bits(np.concatenate([p[0] for p in parts], axis=1)[0], gold[name + "/out"])
        assert same_bits(np.concatenate([p[1] for p in parts], axis=1)[0], gold[name + "/y"])


def test_vectorised_oracle_equals_the_sample_by_sample_loop():
    rng = np.random.default_rng(0xC3)
    for ns in (1, 2, 17):
        coeffs = (rng.uniform(-1, 1, ns) / 4).astype(f32)
        hist = (rng.uniform(size=ns - 1) < 0.5).astype(np.uint8)
        keys = (rng.uniform(size=96) < 0.5).astype(np.uint8) * rng.integers(1, 256, 96).astype(np.uint8)
        e, a, y, sp = co.keyed_sequential(keys, hist, coeffs, -0.8, 0xFFFFF000, 0x0DA740DA, 0.3)
        w = (np.concatenate([hist, keys]) != 0).astype(f32)
        ev = co.shape_env(w, coeffs)
        yv, spv = co.sidetone(ev, 0xFFFFF000, 0x0DA740DA, 0.3)
        assert same_bits(ev, e) and same_bits(ev * f32(-0.8), a) and same_bits(yv, y) and spv == sp
        u = rng.uniform(-1, 1, 200).astype(f32)
        out, ph = co.carrier(u, 0xFFFFFF00, 0x3A5F1C27)
        outs, phs = co.carrier_sequential(u, 0xFFFFFF00, 0x3A5F1C27)
        assert same_bits(out, outs) and ph == phs
    # the break-in flag: gaps shorter than, equal to and longer than the hang time
    keys = np.zeros(16 * 4, np.uint8)
    keys[0], keys[3 * 4 + 1], keys[6 * 4 + 3] = 1, 1, 1          # key-down in blocks 0, 3 and 6: gaps of 2 and 2 blocks, then silence
    seq, on, hold = [], 0, 0
    for b in range(16):
        on, hold = co.breakin(keys[b * 4:(b + 1) * 4], 4, on, hold, 2)
        seq.append((on, hold))
    assert seq[:7] == [(1, 2), (1, 1), (1, 0), (1, 2), (1, 1), (1, 0), (1, 2)]
    assert seq[7:11] == [(1, 1), (1, 0), (0, 0), (0, 0)]
    assert co.breakin(keys, 4, 0, 0, 2) == seq[-1]
    assert co.breakin(np.array([1, 0, 0, 0, 0, 0, 0, 0], np.uint8), 4, 0, 0, 0) == (0, 0)     # hang 0: off in the first silent block


def test_cmsis_and_fma_give_the_same_envelope():
    """e0 is 0 or 1: every product of the shaping FIR is exact, a fused tap rounds what the separate add rounds"""
    rng = np.random.default_rng(0xE0)
    # fma_f32 itself, where fusing matters: products that are not representable
    x, c, acc = (rng.uniform(-1, 1, 4096).astype(f32) for _ in range(3))
    fused = co.fma_f32(x, c, acc)
    exact = x.astype(np.float64) * c.astype(np.float64) + acc.astype(np.float64)         # within half an ulp of f64 of the true value
    assert (np.abs(fused.astype(np.float64) - exact) <= np.abs(np.spacing(fused)).astype(np.float64) * 0.5000001).all()
    assert not same_bits(fused, x * c + acc), "on general inputs the fused and the separate forms differ"
    for ns in (1, 2, 64, 97):
        for coeffs in (sr.keyshape(ns), (rng.uniform(-1, 1, ns) / 8).astype(f32)):
            w = (rng.uniform(size=(3, ns - 1 + 256)) < 0.5).astype(f32)
            w[1] = 1.0
            w[2] = 0.0
            e = co.shape_env(w, coeffs)
            assert same_bits(e, co.shape_env_fma(w, coeffs))
            # the steady states: all down is +0.0f on bits, all up is the in-order sum of the taps
            s = f32(0.0)
            for k in range(ns):
                s = f32(s + coeffs[k])
            assert same_bits(e[2], np.zeros(256, f32)) and same_bits(e[1], np.full(256, s, f32))


def test_design_keyshape():
    assert same_bits(sr.keyshape(1), np.ones(1, f32))
    for ns in (2, 3, 16, 63, 64, 65, 97, 256):
        h = sr.keyshape(ns)
        assert h.dtype == np.float32 and h.shape == (ns,) and (h > 0).all()
        assert same_bits(h, h[::-1].copy()), "symmetric on bits"
        assert abs(h.astype(np.float64).sum() - 1.0) <= ns * np.spacing(f32(1.0))
        k = np.arange(ns, dtype=np.float64)
        w = 0.5 - 0.5 * np.cos(2 * np.pi * (k + 1) / (ns + 1))
        assert np.allclose(h, w / w.sum(), rtol=1e-6, atol=0)
        step = np.cumsum(h.astype(np.float64))                     # a raised-cosine edge: monotone from ~0 to 1
        assert (np.diff(step) > 0).all() and step[0] <= 1.0 / ns and abs(step[-1] - 1.0) < 1e-5
    with pytest.raises(ValueError):
        sr.keyshape(0)


# ---- what the path is for ---------------------------------------------------------------------------------------------------------------
FS_AUDIO, L_RF, PITCH_BIN, NFFT = 12000.0, 4, 240, 4096           # the pitch on an FFT bin of the 4096 outputs: 240 / 4096 * 48 kHz = 2812.5 Hz


def held_carrier(mode, nco):
    step = 0x20000000                                             # fs_out / 8: bin 512
    pitch = PITCH_BIN / NFFT * FS_AUDIO * L_RF
    spec = rc.TxSpec(1, block=64, interp=L_RF, ni_taps=256, nh_taps=63, mode=mode, nco=nco, nco_step_all=step, alc=False)
    n = NFFT // L_RF + 512                                        # 512 audio samples for the filters to fill
    o = co.TxCwOracle(spec)
    o.set_cw(sr.keyshape(64), 0.5, sr.tone_step(pitch, FS_AUDIO * L_RF))
    keyed, _ = o.process_key(np.ones((1, n), np.uint8))
    t = np.arange(n)
    tone = (0.5 * np.sin(2 * np.pi * pitch / FS_AUDIO * t)).astype(f32)[None, :]
    audio = rc.TxCpuChain(spec, "orc").process(tone)
    peak = lambda y: int(np.argmax(np.abs(np.fft.fft(y[0, -NFFT:, 0].astype(np.float64) + 1j * y[0, -NFFT:, 1].astype(np.float64)))))
    return peak(keyed), peak(audio)


def test_the_carrier_lands_where_the_audio_entries_put_a_tone_of_the_pitch():
    up, up_audio = held_carrier(rc.MODE_CW, True)
    assert up == up_audio == 512 + PITCH_BIN
    lo, lo_audio = held_carrier(rc.MODE_CWR, True)
    assert lo == lo_audio == 512 - PITCH_BIN, "CWR: the mirrored bin"
    assert held_carrier(rc.MODE_CW, False) == (PITCH_BIN, PITCH_BIN)
    assert held_carrier(rc.MODE_CWR, False) == (NFFT - PITCH_BIN, NFFT - PITCH_BIN), "zero IF: -pitch"


def test_the_shape_lowers_the_key_clicks():
    """a dit string at 32 audio samples per dit (keying rate 12000 / 64 = 187.5 Hz): the energy further than 5 keying rates from the carrier"""
    dit, n = 32, 4096
    key = np.tile(np.repeat(np.array([1, 0], np.uint8), dit), n // (2 * dit))[None, :]
    spec = rc.TxSpec(1, block=64, interp=1, ni_taps=0, nh_taps=0, mode=rc.MODE_CW, nco=False, alc=False)
    far = {}
    for ns in (1, 64):
        o = co.TxCwOracle(spec)
        o.set_cw(sr.keyshape(ns), 1.0, 0x20000000)               # carrier on bin n / 8
        y, _ = o.process_key(key)
        p = np.abs(np.fft.fft(y[0, :, 0].astype(np.float64) + 1j * y[0, :, 1].astype(np.float64))) ** 2
        d = np.abs(((np.arange(n) - n // 8 + n // 2) % n) - n // 2)            # distance from the carrier in bins
        far[ns] = p[d > 5 * n // (2 * dit)].sum() / p.sum()
    print("out-of-band energy fraction: hard keying %.3e, 64-tap shape %.3e" % (far[1], far[64]))
    assert far[64] < far[1]


# The loop through the receiver.  Audio at 12 kHz, L = 4; RX blocks of 64 audio samples, tone frames of 4 blocks = 256 samples, so bin k of
# a frame is k * 46.875 Hz: the pitch on bin 15 (703.125 Hz), the other tones on bins 9, 12 and 18.  Elements and gaps of 5 frames, edges on
# frame boundaries.  Between key and received audio lie the shape (64 taps: the edge is over after 64 samples), the TX interpolator (256
# taps at the output rate: 32 audio samples), the RX decimator (255 taps: 32) and the RX Hilbert pair (63 taps: 31): every edge has
# passed 64 + 32 + 32 + 31 = 159 < 256 samples after the key moved.  So exactly the first frame behind each edge straddles it -- 2 of the
# 10 frames of an element and its gap -- and the other 8 lie fully inside: 80 % of all frames are asserted.
LOOP_FRAME, LOOP_ELEMENT, LOOP_BINS, LOOP_PITCH = 256, 5, (9, 12, 15, 18), 2
LOOP_STEP = 0x01000000


def loop_keys(channels, elements, shift=None):
    """per channel: gap, element, gap, element ... (5 frames each), channel c starting `shift[c]` frames later; -> keys, expected tone per
    frame (tone index, to.NONE, or -1 for a frame that straddles an edge)"""
    nfr = 2 * LOOP_ELEMENT * elements
    keys = np.zeros((channels, nfr * LOOP_FRAME), np.uint8)
    want = np.full((channels, nfr), -1, np.int64)
    for c in range(channels):
        s = 0 if shift is None else int(shift[c])
        down = np.array([(max(f - s, 0) // LOOP_ELEMENT) % 2 == 1 and f >= s for f in range(nfr)])
        keys[c] = np.repeat(down, LOOP_FRAME)
        for f in range(nfr):
            if f == 0 or down[f] == down[f - 1]:
                want[c, f] = LOOP_PITCH if down[f] else to.NONE
    return keys, want


def loop_cw(tx):
    """the keyed path's setting of the loop on a Tx instance or an oracle"""
    return tx.set_cw(sr.keyshape(64), 0.5, sr.tone_step(LOOP_BINS[LOOP_PITCH] * FS_AUDIO / LOOP_FRAME, FS_AUDIO * L_RF))


def loop_tones():
    return sr.design_tones(np.array(LOOP_BINS, np.float64) / LOOP_FRAME)


LOOP_TONES = dict(frame_blocks=4, confirm=1, release=1, ratio=0.25, min_power=10.0)        # a clean tone of amplitude A: p = (128 A)^2, p / (E N) = 0.5


def test_the_receivers_tone_bank_reads_the_keying_back():
    ch, elements = 3, 2
    keys, want = loop_keys(ch, elements, shift=[0, 1, 3])
    o = co.TxCwOracle(rc.TxSpec(ch, block=64, interp=L_RF, ni_taps=256, nh_taps=63, mode=rc.MODE_CW, alc=False, nco_step_all=LOOP_STEP))
    assert loop_cw(o) == 0
    iq, _ = o.process_key(keys)
    rx = rc.CpuChain(rc.ChainSpec(ch, 64 * L_RF, L_RF, 255, 63, 0, rc.MODE_CW, rc.ARITH_CMSIS, nco=True, nco_step_all=LOOP_STEP, agc=False), "orc")
    assert rx.ok()
    audio = rx.process(iq)
    bank = to.Tones(ch, 64, loop_tones(), **LOOP_TONES)
    got = []
    for f in range(want.shape[1]):
        bank.process(audio[:, f * LOOP_FRAME:(f + 1) * LOOP_FRAME])
        got.append(bank.tone.astype(np.int64).copy())
    got = np.stack(got, axis=1)
    asserted = want >= 0
    assert asserted.mean() >= 0.5 and ((~asserted).reshape(ch, -1).sum(axis=1) <= 2 * elements).all()
    assert (want[asserted] == LOOP_PITCH).any() and (want[asserted] == to.NONE).any()
    assert (got[asserted] == want[asserted]).all(), (got, want)
