"""GPU: the audio input stage of the TX chain (include/selenite_tx_in.h, k_tx_in in csrc/tx_in.hip) through the C-ABI against the fixture made
from the reference's CMSIS-DSP functions (tests/golden/txin.npz) and against the oracle (tests/txin_oracle.py).  Every comparison is on bits
-- the stage's audio (in_audio_device), the I/Q, dec_state, level, open, hold, opens, open_blocks and the chain's own state -- in
SELENITE_ARITH_CMSIS and _FMA: the stage contracts nothing in either, the chain behind it follows cfg.arith."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rxcommon as rc
import test_txin_oracle as tto
import txin_oracle as tio
from rxcommon import ARITH_CMSIS, ARITH_FMA

pytestmark = pytest.mark.gpu
f32 = np.float32
ARITHS = [ARITH_CMSIS, ARITH_FMA]
same_bits = tto.same_bits
MONO, LEFT, RIGHT, MIX = tio.MONO, tio.LEFT, tio.RIGHT, tio.MIX
F32, Q15, Q15F = tio.K_F32, tio.K_Q15, tio.K_Q15_F32
VOX = dict(gate=1, hang=1, attack=0.75, decay=0.875, open_level=2e-3, close_level=1e-3, level_init=0.0)


def small_spec(channels, block, arith=ARITH_CMSIS, **kw):
    """a short chain behind the stage: 15-tap Hilbert pair, interpolation by 2 with 16 taps"""
    kw.setdefault("interp", 2)
    kw.setdefault("ni_taps", 16)
    kw.setdefault("nh_taps", 15)
    return rc.TxSpec(channels, block=block, arith=arith, **kw)


def taps(nt, seed=0):
    """nt finite taps of both signs without symmetry: the order of the taps shows in the bits"""
    return (np.random.default_rng(0x1A90 + nt + seed).uniform(-1, 1, nt) / max(nt, 4) * 4).astype(f32)


def pair(spec, **kw):
    import selenite_rx as sr
    g, o = sr.Tx(spec.config()), tio.TxInOracle(spec)
    assert g.set_in(**kw) == 0 and o.set_in(**kw) == 0
    return g, o


def d2h(ptr, shape, dtype):
    import selenite_rx as sr
    out = np.empty(shape, dtype)
    assert sr.lib().selenite_rx_memcpy_d2h(out.ctypes.data, ptr, out.nbytes) == 0
    return out


def make_frames(nch, words, kind, seed, quiet=None):
    """different data in every channel; `quiet` = (from, to) in words: a stretch 60 dB down"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (nch, words))
    if quiet:
        x[:, quiet[0]:quiet[1]] *= 1e-3
    return x.astype(f32) if kind == F32 else np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)


def frame_call(g, frames, kind=F32, offset=0, expect=0):
    """one call through a device entry -> (the stage's audio, I/Q); offset: elements the source pointer sits behind a 16-byte boundary"""
    import selenite_rx as sr
    frames = np.ascontiguousarray(frames)
    nch = frames.shape[0]
    bs = frames[0].size // (g._in_M * g._in_fw)
    odt = np.int16 if kind == Q15 else np.float32
    d_f, d_iq = sr.DeviceBuffer(frames.nbytes + 64), sr.DeviceBuffer(nch * bs * g.cfg.interp * 2 * np.dtype(odt).itemsize)
    pad = np.zeros(offset, frames.dtype)
    d_f.upload(np.concatenate([pad, frames.reshape(-1)]))
    assert g.process_frames(d_f.ptr + offset * frames.dtype.itemsize, d_iq.ptr, bs, kind) == expect
    assert g.sync() == expect
    if expect:
        return None, None
    return d2h(g.in_audio_device(), (nch, bs), odt), d_iq.download((nch, bs * g.cfg.interp, 2), odt)


def check_call(g, o, frames, kind=F32, offset=0, what=""):
    got, want = frame_call(g, frames, kind, offset), o.process_frames(frames, kind)
    assert same_bits(got[0], want[0]), "the stage's audio " + str(what)
    assert same_bits(got[1], want[1]), "I/Q " + str(what)


def assert_state_equal(g, o, what=""):
    sg, so = g.in_state(), o.in_state()
    assert set(sg) == set(so)
    for k in so:
        assert same_bits(sg[k], so[k]), "stage state %s differs %s" % (k, what)
    cg, cs = g.state(), o.state()
    for k in cs:
        assert same_bits(cg[k], cs[k]), "chain state %s differs %s" % (k, what)


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(rc.GOLDEN_DIR, "txin.npz")) as z:
        return {k: z[k] for k in z.files}


# ---- the fixture through every entry that fits its types -----------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", tto.NAMES)
def test_fixture_through_every_entry(gold, name, arith):
    import selenite_rx as sr
    block, kw = tto.fixture_params(gold, name)
    frames = np.tile(gold[name + "/frames"], (3, 1))
    n = gold[name + "/a"].size
    kinds = [Q15, Q15F] if frames.dtype == np.int16 else [F32]
    for kind in kinds:
        for rounding in ((False, True) if kind == Q15 else (False,)):
            want_a = gold[name + ("/q15_" + ("round" if rounding else "trunc") if kind == Q15 else "/a")]
            for host in ((False, True) if kind != Q15F else (False,)):
                spec = small_spec(3, block, arith, q15_rounding=rounding)
                g = sr.Tx(spec.config())
                assert g.set_in(**kw) == 0
                twin = sr.Tx(spec.config())                      # the audio entry of a twin instance fed the fixture's audio
                audio_in = np.tile(want_a, (3, 1))
                want_iq = twin.process_q15(audio_in) if kind == Q15 else twin.process(audio_in)
                if host:
                    rcode, iq = g.process_frames_host(frames, q15=kind == Q15)
                    assert rcode == 0
                    a = d2h(g.in_audio_device(), (3, n), want_a.dtype)
                else:                                            # the device entries, cut behind the first DSP block
                    cut = g._in_M * g._in_fw * block
                    a0, i0 = frame_call(g, frames[:, :cut], kind)
                    a1, i1 = frame_call(g, frames[:, cut:], kind)
                    a, iq = np.concatenate([a0[:, :block], a1], axis=1), np.concatenate([i0, i1], axis=1)
                for c in range(3):
                    assert same_bits(a[c], want_a), (kind, rounding, host, c)
                assert same_bits(iq, want_iq), (kind, rounding, host)
                st = g.in_state()
                for k in ("level", "open", "hold", "opens", "open_blocks"):
                    assert (st[k] == gold[name + "/" + k][-1]).all(), k
                tail = gold[name + "/g"][gold[name + "/g"].size - (kw["coeffs"].size - 1):] if kw["coeffs"].size > 1 else np.zeros(0, f32)
                assert same_bits(st["dec_state"][1], tail)
                g.close()
                twin.close()


def test_fixture_vox_sequence_block_by_block(gold):
    """the fixture's VOX stream one DSP block per call: level, open, hold and the counters behind every block"""
    import selenite_rx as sr
    block, kw = tto.fixture_params(gold, "vox")
    g = sr.Tx(small_spec(1, block).config())
    assert g.set_in(**kw) == 0
    frames = gold["vox/frames"][None, :]
    per = kw["M"] * block
    vox = d2h(g.in_vox(), (1,), np.uint32)
    assert vox[0] == 0
    for b in range(gold["vox/level"].size):
        frame_call(g, frames[:, b * per:(b + 1) * per])
        st = g.in_state()
        for k in ("level", "open", "hold", "opens", "open_blocks"):
            assert same_bits(st[k][0], gold["vox/" + k][b]), (k, b)
        assert d2h(g.in_vox(), (1,), np.uint32)[0] == gold["vox/open"][b]


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [F32, Q15, Q15F])
@pytest.mark.parametrize("pick", [MONO, LEFT, RIGHT, MIX])
@pytest.mark.parametrize("M", [1, 2, 4, 8])
def test_every_M_pick_and_frame_type(M, pick, kind):
    spec = small_spec(3, 12, ARITH_FMA if M == 2 else ARITH_CMSIS)
    g, o = pair(spec, M=M, coeffs=taps(33, M), pick=pick, gain=0.8, vox=VOX)
    fw = 1 if pick == MONO else 2
    for n, seed in ((3, 1), (1, 2)):
        w = n * 12 * M * fw
        check_call(g, o, make_frames(3, w, kind, 0x100 * M + 0x10 * pick + seed, quiet=(w // 4, w)), kind, what=(M, pick, kind, n))
    assert_state_equal(g, o)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("block", [4, 12, 64])
@pytest.mark.parametrize("nt", [1, 3, 63, 64, 97, 256])
def test_tap_counts_and_dsp_blocks(nt, block, arith):
    """one DSP block, then one DSP block more than the kernel's tile (1024 / M input samples rounded down to whole DSP blocks)"""
    M = 4 if nt != 97 else 2
    spec = small_spec(3, block, arith)
    g, o = pair(spec, M=M, coeffs=taps(nt), pick=LEFT, gain=1.25, vox=VOX)
    tile = block * max(1, (1024 // M) // block)
    for n, seed in ((block, 1), (tile + block, 2)):
        w = n * M * 2
        check_call(g, o, make_frames(3, w, Q15F, 0x2000 + nt + seed, quiet=(w // 3, 2 * w // 3)), Q15F, what=(nt, block, n))
        assert_state_equal(g, o, (nt, block, n))


@pytest.mark.parametrize("channels", [1, 3, 67])
def test_channel_counts(channels):
    spec = small_spec(channels, 12)
    g, o = pair(spec, M=4, coeffs=taps(64), pick=MIX, gain=0.7, vox=VOX)
    for seed in (1, 2):
        check_call(g, o, make_frames(channels, 36 * 4 * 2, Q15, 0x3000 + channels + seed, quiet=(0, 96 * seed)), Q15, what=channels)
    assert_state_equal(g, o)


def test_element_path_rows_and_unaligned_source():
    """int16 MONO at M = 1 with DSP blocks of 12: 24-byte rows; and a source pointer one element behind a 16-byte boundary"""
    g, o = pair(small_spec(3, 12), M=1, coeffs=taps(63), pick=MONO, gain=1.0, vox=VOX)
    for seed in (1, 2, 3):
        check_call(g, o, make_frames(3, 12, Q15, 0x4000 + seed), Q15, what="24-byte rows")
    assert_state_equal(g, o)
    for kind in (F32, Q15, Q15F):
        g, o = pair(small_spec(3, 64), M=2, coeffs=taps(32), pick=RIGHT, gain=1.0, vox=VOX)
        check_call(g, o, make_frames(3, 128 * 2 * 2, kind, 0x4100 + kind), kind, offset=1, what="offset source")
        check_call(g, o, make_frames(3, 128 * 2 * 2, kind, 0x4200 + kind), kind, offset=0)
        assert_state_equal(g, o)


@pytest.mark.parametrize("M,nt,block", [(1, 64, 12), (2, 32, 4)])
def test_calls_shorter_than_the_history_against_one_long_call(M, nt, block):
    spec = small_spec(2, block)
    frames = make_frames(2, 40 * block * M, F32, 0x5000 + nt)
    g, o = pair(spec, M=M, coeffs=taps(nt), pick=MONO, gain=1.0)
    long_a, long_iq = frame_call(pair(spec, M=M, coeffs=taps(nt), pick=MONO, gain=1.0)[0], frames)
    a, iq = [], []
    for k in range(40):
        got = frame_call(g, frames[:, k * block * M:(k + 1) * block * M])
        a.append(got[0])
        iq.append(got[1])
    assert same_bits(np.concatenate(a, axis=1), long_a) and same_bits(np.concatenate(iq, axis=1), long_iq)
    assert same_bits(long_a, o.process_frames(frames)[0])
    assert_state_equal(g, o)


@pytest.mark.parametrize("arith", ARITHS)
def test_one_stream_cut_three_ways(arith):
    spec = small_spec(3, 12, arith)
    M, blocks = 4, 24
    frames = make_frames(3, blocks * 12 * M * 2, Q15, 0x6000, quiet=(3000, 5000))
    whole = tio.TxInOracle(spec)
    whole.set_in(M=M, coeffs=taps(97), pick=MIX, gain=0.9, vox=VOX)
    want = whole.process_frames(frames, Q15)
    for cuts in ([1] * 24, [5, 1, 11, 7], [23, 1]):
        g, o = pair(spec, M=M, coeffs=taps(97), pick=MIX, gain=0.9, vox=VOX)
        a, iq, at = [], [], 0
        for n in cuts:
            part = frames[:, at * 12 * M * 2:(at + n) * 12 * M * 2]
            got = frame_call(g, part, Q15)
            o.process_frames(part, Q15)
            a.append(got[0])
            iq.append(got[1])
            at += n
            assert_state_equal(g, o, (cuts, at))
        assert same_bits(np.concatenate(a, axis=1), want[0]) and same_bits(np.concatenate(iq, axis=1), want[1]), cuts


# ---- VOX -----------------------------------------------------------------------------------------------------------------------------------
def test_gate_against_flag_only():
    spec = small_spec(3, 12)
    w = 30 * 12 * 2
    frames = make_frames(3, w, F32, 0x7000, quiet=(w // 3, w))
    flag, of = pair(spec, M=2, coeffs=taps(32), pick=MONO, gain=1.0, vox=dict(VOX, gate=0))
    gate, og = pair(spec, M=2, coeffs=taps(32), pick=MONO, gain=1.0, vox=VOX)
    a_flag, iq_flag = frame_call(flag, frames)
    a_gate, iq_gate = frame_call(gate, frames)
    want_flag, want_gate = of.process_frames(frames), og.process_frames(frames)
    bits = og.last["bits"]
    assert (bits == 0).any() and (bits == 1).any()
    assert same_bits(a_flag, want_flag[0]) and same_bits(a_flag, og.last["a"]) and same_bits(iq_flag, want_flag[1])
    closed = np.repeat(bits == 0, 12, axis=1)
    assert (a_gate[closed].view(np.uint32) == 0).all() and same_bits(a_gate[~closed], a_flag[~closed])      # +0.0f, and the open blocks as they were
    assert same_bits(a_gate, want_gate[0]) and same_bits(iq_gate, want_gate[1])
    import selenite_rx as sr
    twin = sr.Tx(spec.config())                                  # the I/Q is the audio entry on the gated audio
    assert same_bits(twin.process(a_gate), iq_gate)
    sf, sg = flag.in_state(), gate.in_state()
    for k in sf:
        assert same_bits(sf[k], sg[k]), k                        # the gate changes nothing the VOX sees


def test_nan_and_inf_in_one_block_leave_the_level_and_the_other_channels():
    """(the stage's words are compared on bits; what a NaN does to the chain behind the stage is the audio entries' business, so the I/Q and
    the chain's state are compared on the channels without one)"""
    spec = small_spec(3, 12)
    frames = make_frames(3, 6 * 12 * 2, F32, 0x7100)
    bad = frames.copy()
    bad[1, 2 * 24 + 3], bad[1, 2 * 24 + 9] = np.nan, np.inf
    g, o = pair(spec, M=2, coeffs=taps(8), pick=MONO, gain=1.0, vox=dict(VOX, gate=0))
    clean, _ = pair(spec, M=2, coeffs=taps(8), pick=MONO, gain=1.0, vox=dict(VOX, gate=0))
    with np.errstate(all="ignore"):
        want = o.process_frames(bad)
    got, ref = frame_call(g, bad), frame_call(clean, frames)
    nan = np.isnan(want[0])
    assert nan[1, 24:36].any() and not nan[[0, 2]].any() and not nan[1, :24].any() and not nan[1, 36:].any()      # all of it in one DSP block
    assert (np.isnan(got[0]) == nan).all() and same_bits(got[0][~nan], want[0][~nan])
    lv = o.stage.meter.trace["level"]
    assert not np.isfinite(o.stage.meter.trace["ms"][1, 2]) and lv[1, 2] == lv[1, 1] and np.isfinite(lv).all()
    for c in (0, 2):
        assert same_bits(got[0][c], ref[0][c]) and same_bits(got[1][c], ref[1][c]) and same_bits(got[1][c], want[1][c])
    sg, so = g.in_state(), o.in_state()
    for k in ("level", "open", "hold", "opens", "open_blocks"):
        assert same_bits(sg[k], so[k]), k
    assert same_bits(sg["dec_state"], so["dec_state"])           # (finite again: the bad block lies more than nd_taps - 1 samples back)
    sg, sc = g.in_state(), clean.in_state()
    for k in ("level", "open", "hold", "opens", "open_blocks"):
        assert same_bits(sg[k][[0, 2]], sc[k][[0, 2]]), k


# ---- state and configuration ---------------------------------------------------------------------------------------------------------------
def test_state_round_trip_reset_and_retune():
    spec = small_spec(3, 12)
    kw = dict(M=4, coeffs=taps(64), pick=LEFT, gain=1.0, vox=VOX)
    g, o = pair(spec, **kw)
    w = 5 * 12 * 4 * 2
    check_call(g, o, make_frames(3, w, F32, 0x8000))
    st = g.in_state()
    assert st["dec_state"].any() and st["level"].all()
    # round trip: the state moves to a new instance, which goes on as the first does
    g2, _ = pair(spec, **kw)
    g2.set_state(g.state())
    g2.set_in_state(st)
    nxt = make_frames(3, w, F32, 0x8001, quiet=(0, w))
    a, b = frame_call(g, nxt), frame_call(g2, nxt)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    o.process_frames(nxt)
    assert_state_equal(g, o)
    # NULL members are skipped
    before = g.in_state()
    g.set_in_state({"hold": np.full(3, 5, np.uint32)})
    after = g.in_state()
    assert (after["hold"] == 5).all() and all(same_bits(before[k], after[k]) for k in before if k != "hold")
    g.set_in_state(before)
    # a retune with the same nd_taps keeps everything; a changed nd_taps clears dec_state alone
    kw2 = dict(kw, coeffs=taps(64, 7), gain=0.5, vox=dict(VOX, hang=3))
    assert g.set_in(**kw2) == 0 and o.set_in(**kw2) == 0
    assert all(same_bits(before[k], g.in_state()[k]) for k in before)
    check_call(g, o, make_frames(3, w, F32, 0x8002), what="behind the retune")
    assert_state_equal(g, o)
    kw3 = dict(kw2, coeffs=taps(33))
    mid = g.in_state()
    assert g.set_in(**kw3) == 0 and o.set_in(**kw3) == 0
    now = g.in_state()
    assert now["dec_state"].shape == (3, 32) and not now["dec_state"].any()
    assert all(same_bits(mid[k], now[k]) for k in mid if k != "dec_state")
    check_call(g, o, make_frames(3, w, F32, 0x8003), what="behind the new length")
    assert_state_equal(g, o)
    # a refused setting leaves the previous one in place
    assert g.set_in(**dict(kw3, M=3)) == rc.ARGUMENT_ERROR
    assert g.set_in(**dict(kw3, vox=dict(VOX, attack=0.0))) == rc.ARGUMENT_ERROR
    assert g.set_in(**dict(kw3, vox=dict(VOX, sense=1))) == rc.ARGUMENT_ERROR
    assert g.set_in(**dict(kw3, gain=np.inf)) == rc.ARGUMENT_ERROR
    assert g.set_in(M=2, coeffs=None) == rc.ARGUMENT_ERROR
    bad = taps(33)
    bad[5] = np.nan
    assert g.set_in(**dict(kw3, coeffs=bad)) == rc.ARGUMENT_ERROR
    check_call(g, o, make_frames(3, w, F32, 0x8004), what="behind the refused settings")
    # reset: as after the first set_in
    assert g.reset() == 0 and o.reset() == 0
    st = g.in_state()
    assert not st["dec_state"].any() and (st["level"] == 0).all() and not st["open"].any() and not st["opens"].any()
    check_call(g, o, make_frames(3, w, F32, 0x8005), what="behind reset")
    assert_state_equal(g, o)
    # off and on again: the first setting behind NULL clears
    assert g.clear_in() == 0 and g.process_frames(1, 1, 12) == rc.ARGUMENT_ERROR
    assert g.set_in(**kw3) == 0
    st = g.in_state()
    assert not st["dec_state"].any() and (st["level"] == 0).all() and not st["open_blocks"].any()


@pytest.mark.parametrize("arith", ARITHS)
def test_set_mode_keeps_the_state_and_other_entries_leave_it_alone(arith):
    import selenite_rx as sr
    spec = small_spec(3, 12, arith)
    kw = dict(M=2, coeffs=taps(32), pick=MIX, gain=1.0, vox=VOX)
    g, o = pair(spec, **kw)
    assert g.set_fm(deviation=0.2) == 0 and o.chain.set_fm(0.2) == 0
    shape = sr.keyshape(8)
    assert g.set_cw(shape, offset_step=0x00DA740E) == 0 and o.chain.set_cw(shape, offset_step=0x00DA740E) == 0
    w = 4 * 12 * 2 * 2
    for k, mode in enumerate((rc.MODE_USB, rc.MODE_AM, rc.MODE_FM, rc.MODE_CW, rc.MODE_USB)):
        before = g.in_state()
        assert g.set_mode(mode) == 0 and o.set_mode(mode) == 0
        assert all(same_bits(before[x], g.in_state()[x]) for x in before), mode
        check_call(g, o, make_frames(3, w, F32, 0x9000 + k, quiet=(0, w) if k == 2 else None), what=("mode", mode))
        assert_state_equal(g, o, mode)
        if mode == rc.MODE_CW:                                   # an audio call and a keyed call between two frame calls
            before = g.in_state()
            audio = rc.synth_audio(0, 3, 0, 24)
            assert same_bits(g.process(audio), o.chain.process(audio))
            keys = (np.arange(3 * 24).reshape(3, 24) % 5 < 3).astype(np.uint8)
            rcode, iq, _ = g.process_key_host(keys)
            assert rcode == 0 and same_bits(iq, o.chain.process_key(keys)[0])
            assert all(same_bits(before[x], g.in_state()[x]) for x in before)
            check_call(g, o, make_frames(3, w, F32, 0x9100), what="behind the audio and keyed calls")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_writes_nothing():
    import selenite_rx as sr
    spec = small_spec(3, 12)
    g = sr.Tx(spec.config())
    w = 24 * 4 * 2
    frames = make_frames(3, w, F32, 0xA000)
    d_f, d_iq = sr.DeviceBuffer(frames.nbytes), sr.DeviceBuffer(3 * 24 * 2 * 2 * 4)
    d_f.upload(frames)
    sentinel = np.full((3, 48, 2), 7.5, f32)
    d_iq.upload(sentinel)
    assert g.in_vox() is None and g.in_audio_device() is None
    for kind in (F32, Q15, Q15F):
        assert g.process_frames(d_f.ptr, d_iq.ptr, 24, kind) == rc.ARGUMENT_ERROR      # before set_in
    assert g.process_frames_host(frames)[0] == rc.ARGUMENT_ERROR
    with pytest.raises(sr.RxError):
        g.in_state()
    g.close()
    g = sr.Tx(spec.config())
    assert g.set_in(M=4, coeffs=taps(64), pick=LEFT, gain=1.0, vox=VOX) == 0
    frame_call(g, frames)                                        # the audio buffer and the state now hold something
    audio_ptr = g.in_audio_device()
    d_audio_fill = np.full((3, 24), -3.25, f32)
    assert sr.lib().selenite_rx_memcpy_h2d(audio_ptr, d_audio_fill.ctypes.data, d_audio_fill.nbytes) == 0
    st_fill = g.in_state()
    st_fill["dec_state"][:] = 1.5
    st_fill["level"][:] = 0.25
    st_fill["hold"][:] = 9
    g.set_in_state(st_fill)
    chain = g.state()
    for bs, kind, src, dst, want in ((0, F32, d_f.ptr, d_iq.ptr, rc.LENGTH_ERROR), (13, F32, d_f.ptr, d_iq.ptr, rc.LENGTH_ERROR),
                                     (18, Q15, d_f.ptr, d_iq.ptr, rc.LENGTH_ERROR), (24, F32, None, d_iq.ptr, rc.ARGUMENT_ERROR),
                                     (24, Q15F, d_f.ptr, None, rc.ARGUMENT_ERROR)):
        assert g.process_frames(src, dst, bs, kind) == want, (bs, kind)
    assert g.process_frames_host(frames[:, :13 * 8])[0] == rc.LENGTH_ERROR
    ms = C.c_float(-1.0)
    assert g.L.selenite_tx_time_in_stage_device(g.h, d_f.ptr, 3, 24, 1, C.byref(ms)) == rc.ARGUMENT_ERROR and ms.value == -1.0
    assert g.sync() != 0                                         # the status remembers the first refusal
    assert same_bits(d_iq.download((3, 48, 2), f32), sentinel)
    assert g.in_audio_device() == audio_ptr and same_bits(d2h(audio_ptr, (3, 24), f32), d_audio_fill)
    st = g.in_state()
    assert all(same_bits(st[k], st_fill[k]) for k in st)
    now = g.state()
    assert all(same_bits(now[k], chain[k]) for k in chain)
    # a layout over the kernel's LDS budget: a DSP block of 16 384 audio samples at M = 8
    big = sr.Tx(small_spec(1, 16384, interp=1, ni_taps=0, nh_taps=0).config())
    assert big.set_in(M=8, coeffs=taps(16), pick=MONO, gain=1.0) == 0
    assert big.process_frames(d_f.ptr, d_iq.ptr, 16384, F32) == rc.LENGTH_ERROR
    assert same_bits(d_iq.download((3, 48, 2), f32), sentinel)


# ---- the repeater: a receiver bank's frames handed to a transmitter bank on the device -----------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
def test_repeater_rx_out_frames_into_tx_frames(arith):
    import selenite_rx as sr
    ch, bs = 67, 1024
    rspec = rc.baseline_spec("cfg3", ch, ARITH_CMSIS)
    rx = sr.Rx(rspec.config())
    h = sr.design_interp(32, 4, 0.1)
    rx.set_out(4, h, sr.OUT_STEREO)
    na = rx.out_values(bs) // 2 // 4                             # audio samples per channel and call at the chain's rate
    tspec = small_spec(ch, 64, arith)
    g, o = pair(tspec, M=4, coeffs=taps(64), pick=LEFT, gain=1.0, vox=VOX)
    iq = rc.synth_iq(0, ch, 0, bs)
    q = np.clip(np.round(iq * 32768), -32768, 32767).astype(np.int16)
    d_in, d_fr = sr.DeviceBuffer(q.nbytes), sr.DeviceBuffer(ch * na * 4 * 2 * 2)
    d_iq = sr.DeviceBuffer(ch * na * 2 * 2 * 2)
    for call in range(2):
        d_in.upload(q if call == 0 else (q // 64).astype(np.int16))
        rx.process_q15_device(d_in.ptr, d_fr.ptr, bs)
        rx.check()
        rx.sync()
        assert g.process_frames(d_fr.ptr, d_iq.ptr, na, Q15) == 0 and g.sync() == 0
        frames = d_fr.download((ch, na * 4 * 2), np.int16)
        assert frames.any() and same_bits(frames[:, 0::2], frames[:, 1::2])
        want_a, want_iq = o.process_frames(frames, Q15)
        assert same_bits(d2h(g.in_audio_device(), (ch, na), np.int16), want_a)
        assert same_bits(d_iq.download((ch, na * 2, 2), np.int16), want_iq)
    assert_state_equal(g, o)


# ---- scale ---------------------------------------------------------------------------------------------------------------------------------
def test_scale_4099_channels():
    import selenite_rx as sr
    ch, bs, M = 4099, 256, 4
    spec = small_spec(ch, 64, ARITH_FMA)
    g = sr.Tx(spec.config())
    kw = dict(M=M, coeffs=taps(64), pick=MIX, gain=0.9, vox=VOX)
    assert g.set_in(**kw) == 0
    rng = np.random.default_rng(0xB000)
    frames = rng.integers(-32768, 32768, (ch, bs * M * 2), dtype=np.int16)
    frames[::3, bs * M:] //= 512
    a, iq = frame_call(g, frames, Q15)
    pick = np.unique(np.concatenate([[0, ch - 1], rng.choice(ch, 64, replace=False)]))
    sub = small_spec(pick.size, 64, ARITH_FMA)
    o = tio.TxInOracle(sub)
    o.set_in(**kw)
    want_a, want_iq = o.process_frames(frames[pick], Q15)
    assert same_bits(a[pick], want_a) and same_bits(iq[pick], want_iq)
    st, so = g.in_state(), o.in_state()
    for k in so:
        assert same_bits(st[k][pick], so[k]), k


# ---- the plain-C host of the slot ----------------------------------------------------------------------------------------------------------
def test_dsp_if_mic_slot_runs():
    exe = os.path.join(rc.ROOT, "selenite-lite_amd", "host", "dsp_if_mic_slot")
    assert os.path.exists(exe), "host/dsp_if_mic_slot is built by the Makefile's `all`"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "VOX open on 64 of 64" in r.stdout and "VOX open on 0 of 64" in r.stdout
