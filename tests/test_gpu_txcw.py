"""GPU: the keyed CW path of the TX chain (include/selenite_tx_cw.h, k_tx_cw in csrc/tx_cw.hip) through the C-ABI against the fixture made
from the reference's CMSIS-DSP functions (tests/golden/txcw.npz) and against the oracle (tests/txcw_oracle.py).  Every comparison is on
bits -- I/Q, sidetone, fir_state, interp_state, alc_gain, nco_phase, key_state, side_phase, tx_on, hold -- in SELENITE_ARITH_CMSIS and
_FMA: the carrier's phase is an integer, the products of the shaping FIR are exact."""
import ctypes as C
import os

import numpy as np
import pytest

import rxcommon as rc
import test_txcw_oracle as tco
import tones_oracle as to
import txcw_oracle as co
from rxcommon import ARITH_CMSIS, ARITH_FMA

pytestmark = pytest.mark.gpu
f32 = np.float32
ARITHS = [ARITH_CMSIS, ARITH_FMA]
CW, CWR = rc.MODE_CW, rc.MODE_CWR
same_bits = tco.same_bits


def gpu_tx(spec):
    import selenite_rx as sr
    return sr.Tx(spec.config())


def taps(ns, seed=0):
    """ns finite taps of both signs without symmetry: the order of the taps shows in the bits"""
    return (np.random.default_rng(0x7A90 + ns + seed).uniform(-1, 1, ns) / max(ns, 4) * 4).astype(f32)


def cw_pair(spec, **cw):
    g, o = gpu_tx(spec), co.TxCwOracle(spec)
    assert g.set_cw(**cw) == 0 and o.set_cw(**cw) == 0
    return g, o


def keyed(g, keys, side=None, q15=False):
    """one call through the device entries -> (I/Q, sidetone buffer or None)"""
    import selenite_rx as sr
    keys = np.ascontiguousarray(keys, np.uint8)
    nch, n = keys.shape
    dt = np.int16 if q15 else np.float32
    d_k, d_iq = sr.DeviceBuffer(keys.nbytes), sr.DeviceBuffer(nch * n * g.cfg.interp * 2 * np.dtype(dt).itemsize)
    d_k.upload(keys)
    d_s = None
    if side is not None:
        s = np.ascontiguousarray(side, dt)
        d_s = sr.DeviceBuffer(s.nbytes)
        d_s.upload(s)
    assert g.process_key(d_k.ptr, d_iq.ptr, d_s.ptr if d_s else None, n, q15=q15) == 0
    assert g.sync() == 0
    return d_iq.download((nch, n * g.cfg.interp, 2), dt), (d_s.download((nch, n), dt) if d_s else None)


def check_call(g, o, keys, side=None, q15=False, what=""):
    got, want = keyed(g, keys, side, q15), o.process_key(keys, side, q15)
    assert same_bits(got[0], want[0]), "I/Q " + what
    assert (side is None and got[1] is None) or same_bits(got[1], want[1]), "sidetone " + what


def gpu_state(g):
    st = g.state()
    st.update(g.cw_state())
    return st


def assert_state_equal(g, o):
    sg, so = gpu_state(g), o.state()
    so.pop("tone_phase")
    assert set(sg) == set(so)
    for k in so:
        assert same_bits(sg[k], so[k]), "state %s differs" % k


def random_keys(nch, n, seed, run=7):
    """elements of random length around `run` samples: edges anywhere, stretches that fill a whole key window now and then"""
    rng = np.random.default_rng(seed)
    k = np.zeros((nch, n), np.uint8)
    for c in range(nch):
        at, v = 0, int(rng.integers(0, 2))
        while at < n:
            ln = int(rng.integers(1, 2 * run))
            k[c, at:at + ln] = v
            at, v = at + ln, 1 - v
    return k


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(rc.GOLDEN_DIR, "txcw.npz")) as z:
        return {k: z[k] for k in z.files}


# ---- the fixture through all four entries ------------------------------------------------------------------------------------------------
def fixture_instance(gold, name, arith, rounding, side_mix):
    spec, cw, phase0, side_phase0 = tco.fixture_spec(gold, name, arith=arith, q15_rounding=rounding, channels=3)
    g = gpu_tx(spec)
    assert g.set_cw(side_mix=side_mix, **cw) == 0
    st = g.state()
    st["nco_phase"][:] = phase0
    g.set_state(st)
    g.set_cw_state({"side_phase": np.full(3, side_phase0, np.uint32)})
    return g


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", tco.NAMES)
def test_fixture_through_all_four_entries(gold, name, arith):
    key = np.tile(gold[name + "/key"], (3, 1))
    block = int(gold[name + "/cfg"][0])
    for q15 in (False, True):
        for rounding in ((False, True) if q15 else (False,)):
            tag = "round" if rounding else "trunc"
            out = gold[name + ("/q15_" + tag if q15 else "/out")]
            y = gold[name + ("/yq_" + tag if q15 else "/y")]
            side_in = np.tile(gold[name + ("/side_in_q15" if q15 else "/side_in")], (3, 1))
            mixed = gold[name + ("/side_mix_q_" + tag if q15 else "/side_mix")]
            if arith != ARITH_CMSIS and gold[name + "/ic"].size:         # the fixture's interpolator is the CMSIS one: the fused one from the oracle
                out = tco.fixture_oracle(gold, name, arith=arith, q15_rounding=rounding).process_key(key[:1], None, q15)[0][0]
                assert not same_bits(out, gold[name + ("/q15_" + tag if q15 else "/out")]) or q15
            for mix in (0, 1):
                for host in (False, True):
                    g = fixture_instance(gold, name, arith, rounding, mix)
                    if host:
                        rcode, iq, sd = g.process_key_host(key, side_in, q15=q15)
                        assert rcode == 0
                    else:                                        # the device entries, cut behind the first DSP block
                        a = keyed(g, key[:, :block], side_in[:, :block], q15)
                        b = keyed(g, key[:, block:], side_in[:, block:], q15)
                        iq, sd = np.concatenate([a[0], b[0]], axis=1), np.concatenate([a[1], b[1]], axis=1)
                    for c in range(3):
                        assert same_bits(iq[c], out), (q15, rounding, mix, host, c)
                        assert same_bits(sd[c], mixed if mix else y), (q15, rounding, mix, host, c)
                    st = gpu_state(g)
                    assert (st["nco_phase"] == gold[name + "/phases"][0]).all() and (st["side_phase"] == gold[name + "/phases"][1]).all()
                    g.close()


# ---- channels, lengths ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("nch", [1, 3, 67])
def test_channels_with_their_own_steps(nch, arith):
    steps = (np.arange(nch, dtype=np.uint64) * 0x03131313 + 0x00800001).astype(np.uint32)
    ssteps = (np.arange(nch, dtype=np.uint64) * 0x05010101 + 0x0DA740DA).astype(np.uint32)
    spec = rc.TxSpec(nch, block=64, interp=4, ni_taps=32, nh_taps=0, mode=CW, arith=arith, nco_steps=steps, alc=False)
    g, o = cw_pair(spec, shape=taps(16), amplitude=0.8, offset_step=0x00DA740E, side_level=0.4, side_step=ssteps, hang_blocks=1)
    for k in range(2):
        check_call(g, o, random_keys(nch, 128, 100 + k, run=20), side=np.zeros((nch, 128), f32), what="call %d" % k)
    assert_state_equal(g, o)
    assert len(set(o.state()["nco_phase"])) == nch and len(set(o.state()["side_phase"])) == nch
    g.close()


# (block, ns_taps, L, P): every block length with 1, 2 and 3 blocks per call; shapes around one and two wave widths, one with a history
# longer than the block, the longest; every L with every P; odd L with a filter (a lane's two outputs lie in different input samples), an
# odd block (key bytes one by one, an odd number of outputs)
GEOMETRY = ([(b, 16, 4, 4) for b in (32, 64, 96, 256)] + [(64, ns, 2, 4) for ns in (1, 2, 63, 64, 65, 256)] + [(32, 97, 2, 4)] +
            [(64, 8, L, P) for L in (1, 2, 4, 8) for P in (1, 4, 16) if not (L == 1 and P > 1)] + [(32, 5, 3, 5), (25, 7, 3, 2), (25, 7, 2, 3), (7, 3, 1, 1)])


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("block,ns,L,P", GEOMETRY)
def test_geometry(block, ns, L, P, arith):
    nch = 3
    spec = rc.TxSpec(nch, block=block, interp=L, ni_taps=L * P if L > 1 else 0, nh_taps=0, mode=CWR, arith=arith,
                     nco_steps=np.array([0x3A5F1C27, 0xC0000001, 0x7FFFFF01], np.uint32), alc=False)
    if L > 1:
        spec.ic = taps(L * P, 1)
    g, o = cw_pair(spec, shape=taps(ns), amplitude=-0.9, offset_step=0x01234567, side_level=0.5, side_step=0x0B4E81B5, hang_blocks=2)
    at = 0
    for nblk in (1, 2, 3):
        keys = random_keys(nch, 6 * block, 7 * ns + block, run=max(ns // 3, 3))[:, at:at + nblk * block]
        check_call(g, o, keys, side=np.zeros((nch, nblk * block), f32), what="%d block(s)" % nblk)
        at += nblk * block
    assert_state_equal(g, o)
    assert o.state()["key_state"].shape == (nch, ns - 1)
    g.close()


def test_a_destination_that_is_only_8_byte_aligned():
    """an even L stores a lane's two outputs as one 16-byte word only where the destination allows it"""
    import selenite_rx as sr
    nch, n, L = 2, 64, 4
    spec = rc.TxSpec(nch, block=64, interp=L, ni_taps=16, nh_taps=0, mode=CW, nco_step_all=0x01000000, alc=False)
    g, o = cw_pair(spec, shape=taps(8), offset_step=0x00DA740E)
    keys = random_keys(nch, n, 0x33, run=10)
    d_k, d_iq = sr.DeviceBuffer(keys.nbytes), sr.DeviceBuffer(nch * n * L * 8 + 16)
    d_k.upload(keys)
    d_iq.upload(np.full(nch * n * L * 2 + 4, 5.0, f32))
    assert g.process_key(d_k.ptr, d_iq.ptr + 8, None, n) == 0 and g.sync() == 0
    raw = d_iq.download((nch * n * L * 2 + 4,), f32)
    assert same_bits(raw[2:-2].reshape(nch, n * L, 2), o.process_key(keys)[0]) and (raw[:2] == 5.0).all() and (raw[-2:] == 5.0).all()
    g.close()


# ---- key patterns, call cutting ---------------------------------------------------------------------------------------------------------
def pattern_keys(block, nblk):
    n = block * nblk
    k = np.zeros((9, n), np.uint8)
    k[0] = 1                                                     # held: every window all up (the shortcut)
    #  [1] stays up: every window all down
    k[2, n // 2 + 3] = 1                                         # a single-sample dit
    k[3, ::2] = 1                                                # alternating
    k[4] = random_keys(1, n, 0x51, run=4)[0]
    k[5, n // 2 - 1] = 1                                         # an edge on the last sample of the first call (cut in the middle)
    k[6, n // 2:] = 1                                            # an edge on the first sample of the second call
    k[7] = random_keys(1, n, 0x52, run=9)[0] * np.random.default_rng(3).integers(2, 256, n).astype(np.uint8)     # non-zero bytes other than 1
    k[8, :block + 5] = 1                                         # held, then released inside a block: both paths in one call
    return k


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("ns", [1, 24])
def test_key_patterns(ns, arith):
    block, nblk = 64, 6
    keys = pattern_keys(block, nblk)
    assert (keys[7] > 1).any()
    spec = rc.TxSpec(keys.shape[0], block=block, interp=4, ni_taps=32, nh_taps=0, mode=CW, arith=arith, nco_step_all=0x01000000, alc=False)
    g, o = cw_pair(spec, shape=taps(ns), amplitude=1.0, offset_step=0x00DA740E, side_level=0.5, side_step=0x0DA740DA)
    half = keys.shape[1] // 2
    for k in range(2):
        check_call(g, o, keys[:, k * half:(k + 1) * half], side=np.zeros((keys.shape[0], half), f32), what="call %d" % k)
    assert_state_equal(g, o)
    # the steady states on bits: +0.0f with the key up, the in-order sum of the taps with the key down
    s = f32(0.0)
    for c in taps(ns):
        s = f32(s + c)
    assert same_bits(o.last_e[1], np.zeros(half, f32)) and same_bits(o.last_e[0], np.full(half, s, f32))
    g.close()


@pytest.mark.parametrize("arith", ARITHS)
def test_call_cutting(arith):
    block = 32
    keys = pattern_keys(block, 4)
    nch = keys.shape[0]
    spec = rc.TxSpec(nch, block=block, interp=3, ni_taps=45, nh_taps=0, mode=CW, arith=arith, nco_step_all=0x3A5F1C27, alc=False)
    cw = dict(shape=taps(40), amplitude=0.7, offset_step=0x00DA740E, side_level=0.5, side_step=0x0DA740DA, hang_blocks=1)
    runs = []
    for cut in ((4,), (1, 1, 1, 1), (1, 3)):
        g = gpu_tx(spec)
        assert g.set_cw(**cw) == 0
        at, ys, ss = 0, [], []
        for nb in cut:
            iq, sd = keyed(g, keys[:, at * block:(at + nb) * block], side=np.zeros((nch, nb * block), f32))
            ys.append(iq)
            ss.append(sd)
            at += nb
        runs.append((np.concatenate(ys, axis=1), np.concatenate(ss, axis=1), gpu_state(g)))
        g.close()
    for y, s, st in runs[1:]:
        assert same_bits(y, runs[0][0]) and same_bits(s, runs[0][1])
        for k in st:
            assert same_bits(st[k], runs[0][2][k]), k
    o = co.TxCwOracle(spec)
    o.set_cw(**cw)
    want = o.process_key(keys, np.zeros(keys.shape, f32))
    assert same_bits(runs[0][0], want[0]) and same_bits(runs[0][1], want[1])


# ---- phases, modes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("mode,nco,offset", [(CW, True, 0x00DA740E), (CWR, True, 0x00DA740E), (CW, False, 0x00DA740E), (CWR, False, 0x00DA740E),
                                             (CW, True, 0), (CWR, False, 0)])
def test_modes_and_wrapping_phases(mode, nco, offset, arith):
    nch = 2
    spec = rc.TxSpec(nch, block=64, interp=4, ni_taps=32, nh_taps=0, mode=mode, arith=arith, nco=nco, nco_step_all=0x01000040, alc=False)
    g, o = cw_pair(spec, shape=taps(16), amplitude=1.0, offset_step=offset, side_level=0.5, side_step=0x00000111)
    st = g.state()
    st["nco_phase"][:] = 0xFFFFFF00
    g.set_state(st)
    g.set_cw_state({"side_phase": np.full(nch, 0xFFFFFF00, np.uint32)})
    o.set_phase(0xFFFFFF00)
    o.set_cw_state({"side_phase": np.full(nch, 0xFFFFFF00, np.uint32)})
    check_call(g, o, random_keys(nch, 128, 9, run=30), side=np.zeros((nch, 128), f32))
    assert_state_equal(g, o)
    so = o.state()
    step = ((0x01000040 if nco else 0) + (offset if mode == CW else -offset)) & 0xFFFFFFFF
    assert (so["nco_phase"] == ((0xFFFFFF00 + 512 * step) & 0xFFFFFFFF)).all() and (so["side_phase"] == ((0xFFFFFF00 + 128 * 0x111) & 0xFFFFFFFF)).all()
    g.close()


# ---- int16 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("rounding", [False, True])
def test_int16_output_sidetone_mix_and_no_sidetone(rounding, arith):
    nch, n = 3, 128
    spec = rc.TxSpec(nch, block=64, interp=2, ni_taps=16, nh_taps=0, mode=CW, arith=arith, nco_step_all=0x3A5F1C27, alc=False, q15_rounding=rounding)
    keys = random_keys(nch, 2 * n, 0x15, run=25)
    buf = np.random.default_rng(5).integers(-3000, 3000, (nch, n)).astype(np.int16)
    buf[:, ::3], buf[:, 1::3] = 32767, -32767                    # the mix saturates at both ends
    for mix in (0, 1):
        g, o = cw_pair(spec, shape=taps(16), amplitude=0.95, offset_step=0x00DA740E, side_level=0.9, side_step=0x0DA740DA, side_mix=mix)
        got, want = keyed(g, keys[:, :n], buf, True), o.process_key(keys[:, :n], buf, True)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), "mix %d" % mix
        if mix:
            assert (want[1] == 32767).any() and (want[1] == -32768).any() and not same_bits(want[1], buf)
        sp = o.state()["side_phase"].copy()
        check_call(g, o, keys[:, n:], side=None, q15=True, what="no sidetone")
        assert_state_equal(g, o)
        assert (o.state()["side_phase"] != sp).all(), "the sidetone's phase advances without a destination"
        g.close()


# ---- state ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
def test_state_round_trip_reset_and_retune(arith):
    nch, n = 5, 128
    spec = rc.TxSpec(nch, block=64, interp=4, ni_taps=64, nh_taps=15, mode=CW, arith=arith, nco_steps=np.arange(1, 6, dtype=np.uint32) * 0x01111111)
    cw = dict(shape=taps(33), amplitude=0.8, offset_step=0x00DA740E, side_level=0.5, side_step=0x0DA740DA, hang_blocks=3)
    g, o = cw_pair(spec, **cw)
    with pytest.raises(Exception):
        gpu_tx(spec).cw_state()                                  # no state before set_cw
    keys = random_keys(nch, 4 * n, 0x77, run=40)
    side = np.zeros((nch, n), f32)
    check_call(g, o, keys[:, :n], side)
    # checkpoint, run, restore, run again: the same bits
    snap = gpu_state(g)
    assert snap["key_state"].any() and snap["side_phase"].all() and snap["tx_on"].any()
    y = keyed(g, keys[:, n:2 * n], side)
    after = gpu_state(g)
    g.set_state({k: snap[k] for k in ("fir_state", "interp_state", "alc_gain", "nco_phase")})
    g.set_cw_state(snap)
    again = keyed(g, keys[:, n:2 * n], side)
    assert same_bits(again[0], y[0]) and same_bits(again[1], y[1])
    for k in after:
        assert same_bits(gpu_state(g)[k], after[k]), k
    o.process_key(keys[:, n:2 * n], side)
    assert_state_equal(g, o)
    # a retune keeps the state; a changed ns_taps clears key_state and nothing else
    cw2 = dict(cw, amplitude=0.3, offset_step=0x01000000, side_level=0.1, side_step=0x01000000, hang_blocks=0)
    assert g.set_cw(**cw2) == 0 and o.set_cw(**cw2) == 0
    assert_state_equal(g, o)
    assert same_bits(gpu_state(g)["key_state"], after["key_state"])
    check_call(g, o, keys[:, 2 * n:3 * n], side, what="retuned")
    cw3 = dict(cw2, shape=taps(20))
    assert g.set_cw(**cw3) == 0 and o.set_cw(**cw3) == 0
    st = gpu_state(g)
    assert st["key_state"].shape == (nch, 19) and not st["key_state"].any() and st["side_phase"].all()
    assert_state_equal(g, o)
    check_call(g, o, keys[:, 3 * n:], side, what="new ns_taps")
    assert_state_equal(g, o)
    # set_mode keeps all state; reset clears it; off and on again starts from a cleared state
    assert g.set_mode(CWR) == 0 and o.set_mode(CWR) == 0
    assert_state_equal(g, o)
    assert g.reset() == 0 and o.reset() == 0
    st = gpu_state(g)
    assert not any(st[k].any() for k in ("key_state", "side_phase", "tx_on", "hold", "nco_phase"))
    assert_state_equal(g, o)
    check_call(g, o, keys[:, :n], side, what="behind reset")
    assert g.clear_cw() == 0 and g.set_cw(**cw3) == 0
    st = gpu_state(g)
    assert not any(st[k].any() for k in ("key_state", "side_phase", "tx_on", "hold"))
    g.close()


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("between", ["usb", "fm"])
def test_an_audio_call_between_two_keyed_calls(between, arith):
    """the I rail of interp_state and nco_phase are shared with the audio entries; ALC gain, fir_state and the FM state are not touched by
    the keyed path.  The BASELINE-like shape: the audio call runs on the fused kernel, whose shared LO must not be trusted behind a
    keyed call."""
    nch, n = 4, 256
    spec = rc.TxSpec(nch, block=64, interp=4, ni_taps=256, nh_taps=63, mode=CW, arith=arith, nco_step_all=0x01000000)
    g, o = cw_pair(spec, shape=taps(48), amplitude=0.8, offset_step=0x00DA740E, side_level=0.5, side_step=0x0DA740DA, hang_blocks=1)
    assert g.set_fm(0.4, 0.9, 0.15, 0x00345678) == 0 and o.set_fm(0.4, 0.9, 0.15, 0x00345678) == 0
    keys = random_keys(nch, 2 * n, 0x99, run=50)
    side = np.zeros((nch, n), f32)
    a0 = rc.synth_audio(0, nch, 0, n)
    assert same_bits(g.process(a0), o.process(a0)), "audio in CW before any keyed call"
    check_call(g, o, keys[:, :n], side, what="first keyed call")
    before = gpu_state(g)
    mode = rc.MODE_USB if between == "usb" else rc.MODE_FM
    assert g.set_mode(mode) == 0 and o.set_mode(mode) == 0
    a1 = rc.synth_audio(0, nch, n, n)
    assert same_bits(g.process(a1), o.process(a1)), "the audio call in between"
    st = gpu_state(g)
    for k in ("key_state", "side_phase", "tx_on", "hold"):
        assert same_bits(st[k], before[k]), "%s is the keyed path's alone" % k
    fm_tone = g.fm_state()["tone_phase"]
    assert g.set_mode(CW) == 0 and o.set_mode(CW) == 0
    check_call(g, o, keys[:, n:], side, what="second keyed call")
    assert_state_equal(g, o)
    end = gpu_state(g)
    for k in ("fir_state", "alc_gain"):
        assert same_bits(end[k], st[k]), "%s is not the keyed path's" % k
    assert same_bits(g.fm_state()["tone_phase"], fm_tone) and same_bits(fm_tone, o.state()["tone_phase"])
    g.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def raw_cw_config(shape, **kw):
    import selenite_rx as sr
    g = sr.TxCwConfig()
    g.struct_size, g.ns_taps, g.shape_coeffs = C.sizeof(sr.TxCwConfig), shape.size, shape.ctypes.data_as(sr.f32p)
    g.amplitude, g.offset_step, g.side_level, g.side_step_all, g.side_mix, g.hang_blocks, g.reserved = 0.5, 0x01000000, 0.25, 0x02000000, 0, 1, 0
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_refusals_write_nothing_and_keep_the_previous_setting():
    import selenite_rx as sr
    nch, n = 2, 64
    spec = rc.TxSpec(nch, block=64, interp=2, ni_taps=16, nh_taps=0, mode=CW, nco_step_all=0x01000000, alc=False)
    g, o = cw_pair(spec, shape=taps(9), amplitude=0.8, offset_step=0x00DA740E, side_level=0.5, side_step=0x0DA740DA)
    L = sr.lib()
    good, nan, inf = taps(9), taps(9).copy(), taps(9).copy()
    nan[4], inf[8] = np.nan, np.inf
    bad = [raw_cw_config(good, struct_size=52), raw_cw_config(good, struct_size=0), raw_cw_config(good, ns_taps=0), raw_cw_config(good, shape_coeffs=None),
           raw_cw_config(nan), raw_cw_config(inf), raw_cw_config(good, amplitude=float("nan")), raw_cw_config(good, amplitude=float("inf")),
           raw_cw_config(good, side_level=float("nan")), raw_cw_config(good, side_level=float("-inf")), raw_cw_config(good, side_mix=2),
           raw_cw_config(good, reserved=1)]
    for b in bad:
        assert L.selenite_tx_set_cw(g.h, C.byref(b)) == rc.ARGUMENT_ERROR
    keys = random_keys(nch, n, 1)
    check_call(g, o, keys, np.zeros((nch, n), f32), what="behind the refused settings")
    assert_state_equal(g, o)
    # refused calls: before set_cw, in another mode, a bad blockSize, a layout over the LDS budget; every buffer stays as it was
    d_k, d_iq, d_s = sr.DeviceBuffer(nch * 128), sr.DeviceBuffer(nch * 128 * 2 * 8), sr.DeviceBuffer(nch * 128 * 4)
    d_k.upload(np.ones((nch, 128), np.uint8))
    iq0, s0 = np.full((nch, 256, 2), 7.5, f32), np.full((nch, 128), -3.25, f32)

    def refused(t, bs, code, q15=False):
        d_iq.upload(iq0)
        d_s.upload(s0)
        before = t.state()
        assert t.process_key(d_k.ptr, d_iq.ptr, d_s.ptr, bs, q15=q15) == code
        t.sync()
        assert same_bits(d_iq.download(iq0.shape, f32), iq0) and same_bits(d_s.download(s0.shape, f32), s0)
        after = t.state()
        assert all(same_bits(before[k], after[k]) for k in before)
        hk, hiq, hs = np.ones((nch, max(bs, 1)), np.uint8), iq0.copy(), s0.copy()
        f = L.selenite_tx_process_key_q15 if q15 else L.selenite_tx_process_key_f32
        assert f(t.h, hk.ctypes.data, hiq.ctypes.data, hs.ctypes.data, bs) == code
        assert same_bits(hiq, iq0) and same_bits(hs, s0)
        ms = C.c_float(-1.0)
        assert L.selenite_tx_time_process_key_device(t.h, d_k.ptr, d_iq.ptr, None, bs, 2, C.byref(ms)) == code and ms.value == -1.0

    fresh = gpu_tx(spec)
    assert fresh.cw_txon() is None
    refused(fresh, 64, rc.ARGUMENT_ERROR)                        # before selenite_tx_set_cw
    assert L.selenite_tx_status(fresh.h) == rc.ARGUMENT_ERROR, "recorded as the audio entries record a refusal"
    fresh.close()
    for bs in (0, 63, 96):
        t = gpu_tx(spec)
        assert t.set_cw(shape=good) == 0
        refused(t, bs, rc.LENGTH_ERROR, q15=bs == 96)
        assert L.selenite_tx_status(t.h) == rc.LENGTH_ERROR
        t.close()
    t = gpu_tx(spec)
    assert t.set_cw(shape=good) == 0 and t.set_mode(rc.MODE_USB) == 0
    refused(t, 64, rc.ARGUMENT_ERROR)                            # the mode is neither CW nor CWR
    assert t.clear_cw() == 0, "off again in any mode"
    t.close()
    t = gpu_tx(spec)
    assert t.set_cw(shape=np.full(16000, 1e-4, f32)) == 0         # the taps and the key window alone are 128 KB of LDS: over the 64 KB budget
    refused(t, 64, rc.LENGTH_ERROR)
    t.close()
    # the instance of the first part never saw a refused call
    assert g.sync() == 0
    g.check()
    assert g.cw_txon() is not None
    g.close()


# ---- break-in ---------------------------------------------------------------------------------------------------------------------------
def test_break_in_flag_over_gaps_shorter_equal_and_longer_than_the_hang_time():
    import selenite_rx as sr
    block, hang = 32, 2
    # key-down blocks: 0, then a gap of 1 block, 2, then a gap of 2 blocks (= hang), 5, then a gap of 3 blocks (hang + 1: off in block 8), 9
    down = [1, 0, 1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0]
    keys = np.zeros((3, len(down) * block), np.uint8)
    for b, d in enumerate(down):
        if d:
            keys[0, b * block + (b * 7) % block] = 1             # one sample anywhere in the block is enough
            keys[1, b * block:(b + 1) * block] = 0x40
    spec = rc.TxSpec(3, block=block, interp=1, ni_taps=0, nh_taps=0, mode=CW, nco_step_all=0x01000000, alc=False)
    g, o = cw_pair(spec, shape=taps(4), hang_blocks=hang)
    seq = []
    for b in range(len(down)):                                   # block by block: the readout behind every block
        check_call(g, o, keys[:, b * block:(b + 1) * block])
        st = g.cw_state()
        assert same_bits(st["tx_on"], o.state()["tx_on"]) and same_bits(st["hold"], o.state()["hold"])
        seq.append((int(st["tx_on"][0]), int(st["hold"][0])))
        assert (st["tx_on"][0], st["hold"][0]) == (st["tx_on"][1], st["hold"][1]) and st["tx_on"][2] == 0
    assert seq == [(1, 2), (1, 1), (1, 2), (1, 1), (1, 0), (1, 2), (1, 1), (1, 0), (0, 0), (1, 2), (1, 1), (1, 0), (0, 0), (0, 0)]
    # the same stream in one call ends in the same state, and the device readout is the state's tx_on
    g2, o2 = cw_pair(spec, shape=taps(4), hang_blocks=hang)
    check_call(g2, o2, keys[:, :10 * block])
    assert_state_equal(g2, o2)
    on = np.full(3, 9, np.uint32)
    assert sr.lib().selenite_rx_memcpy_d2h(on.ctypes.data, g2.cw_txon(), on.nbytes) == 0
    assert list(on) == list(g2.cw_state()["tx_on"]) == [1, 1, 0]
    g.close()
    g2.close()


# ---- the loop through the GPU receiver --------------------------------------------------------------------------------------------------
def test_scale_sampled_channels_and_the_gpu_receiver_reads_the_keying_back():
    """4 099 channels (past any multiple of a workgroup packing), one call per tone frame of 256 audio samples; sampled channels against the
    oracle on every call; the GPU RX chain in CW mode with the tone bank reports the pitch in every frame that lies fully inside an
    element and NONE in every frame fully inside a gap (the device form of tests/test_txcw_oracle.py's loop)."""
    import selenite_rx as sr
    nch, L, fr = 4099, tco.L_RF, tco.LOOP_FRAME
    chans = [0, 1, 63, 64, 4095, 4098]
    shift = np.arange(nch) % 5
    keys, want = tco.loop_keys(nch, 1, shift=shift)
    nfr = want.shape[1]
    spec = rc.TxSpec(nch, block=64, interp=L, ni_taps=256, nh_taps=63, mode=CW, alc=False, nco_step_all=tco.LOOP_STEP)
    g = gpu_tx(spec)
    assert tco.loop_cw(g) == 0
    o = co.TxCwOracle(rc.TxSpec(len(chans), block=64, interp=L, ni_taps=256, nh_taps=63, mode=CW, alc=False, nco_step_all=tco.LOOP_STEP))
    assert tco.loop_cw(o) == 0
    rx = sr.Rx(rc.ChainSpec(nch, 64 * L, L, 256, 63, 0, CW, ARITH_CMSIS, nco=True, nco_step_all=tco.LOOP_STEP, agc=False).config())
    rx.set_tones(tco.loop_tones(), **tco.LOOP_TONES)
    d_k, d_iq, d_y = sr.DeviceBuffer(nch * fr), sr.DeviceBuffer(nch * fr * L * 8), sr.DeviceBuffer(nch * fr * 4)
    got = np.zeros((nch, nfr), np.int64)
    for f in range(nfr):
        k = np.ascontiguousarray(keys[:, f * fr:(f + 1) * fr])
        d_k.upload(k)
        assert g.process_key(d_k.ptr, d_iq.ptr, None, fr) == 0
        assert g.sync() == 0
        iq = d_iq.download((nch, fr * L, 2), np.float32)
        assert same_bits(iq[chans], o.process_key(k[chans])[0]), "frame %d" % f
        rx.process_device(d_iq.ptr, d_y.ptr, fr * L)
        rx.sync()
        rx.check()
        tone, _, frames = rx.tones()
        assert frames == f + 1
        got[:, f] = tone
    st, so = gpu_state(g), o.state()
    so.pop("tone_phase")
    for key in so:
        assert same_bits(st[key][chans], so[key]), key
    asserted = want >= 0
    assert asserted.mean() >= 0.5 and ((~asserted).sum(axis=1) <= 2).all()
    assert (want[asserted] == tco.LOOP_PITCH).any() and (want[asserted] == to.NONE).any()
    bad = asserted & (got != want)
    assert not bad.any(), "channels %s" % np.unique(np.nonzero(bad)[0])[:10]
    g.close()
    rx.close()
