"""GPU: the keyer stage (selenite_tx_set_keyer, csrc/tx_keyer.hip: k_tx_keyer) against the oracle (tests/txkeyer_oracle.py) and the fixture
(tests/golden/txkeyer.npz), bit for bit: key bytes, the eleven state rows and the text rings.  Behind the stage the keyed CW path is held
against a twin instance that is given the oracle's key bytes through process_key.  The shapes are the smallest that can go wrong: channels
around a wave (1, 3, 64, 65, 67), DSP blocks of 24, 64 and 128, calls of 1, 2 and 5 blocks, units shorter than, equal to and longer than a
64-sample tile, a block and a call, mixed within a wave.  The oracle's run-length statement stands in for its sample statement where the
rows are long (tests/test_txkeyer_oracle.py holds the two against each other)."""
import ctypes as C
import os

import numpy as np
import pytest

import rxcommon as rc
import selenite_rx as sr
import txkeyer_cases as kc
import txkeyer_oracle as ko

pytestmark = pytest.mark.gpu
CW, CWR = rc.MODE_CW, rc.MODE_CWR
UNITS = (1, 2, 7, 63, 64, 65, 200, 5000)
MODES = (ko.STRAIGHT, ko.IAMBIC_A, ko.IAMBIC_B)
TEXTS = ("", "E", "AB C", "x  Y", " K~k ", "5 =", "TEST DE K1ABC")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def d2h(ptr, shape, dtype):
    a = np.zeros(shape, dtype)
    assert ptr and sr.lib().selenite_rx_memcpy_d2h(a.ctypes.data, ptr, a.nbytes) == 0
    return a


def make_tx(ch, block=24, mode=CW, arith=rc.ARITH_CMSIS, side=True, rounding=False, steps=None):
    """a small keyed transmitter: L = 2, 8 interpolator taps, 5 shape taps, a pitch offset and (side) a sidetone"""
    spec = rc.TxSpec(ch, block=block, interp=2, ni_taps=8, nh_taps=0, mode=mode, arith=arith, alc=False, nco_step_all=0x03100000,
                     q15_rounding=rounding)
    tx = sr.Tx(spec.config())
    tx._spec = spec
    assert tx.set_cw(sr.keyshape(5), 0.5, offset_step=0x00770000, side_level=0.25 if side else 0.0,
                     side_step=steps if steps is not None else 0x05000000, hang_blocks=2) == 0
    return tx


def mixed_units(ch, seed=0):
    """every unit of UNITS within the first wave where there is room, in an order of its own"""
    rng = np.random.default_rng(0xA11 + seed)
    return np.array([UNITS[i % len(UNITS)] for i in rng.permutation(max(ch, len(UNITS)))[:ch]], np.uint32)


def stage(tx, paddles, n=None, status=0):
    """keyer_run on device buffers -> key bytes; `status`: what the instance has latched by now (a refused call latches its code)"""
    ch = tx.cfg.channels
    n = paddles.shape[1] if paddles is not None else n
    d_k = sr.DeviceBuffer(ch * n)
    d_k.upload(np.full((ch, n), 0xEE, np.uint8))
    d_p = None
    if paddles is not None:
        d_p = sr.DeviceBuffer(ch * n)
        d_p.upload(np.ascontiguousarray(paddles, np.uint8))
    assert tx.keyer_run(d_p.ptr if d_p else None, d_k.ptr, n) == 0
    assert tx.sync() == status
    key = d_k.download((ch, n), np.uint8)
    d_k.free()
    if d_p:
        d_p.free()
    return key


def assert_state(tx, bank, what=""):
    got, want = tx.keyer_state(), bank.state()
    assert set(got) == set(want)
    for k in want:
        assert same_bits(got[k], want[k]), "state %s differs %s: %s / %s" % (k, what, got[k][:8], want[k][:8])
    assert same_bits(tx.keyer_pending(), bank.pending())


class GpuBackend:
    """plays a named case (tests/txkeyer_cases.py) on the stage"""

    def setup(self, mode, units, ring):
        self.tx = make_tx(kc.CHANNELS, kc.BLOCK)
        self.ring = ring
        assert self.tx.set_keyer(mode, np.array(units, np.uint32), ring) == 0

    def send(self, first, texts):
        return self.tx.keyer_send(texts, first, len(texts)) == 0

    def retune(self, mode, units):
        assert self.tx.set_keyer(mode, np.array(units, np.uint32), self.ring) == 0

    def run(self, paddles, n):
        return stage(self.tx, paddles, n)

    def pending(self):
        return self.tx.keyer_pending()

    def state(self):
        return self.tx.keyer_state()


# ---- 1. the fixture ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(rc.GOLDEN_DIR, "txkeyer.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_the_fixture_through_keyer_run(gold, name):
    be = GpuBackend()
    key = kc.play(kc.CASES[name], be)
    assert same_bits(key, gold[name + "/key"]), np.argwhere(key != gold[name + "/key"])[:4]
    st = be.state()
    assert same_bits(np.stack([st[w] for w in ko.WORDS]), gold[name + "/words"]) and same_bits(st["text"], gold[name + "/text"])
    be.tx.close()


# ---- 2. seeded paddles and text, every mode, shapes around a wave, a tile, a block and a call ------------------------------------
@pytest.mark.parametrize("block", [24, 64, 128])
@pytest.mark.parametrize("ch", [1, 3, 64, 65, 67])
def test_random_paddles_and_text_against_the_oracle(ch, block):
    for mode in MODES:
        rng = np.random.default_rng(1000 * ch + 10 * block + mode)
        units = mixed_units(ch, mode)
        tx = make_tx(ch, block)
        assert tx.set_keyer(mode, units, 16) == 0
        bank = ko.Bank(ch, mode, units, 16)
        texts = [TEXTS[int(i)] for i in rng.integers(0, len(TEXTS), ch)]
        for c, t in enumerate(texts):
            assert tx.keyer_send(t, c, 1) == 0 and bank.send(t, c, 1)
        assert_state(tx, bank, "behind keyer_send")
        for call, nblk in enumerate((1, 2, 5, 1)):
            n = nblk * block
            pad = ko.random_paddles(rng, ch, n, np.minimum(units, 300), p_idle=0.9 if call == 0 else 0.5)
            if call == 0:
                pad[::2] = 0                     # every other channel sends its text undisturbed at first
            got, want = stage(tx, pad), bank.run(pad, events=True)
            assert same_bits(got, want), (mode, call, np.argwhere(got != want)[:4])
        assert_state(tx, bank, "mode %d" % mode)
        tx.close()


@pytest.mark.parametrize("unit", [1, 2, 7, 64])
def test_edges_on_the_last_and_first_sample_of_tiles_blocks_and_calls(unit):
    block, ch = 24, 8
    for mode in MODES:
        tx = make_tx(ch, block)
        assert tx.set_keyer(mode, unit, 8) == 0
        bank = ko.Bank(ch, mode, unit, 8)
        assert tx.keyer_send("EN", 4, 4) == 0 and bank.send("EN", 4, 4)
        for nblk in (1, 5, 6, 2):                # calls of 24, 120, 144 and 48 samples
            n = nblk * block
            pad = np.zeros((ch, n), np.uint8)
            marks = sorted({0, n - 1} | {e for e in (23, 24, 47, 48, 63, 64, 65, 71, 72, 127, 128) if e < n})
            for c in range(ch):
                bit = (1, 2, 3, 4, 5, 6, 7, 1)[c]
                for i, e in enumerate(marks):    # channel c: a press from mark i to mark i + 1 for every (i + c) % 3 == 0, one sample long at the end
                    if (i + c) % 3 == 0:
                        pad[c, e:(marks[i + 1] if i + 1 < len(marks) else n)] |= bit
                    if (i + c) % 3 == 1:
                        pad[c, e] |= bit
            got, want = stage(tx, pad), bank.run(pad)
            assert same_bits(got, want), (mode, nblk, np.argwhere(got != want)[:4])
        assert_state(tx, bank)
        tx.close()


def test_a_dah_longer_than_a_call_and_text_at_a_unit_of_5000():
    ch, block = 3, 64
    tx = make_tx(ch, block)
    units = np.array([5000, 700, 5000], np.uint32)
    assert tx.set_keyer(ko.IAMBIC_B, units, 8) == 0
    bank = ko.Bank(ch, ko.IAMBIC_B, units, 8)
    assert tx.keyer_send("T", 2, 1) == 0 and bank.send("T", 2, 1)
    pad = np.zeros((ch, 5 * block), np.uint8)
    pad[0, 3:9], pad[1, 100:] = 2, 3
    for call in range(4):                        # 1280 samples: channel 0's dah (15000 samples) outlasts them all
        p = pad if call == 0 else np.zeros_like(pad)
        got, want = stage(tx, p), bank.run(p, events=True)
        assert same_bits(got, want), call
    st = tx.keyer_state()
    assert st["phase"][0] == ko.MARK and st["phase"][2] == ko.MARK and st["left"][0] == 15000 - 1280 + 3 and st["left"][2] == 15000 - 1280
    assert_state(tx, bank)
    tx.close()


# ---- 3. however the stream is cut ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [24, 64])
def test_ten_blocks_as_one_call_ten_calls_and_three_plus_seven(block):
    ch, mode = 67, ko.IAMBIC_B
    rng = np.random.default_rng(0xC07 + block)
    units = mixed_units(ch)
    pad = ko.random_paddles(rng, ch, 10 * block, np.minimum(units, 100), p_idle=0.6)
    pad[:5] = 0
    outs, states = [], []
    for cuts in ([10], [1] * 10, [3, 7]):
        tx = make_tx(ch, block)
        assert tx.set_keyer(mode, units, 16) == 0 and tx.keyer_send("CQ K", 0, ch) == 0
        at, keys = 0, []
        for nb in cuts:
            keys.append(stage(tx, pad[:, at:at + nb * block]))
            at += nb * block
        outs.append(np.concatenate(keys, axis=1))
        states.append(tx.keyer_state())
        tx.close()
    bank = ko.Bank(ch, mode, units, 16)
    assert bank.send("CQ K")
    want = bank.run(pad, events=True)
    for o, st in zip(outs, states):
        assert same_bits(o, want)
        for k, v in bank.state().items():
            assert same_bits(st[k], v), k


# ---- 4. state, reset, retune -------------------------------------------------------------------------------------------------------------------
def test_state_round_trip_mid_mark_and_mid_character_reset_and_retune():
    ch, block = 5, 24
    units = np.array([7, 9, 64, 3, 30], np.uint32)
    rng = np.random.default_rng(0x57A7E)
    a, fresh = make_tx(ch, block), make_tx(ch, block)
    for t in (a, fresh):
        assert t.set_keyer(ko.IAMBIC_A, units, 8) == 0
    bank = ko.Bank(ch, ko.IAMBIC_A, units, 8)
    assert_state(a, bank, "behind set_keyer")
    assert a.keyer_send("QRL?", 0, ch) == 0 and bank.send("QRL?")
    pad = ko.random_paddles(rng, ch, 2 * block, units)
    pad[:3] = 0
    assert same_bits(stage(a, pad), bank.run(pad))
    st = a.keyer_state()
    assert (st["phase"][:3] != ko.IDLE).all() and (st["code"][:2] > 1).all(), "mid-mark or mid-gap, mid-character"
    fresh.set_keyer_state(st)
    assert_state(fresh, bank, "after set_keyer_state")
    pad2 = ko.random_paddles(rng, ch, 5 * block, units)
    pad2[:3] = 0
    want = bank.run(pad2)
    assert same_bits(stage(a, pad2), want) and same_bits(stage(fresh, pad2), want)
    assert_state(fresh, bank)
    # members that are missing stay
    fresh.set_keyer_state({"skipped": np.full(ch, 9, np.uint32)})
    for k in bank.ch:
        k.skipped = 9
    assert_state(fresh, bank, "one member")
    for k in bank.ch:
        k.skipped = 0                            # (`bank` follows `a` from here on)
    # a retune keeps the state; a new ring clears the text queue and nothing else
    assert a.set_keyer(ko.IAMBIC_B, 11, 8) == 0
    bank.retune(ko.IAMBIC_B, 11)
    assert_state(a, bank, "after a retune")
    assert a.keyer_send("K", 0, ch) == 0 and bank.send("K")
    assert a.set_keyer(ko.IAMBIC_B, 11, 4) == 0
    before = bank.state()
    b4 = ko.Bank(ch, ko.IAMBIC_B, 11, 4)
    b4.set_state({k: v for k, v in before.items() if k != "text"})
    for k in b4.ch:
        k.tail = k.head = k.tgap = 0
        k.code = 1
    a._keyer_ring = 4
    assert_state(a, b4, "after a new ring")
    # reset: the state of the first set_keyer; so is the first call behind NULL
    assert a.reset() == 0
    assert_state(a, ko.Bank(ch, ko.IAMBIC_B, 11, 4), "after reset")
    assert fresh.clear_keyer() == 0 and fresh.set_keyer(ko.IAMBIC_A, units, 8) == 0
    assert_state(fresh, ko.Bank(ch, ko.IAMBIC_A, units, 8), "after NULL and set_keyer")
    a.close(); fresh.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def raw_config(**kw):
    g = sr.TxKeyerConfig()
    g.struct_size, g.mode, g.unit_all, g.ring, g.reserved = C.sizeof(sr.TxKeyerConfig), ko.IAMBIC_A, 6, 8, 0
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_refusals_write_nothing_and_keep_the_previous_setting():
    ch, block, n = 3, 24, 48
    L = sr.lib()
    tx = make_tx(ch, block)
    # before set_keyer
    d_p, d_iq, d_s, d_k = (sr.DeviceBuffer(ch * n), sr.DeviceBuffer(ch * n * 2 * 8), sr.DeviceBuffer(ch * n * 4), sr.DeviceBuffer(ch * n))
    iq_fill, s_fill, k_fill = np.full((ch, n * 2, 2), 7.0, np.float32), np.full((ch, n), 5.0, np.float32), np.full((ch, n), 0xEE, np.uint8)
    pad = np.full((ch, n), 1, np.uint8)
    d_p.upload(pad); d_iq.upload(iq_fill); d_s.upload(s_fill); d_k.upload(k_fill)

    def untouched():
        return (same_bits(d_iq.download(iq_fill.shape, np.float32), iq_fill) and same_bits(d_s.download(s_fill.shape, np.float32), s_fill)
                and same_bits(d_k.download(k_fill.shape, np.uint8), k_fill))

    assert tx.process_paddles(d_p.ptr, d_iq.ptr, d_s.ptr, n) == sr.ARGUMENT_ERROR
    assert tx.keyer_run(d_p.ptr, d_k.ptr, n) == sr.ARGUMENT_ERROR
    assert tx.keyer_send("E") == sr.ARGUMENT_ERROR and tx.keyer_key_device() is None
    assert L.selenite_tx_keyer_pending(tx.h, np.zeros(ch, np.uint32).ctypes.data_as(sr.u32p)) == sr.ARGUMENT_ERROR
    assert L.selenite_tx_get_keyer_state(tx.h, C.byref(sr.TxKeyerStateView())) == sr.ARGUMENT_ERROR
    ms = C.c_float()
    assert L.selenite_tx_time_keyer_stage_device(tx.h, None, n, 1, C.byref(ms)) == sr.ARGUMENT_ERROR
    assert untouched()
    tx.close()
    # set_keyer needs set_cw
    bare = sr.Tx(rc.TxSpec(ch, block=block, interp=2, ni_taps=8, nh_taps=0, mode=CW, alc=False).config())
    assert bare.set_keyer(ko.IAMBIC_A, 6, 8) == sr.ARGUMENT_ERROR
    bare.close()

    tx = make_tx(ch, block)
    units = np.array([6, 4, 9], np.uint32)
    assert tx.set_keyer(ko.IAMBIC_A, units, 8) == 0 and tx.keyer_send("AR", 0, ch) == 0
    bank = ko.Bank(ch, ko.IAMBIC_A, units, 8)
    assert bank.send("AR")
    warm = np.zeros((ch, block), np.uint8)
    assert same_bits(stage(tx, warm), bank.run(warm))
    chain0, cw0 = tx.state(), tx.cw_state()
    # every bad field: ARGUMENT_ERROR, the previous setting and the state stay
    zero_unit, big_unit = np.array([6, 0, 6], np.uint32), np.array([6, 6, (1 << 24) + 1], np.uint32)
    bad = [dict(struct_size=44), dict(mode=3), dict(unit_all=0), dict(unit_all=(1 << 24) + 1), dict(unit=zero_unit.ctypes.data_as(sr.u32p)),
           dict(unit=big_unit.ctypes.data_as(sr.u32p)), dict(ring=0), dict(ring=65537), dict(reserved=1)]
    for kw in bad:
        assert L.selenite_tx_set_keyer(tx.h, C.byref(raw_config(**kw))) == sr.ARGUMENT_ERROR, kw
        assert_state(tx, bank, "after a refused set_keyer %s" % kw)
    assert L.selenite_tx_set_keyer(tx.h, C.byref(raw_config(unit_all=1 << 24, ring=65536))) == 0, "the largest unit and ring"
    assert tx.set_keyer(ko.IAMBIC_A, units, 8) == 0
    bank = ko.Bank(ch, ko.IAMBIC_A, units, 8)    # (the ring changed twice: the queue is empty, the element under way stayed)
    st = tx.keyer_state()
    bank.set_state(st)
    assert tx.keyer_send("N", 0, ch) == 0 and bank.send("N")

    def refused(code, call):
        assert call() == code
        assert untouched()
        assert_state(tx, bank)
        for k, v in tx.state().items():
            assert same_bits(v, chain0[k]), k
        for k, v in tx.cw_state().items():
            assert same_bits(v, cw0[k]), k

    refused(sr.LENGTH_ERROR, lambda: tx.process_paddles(d_p.ptr, d_iq.ptr, d_s.ptr, 0))
    refused(sr.LENGTH_ERROR, lambda: tx.process_paddles(d_p.ptr, d_iq.ptr, d_s.ptr, block + 1))
    refused(sr.ARGUMENT_ERROR, lambda: tx.process_paddles(d_p.ptr, None, d_s.ptr, n))
    refused(sr.LENGTH_ERROR, lambda: tx.keyer_run(d_p.ptr, d_k.ptr, block - 1))
    refused(sr.ARGUMENT_ERROR, lambda: tx.keyer_run(d_p.ptr, None, n))
    refused(sr.LENGTH_ERROR, lambda: tx.process_paddles_host(pad[:, :block + 2])[0])
    assert tx.set_mode(rc.MODE_USB) == 0
    refused(sr.ARGUMENT_ERROR, lambda: tx.process_paddles(d_p.ptr, d_iq.ptr, d_s.ptr, n))
    refused(sr.ARGUMENT_ERROR, lambda: tx.process_paddles(d_p.ptr, d_iq.ptr, d_s.ptr, n, q15=True))
    refused(sr.ARGUMENT_ERROR, lambda: tx.process_paddles_host(pad)[0])
    assert same_bits(stage(tx, warm, status=sr.LENGTH_ERROR), bank.run(warm)), "the stage alone runs in any mode"
    assert tx.set_mode(CW) == 0
    # keyer_send: a text that one channel of the range has no room for writes nothing anywhere
    assert tx.keyer_send("ABCDEFG", 0, 1) == 0 and bank.send("ABCDEFG", 0, 1)
    refused(sr.LENGTH_ERROR, lambda: tx.keyer_send("XY", 0, ch))
    refused(sr.LENGTH_ERROR, lambda: tx.keyer_send(["XY", "XY"], 0, 2))
    refused(sr.LENGTH_ERROR, lambda: tx.keyer_send("123456789", 1, 1))
    refused(sr.ARGUMENT_ERROR, lambda: tx.keyer_send("E", 2, 2))
    refused(sr.ARGUMENT_ERROR, lambda: tx.keyer_send("E", 4, 0))
    refused(sr.ARGUMENT_ERROR, lambda: L.selenite_tx_keyer_send(tx.h, 0, 1, None, 2, 0))
    refused(sr.ARGUMENT_ERROR, lambda: L.selenite_tx_keyer_send(tx.h, 0, 1, b"E", 1, 2))
    assert tx.keyer_send("XY", 1, 2) == 0 and bank.send("XY", 1, 2)
    assert_state(tx, bank, "behind the sends that fit")
    assert tx.clear_cw() == 0                    # the keyed path off: the paddle entries are the key entries
    assert tx.process_paddles(d_p.ptr, d_iq.ptr, d_s.ptr, n) == sr.ARGUMENT_ERROR and untouched()
    assert_state(tx, bank, "after the call without set_cw")
    for d in (d_p, d_iq, d_s, d_k):
        d.free()
    tx.close()


# ---- 6. behind the stage: the keyed path against a twin instance ---------------------------------------------------------------
def twin_call(tw, key, side, q15, host):
    """the twin's key call -> (I/Q, sidetone or None)"""
    ch, n = key.shape
    dt = np.int16 if q15 else np.float32
    if host:
        rcode, iq, sd = tw.process_key_host(key, side=side, q15=q15)
        assert rcode == 0
        return iq, sd
    d_k, d_iq = sr.DeviceBuffer(key.nbytes), sr.DeviceBuffer(ch * n * 2 * 2 * np.dtype(dt).itemsize)
    d_k.upload(key)
    d_s = None
    if side is not None:
        d_s = sr.DeviceBuffer(side.nbytes)
        d_s.upload(np.ascontiguousarray(side, dt))
    assert tw.process_key(d_k.ptr, d_iq.ptr, d_s.ptr if d_s else None, n, q15=q15) == 0 and tw.sync() == 0
    out = d_iq.download((ch, n * 2, 2), dt), (d_s.download((ch, n), dt) if d_s else None)
    d_k.free(); d_iq.free()
    if d_s:
        d_s.free()
    return out


def paddle_call(tx, pad, n, side, q15, host):
    ch = tx.cfg.channels
    dt = np.int16 if q15 else np.float32
    if host:
        rcode, iq, sd = tx.process_paddles_host(pad, n, side=side, q15=q15)
        assert rcode == 0
        return iq, sd
    d_iq = sr.DeviceBuffer(ch * n * 2 * 2 * np.dtype(dt).itemsize)
    d_p = d_s = None
    if pad is not None:
        d_p = sr.DeviceBuffer(pad.nbytes)
        d_p.upload(pad)
    if side is not None:
        d_s = sr.DeviceBuffer(side.nbytes)
        d_s.upload(np.ascontiguousarray(side, dt))
    assert tx.process_paddles(d_p.ptr if d_p else None, d_iq.ptr, d_s.ptr if d_s else None, n, q15=q15) == 0 and tx.sync() == 0
    out = d_iq.download((ch, n * 2, 2), dt), (d_s.download((ch, n), dt) if d_s else None)
    d_iq.free()
    for d in (d_p, d_s):
        if d:
            d.free()
    return out


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("q15", [False, True])
@pytest.mark.parametrize("mode", [CW, CWR])
def test_process_paddles_is_process_key_on_the_oracles_bytes(mode, q15, host):
    ch, block = 67, 24
    dt = np.int16 if q15 else np.float32
    units = mixed_units(ch)
    steps = (np.arange(ch, dtype=np.uint32) * 0x00310000 + 0x04000000).astype(np.uint32)
    for with_side in (True, False):
        for arith in (rc.ARITH_CMSIS, rc.ARITH_FMA):
            rng = np.random.default_rng(0x7717 + mode)
            tx, tw = (make_tx(ch, block, mode, arith, steps=steps, rounding=q15) for _ in range(2))
            assert tx.set_keyer(ko.IAMBIC_B, units, 16) == 0 and tx.keyer_send("DE K", 0, ch) == 0
            bank = ko.Bank(ch, ko.IAMBIC_B, units, 16)
            assert bank.send("DE K")
            for call, nblk in enumerate((2, 5, 1)):
                n = nblk * block
                pad = ko.random_paddles(rng, ch, n, np.minimum(units, 60), p_idle=0.7)
                pad[1::2] = 0
                if call == 2:
                    pad = None                   # NULL paddles: the text memory alone
                side = (rng.uniform(-0.5, 0.5, (ch, n)) * (32768 if q15 else 1)).astype(dt) if with_side else None
                key = bank.run(pad, n, events=True)
                got = paddle_call(tx, pad, n, side, q15, host)
                want = twin_call(tw, key, side, q15, host)
                assert same_bits(got[0], want[0]), "I/Q, call %d" % call
                assert (side is None and got[1] is None) or same_bits(got[1], want[1]), "sidetone, call %d" % call
                assert same_bits(d2h(tx.keyer_key_device(), (ch, n), np.uint8), key), "the stage's key bytes, call %d" % call
                assert same_bits(d2h(tx.cw_txon(), ch, np.uint32), d2h(tw.cw_txon(), ch, np.uint32))
            for k, v in tw.cw_state().items():
                assert same_bits(tx.cw_state()[k], v), k
            for k, v in tw.state().items():
                assert same_bits(tx.state()[k], v), k
            assert (tx.cw_state()["tx_on"] != 0).any()
            assert_state(tx, bank)
            tx.close(); tw.close()


def test_null_paddles_are_zero_paddles():
    ch, block, n = 65, 64, 128
    a, b = make_tx(ch, block), make_tx(ch, block)
    units = mixed_units(ch)
    outs = []
    for t, pad in ((a, None), (b, np.zeros((ch, n), np.uint8))):
        assert t.set_keyer(ko.IAMBIC_A, units, 8) == 0 and t.keyer_send("VVV", 0, ch) == 0
        outs.append(paddle_call(t, pad, n, np.zeros((ch, n), np.float32), False, False) + (d2h(t.keyer_key_device(), (ch, n), np.uint8),))
    for x, y in zip(*outs):
        assert same_bits(x, y)
    assert outs[0][2].any()
    for k, v in a.keyer_state().items():
        assert same_bits(v, b.keyer_state()[k]), k
    a.close(); b.close()


@pytest.mark.parametrize("block", [24, 64])
def test_the_timed_stage_runs_the_same_law(block):
    """time_keyer_stage: an untimed launch and `iters` timed ones, each a call of its own"""
    ch, n = 67, 5 * block
    rng = np.random.default_rng(0x71ED)
    units = mixed_units(ch)
    for mode in MODES:
        tx = make_tx(ch, block)
        assert tx.set_keyer(mode, units, 16) == 0 and tx.keyer_send("R TU", 0, ch) == 0
        bank = ko.Bank(ch, mode, units, 16)
        assert bank.send("R TU")
        pad = ko.random_paddles(rng, ch, n, np.minimum(units, 40), p_idle=0.6)
        pad[::3] = 0
        d_p = sr.DeviceBuffer(pad.nbytes)
        d_p.upload(pad)
        assert tx.time_keyer_stage(d_p.ptr, n, 2) > 0.0
        for _ in range(3):
            want = bank.run(pad, events=True)
        assert same_bits(d2h(tx.keyer_key_device(), (ch, n), np.uint8), want)
        assert_state(tx, bank, "mode %d" % mode)
        if mode == ko.IAMBIC_A:                  # and without paddles
            assert tx.time_keyer_stage(None, n, 1) > 0.0
            for _ in range(2):
                want = bank.run(None, n, events=True)
            assert same_bits(d2h(tx.keyer_key_device(), (ch, n), np.uint8), want)
            assert_state(tx, bank)
        d_p.free()
        tx.close()


# ---- 7. the loop: text -> keyer -> k_tx_cw -> the chain's RX in CW -> k_cwdec -> the same text ----------------------------------
def loop_text(c):
    """channel c's own text: a word and a call sign of its own, lower case on the odd channels"""
    word = ("CQ", "DE", "TU", "QRZ?", "73", "R", "= K", "QSL")[c % 8]
    call = "%s%d%s%s%s" % ("KWNA"[c % 4], c % 10, chr(65 + c % 26), chr(65 + (7 * c + 3) % 26), chr(65 + (3 * c + 11) % 26))
    t = "%s %s" % (word, call)
    return t.lower() if c % 2 else t


def test_the_loop_67_transmitters_send_their_own_text_at_their_own_speed_and_the_receiver_reads_it():
    """67 channels, units of 1000 down to 300 audio samples (12 to 40 WPM at 10 kHz of audio), DSP blocks of 64: the transmitter of
    tests/test_gpu_cwdec.py's read-back (the same pitch, L = 4) keyed by the keyer from its text memory, every channel a text of its own.
    The receiver's decoder runs at its defaults, and, as an operator tunes a decoder to the station he listens to, every channel's `unit`
    row is set to its transmitter's speed before the first mark (Rx.set_cwdec_state): from the default of 10 blocks a decoder has to see
    dits before it can tell the dahs and the gaps between characters of a 40 WPM station (a dah of 14 blocks), which would tie the texts
    to what the decoder can acquire.  Behind the last character come four units of key-up."""
    import test_txcw_oracle as tco
    ch, L, fs, block = 67, tco.L_RF, 10000, 64
    wpm = np.linspace(12.0, 40.0, ch)
    units = np.array([sr.keyer_unit(w, fs) for w in wpm], np.uint32)
    assert units[0] == 1000 and units[-1] == 300 and len(set(units.tolist())) > 60
    texts = [loop_text(c) for c in range(ch)]
    assert len({t.upper() for t in texts}) == ch and max(len(t) for t in texts) <= 16
    tx = sr.Tx(rc.TxSpec(ch, block=block, interp=L, ni_taps=256, nh_taps=63, mode=CW, alc=False, nco_step_all=tco.LOOP_STEP).config())
    assert tco.loop_cw(tx) == 0
    assert tx.set_keyer(ko.IAMBIC_B, units, 16) == 0
    rx = sr.Rx(rc.ChainSpec(ch, block * L, L, 256, 63, 0, CW, rc.ARITH_CMSIS, nco=True, nco_step_all=tco.LOOP_STEP, agc=False).config())
    rx.set_cwdec()
    rx.set_cwdec_state({"unit": np.round(units.astype(np.float64) * 256.0 / block).astype(np.uint32)})       # Q8 blocks
    need = max(len(sr.morse_key(t, int(u))) + 4 * int(u) for t, u in zip(texts, units))
    call = 64 * block
    d_iq, d_y = sr.DeviceBuffer(ch * call * L * 8), sr.DeviceBuffer(ch * call * 4)
    assert tx.process_paddles(None, d_iq.ptr, None, 40 * block) == 0     # the lead of the read-back: the receiver's filters and floor settle
    assert tx.sync() == 0                        # (two instances, two streams, one I/Q buffer)
    rx.process_device(d_iq.ptr, d_y.ptr, 40 * block * L)
    rx.sync()
    for c in range(ch):
        assert tx.keyer_send(texts[c], c, 1) == 0
    for _ in range(-(-need // call)):
        assert tx.process_paddles(None, d_iq.ptr, None, call) == 0
        assert tx.sync() == 0
        rx.process_device(d_iq.ptr, d_y.ptr, call * L)
        rx.sync()
    rx.check()
    st = tx.keyer_state()
    assert (tx.keyer_pending() == 0).all() and (st["phase"] == ko.IDLE).all() and (st["skipped"] == 0).all()
    got = rx.cw_text()
    print("read back: %r" % (got,))
    for c in range(ch):
        assert got[c].rstrip(" ") == texts[c].upper(), (c, float(wpm[c]), got[c], texts[c])
    d_iq.free(); d_y.free()
    tx.close(); rx.close()
