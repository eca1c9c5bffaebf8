"""GPU: the key and frame entries of the TX chain at the smallest shapes that reach code no other test runs (read against csrc/tx_in.hip and
csrc/tx_cw.hip), every comparison against the oracle (tests/txin_oracle.py's TxInOracle over tests/txcw_oracle.py's TxCwOracle) through
tx_fuzz_runner.EntryPair: the stage's audio, the sidetone, the I/Q and every state array on bits, the I/Q of a call k_tx_split16 serves at
the bar of tests/test_gpu_tx.py against the CMSIS twin.

  (a) k_tx_in with more than one 1024-sample chunk in a tile (block * M > 1024): the loop over the further chunks, 16-byte and element loads
  (b) k_tx_in with 48 ... 64 KB of dynamic LDS (the hipFuncSetAttribute branch), and the boundary: 65 508 bytes run, 65 540 are refused
  (c) frame calls served by k_tx_fused and k_tx_split16 (whole passes) and k_tx_generic behind them, in all three arithmetics
  (d) key calls on a SELENITE_ARITH_SPLIT16 instance: k_tx_cw runs as FMA, the next whole pass goes to k_tx_split16 with a per-channel LO
  (e) key calls shorter than the interpolator history: the Q rail of interp_state is shifted, not cleared
  (f) k_tx_cw with 48 ... 64 KB of dynamic LDS

The byte counts come from in_layout and cw_layout as tests/tx_entry_fuzz_cases.py restates them; they are recomputed here."""
import numpy as np
import pytest

import rxcommon as rc
import tx_entry_fuzz_cases as ez
import tx_fuzz_cases as fz
import tx_fuzz_runner as fr
from rxcommon import ARITH_CMSIS, ARITH_FMA, ARITH_SPLIT16

pytestmark = pytest.mark.gpu
f32 = np.float32
ARITHS = [ARITH_CMSIS, ARITH_FMA, ARITH_SPLIT16]
MONO, LEFT, RIGHT, MIX = ez.MONO, ez.LEFT, ez.RIGHT, ez.MIX
# attack = decay = 1: the level is the block's mean square, so the gate follows the quiet DSP blocks of make_frames at once
VOX = dict(gate=1, hang=0, attack=1.0, decay=1.0, open_level=5e-4, close_level=2.5e-4, level_init=0.0)


def taps(nt, seed=0):
    """nt finite taps of both signs without symmetry: the order of the taps shows in the bits"""
    return (np.random.default_rng(0x3E90 + nt + seed).uniform(-1, 1, nt) / max(nt, 4) * 4).astype(f32)


def make_frames(nch, words, entry, seed, quiet=None):
    """different data in every channel; `quiet` = (channel, from, to) in words: a stretch 60 dB down"""
    x = np.random.default_rng(seed).uniform(-1, 1, (nch, words))
    if quiet:
        x[quiet[0], quiet[1]:quiet[2]] *= 1e-3
    return x.astype(f32) if entry.startswith("f32") else np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)


def random_keys(nch, n, seed, run=7):
    rng = np.random.default_rng(seed)
    k = np.zeros((nch, n), np.uint8)
    for c in range(nch):
        at, v = 0, int(rng.integers(0, 2))
        while at < n:
            ln = int(rng.integers(1, 2 * run))
            k[c, at:at + ln] = v
            at, v = at + ln, 1 - v
    return k


def one_block_then_two(p, block, M, pick, entry, seed):
    """one call of one DSP block, then one call of two (the next tile's prefetch runs); the gate closes on one channel's quiet block"""
    per = block * M * (1 if pick == MONO else 2)
    p.frame_call(make_frames(p.spec.channels, per, entry, seed, quiet=(1, 0, per)), entry, what="one block")
    p.frame_call(make_frames(p.spec.channels, 2 * per, entry, seed + 1, quiet=(0, 0, per)), entry, what="two blocks")
    st = p.g.in_state()
    assert st["dec_state"].any() and (st["opens"] >= 1).all() and (st["open_blocks"] < 3).any()
    p.assert_state("behind both calls")


# ---- (a) more than one chunk in a tile -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [97, 256])
@pytest.mark.parametrize("block,M,entry,pick", [(136, 8, "f32_dev", MONO), (264, 8, "q15_dev", LEFT), (520, 2, "f32_dev", MIX),
                                                (1030, 1, "q15_dev", MONO)])
def test_tiles_of_more_than_one_chunk(block, M, entry, pick, nd):
    fw, isz = (1 if pick == MONO else 2), (4 if entry.startswith("f32") else 2)
    assert ez.in_tile(block, M) == block and block * M > 1024, "a tile is one DSP block of more than one 1024-sample chunk"
    assert ez.in_wide(block, M, fw, isz, block) == (block != 1030), "2060-byte rows take the element loads"
    assert ez.in_lds_bytes(block, M, nd) <= 48 * 1024
    spec = rc.TxSpec(3, block=block, interp=2, ni_taps=16, nh_taps=15, arith=ARITH_FMA if nd == 97 else ARITH_CMSIS)
    p = fr.EntryPair(spec, kernel=fz.GENERIC)
    try:
        p.set_in(M=M, coeffs=taps(nd), pick=pick, gain=0.8, vox=VOX)
        one_block_then_two(p, block, M, pick, entry, 0xA000 + block + nd)
    finally:
        p.close()


# ---- (b) dynamic LDS between 48 and 64 KB, and the boundary --------------------------------------------------------------------------------
def bare_spec(block):
    """interp 1, no filters: the stage's layout is the binding one"""
    spec = rc.TxSpec(2, block=block, interp=1, ni_taps=0, nh_taps=0)
    assert fz.tx_lds_bytes(block, 1, 0, 0) < 48 * 1024
    return spec


@pytest.mark.parametrize("block,lds", [(1700, 61476), (1812, 65508)])
def test_stage_layouts_between_48_and_64_kb(block, lds):
    assert 48 * 1024 < ez.in_lds_bytes(block, 8, 64) == lds <= 64 * 1024
    p = fr.EntryPair(bare_spec(block), kernel=fz.GENERIC)
    try:
        p.set_in(M=8, coeffs=taps(64), pick=MONO, gain=1.1, vox=VOX)
        one_block_then_two(p, block, 8, MONO, "f32_dev", 0xB000 + block)
    finally:
        p.close()


def test_the_first_stage_layout_over_64_kb_is_refused_and_writes_nothing():
    import selenite_rx as sr
    block = 1813
    assert ez.in_lds_bytes(block, 8, 64) == 65540 > 64 * 1024 >= ez.in_lds_bytes(block - 1, 8, 64)
    g = sr.Tx(bare_spec(block).config())
    assert g.set_in(M=8, coeffs=taps(64), pick=MONO, gain=1.1, vox=VOX) == 0
    fill = g.in_state()
    fill["dec_state"][:], fill["level"][:], fill["hold"][:], fill["opens"][:] = 1.5, 0.25, 9, 4
    g.set_in_state(fill)
    chain = g.state()
    frames = make_frames(2, block * 8, "f32_dev", 0xB813)
    d_f, d_iq = sr.DeviceBuffer(frames.nbytes), sr.DeviceBuffer(2 * block * 2 * 4)
    d_f.upload(frames)
    sentinel = np.full((2, block, 2), 7.5, f32)
    d_iq.upload(sentinel)
    assert g.process_frames(d_f.ptr, d_iq.ptr, block, fr.KINDS["f32"]) == rc.LENGTH_ERROR
    assert g.sync() == rc.LENGTH_ERROR
    fr.assert_bits(d_iq.download((2, block, 2), f32), sentinel, "the destination")
    now, now_chain = g.in_state(), g.state()
    for k in fill:
        fr.assert_bits(now[k], fill[k], "stage state " + k)
    for k in chain:
        fr.assert_bits(now_chain[k], chain[k], "chain state " + k)
    g.close()


# ---- (c) frames into the matrix kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("entry", ["f32_dev", "q15_dev", "q15f_dev"])
def test_frames_into_the_matrix_kernels(entry, arith):
    spec = rc.TxSpec(5, arith=arith, nco_step_all=0x03000000)       # the fused geometry, designed taps, a grid step shared by all channels
    name = fz.SPLIT16 if arith == ARITH_SPLIT16 else fz.FUSED
    inst = fz.FAMILY[name]
    p = fr.EntryPair(spec, kernel=name)
    try:
        p.set_in(M=2, coeffs=taps(33), pick=RIGHT, gain=0.7, vox=VOX)
        for k, (bs, served) in enumerate(((256, inst), (512, inst), (64, "generic"), (256, inst))):
            w = bs * 2 * 2
            x = make_frames(5, w, entry, 0xC000 + 16 * arith + k, quiet=(k % 5, w // 4, w // 2))
            p.frame_call(x, entry, served, what="%d samples on %s" % (bs, served))
            assert p.g.kernel_name() == name
    finally:
        p.close()


# ---- (d) key calls on a SPLIT16 instance ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q15", [False, True])
def test_key_calls_on_a_split16_instance(q15):
    nch = 3
    spec = rc.TxSpec(nch, arith=ARITH_SPLIT16, mode=rc.MODE_CW, nco_step_all=0x05000000, q15_rounding=q15)
    p = fr.EntryPair(spec, kernel=fz.SPLIT16)
    dt = np.int16 if q15 else f32
    try:
        p.set_cw(shape=taps(16), amplitude=0.8, offset_step=0x00DA740E, side_level=0.4, side_step=0x0B4E81B5, side_mix=0, hang_blocks=1)

        def audio(k, n):
            a = rc.synth_audio(0, nch, 700 * k, n) * f32(0.5)
            return np.clip(np.trunc(a * f32(32768.0)), -32768, 32767).astype(np.int16) if q15 else a

        p.key_call(random_keys(nch, 128, 0xD001, run=20), np.zeros((nch, 128), dt), q15, device=True, what="key call")
        assert len(set(p.g.state()["nco_phase"].tolist())) == 1, "one step and one offset: the phases are equal, and off the host's"
        p.call(audio(0, 256), served="split16", what="a whole pass behind the key call: per-channel LO")
        p.call(audio(1, 64), served="generic", what="one block behind it")
        p.reset()
        p.call(audio(2, 256), device=True, served="split16", what="behind reset: the periodic LO")
        p.key_call(random_keys(nch, 64, 0xD002, run=9), np.zeros((nch, 64), dt), q15, what="a key call again")
        p.set_mode(rc.MODE_CWR, fz.SPLIT16)
        p.key_call(np.ones((nch, 64), np.uint8), None, q15, device=True, what="held, CWR")
        p.call(audio(3, 512), served="split16", what="two whole passes behind it")
    finally:
        p.close()


# ---- (e) a key call shorter than the interpolator history ----------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
def test_key_calls_shorter_than_the_interpolator_history(arith):
    nch, block = 3, 8
    spec = rc.TxSpec(nch, block=block, interp=2, ni_taps=80, nh_taps=15, mode=rc.MODE_USB, arith=arith,
                     nco_steps=np.array([0x3A5F1C27, 0xC0000001, 0x7FFFFF01], np.uint32))
    assert spec.ni_taps // spec.interp - 1 == 39
    p = fr.EntryPair(spec, kernel=fz.GENERIC)
    try:
        p.set_cw(shape=taps(5), amplitude=0.9, offset_step=0x01234567, side_level=0.5, side_step=0x0B4E81B5)
        p.call(rc.synth_audio(0, nch, 0, 5 * block), what="USB audio fills both rails")
        q = p.g.state()["interp_state"][:, 1]
        assert q.shape == (nch, 39) and q.any(axis=1).all()
        p.set_mode(rc.MODE_CW, fz.GENERIC)
        at = 0
        for nblk in (1, 2, 5):
            n = nblk * block
            p.key_call(random_keys(nch, 8 * block, 0xE000, run=5)[:, at:at + n], np.zeros((nch, n), f32), what="key call of %d block(s)" % nblk)
            at += n
            q = p.g.state()["interp_state"][:, 1]
            keep = max(39 - at, 0)
            assert not q[:, keep:].any() and (keep == 0 or q[:, :keep].any(axis=1).all()), "the Q rail moved down by the call, +0.0f behind"
        p.call(rc.synth_audio(0, nch, 40, 2 * block), what="an audio call behind them")
    finally:
        p.close()


# ---- (f) k_tx_cw between 48 and 64 KB ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", [ARITH_CMSIS, ARITH_FMA])
def test_key_call_layout_between_48_and_64_kb(arith):
    nch, ns = 2, 6000
    assert 48 * 1024 < ez.cw_lds_bytes(64, 2, 16, ns) == 50672 <= 64 * 1024
    spec = rc.TxSpec(nch, block=64, interp=2, ni_taps=16, nh_taps=0, mode=rc.MODE_CW, arith=arith, alc=False,
                     nco_steps=np.array([0x3A5F1C27, 0xC0000001], np.uint32))
    p = fr.EntryPair(spec, kernel=fz.GENERIC)
    try:
        p.set_cw(shape=taps(ns), amplitude=0.9, offset_step=0x00DA740E, side_level=0.5, side_step=0x0B4E81B5, side_mix=1)
        side = np.random.default_rng(0xF0).uniform(-0.5, 0.5, (nch, 128)).astype(f32)
        p.key_call(random_keys(nch, 128, 0xF001, run=40), side, device=True, what="random keys")
        p.key_call(np.ones((nch, 128), np.uint8), side, what="held")
        assert p.g.cw_state()["key_state"].shape == (nch, ns - 1)
    finally:
        p.close()
