"""CPU: the numpy restatement of the audio input stage of the TX chain (tests/txin_oracle.py) against the fixture made from the reference's
CMSIS-DSP functions (tests/golden/txin.npz, tests/golden/make_txin_golden.py) bit for bit; cutting a stream into calls of different lengths
gives the same bits and state; and the decimator keeps a tone above the new Nyquist out by what its taps' own frequency response says."""
import os

import numpy as np
import pytest

import rxcommon as rc
import txin_oracle as tio

f32 = np.float32
NAMES = ["left", "mix", "mono8", "right", "vox"]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(rc.GOLDEN_DIR, "txin.npz")) as z:
        return {k: z[k] for k in z.files}


def fixture_params(gold, name):
    """-> (block, dict of set_in arguments) of a fixture stream; the vox stream alone has hang > 0 and is the one with the VOX on"""
    M, pick, block, hang, _ = (int(v) for v in gold[name + "/ipar"])
    gain, attack, decay, open_level, close_level, level_init = (f32(v) for v in gold[name + "/par"])
    vox = dict(gate=0, hang=hang, attack=attack, decay=decay, open_level=open_level, close_level=close_level, level_init=level_init)
    return block, dict(M=M, coeffs=gold[name + "/coeffs"], pick=pick, gain=gain, vox=vox)


def fixture_stage(gold, name, channels=1, **over):
    block, kw = fixture_params(gold, name)
    kw.update(over)
    return tio.TxInStage(channels, block, **kw)


def test_fixture_names(gold):
    assert sorted(gold["names"]) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_fixture_bit_for_bit(gold, name):
    frames = gold[name + "/frames"][None, :]
    block = int(gold[name + "/ipar"][2])
    # the steps one by one
    x = tio.q15_to_float(frames) if frames.dtype == np.int16 else frames
    assert same_bits(x[0], gold[name + "/x"])
    st = fixture_stage(gold, name)
    with np.errstate(all="ignore"):
        g = tio.pick_frames(x, st.pick) * st.gain
    assert same_bits(g[0], gold[name + "/g"])
    # the stage, one DSP block per call as the harness ran it, then in one call
    for step in (block, None):
        for rounding, tag in ((False, "trunc"), (True, "round")):
            st = fixture_stage(gold, name)
            n = gold[name + "/a"].size
            step_ = step or n
            a, q, tr = [], [], {k: [] for k in ("level", "open", "hold", "opens", "open_blocks")}
            for at in range(0, n, step_):
                r = st.process(frames[:, st.words(at):st.words(at + step_)], True, rounding)
                a.append(r["a"])
                q.append(r["audio"])
                tr["level"].append(st.meter.trace["level"][0])
                tr["open"].append(st.meter.trace["open"][0].astype(np.uint32))
                if step:
                    s = st.state()
                    for k in ("hold", "opens", "open_blocks"):
                        tr[k].append(s[k])
            assert same_bits(np.concatenate(a, axis=1)[0], gold[name + "/a"]), (name, step)
            assert same_bits(np.concatenate(q, axis=1)[0], gold[name + "/q15_" + tag]), (name, step, tag)
            assert same_bits(np.concatenate(tr["level"]), gold[name + "/level"])
            assert same_bits(np.concatenate(tr["open"]), gold[name + "/open"])
            if step:
                for k in ("hold", "opens", "open_blocks"):
                    assert same_bits(np.concatenate(tr[k]), gold[name + "/" + k]), k
            else:
                s = st.state()
                for k in ("hold", "opens", "open_blocks", "level", "open"):
                    assert s[k][0] == gold[name + "/" + k][-1], k
    pw = tio.mo.power(gold[name + "/a"].reshape(-1, block))
    assert same_bits(pw, gold[name + "/pw"])


def test_fixture_holds_what_it_is_for(gold):
    assert (gold["mix/q15_trunc"] == 32767).any() and (gold["mix/q15_trunc"] == -32768).any()
    assert np.signbit(gold["right/a"][0]) and gold["right/a"][0] == 0 and 0 < gold["right/a"][2] < np.finfo(f32).tiny
    op = gold["vox/open"]
    assert ((op[1:] == 1) & (op[:-1] == 0)).sum() + op[0] >= 2 and ((op[1:] == 0) & (op[:-1] == 1)).sum() >= 2
    assert gold["vox/opens"][-1] >= 2


@pytest.mark.parametrize("M,nt,pick,block", [(4, 64, tio.LEFT, 12), (2, 97, tio.MIX, 4), (8, 256, tio.MONO, 4), (1, 0, tio.RIGHT, 12),
                                             (1, 63, tio.MONO, 4)])
def test_cutting_a_stream_gives_the_same_bits_and_state(M, nt, pick, block):
    rng = np.random.default_rng(0x7C17 + nt)
    C_, N = 3, 20 * block
    fw = 1 if pick == tio.MONO else 2
    frames = rng.uniform(-1, 1, (C_, N * M * fw)).astype(f32)
    frames[:, 5 * block * M * fw:13 * block * M * fw] *= f32(1e-3)
    coeffs = (rng.uniform(-1, 1, nt) / max(nt, 1) * 4).astype(f32)
    vox = dict(gate=1, hang=1, attack=0.75, decay=0.875, open_level=2e-3, close_level=1e-3, level_init=0.0)
    whole = tio.TxInStage(C_, block, M, coeffs, pick, 1.5, vox)
    want = whole.process(frames, False)
    assert (want["bits"] == 0).any() and (want["bits"] == 1).any()
    for cuts in ([1] * 20, [3, 1, 7, 2, 7], [19, 1]):
        st = tio.TxInStage(C_, block, M, coeffs, pick, 1.5, vox)
        got, at = [], 0
        for n in cuts:
            got.append(st.process(frames[:, st.words(at * block):st.words((at + n) * block)], False)["audio"])
            at += n
        assert same_bits(np.concatenate(got, axis=1), want["audio"]), cuts
        sa, sb = st.state(), whole.state()
        for k in sb:
            assert same_bits(sa[k], sb[k]), (cuts, k)


def test_a_tone_above_the_new_nyquist_is_attenuated_as_the_taps_say():
    import selenite_rx as sr
    M, nt, N = 4, 64, 2048
    taps = sr.design_lowpass(nt, 0.4 / M)
    f = 0.31                                                          # cycles per input sample: above 0.5 / M = 0.125, the new Nyquist
    n_in = N * M
    x = (0.5 * np.sin(2 * np.pi * f * np.arange(n_in))).astype(f32)[None, :]
    st = tio.TxInStage(1, 64, M, taps, tio.MONO, 1.0, None)
    a = st.process(x, False)["a"][0][nt:].astype(np.float64)          # behind the filter's transient
    h = abs(np.sum(taps.astype(np.float64) * np.exp(-2j * np.pi * f * np.arange(nt))))       # |H(f)| in double from the taps
    want_db = 20 * np.log10(h)
    got_db = 10 * np.log10(np.mean(a * a) / 0.125)                    # against the tone's own mean square 0.5^2 / 2
    print("stop band at f = %.2f: |H| = %.2f dB, measured %.2f dB" % (f, want_db, got_db))
    assert want_db < -40.0                                            # the tone does sit in the stop band
    assert got_db <= want_db + 1.0                                    # the bar: the taps' figure minus 1 dB of attenuation (f32 rounding, finite record)
    # and a tone in the pass band comes through
    xp = (0.5 * np.sin(2 * np.pi * 0.02 * np.arange(n_in))).astype(f32)[None, :]
    ap = tio.TxInStage(1, 64, M, taps, tio.MONO, 1.0, None).process(xp, False)["a"][0][nt:].astype(np.float64)
    assert abs(10 * np.log10(np.mean(ap * ap) / 0.125)) < 0.5
