"""CPU: the numpy restatement of the FSK teleprinter decoder (tests/fskdec_oracle.py) against tests/golden/fskdec.npz -- the reference's
arm_biquad_cascade_df1_f32 and arm_power_f32 and a second, independent statement of the scalar law in C (tests/golden/make_fskdec_golden.py)
-- on bits, every row, whatever the cut of the stream into calls; against a third statement of the bit clock, frame by frame, on random
level sequences; and the properties the law promises: NaN / Inf, `reverse`, a `bit` per channel through the state, texts read back whole."""
import os

import numpy as np
import pytest

import fskdec_oracle as fo
import rxcommon as rc

FS, F_MARK, F_SPACE = 12000.0, 2125.0, 2295.0


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(rc.GOLDEN_DIR, "fskdec.npz")) as z:
        return {k: z[k] for k in z.files}


def gold_par(g):
    return {k[4:]: (float(g[k]) if g[k].dtype == np.float32 else int(g[k])) for k in g if k.startswith("par/")}


def gold_dec(g):
    d = fo.FskDec(g["x"].shape[0], g["mark"], g["space"], table=g["table"], **gold_par(g))
    d.set_state({"bit": g["bit"]})
    return d


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), "%s: %d values differ" % (what, int((a.view(np.uint8) != b.view(np.uint8)).sum()))


def test_the_fixture_is_what_its_script_says(gold):
    g = gold
    assert g["x"].shape == (4, 7200) and int(g["lens"].sum()) * int(g["par/tick"]) == 7200
    assert np.isnan(g["x"][2]).sum() == 1 and np.isinf(g["x"][3]).sum() == 1
    same(g["table"], fo.table(), "table")
    m, s = fo.design(0.15, 0.20, 0.02)
    same(g["mark"], m, "mark"); same(g["space"], s, "space")
    assert set(k[5:] for k in g if k.startswith("call/")) == set(fo.ROWS)
    assert g["call/count"][-1].tolist() == [7, 11, 4, 0] and not g["call/ferr"].any()


@pytest.mark.parametrize("cut", ["fixture", "whole", 1, 7, 64], ids=str)
def test_restatement_equals_the_fixture_on_bits_whatever_the_cut(gold, cut):
    g = gold
    T, total = int(g["par/tick"]), int(g["lens"].sum())
    d = gold_dec(g)
    lens = [int(v) for v in g["lens"]] if cut == "fixture" else [total] if cut == "whole" else [cut] * (total // cut) + ([total % cut] if total % cut else [])
    ends = np.cumsum([int(v) for v in g["lens"]]).tolist()
    at = 0
    for n in lens:
        pm, ps, pw = d.process(g["x"][:, at * T:(at + n) * T])
        same(pm, g["pm"][:, at:at + n], "pm at %d" % at); same(ps, g["ps"][:, at:at + n], "ps at %d" % at); same(pw, g["pw"][:, at:at + n], "pw at %d" % at)
        at += n
        same(d.filt, g["trace"][:, at - 1], "filt behind tick %d" % (at - 1))
        if at in ends:                                   # a call of the fixture ends here: every row
            i = ends.index(at)
            for k, v in d.state().items():
                same(v, g["call/" + k][i], "%s behind call %d" % (k, i))
    assert at == total
    assert [d.fsk_text(c) for c in range(2)] == [str(s) for s in g["sent"][:2]] and d.fsk_text(2).startswith("CQ ") and d.fsk_text(3) == ""


# ---- the bit clock against a third statement, frame by frame ------------------------------------------------------------------------------------
def frames(levels, bit, tab, usos, ring_len):
    """the law by frames: a start edge at tick i (1 -> 0 while idle), then the level at the first tick m_j > i with
    (m_j - i) * 256 >= j * bit + bit // 2 for j = 0 (start) .. 6 (stop); idle again from the tick behind the decision"""
    ring, count, ferr, figs = np.zeros(ring_len, np.uint8), 0, 0, 0
    k_end, i, n = 0, 1, len(levels)                       # levels[0] is the level before the first tick
    while i < n:
        if not (levels[i - 1] == 1 and levels[i] == 0):
            i += 1
            continue
        at = [i + -(-(j * bit + bit // 2) // 256) for j in range(7)]
        if at[0] >= n:
            k_end = 1
            break
        if levels[at[0]] == 1:                           # false start
            i = at[0] + 1
            continue
        if at[6] >= n:
            k_end = 2 + sum(1 for m in at[1:6] if m < n)
            break
        if levels[at[6]] == 0:
            ferr += 1
        else:
            c = sum(int(levels[m]) << j for j, m in enumerate(at[1:6]))
            if c == 31:
                figs = 0
            elif c == 27:
                figs = 1
            else:
                if tab[figs * 32 + c]:
                    ring[count % ring_len] = tab[figs * 32 + c]
                    count += 1
                if usos and c == 4:
                    figs = 0
        i = at[6] + 1
    return ring, count, ferr, figs, k_end


def random_levels(rng, bit_ticks, n_frames):
    """idle, frames of random codes (LTRS, FIGS, blank and the codes without a character among them) with jittered edges, false starts,
    frames whose stop bit is a space, and stretches of coin flips"""
    out = [np.ones(3, np.uint8)]
    for _ in range(n_frames):
        kind = rng.choice(["frame", "frame", "frame", "false", "ferr", "noise", "idle"])
        bt = lambda: max(1, int(round(bit_ticks + rng.uniform(-0.4, 0.4))))     # noqa: E731
        if kind == "idle":
            out.append(np.ones(rng.integers(1, 3 * int(bit_ticks)), np.uint8))
        elif kind == "noise":
            out.append(rng.integers(0, 2, rng.integers(1, 40)).astype(np.uint8))
        elif kind == "false":
            out.append(np.zeros(rng.integers(1, max(2, int(bit_ticks // 2))), np.uint8))
            out.append(np.ones(rng.integers(1, 2 * int(bit_ticks)), np.uint8))
        else:
            c = int(rng.choice([27, 31, 4, 0, rng.integers(0, 32), rng.integers(0, 32)]))
            out.append(np.zeros(bt(), np.uint8))
            for b in range(5):
                out.append(np.full(bt(), (c >> b) & 1, np.uint8))
            out.append(np.full(int(round(1.5 * bit_ticks)), 0 if kind == "ferr" else 1, np.uint8))
            if kind == "ferr":
                out.append(np.ones(rng.integers(1, int(bit_ticks)), np.uint8))
    return np.concatenate(out)


@pytest.mark.parametrize("usos", [0, 1])
@pytest.mark.parametrize("bit", [8 * 256, 2347, 4224, 11 * 256 + 128, 40 * 256 + 1])
def test_the_bit_clock_agrees_with_the_law_by_frames_on_random_levels(bit, usos):
    rng = np.random.default_rng(bit + usos)
    tab = fo.table()
    tab[[5, 32 + 9]] = 0                                 # two more codes that print nothing
    lv = random_levels(rng, bit / 256.0, 400)
    # alpha = 1: the followers ARE the tick's powers, so (pm, ps) = (1, 0) reads as mark and (0, 1) as space
    d = fo.FskDec(1, np.zeros(5), np.zeros(5), table=tab, tick=4, bit_q8=bit, usos=usos, ring=16, alpha=1.0, hyst=0.1, frac=0.0, min_power=0.5)
    pm = lv[None, 1:].astype(np.float32)
    d.process_powers(pm, 1.0 - pm, np.ones_like(pm))
    ring, count, ferr, figs, k_end = frames(lv, bit, tab, usos, 16)
    assert count > 16 and ferr > 0                       # the ring wrapped; framing errors happened
    assert (int(d.count[0]), int(d.ferr[0]), int(d.figs[0]), int(d.k[0])) == (count, ferr, figs, k_end)
    same(d.text[0], ring, "text")
    assert int(d.lvl[0]) == lv[-1]


def test_a_quiet_band_reads_as_mark_whatever_the_tones_say():
    """not present (tot <= frac * ew, or tot <= min_power): lvl = 1 even where the space filter leads"""
    d = fo.FskDec(1, np.zeros(5), np.zeros(5), tick=4, bit_q8=8 * 256, alpha=1.0, hyst=0.1, frac=0.5, min_power=0.5)
    for pm, ps, pw, want in ((0.0, 1.0, 1.0, 0), (0.0, 0.4, 0.1, 1), (0.0, 1.0, 3.0, 1), (0.0, 1.0, 1.9, 0), (0.52, 0.48, 1.0, 0), (0.6, 0.4, 1.0, 1)):
        d.process_powers(*(np.full((1, 1), v, np.float32) for v in (pm, ps, pw)))
        assert int(d.lvl[0]) == want, (pm, ps, pw)


# ---- NaN / Inf ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_sample_poisons_the_filters_and_freezes_the_followers(bad):
    mark, space = fo.design(F_MARK / FS, F_SPACE / FS, 90.0 / FS)
    rng = np.random.default_rng(3)
    x = rng.normal(0.0, 0.1, (2, 16 * 40)).astype(np.float32)
    x[1] += (0.3 * np.sin(2 * np.pi * F_SPACE / FS * np.arange(x.shape[1]))).astype(np.float32)
    d = fo.FskDec(2, mark, space)
    x0 = x.copy()
    x0[0, 5] = bad                                       # channel 0: in its first tick, before anything was followed
    d.process(x0[:, :16 * 20])
    before = d.state()
    assert not np.isfinite(d.filt[0]).any() or np.isnan(d.filt[0, :, 2:]).all()
    assert np.isnan(d.filt[0, :, 2]).all()               # both y1: poisoned for good
    assert before["em"][0] == 0 and before["es"][0] == 0 and before["ew"][0] == 0 and before["lvl"][0] == 1 and before["count"][0] == 0
    x1 = x[:, 16 * 20:].copy()
    x1[1, 7] = bad                                       # channel 1: with its followers up
    d.process(x1)
    after = d.state()
    assert np.isnan(after["filt"][1, :, 2]).all()
    for k in ("em", "es", "ew"):
        assert after[k][0] == 0                          # never present: every tick of channel 0 reads as mark
        same(after[k][1:], before[k][1:], k)             # channel 1: the followers stand where they stood before the bad tick
    assert after["lvl"][0] == 1 and after["k"][0] == 0 and after["count"][0] == 0 and after["ferr"][0] == 0
    # set_state puts a channel back to work
    d.set_state(dict(before, filt=np.zeros_like(before["filt"])))
    d.process(x[:, :16 * 4])
    assert np.isfinite(d.filt).all() and (d.ew != before["ew"]).all()


# ---- decoding -------------------------------------------------------------------------------------------------------------------------------------
TEXTS = ("THE QUICK BROWN FOX 1234567890 DE K1ABC (73) $5.00 #2 OK", "RYRYRY CQ CQ DE W1AW W1AW K", "UR 599 599 NR 001 TU")
SPEEDS = ((45.45, 90.0), (50.0, 90.0), (75.0, 140.0))            # baud, design_fsk bandwidth in Hz


def rtty(text, baud, sigma, seed, f_mark=F_MARK, f_space=F_SPACE, tick=16, amp=0.3):
    a = amp * fo.afsk(fo.encode(text), FS, baud, f_mark, f_space, 1.5, lead=8, tail=4)
    x = a + np.random.default_rng(seed).normal(0.0, sigma, a.size)
    return x[:x.size // tick * tick].astype(np.float32)


def test_encode_sends_the_shifts_a_receiver_needs():
    assert fo.encode("E") == [1] and fo.encode("e 3") == [1, 4, 27, 1]
    assert fo.encode("3 3") == [27, 1, 4, 27, 1] and fo.encode("3 3", usos=False) == [27, 1, 4, 1]
    assert fo.encode("3E") == [27, 1, 31, 1] and fo.encode("\r\n") == [8, 2]
    with pytest.raises(ValueError):
        fo.encode("~")


def test_afsk_is_phase_continuous_and_keys_lsb_first():
    a = fo.afsk([1], 8000.0, 100.0, 1000.0, 2000.0, 1.5, lead=1, tail=0.5)
    assert a.size == int(9 * 80) and np.abs(np.diff(a)).max() <= 2 * np.pi * 2000.0 / 8000.0 + 1e-9
    zc = lambda seg: int((np.diff(np.signbit(seg)) != 0).sum())     # noqa: E731
    per_bit = [zc(a[i * 80:(i + 1) * 80]) for i in range(9)]          # lead, start, 1 0 0 0 0, stop 1.5
    assert [round(z / 10.0) for z in per_bit] == [2, 4, 2, 4, 4, 4, 4, 2, 2]


@pytest.mark.parametrize("tick,speeds", [(16, SPEEDS), (8, SPEEDS[:1])], ids=["T16", "T8"])
def test_it_reads_texts_back_whole_in_noise_each_channel_at_its_own_speed(tick, speeds):
    """the issue's inputs: 12 kHz audio, mark 2125 Hz, space 2295 Hz, amplitude 0.3, sigma 0.1, alpha 0.25, hyst 0.1, frac 0.35, min_power
    1e-6; one decoder per bandwidth, the speeds on different channels through the `bit` row; a channel of noise alone and one of zeros"""
    for baud, bw in speeds:
        mark, space = fo.design(F_MARK / FS, F_SPACE / FS, bw / FS)
        xs = [rtty(t, baud, 0.1, 10 * i + 1, tick=tick) for i, t in enumerate(TEXTS)]
        n = max(x.size for x in xs)
        x = np.zeros((len(xs) + 2, n), np.float32)
        for i, v in enumerate(xs):
            x[i, :v.size] = v
        x[len(xs)] = np.random.default_rng(99).normal(0.0, 0.1, n)
        d = fo.FskDec(len(xs) + 2, mark, space, tick=tick, bit_q8=fo.bit_q8(FS, 60.0, tick))      # (the config's speed fits no channel)
        d.set_state({"bit": np.full(len(xs) + 2, fo.bit_q8(FS, baud, tick), np.uint32)})
        d.process(x)
        print("%g baud, T %d: %r, ferr %s" % (baud, tick, [d.fsk_text(c) for c in range(len(xs))], d.ferr.tolist()))
        for c, t in enumerate(TEXTS):
            assert d.fsk_text(c) == t, (baud, c)
        assert d.count[len(xs)] == 0 and d.count[len(xs) + 1] == 0


def test_three_speeds_side_by_side_through_the_bit_row():
    """one decoder, one coefficient pair (140 Hz wide), channels at 45.45, 50 and 75 baud"""
    mark, space = fo.design(F_MARK / FS, F_SPACE / FS, 140.0 / FS)
    xs = [rtty(TEXTS[i], baud, 0.05, 7 + i) for i, (baud, _) in enumerate(SPEEDS)]
    n = max(x.size for x in xs)
    x = np.zeros((3, n), np.float32)
    for i, v in enumerate(xs):
        x[i, :v.size] = v
    d = fo.FskDec(3, mark, space)
    d.set_state({"bit": np.array([fo.bit_q8(FS, b, 16) for b, _ in SPEEDS], np.uint32)})
    d.process(x)
    assert [d.fsk_text(c) for c in range(3)] == list(TEXTS)
    same(d.bit, np.array([4224, 3840, 2560], np.uint32), "bit")


def test_reverse_reads_swapped_tones_and_equals_swapped_filters():
    mark, space = fo.design(F_MARK / FS, F_SPACE / FS, 90.0 / FS)
    x = rtty(TEXTS[2], 45.45, 0.1, 5, f_mark=F_SPACE, f_space=F_MARK)[None]       # keyed upside down
    up, rev, swp = fo.FskDec(1, mark, space), fo.FskDec(1, mark, space, reverse=1), fo.FskDec(1, space, mark)
    for d in (up, rev, swp):
        d.process(x)
    assert rev.fsk_text(0) == TEXTS[2] and up.fsk_text(0) != TEXTS[2]
    a, b = rev.state(), swp.state()
    same(a.pop("filt"), b.pop("filt")[:, ::-1], "filt")
    for k in a:
        same(a[k], b[k], k)
