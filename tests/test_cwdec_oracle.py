"""CPU: the numpy restatement of the Morse decoder (tests/cwdec_oracle.py) against tests/golden/cwdec.npz -- the reference's own
arm_power_f32 and a second, independent statement of the scalar law in C (tests/golden/make_cwdec_golden.py) -- on bits, every row, whatever
the cut of the stream into calls; the named cases of the law on hand-made mean-square sequences; and that the law decodes keyed, noisy
audio at 12 - 40 WPM and emits nothing on noise."""
import os

import numpy as np
import pytest

import cwdec_oracle as co
import rxcommon as rc
import selenite_rx as sr

F32 = np.float32
TEXT = "CQ CQ DE K1ABC K1ABC PSE K = 5NN TU 73"
TABLE = sr.morse_table()            # the library's built-in table (selenite_rx_design_morse): what the named cases and the decode run on


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(rc.GOLDEN_DIR, "cwdec.npz")) as z:
        return {k: z[k] for k in z.files}


def gold_par(g):
    return {k[4:]: (float(g[k]) if g[k].dtype == np.float32 else int(g[k])) for k in g if k.startswith("par/")}


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------
def test_power_and_mean_square_equal_the_reference(gold):
    n = int(gold["n"])
    x = gold["x"].reshape(3, -1, n)
    import meter_oracle as mo
    assert mo.power(x).tobytes() == gold["pw"].tobytes() and mo.mean_square(x).tobytes() == gold["ms"].tobytes()
    assert np.isnan(gold["ms"][2, 100]) and np.isinf(gold["ms"][2, 300])


@pytest.mark.parametrize("cut", ["fixture", 1, 7, 64, 420])
def test_restatement_equals_the_fixture_on_bits_whatever_the_cut(gold, cut):
    n, lens = int(gold["n"]), [int(v) for v in gold["lens"]]
    d = co.CwDec(3, n, table=gold["table"], **gold_par(gold))
    ends = {int(e): i for i, e in enumerate(np.cumsum(lens))}
    total = sum(lens)
    cuts = lens if cut == "fixture" else [min(cut, total - a) for a in range(0, total, cut)]
    at, seen = 0, 0
    for nb in cuts:
        d.process(gold["x"][:, at * n:(at + nb) * n])
        at += nb
        if at in ends:
            st = d.state()
            for k in st:
                same(st[k], gold["call/" + k][ends[at]], "%s behind block %d" % (k, at))
            seen += 1
    assert at == total and seen >= 1 and (cut not in ("fixture", 1) or seen == len(lens))
    assert [d.cw_text(c).rstrip() for c in range(2)] == [str(s) for s in gold["sent"]]
    assert gold["call/key"].any() and gold["call/flip"].any() and len({int(u) for u in gold["call/unit"][-1]}) > 1


# ---- named cases on hand-made sequences: blocks of constant samples -----------------------------------------------------------------------
HI, LO = 1.0, 0.01            # sample values: mean squares 1 and 1e-4


def feed(d, pattern):
    """pattern: a string of H / L (one block each of constant samples) or a list of sample values"""
    vals = [HI if ch == "H" else LO for ch in pattern] if isinstance(pattern, str) else list(pattern)
    x = np.repeat(np.array(vals, np.float32), d.n)[None, :]
    d.process(x)


def dec(**par):
    """instant followers and fixed timing: thr halfway, unit 4 blocks, so H / L blocks read as the key itself"""
    p = dict(peak_attack=1.0, peak_decay=0.001, floor_attack=1.0, floor_decay=0.001, on_frac=0.5, off_frac=0.5, snr=2.0, min_power=1e-8,
             debounce=2, adapt=0, track=2, unit_min=256, unit_init=4 * 256, unit_max=64 * 256, ring=16)
    p.update(par)
    d = co.CwDec(1, 8, **dict(dict(table=TABLE), **p))
    feed(d, "LL")             # primes the followers at the floor
    return d


DIT, DAH, GAP, CHAR = "HHHH", "H" * 12, "LLLL", "L" * 12


def test_a_glitch_shorter_than_debounce_is_absorbed_into_the_running_run():
    d = dec(debounce=2)
    feed(d, "HHHHH")
    assert d.key[0] == 1 and d.run[0] == 5
    feed(d, "L")
    assert d.key[0] == 1 and d.flip[0] == 1 and d.run[0] == 5
    feed(d, "H")
    assert d.key[0] == 1 and d.flip[0] == 0 and d.run[0] == 7              # run + flip + 1
    feed(d, "LL")
    assert d.key[0] == 0 and d.run[0] == 2 and d.code[0] == 0b10             # a mark of 7 < 8 blocks: a dit


def test_debounce_1_follows_every_block():
    d = dec(debounce=1)
    feed(d, "H")
    assert d.key[0] == 1 and d.run[0] == 1 and d.flip[0] == 0
    feed(d, "L")
    assert d.key[0] == 0 and d.run[0] == 1 and d.code[0] == 0b10
    feed(d, "H" * 9 + "L")
    assert d.code[0] == 0b101 and d.count[0] == 0
    feed(d, "L" * 7)
    assert d.cw_text(0) == "A"


def test_an_8_element_character_gives_table_0_once_and_recovers():
    d = dec(table=sr.morse_table("~"))
    feed(d, (DIT + GAP) * 7)
    assert d.code[0] == 0b10000000 and d.count[0] == 0
    feed(d, DIT + GAP)
    assert d.code[0] == 0
    feed(d, DIT + CHAR)                                                       # a ninth element: still one overflow character
    assert d.cw_text(0) == "~" and d.code[0] == 1
    feed(d, DAH + GAP + DIT + CHAR)
    assert d.cw_text(0) == "~N"


def test_unit_clamps_at_both_ends():
    d = dec(adapt=1, track=0, unit_min=3 * 256, unit_max=6 * 256)          # track 0: unit jumps to the measured length
    feed(d, "HH" + "L" * 40)
    assert d.unit[0] == 3 * 256                                              # a dit of 2 blocks against unit_min 3
    feed(d, "H" * 5 + "L" * 40)
    assert d.unit[0] == 5 * 256                                              # inside the range: taken as it is
    feed(d, "H" * 30 + "L" * 40)
    assert d.unit[0] == 6 * 256                                              # a dah of 30 blocks: 10 per unit, against unit_max 6


def test_adapt_0_keeps_unit():
    d = dec(adapt=0)
    feed(d, "HH" + "L" * 30 + "H" * 40 + "L" * 30)
    assert d.unit[0] == 4 * 256 and d.cw_text(0) == "E T "


def test_run_saturates_without_a_second_word_space():
    d = dec()
    feed(d, DIT + "L" * 30)
    assert d.cw_text(0) == "E " and d.word[0] == 0
    d.process_ms(np.full((1, 66000), LO * LO, np.float32))
    assert d.run[0] == 65535 and d.cw_text(0) == "E " and d.count[0] == 2
    feed(d, DIT + "L" * 30)
    assert d.cw_text(0) == "E E "


def test_the_ring_wraps():
    d = dec(ring=16)
    want = ""
    for i in range(12):
        feed(d, (DAH if i % 2 else DIT) + "L" * 24)
        want += "T " if i % 2 else "E "
    assert d.count[0] == 24 and d.cw_text(0) == want[-16:]
    assert d.text[0].tobytes().decode() == want[16:] + want[8:16]          # character i lies at i % ring


def test_nan_and_inf_blocks_leave_the_followers_and_read_as_key_up():
    d = dec()
    feed(d, "HHH")
    peak, floor = d.peak.copy(), d.floor.copy()
    assert d.key[0] == 1
    feed(d, [np.nan])
    assert d.peak.tobytes() == peak.tobytes() and d.floor.tobytes() == floor.tobytes() and d.flip[0] == 1 and d.key[0] == 1
    feed(d, [np.inf])                                                        # the second block against the key: it goes up
    assert d.peak.tobytes() == peak.tobytes() and d.floor.tobytes() == floor.tobytes() and d.key[0] == 0 and d.run[0] == 2
    assert d.code[0] == 0b10


# ---- it decodes ------------------------------------------------------------------------------------------------------------------------------
N, FS = 64, 12000


def keyed_audio(text, wpm, seed):
    """a 600-cycle-per-12000-sample tone of amplitude 0.1 keyed by sr.morse_key, edges softened by a 61-sample
    Hann window, uniform noise +-0.03; 40 blocks of lead-in noise, and behind the text 3.5 units of it: the last character leaves, its blank
    does not"""
    unit = int(round(1.2 / wpm * FS))
    k = sr.morse_key(text, unit)
    total = -(-(40 * N + len(k) + (7 * unit) // 2) // N) * N
    down = np.zeros(total)
    down[40 * N:40 * N + len(k)] = k
    w = np.hanning(61)
    env = np.convolve(down, w / w.sum(), mode="same")
    x = 0.1 * env * np.sin(2 * np.pi * 600 * np.arange(total) / FS) + np.random.default_rng(seed).uniform(-0.03, 0.03, total)
    return x.astype(np.float32)[None, :]


@pytest.mark.parametrize("wpm,unit_init,settles", [(12, 10, (18.2, 19.4)), (20, 10, (10.7, 11.8)), (30, 10, (7.2, 8.1)), (40, 6, (5.2, 6.1))])
def test_it_decodes(wpm, unit_init, settles):
    """`settles`: the dit length in blocks, 1.2 / wpm * 12000 / 64 = 18.75, 11.25, 7.5, 5.63, give or take half a block of edge placement"""
    for seed in range(5):
        d = co.CwDec(1, N, table=TABLE, **dict(sr.CWDEC_DEFAULTS, unit_init=unit_init * 256))
        d.process(keyed_audio(TEXT, wpm, seed))
        print("%d WPM, seed %d: %r, unit %.2f blocks" % (wpm, seed, d.cw_text(0), d.unit[0] / 256.0))
        assert d.cw_text(0) == TEXT, (wpm, seed)
        assert settles[0] <= d.unit[0] / 256.0 <= settles[1]


def test_noise_alone_emits_nothing():
    rng = np.random.default_rng(1000)
    d = co.CwDec(8, N, table=TABLE, **sr.CWDEC_DEFAULTS)
    d.process(rng.uniform(-0.1, 0.1, (8, 3000 * N)).astype(np.float32))
    assert not d.count.any() and not d.text.any() and (d.primed == 1).all()
