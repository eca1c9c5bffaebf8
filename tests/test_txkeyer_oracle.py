"""CPU: the keyer's law (include/selenite_tx_keyer.h).  The oracle's two statements of it (tests/txkeyer_oracle.py: sample by sample, and
over run lengths) against each other, against the fixture (tests/golden/txkeyer.npz), against sr.morse_key for text alone, and the named
cases against what a keyer is expected to do, in plain run lengths of the key."""
import os

import numpy as np
import pytest

import rxcommon as rc
import selenite_rx as sr
import txkeyer_cases as kc
import txkeyer_oracle as ko
from txkeyer_cases import runs

MODES = [ko.STRAIGHT, ko.IAMBIC_A, ko.IAMBIC_B]


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(rc.GOLDEN_DIR, "txkeyer.npz")) as z:
        return {k: z[k] for k in z.files}


def test_the_fixture_holds_every_named_case(gold):
    assert sorted(gold["names"].tolist()) == sorted(kc.CASES)


@pytest.mark.parametrize("name", sorted(kc.CASES))
@pytest.mark.parametrize("events", [False, True])
def test_both_statements_give_the_fixture(gold, name, events):
    be = kc.OracleBackend(events)
    key = kc.play(kc.CASES[name], be)
    assert np.array_equal(key, gold[name + "/key"])
    st = be.state()
    assert np.array_equal(np.stack([st[w] for w in ko.WORDS]), gold[name + "/words"]) and np.array_equal(st["text"], gold[name + "/text"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("unit", [1, 2, 7, 64])
def test_both_statements_agree_on_random_paddles_however_the_stream_is_cut(mode, unit):
    rng = np.random.default_rng(100 * mode + unit)
    texts = ["", "E", "AB C", "x  Y", " K~k "]
    for trial in range(8):
        n = int(rng.integers(1, 40 * unit + 5))
        a, b = ko.Keyer(mode, unit, 16), ko.Keyer(mode, unit, 16)
        assert a.send(texts[trial % 5]) and b.send(texts[trial % 5])
        pad = ko.random_paddles(rng, 1, n, unit, max_units=5, p_idle=0.95 if trial % 3 == 0 else 0.5)[0]
        cuts = sorted(set(rng.integers(0, n + 1, size=3).tolist() + [0, n]))
        ka = a.run(pad)
        kb = np.concatenate([b.run_events(pad[i:j]) for i, j in zip(cuts[:-1], cuts[1:])])
        assert np.array_equal(ka, kb), (trial, np.flatnonzero(ka != kb)[:4])
        assert a.words() == b.words() and np.array_equal(a.text, b.text), trial


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("unit", [1, 2, 7])
def test_text_alone_is_morse_key(mode, unit):
    for text in ("CQ DE K1ABC", "5nn tu 73", "PSE K = QRZ?", "W1AW/3 @ 7.030", "E"):
        want = sr.morse_key(text, unit)
        for events in (False, True):
            k = ko.Keyer(mode, unit, 64)
            assert k.send(text)
            f = k.run_events if events else k.run
            got = np.concatenate([f(None, 17), f(None, len(want) + 9 * unit)])
            assert np.array_equal(got[:len(want)], want) and not got[len(want):].any(), (text, events)
            assert k.phase == ko.IDLE and k.pending() == 0 and k.skipped == 0


# ---- the named cases ----
def u_of(name, c):
    return kc.CASES[name]["units"][c]


@pytest.mark.parametrize("tag", ["A", "B"])
def test_1_a_dit_tapped_during_a_dah_is_sent_after_it(gold, tag):
    for c in range(kc.CHANNELS):
        u = u_of("opposite_" + tag, c)
        n = gold["opposite_%s/key" % tag].shape[1]
        assert runs(gold["opposite_%s/key" % tag][c]) == [(0, u // 2), (1, 3 * u), (0, u), (1, u), (0, n - u // 2 - 5 * u)]


@pytest.mark.parametrize("tag", ["A", "B"])
def test_2_a_dah_tapped_in_its_own_gap_is_not_remembered(gold, tag):
    for c in range(kc.CHANNELS):
        u = u_of("same_tap_" + tag, c)
        n = gold["same_tap_%s/key" % tag].shape[1]
        assert runs(gold["same_tap_%s/key" % tag][c]) == [(0, u // 2), (1, 3 * u), (0, n - u // 2 - 3 * u)]


def test_3_a_squeeze_let_go_inside_a_dah_mode_a_stops_mode_b_adds_one_dit(gold):
    for c in range(kc.CHANNELS):
        u = u_of("squeeze_release_A", c)
        n = gold["squeeze_release_A/key"].shape[1]
        head = [(0, u // 2), (1, u), (0, u), (1, 3 * u)]
        assert runs(gold["squeeze_release_A/key"][c]) == head + [(0, n - u // 2 - 5 * u)]
        assert runs(gold["squeeze_release_B/key"][c]) == head + [(0, u), (1, u), (0, n - u // 2 - 7 * u)]


@pytest.mark.parametrize("tag", ["A", "B"])
def test_4_a_held_squeeze_alternates_and_starts_with_a_dit(gold, tag):
    for c in range(kc.CHANNELS):
        u = u_of("squeeze_held_" + tag, c)
        r = runs(gold["squeeze_held_%s/key" % tag][c])[:-1]      # (the last run is cut by the end)
        assert r[0] == (0, u // 2) and len(r) >= 8
        marks, gaps = [x[1] for x in r[1::2]], [x[1] for x in r[2::2]]
        assert marks == [u if i % 2 == 0 else 3 * u for i in range(len(marks))] and set(gaps) == {u}


@pytest.mark.parametrize("tag", ["A", "B"])
def test_5_a_paddle_drops_the_queued_text_and_the_running_mark_keeps_its_length(gold, tag):
    name = "takeover_" + tag
    for c in range(kc.CHANNELS):
        u = u_of(name, c)
        assert runs(gold[name + "/key"][c])[:3] == [(1, 3 * u), (0, u), (1, u)] and len(runs(gold[name + "/key"][c])) == 4
    words = dict(zip(ko.WORDS, gold[name + "/words"]))
    assert (words["tail"] == words["head"]).all() and (words["head"] == 2).all() and (words["code"] == 1).all() and (words["tgap"] == 0).all()


def test_6_the_straight_key_bit_is_ored_over_everything(gold):
    pad = kc.CASES["key_bit_A"]["steps"][0][1]
    assert np.array_equal(gold["key_bit_A/key"], (pad >> 2) & 1)
    pad = kc.CASES["paddles_are_the_key_S"]["steps"][0][1]
    assert np.array_equal(gold["paddles_are_the_key_S/key"], (pad & 7) != 0)
    for c in range(kc.CHANNELS):                 # STRAIGHT sends text; the key bit drops what is left of it and shows as it is
        u = u_of("key_bit_over_text_S", c)
        n = gold["key_bit_over_text_S/key"].shape[1]
        assert runs(gold["key_bit_over_text_S/key"][c]) == [(1, u), (0, u), (1, u), (0, n - 3 * u)]
    words = dict(zip(ko.WORDS, gold["key_bit_over_text_S/words"]))
    assert (words["tail"] == 3).all() and (words["head"] == 3).all()


@pytest.mark.parametrize("name", ["timing_A", "timing_B", "squeeze_held_A", "ring_wrap", "skipped"])
def test_7_every_mark_is_one_or_three_units_and_every_gap_at_least_one(gold, name):
    for c in range(kc.CHANNELS):
        u = u_of(name, c)
        r = runs(gold[name + "/key"][c])
        if r[0][0] == 0:
            r = r[1:]
        r = r[:-1]
        assert len(r) > 4
        assert {x[1] for x in r if x[0] == 1} <= {u, 3 * u}
        gaps = {x[1] for x in r if x[0] == 0}
        assert min(gaps) == u and (name.startswith("timing") or gaps <= {u, 3 * u, 7 * u})


@pytest.mark.parametrize("name", ["timing_A", "timing_B"])
def test_7_a_gap_between_elements_is_exactly_one_unit(gold, name):
    """a gap is between two elements, not idle time, when a paddle is down on the sample where one unit of gap has run out: the keyer
    decides there, so the next mark starts there.  Every longer gap has both paddles up on that sample."""
    pad = kc.CASES[name]["steps"][0][1]
    checked = 0
    for c in range(kc.CHANNELS):
        u = u_of(name, c)
        key = gold[name + "/key"][c]
        at = 0
        for value, length in runs(key):
            if value == 0 and at > 0 and at + u < len(key):        # a gap behind a mark whose first unit lies inside the row
                held = (pad[c, at + u] & 3) != 0
                assert length >= u, (c, at, length)
                if held:
                    assert length == u, (c, at, length)
                    checked += 1
                elif length > u:
                    assert (pad[c, at + u] & 3) == 0
            at += length
    assert checked >= 10


def test_8_twenty_characters_through_a_ring_of_four(gold):
    for c in range(kc.CHANNELS):
        want = sr.morse_key(kc.WRAP_TEXT, u_of("ring_wrap", c))
        got = gold["ring_wrap/key"][c]
        assert np.array_equal(got[:len(want)], want) and not got[len(want):].any()
    words = dict(zip(ko.WORDS, gold["ring_wrap/words"]))
    assert (words["tail"] == 20).all() and (words["head"] == 20).all()
    k = ko.Keyer(ko.IAMBIC_A, 2, 4)
    assert k.send("ABCD") and not k.send("E") and k.pending() == 4, "a full ring takes nothing"


def test_9_bytes_without_a_pattern_are_skipped_and_counted(gold):
    for c in range(kc.CHANNELS):
        want = sr.morse_key("ABC", u_of("skipped", c))
        got = gold["skipped/key"][c]
        assert np.array_equal(got[:len(want)], want) and not got[len(want):].any()
    assert (dict(zip(ko.WORDS, gold["skipped/words"]))["skipped"] == 2).all()


def test_10_a_unit_changed_in_a_gap_holds_from_the_next_element(gold):
    for c in range(kc.CHANNELS):
        r = runs(gold["speed/key"][c])
        assert r[:2] == [(1, 16), (0, 16)] and all(x[1] == 5 for x in r[2:-1]) and len(r) > 6
