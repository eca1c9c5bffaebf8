"""The keyer's named cases (tests/golden/txkeyer.npz): what is sent, pressed and retuned, as steps that any backend can play -- the oracle
(tests/txkeyer_oracle.py: both statements) and the GPU stage (tests/test_gpu_txkeyer.py).  Times are in units of the channel's dit, so a
case means the same thing on every channel whatever its unit.  Every run is a whole number of BLOCK samples."""
import numpy as np

import txkeyer_oracle as ko

BLOCK = 24
CHANNELS = 3
UNITS = (4, 6, 2)                                # even: half units are whole samples
DIT, DAH, KEY = 1, 2, 4
A, B, S = ko.IAMBIC_A, ko.IAMBIC_B, ko.STRAIGHT
WRAP_TEXT = "PARIS PARIS 73 DE K1"               # 20 characters through a ring of 4
SKIP_TEXT = "A~B\x01c"                           # two bytes without a pattern


def blocks(n):
    return -(-int(n) // BLOCK) * BLOCK


def pads(n, presses, units=UNITS):
    """presses: (bit, from, to) in units -> uint8 [CHANNELS][n]"""
    p = np.zeros((CHANNELS, n), np.uint8)
    for c, u in enumerate(units):
        for bit, a, b in presses:
            p[c, int(a * u):min(int(b * u), n)] |= bit
    return p


def case(mode, steps, units=UNITS, ring=16):
    return dict(mode=mode, units=tuple(units), ring=ring, steps=steps)


def make_cases():
    n = blocks(14 * max(UNITS))
    c = {}
    for tag, mode in (("A", A), ("B", B)):
        # 1. a dit tapped and released during a dah (the dah paddle is up again by then): sent after it
        c["opposite_" + tag] = case(mode, [("run", pads(n, [(DAH, 0.5, 1.5), (DIT, 2, 2.5)]))])
        # 2. a dah tapped during the gap behind a dah: not remembered
        c["same_tap_" + tag] = case(mode, [("run", pads(n, [(DAH, 0.5, 1.5), (DAH, 3.5, 4)]))])
        # 3. both paddles down, both let go inside the dah
        c["squeeze_release_" + tag] = case(mode, [("run", pads(n, [(DIT | DAH, 0.5, 4)]))])
        # 4. both paddles held
        c["squeeze_held_" + tag] = case(mode, [("run", pads(n, [(DIT | DAH, 0.5, 1000)]))])
        # 5. a paddle pressed while text is queued
        c["takeover_" + tag] = case(mode, [("send", "TT"), ("run", pads(n, [(DIT, 1, 1.5)]))])
    # 6. the straight-key bit is ORed over everything; in STRAIGHT the paddles are the key
    c["key_bit_A"] = case(A, [("run", pads(n, [(KEY, 0.5, 2), (KEY, 5, 5.5)]))])
    c["key_bit_over_text_S"] = case(S, [("send", "E E"), ("run", pads(n, [(KEY, 2, 3)]))])
    c["paddles_are_the_key_S"] = case(S, [("run", pads(n, [(DIT, 0.5, 1), (DAH, 2, 2.5), (KEY, 3, 4), (DIT | DAH, 6, 9)]))])
    # 7. element timing under paddles that come and go
    rng = np.random.default_rng(0x7E)
    for tag, mode in (("A", A), ("B", B)):
        c["timing_" + tag] = case(mode, [("run", ko.random_paddles(rng, CHANNELS, blocks(40 * max(UNITS)), UNITS, bits=3))])
    # 8. the ring wraps: 20 characters through 4 bytes, fed as pending allows
    c["ring_wrap"] = case(A, [("feed", WRAP_TEXT)], units=(2, 3, 1), ring=4)
    # 9. bytes without a pattern are skipped and counted
    c["skipped"] = case(B, [("send", SKIP_TEXT), ("run", None, blocks(40 * max(UNITS)))])
    # 10. the unit changes in the middle of a gap: the next element has the new length
    held = np.full((CHANNELS, 5 * BLOCK), DIT, np.uint8)
    c["speed"] = case(A, [("run", held[:, :BLOCK]), ("retune", A, (5, 5, 5)), ("run", held[:, BLOCK:])], units=(16, 16, 16))
    return c


CASES = make_cases()


def play(cs, be):
    """plays a case on a backend (setup, send, retune, run, pending, state) -> the key bytes of all its runs, [CHANNELS][n]"""
    be.setup(cs["mode"], cs["units"], cs["ring"])
    keys = []
    for st in cs["steps"]:
        if st[0] == "send":
            assert be.send(0, [st[1]] * CHANNELS)
        elif st[0] == "retune":
            be.retune(st[1], st[2])
        elif st[0] == "run":
            keys.append(be.run(st[1], st[1].shape[1] if st[1] is not None else st[2]))
        elif st[0] == "feed":                    # as much of the text as every channel's ring has room for, then a block; until all is out
            text, sent = st[1], [0] * CHANNELS
            for _ in range(2000):
                room = cs["ring"] - be.pending().astype(np.int64)
                for ch in range(CHANNELS):
                    piece = text[sent[ch]:sent[ch] + int(room[ch])]
                    if piece:
                        assert be.send(ch, [piece])
                        sent[ch] += len(piece)
                if keys and min(sent) == len(text) and not (be.state()["phase"] != ko.IDLE).any():
                    break
                keys.append(be.run(None, BLOCK))
            else:
                raise AssertionError("the text never ran out")
    return np.concatenate(keys, axis=1)


class OracleBackend:
    def __init__(self, events=False):
        self.events = events

    def setup(self, mode, units, ring):
        self.bank = ko.Bank(CHANNELS, mode, np.array(units), ring)

    def send(self, first, texts):
        return self.bank.send(texts, first, len(texts))

    def retune(self, mode, units):
        self.bank.retune(mode, np.array(units))

    def run(self, paddles, n):
        return self.bank.run(paddles, n, events=self.events)

    def pending(self):
        return self.bank.pending()

    def state(self):
        return self.bank.state()


def runs(key):
    """run lengths of one channel's key bytes: [(value, length), ...]"""
    key = np.asarray(key, np.uint8)
    edges = np.flatnonzero(np.diff(key)) + 1
    bounds = np.concatenate([[0], edges, [len(key)]])
    return [(int(key[a]), int(b - a)) for a, b in zip(bounds[:-1], bounds[1:])]
