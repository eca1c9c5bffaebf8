"""The keyer's law (include/selenite_tx_keyer.h) in plain Python / numpy, stated twice.

`Keyer.run` is the law as the header writes it: one channel, sample by sample.  `Keyer.run_events` says the same thing over run lengths: a
phase that has `left` samples to go puts out `left` equal key values and watches the paddles of those samples as ORs over the range; only
the sample on which a phase ends, or on which an idle keyer meets a dit or dah bit, is decided on its own.  The two share the state words
and nothing else; the tests hold them against each other and, for text alone, against sr.morse_key.
"""
import numpy as np

IDLE, MARK, GAP = 0, 1, 2
STRAIGHT, IAMBIC_A, IAMBIC_B = 0, 1, 2
WORDS = ("phase", "left", "last", "dit_mem", "dah_mem", "squeeze", "code", "tgap", "tail", "head", "skipped")
M32 = 0xFFFFFFFF


def builtin_codes():
    """character -> pattern of the built-in Morse table, written out here (not taken from the library)"""
    pats = {"A": ".-", "B": "-...", "C": "-.-.", "D": "-..", "E": ".", "F": "..-.", "G": "--.", "H": "....", "I": "..", "J": ".---",
            "K": "-.-", "L": ".-..", "M": "--", "N": "-.", "O": "---", "P": ".--.", "Q": "--.-", "R": ".-.", "S": "...", "T": "-",
            "U": "..-", "V": "...-", "W": ".--", "X": "-..-", "Y": "-.--", "Z": "--..",
            "0": "-----", "1": ".----", "2": "..---", "3": "...--", "4": "....-", "5": ".....", "6": "-....", "7": "--...", "8": "---..",
            "9": "----.", ".": ".-.-.-", ",": "--..--", "?": "..--..", "/": "-..-.", "=": "-...-", "+": ".-.-.", "-": "-....-",
            "@": ".--.-."}
    codes = np.zeros(256, np.uint8)
    for ch, pat in pats.items():
        code = 1
        for e in pat:
            code = (code << 1) | (e == "-")
        codes[ord(ch)] = code
        if ch.isalpha():
            codes[ord(ch.lower())] = code
    codes[ord(" ")] = 1
    return codes


class Keyer:
    """one channel"""

    def __init__(self, mode=IAMBIC_B, unit=4, ring=64, codes=None):
        self.mode, self.unit, self.ring = int(mode), int(unit), int(ring)
        self.codes = builtin_codes() if codes is None else np.asarray(codes, np.uint8)
        self.text = np.zeros(self.ring, np.uint8)
        self.phase, self.left, self.last, self.dit_mem, self.dah_mem, self.squeeze = IDLE, 0, 0, 0, 0, 0
        self.code, self.tgap, self.tail, self.head, self.skipped = 1, 0, 0, 0, 0

    # ---- what both statements share: the state words and the text memory ----
    def words(self):
        return {k: int(getattr(self, k)) for k in WORDS}

    def set_words(self, w):
        for k in WORDS:
            if k in w:
                setattr(self, k, int(w[k]))

    def copy(self):
        k = Keyer(self.mode, self.unit, self.ring, self.codes)
        k.set_words(self.words())
        k.text = self.text.copy()
        return k

    def pending(self):
        return (self.head - self.tail) & M32

    def send(self, text):
        """selenite_tx_keyer_send for this channel: False (nothing written) if the ring lacks room"""
        b = text.encode("latin-1") if isinstance(text, str) else bytes(text)
        if self.pending() + len(b) > self.ring:
            return False
        for i, x in enumerate(b):
            self.text[((self.head + i) & M32) % self.ring] = x
        self.head = (self.head + len(b)) & M32
        return True

    def _queued(self):
        return self.tail != self.head or self.code > 1 or self.tgap != 0

    def _bits(self, p):
        d, h, s = p & 1, (p >> 1) & 1, (p >> 2) & 1
        if self.mode == STRAIGHT:
            return 0, 0, s | d | h
        return d, h, s

    # ---- statement 1: the law, sample by sample ----
    def _next_from_text(self):
        """0 / 1: an element; 'gap': a gap has begun; None: nothing"""
        while True:
            if self.tgap:
                self.phase, self.left, self.tgap = GAP, (self.tgap * self.unit) & M32, 0
                return "gap"
            if self.code > 1:
                top = self.code.bit_length() - 2
                el = (self.code >> top) & 1
                self.code = (1 << top) | (self.code & ((1 << top) - 1))
                if self.code == 1:
                    self.tgap = 2
                return el
            if self.tail == self.head:
                return None
            k = int(self.codes[self.text[self.tail % self.ring]])
            self.tail = (self.tail + 1) & M32
            if k == 1:
                self.tgap = (self.tgap + 4) & M32
            elif k >= 2:
                self.code = k
            else:
                self.skipped = (self.skipped + 1) & M32

    def _sample(self, p):
        d, h, s = self._bits(int(p))
        if (d | h | s) and self._queued():
            self.tail, self.code, self.tgap = self.head, 1, 0
        if self.phase != IDLE:
            if self.last == 1:
                self.dit_mem |= d
            else:
                self.dah_mem |= h
            if self.phase == MARK:
                self.squeeze |= d & h
        if self.phase == MARK and self.left == 0:
            self.phase, self.left = GAP, self.unit
        elif self.phase != MARK and self.left == 0:
            if self.mode == IAMBIC_A and self.squeeze and not (d | h):
                self.dit_mem = self.dah_mem = 0
            wd, wh = d | self.dit_mem, h | self.dah_mem
            other = 0 if self.last == 1 else 1
            if wd and wh:
                el = 0 if self.phase == IDLE else other
            elif wd:
                el = 0
            elif wh:
                el = 1
            elif self.mode == IAMBIC_B and self.squeeze:
                el = other
            else:
                el = self._next_from_text()
            if el in (0, 1):
                self.phase, self.left, self.last, self.squeeze = MARK, (3 if el else 1) * self.unit, el, 0
                if el:
                    self.dah_mem = 0
                else:
                    self.dit_mem = 0
            elif el is None:
                self.phase, self.left, self.squeeze = IDLE, 0, 0
        key = int(self.phase == MARK) | s
        if self.phase != IDLE:
            self.left = (self.left - 1) & M32
        return key

    def run(self, paddles=None, n=None):
        """key bytes of the next n samples (paddles: uint8 [n], or None = all zero)"""
        pad = np.zeros(int(n), np.uint8) if paddles is None else np.asarray(paddles, np.uint8)
        return np.array([self._sample(p) for p in pad], np.uint8)

    # ---- statement 2: over run lengths ----
    def _elements(self):
        """the text memory as a stream of ("gap", units) and ("mark", dah): the next thing to send, the queue moved past it; None: empty"""
        while not self.tgap and self.code <= 1 and self.tail != self.head:
            k = int(self.codes[self.text[self.tail % self.ring]])       # one character at a time: a blank's gap comes before what follows it
            self.tail = (self.tail + 1) & M32
            if k == 0:
                self.skipped = (self.skipped + 1) & M32
            elif k == 1:
                self.tgap = 4
            else:
                self.code = k
        if self.tgap:
            units, self.tgap = self.tgap, 0
            return ("gap", units)
        if self.code <= 1:
            return None
        bits = bin(self.code)[3:]                # the elements behind the leading 1
        self.code = int("1" + bits[1:], 2)
        if not bits[1:]:
            self.tgap = 2
        return ("mark", int(bits[0]))

    def run_events(self, paddles=None, n=None):
        pad = np.zeros(int(n), np.uint8) if paddles is None else np.asarray(paddles, np.uint8)
        N = len(pad)
        s = (pad >> 2) & 1
        if self.mode == STRAIGHT:
            s = s | ((pad & 3) != 0).astype(np.uint8)
            d = h = np.zeros(N, np.uint8)
        else:
            d, h = pad & 1, (pad >> 1) & 1
        touched = (d | h | s) != 0
        call = np.flatnonzero(d | h)             # where an idle keyer wakes
        key = s.copy()
        at = 0
        while at < N:
            if self.left > 0:                    # `left` samples of this phase: [at, at + r)
                r = N - at if self.phase == IDLE else min(self.left, N - at)
                rng = slice(at, at + r)
                if touched[rng].any() and self._queued():
                    self.tail, self.code, self.tgap = self.head, 1, 0
                if self.phase != IDLE:
                    if self.last == 1:
                        self.dit_mem |= int(d[rng].any())
                    else:
                        self.dah_mem |= int(h[rng].any())
                    if self.phase == MARK:
                        self.squeeze |= int((d[rng] & h[rng]).any())
                        key[rng] = 1
                    self.left -= r
                at += r
                continue
            asleep = (self.phase == IDLE and not self._queued() and not (self.dit_mem or self.dah_mem)
                      and not (self.mode == IAMBIC_B and self.squeeze))
            if asleep:
                later = call[np.searchsorted(call, at):]
                wake = int(later[0]) if later.size else N
                if wake > at:
                    self.squeeze = 0
                    at = wake
                    continue
            # a phase ends on sample `at` (or an idle keyer is called): that sample is watched by the phase that ends
            dn, hn = int(d[at]), int(h[at])
            if touched[at] and self._queued():
                self.tail, self.code, self.tgap = self.head, 1, 0
            if self.phase != IDLE:
                if self.last == 1:
                    self.dit_mem |= dn
                else:
                    self.dah_mem |= hn
                if self.phase == MARK:
                    self.squeeze |= dn & hn
            if self.phase == MARK:
                nxt = ("gap", 1)
            else:
                if self.mode == IAMBIC_A and self.squeeze and dn == 0 and hn == 0:       # a squeeze let go
                    self.dit_mem, self.dah_mem = 0, 0
                want = (dn | self.dit_mem, hn | self.dah_mem)
                other = 0 if self.last == 1 else 1
                if want == (1, 1):
                    nxt = ("mark", 0 if self.phase == IDLE else other)
                elif want[0] or want[1]:
                    nxt = ("mark", 0 if want[0] else 1)
                elif self.mode == IAMBIC_B and self.squeeze:
                    nxt = ("mark", other)
                else:
                    nxt = self._elements()
            if nxt is None:
                self.phase, self.left, self.squeeze = IDLE, 0, 0
                at += 1
                continue
            kind, x = nxt
            if kind == "gap":
                self.phase, self.left = GAP, (x * self.unit) & M32
            else:
                self.phase, self.left, self.last, self.squeeze = MARK, (3 if x else 1) * self.unit, x, 0
                if x:
                    self.dah_mem = 0
                else:
                    self.dit_mem = 0
                key[at] = 1
            self.left = (self.left - 1) & M32    # sample `at` is the phase's first
            at += 1
        return key


class Bank:
    """channels x the law: what the stage computes for paddles [channels][n]"""

    def __init__(self, channels, mode=IAMBIC_B, unit=4, ring=64, codes=None):
        units = np.broadcast_to(np.asarray(unit, np.int64), (channels,))
        self.ch = [Keyer(mode, int(units[c]), ring, codes) for c in range(channels)]

    def retune(self, mode=None, unit=None):
        for c, k in enumerate(self.ch):
            if mode is not None:
                k.mode = int(mode)
            if unit is not None:
                k.unit = int(np.broadcast_to(np.asarray(unit, np.int64), (len(self.ch),))[c])

    def send(self, text, first=0, n=None):
        n = len(self.ch) - first if n is None else n
        texts = [text] * n if isinstance(text, (str, bytes)) else list(text)
        if any(self.ch[first + j].pending() + len(texts[j]) > self.ch[first + j].ring for j in range(n)):
            return False
        for j in range(n):
            self.ch[first + j].send(texts[j])
        return True

    def run(self, paddles=None, n=None, events=False):
        rows = []
        for c, k in enumerate(self.ch):
            f = k.run_events if events else k.run
            rows.append(f(None if paddles is None else paddles[c], n))
        return np.stack(rows)

    def state(self):
        a = {w: np.array([getattr(k, w) for k in self.ch], np.uint32) for w in WORDS}
        a["text"] = np.stack([k.text for k in self.ch])
        return a

    def set_state(self, a):
        for c, k in enumerate(self.ch):
            k.set_words({w: a[w][c] for w in WORDS if w in a})
            if "text" in a:
                k.text = np.array(a["text"][c], np.uint8)

    def pending(self):
        return np.array([k.pending() for k in self.ch], np.uint32)


def random_paddles(rng, channels, n, unit, max_units=5, bits=7, p_idle=0.4):
    """seeded paddles: runs of 1 ... max_units * unit samples (plus or minus a few), each run one byte of `bits`, often released"""
    out = np.zeros((channels, n), np.uint8)
    units = np.broadcast_to(np.asarray(unit, np.int64), (channels,))
    for c in range(channels):
        at = 0
        while at < n:
            r = int(rng.integers(1, max_units * int(units[c]) + 1))
            v = 0 if rng.random() < p_idle else int(rng.integers(0, 8)) & bits
            out[c, at:at + r] = v
            at += r
    return out
