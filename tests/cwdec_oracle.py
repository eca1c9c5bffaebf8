"""numpy restatement of the Morse decoder (include/selenite_rx.h: selenite_rx_set_cwdec), every float operation
one float32 operation, in the order the header states them:

    pw = arm_power_f32(x, n);  ms = pw / (float)n
    ms <= FLT_MAX:  peak / floor followers, thr = floor + f * (peak - floor), active = peak > snr * floor && peak > min_power
    raw -> debounce (flip, run) -> key;  a mark's end: dit / dah against 2 * unit, unit tracking, code;  a space: character at 2 units,
    blank at 5 units;  emit into text[count % ring]

`power` is the meter's (tests/meter_oracle.py), pinned to the reference's arm_power_f32 by tests/golden/meter.npz; the whole law is pinned
by tests/golden/cwdec.npz (tests/test_cwdec_oracle.py).  `step` is the law of one block on scalars; `CwDec` runs it for every channel."""
import numpy as np

import meter_oracle as mo

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max

MORSE = {"A": ".-", "B": "-...", "C": "-.-.", "D": "-..", "E": ".", "F": "..-.", "G": "--.", "H": "....", "I": "..", "J": ".---", "K": "-.-",
         "L": ".-..", "M": "--", "N": "-.", "O": "---", "P": ".--.", "Q": "--.-", "R": ".-.", "S": "...", "T": "-", "U": "..-", "V": "...-",
         "W": ".--", "X": "-..-", "Y": "-.--", "Z": "--..", "0": "-----", "1": ".----", "2": "..---", "3": "...--", "4": "....-",
         "5": ".....", "6": "-....", "7": "--...", "8": "---..", "9": "----.", ".": ".-.-.-", ",": "--..--", "?": "..--..", "/": "-..-.",
         "=": "-...-", "+": ".-.-.", "-": "-....-", "@": ".--.-."}
DEFAULTS = dict(peak_attack=0.5, peak_decay=0.002, floor_attack=0.25, floor_decay=0.002, on_frac=0.4, off_frac=0.25, snr=4.0, min_power=1e-8,
                debounce=2, adapt=1, track=2, unit_min=2 * 256, unit_init=10 * 256, unit_max=64 * 256, ring=256)
FLOATS = ("peak_attack", "peak_decay", "floor_attack", "floor_decay", "on_frac", "off_frac", "snr", "min_power")
ROWS = dict(peak=np.float32, floor=np.float32, primed=np.uint32, key=np.uint32, flip=np.uint32, run=np.uint32, unit=np.uint32, code=np.uint32,
            word=np.uint32, count=np.uint64, text=np.uint8)


def code_of(pattern):
    """the table index of a pattern of . and -: the elements behind a leading 1"""
    code = 1
    for e in pattern:
        code = (code << 1) | (e == "-")
    return code


def table(unknown="#"):
    t = np.full(256, ord(unknown), np.uint8)
    for ch, pat in MORSE.items():
        t[code_of(pat)] = ord(ch)
    return t


def key_of(text, unit_samples):
    """key bytes of `text`: 1 / 3 units down, 1 / 3 / 7 units up between elements / characters / words; no silence around it"""
    out = []
    for w, word in enumerate(text.upper().split()):
        if w:
            out.append(np.zeros(7 * unit_samples, np.uint8))
        for c, ch in enumerate(word):
            if c:
                out.append(np.zeros(3 * unit_samples, np.uint8))
            for e, el in enumerate(MORSE[ch]):
                if e:
                    out.append(np.zeros(unit_samples, np.uint8))
                out.append(np.ones((3 if el == "-" else 1) * unit_samples, np.uint8))
    return np.concatenate(out)


def step(ms, s, p, tab, ring):
    """one block of one channel.  s: dict of Python ints and np.float32 (peak, floor), changed in place; ring: that channel's text row"""
    ms = F32(ms)
    raw = 0
    if ms <= FLT_MAX:                                    # (false for NaN)
        if not s["primed"]:
            s["peak"], s["floor"], s["primed"] = ms, ms, 1
        else:
            r = p["peak_attack"] if ms > s["peak"] else p["peak_decay"]
            d = F32(ms - s["peak"])
            t = F32(r * d)
            s["peak"] = F32(s["peak"] + t)
            r = p["floor_attack"] if ms < s["floor"] else p["floor_decay"]
            d = F32(ms - s["floor"])
            t = F32(r * d)
            s["floor"] = F32(s["floor"] + t)
        span = F32(s["peak"] - s["floor"])
        f = p["off_frac"] if s["key"] else p["on_frac"]
        t = F32(f * span)
        thr = F32(s["floor"] + t)
        q = F32(p["snr"] * s["floor"])
        active = s["peak"] > q and s["peak"] > p["min_power"]
        raw = int(bool(active and ms > thr))
    edge, ended = False, 0
    if raw == s["key"]:
        s["run"] = min(s["run"] + s["flip"] + 1, 65535)
        s["flip"] = 0
    else:
        s["flip"] += 1
        if s["flip"] >= p["debounce"]:
            ended, s["key"], s["run"], s["flip"], edge = s["run"], raw, s["flip"], 0, True
    if edge and s["key"] == 0:
        m = ended << 8
        unit = s["unit"]
        dah = int(m >= 2 * unit)
        if p["adapt"]:
            g = m // 3 if dah else m
            if g >= unit:
                unit += (g - unit) >> p["track"]
            else:
                unit -= (unit - g) >> p["track"]
            s["unit"] = min(max(unit, p["unit_min"]), p["unit_max"])
        s["code"] = 0 if (s["code"] == 0 or s["code"] >= 128) else (s["code"] << 1) | dah
    if s["key"] == 0:
        sp = s["run"] << 8
        if s["code"] != 1 and sp >= 2 * s["unit"]:
            ring[s["count"] % len(ring)] = tab[s["code"]]
            s["count"] += 1
            s["code"], s["word"] = 1, 1
        if s["word"] and sp >= 5 * s["unit"]:
            ring[s["count"] % len(ring)] = ord(" ")
            s["count"] += 1
            s["word"] = 0


class CwDec:
    """the stage of `channels` channels with DSP blocks of n audio samples"""

    def __init__(self, channels, n, table=None, **par):
        assert not set(par) - set(DEFAULTS), par
        self.channels, self.n = channels, n
        p = dict(DEFAULTS, **par)
        self.par = {k: (F32(v) if k in FLOATS else int(v)) for k, v in p.items()}
        self.table = globals()["table"]() if table is None else np.array(table, np.uint8)
        self.reset()

    def reset(self):
        c = self.channels
        z = lambda t: np.zeros(c, t)  # noqa: E731
        self.peak, self.floor = z(np.float32), z(np.float32)
        self.primed, self.key, self.flip, self.run, self.word = (z(np.uint32) for _ in range(5))
        self.unit, self.code = np.full(c, self.par["unit_init"], np.uint32), np.ones(c, np.uint32)
        self.count = z(np.uint64)
        self.text = np.zeros((c, self.par["ring"]), np.uint8)

    def state(self):
        return {k: getattr(self, k).copy() for k in ROWS}

    def set_state(self, d):
        for k in d:
            setattr(self, k, np.array(d[k], dtype=ROWS[k]))

    def process_ms(self, ms):
        """ms f32 [channels][blocks]: the mean squares themselves"""
        ms = np.asarray(ms, np.float32)
        assert ms.shape[0] == self.channels
        with np.errstate(all="ignore"):
            for c in range(self.channels):
                s = {k: (getattr(self, k)[c] if k in ("peak", "floor") else int(getattr(self, k)[c])) for k in ROWS if k != "text"}
                for b in range(ms.shape[1]):
                    step(ms[c, b], s, self.par, self.table, self.text[c])
                for k, v in s.items():
                    getattr(self, k)[c] = v
        return ms

    def process(self, x):
        """x: the un-scaled audio [channels][blocks * n]; returns the mean squares f32 [channels][blocks]"""
        x = np.asarray(x, np.float32)
        assert x.shape[0] == self.channels and x.shape[1] % self.n == 0, x.shape
        return self.process_ms(mo.mean_square(x.reshape(self.channels, -1, self.n)))

    def cw_text(self, c):
        n, ring = int(self.count[c]), self.text[c]
        if n <= len(ring):
            return ring[:n].tobytes().decode("latin-1")
        at = n % len(ring)
        return (ring[at:].tobytes() + ring[:at].tobytes()).decode("latin-1")
