"""numpy restatement of the FSK teleprinter decoder (include/selenite_rx.h: selenite_rx_set_fskdec), every float
operation one float32 operation, in the order the header states them:

    two one-section arm_biquad_cascade_df1_f32 (mark, space) running on across ticks:  acc = b0*x; acc += b1*x1; acc += b2*x2; acc += a1*y1;
    acc += a2*y2 (each product rounded, then the sum)
    pm, ps, pw = arm_power_f32 of ym, ys, x over the tick's T samples;  reverse swaps pm and ps
    all three <= FLT_MAX:  em, es, ew follow them (d = p - e; t = alpha * d; e = e + t)
    present, lvl with hysteresis, the start / data / stop bit clock in Q8 ticks, ITA2 with shifts, emit into text[count % ring]

`biquad` is the audio filter's law (tests/afilt_oracle.py) for one section, `power` is the meter's (tests/meter_oracle.py); both and the
whole law are pinned to the reference's code by tests/golden/fskdec.npz (tests/test_fskdec_oracle.py).  `step` is the law of one tick on
scalars behind the three powers; `FskDec` runs it for every channel.  `encode` and `afsk` make what the decoder reads."""
import numpy as np

import meter_oracle as mo

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max

LETTERS = "\0E\nA SIU\rDRJNFCKTZLWHYPQOBG\0MXV\0"
FIGURES = "\0" "3\n- \a87\r$4',!:(5\")2#6019?&\0./;\0"
LTRS, FIGS, SPACE = 31, 27, 4
DEFAULTS = dict(tick=16, bit_q8=4224, reverse=0, usos=1, ring=256, alpha=0.25, hyst=0.1, frac=0.35, min_power=1e-6)
FLOATS = ("alpha", "hyst", "frac", "min_power")
ROWS = dict(filt=np.float32, em=np.float32, es=np.float32, ew=np.float32, lvl=np.uint32, k=np.uint32, t_q8=np.uint32, shift=np.uint32,
            figs=np.uint32, ferr=np.uint32, bit=np.uint32, count=np.uint64, text=np.uint8)
INTS = ("lvl", "k", "t_q8", "shift", "figs", "ferr", "bit", "count")


def table():
    """ITA2 letters, then the US-TTY figures, by the 5-bit code; 0: prints nothing"""
    assert len(LETTERS) == len(FIGURES) == 32
    return np.frombuffer((LETTERS + FIGURES).encode("latin-1"), np.uint8).copy()


def design(f_mark, f_space, bandwidth):
    """(mark, space): {alpha, 0, -alpha, 2 cos w, -(1 - alpha)} / (1 + alpha), alpha = sin w / (2 f0 / bandwidth); double, rounded once"""
    out = []
    for f0 in (f_mark, f_space):
        w = 2.0 * np.pi * f0
        al = np.sin(w) / (2.0 * f0 / bandwidth)
        out.append(np.array([al, 0.0, -al, 2.0 * np.cos(w), -(1.0 - al)], np.float64) / (1.0 + al))
    return out[0].astype(np.float32), out[1].astype(np.float32)


def bit_q8(fs, baud, tick):
    """a bit of `baud` in Q8 ticks of `tick` samples at the audio rate fs"""
    return int(round(fs / baud / tick * 256.0))


def encode(text, usos=True):
    """the 5-bit codes of `text` with the shifts a receiver in letters needs; with usos a blank puts the receiver back into letters, so
    FIGS is sent again behind it.  Lower case is sent as upper case; a character in neither case raises ValueError."""
    codes, figs = [], 0
    for ch in text.upper():
        if ch == "\0":
            raise ValueError("encode: NUL")
        in_l, in_f = LETTERS.find(ch), FIGURES.find(ch)
        if in_l < 0 and in_f < 0:
            raise ValueError("encode: no code for %r" % ch)
        if (in_f if figs else in_l) < 0:
            figs ^= 1
            codes.append(FIGS if figs else LTRS)
        c = in_f if figs else in_l
        codes.append(c)
        if usos and c == SPACE:
            figs = 0
    return codes


def afsk(codes, fs, baud, f_mark, f_space, stop_bits=1.5, lead=0.0, tail=0.0):
    """phase-continuous audio of amplitude 1 (float64): per code a start bit (space), five data bits LSB first (1 = mark) and `stop_bits`
    of mark; `lead` and `tail` bits of mark around it.  Bit edges fall where they fall between the samples."""
    halves = [1] * int(round(2 * lead))                     # the keying in half bits
    for c in codes:
        halves += [0, 0]
        for b in range(5):
            halves += [(c >> b) & 1] * 2
        halves += [1] * int(round(2 * stop_bits))
    halves += [1] * int(round(2 * tail))
    halves = np.array(halves, np.int64)
    n = int(np.floor(len(halves) * fs / (2.0 * baud)))
    idx = np.minimum((np.arange(n) * (2.0 * baud) / fs).astype(np.int64), len(halves) - 1)
    f = np.where(halves[idx] == 1, f_mark, f_space)
    phase = 2.0 * np.pi * np.cumsum(f) / fs
    return np.sin(phase)


def biquad(x, coef, st):
    """one section of arm_biquad_cascade_df1_f32 over the last axis of x [..., L]; st [..., 4] {x1, x2, y1, y2}, changed in place"""
    x = np.asarray(x, np.float32)
    b0, b1, b2, a1, a2 = (F32(v) for v in coef)
    x1, x2, y1, y2 = (st[..., i].copy() for i in range(4))
    y = np.empty_like(x)
    with np.errstate(all="ignore"):
        for i in range(x.shape[-1]):
            xn = x[..., i]
            acc = b0 * xn
            acc = acc + b1 * x1
            acc = acc + b2 * x2
            acc = acc + a1 * y1
            acc = acc + a2 * y2
            x2, x1, y2, y1 = x1, xn, y1, acc
            y[..., i] = acc
    st[..., 0], st[..., 1], st[..., 2], st[..., 3] = x1, x2, y1, y2
    assert y.dtype == np.float32
    return y


def step(pm, ps, pw, s, p, tab, ring):
    """one tick of one channel behind its three powers.  s: dict of Python ints and np.float32 (em, es, ew), changed in place; ring: that
    channel's text row"""
    pm, ps, pw = F32(pm), F32(ps), F32(pw)
    if p["reverse"]:
        pm, ps = ps, pm
    with np.errstate(all="ignore"):
        if pm <= FLT_MAX and ps <= FLT_MAX and pw <= FLT_MAX:           # (false for NaN)
            for e, v in (("em", pm), ("es", ps), ("ew", pw)):
                d = F32(v - s[e])
                t = F32(p["alpha"] * d)
                s[e] = F32(s[e] + t)
        tot = F32(s["em"] + s["es"])
        dd = F32(s["em"] - s["es"])
        th = F32(p["hyst"] * tot)
        q = F32(p["frac"] * s["ew"])
    present = bool(tot > q and tot > p["min_power"] and tot <= FLT_MAX)
    prev = s["lvl"]
    if not present:
        s["lvl"] = 1
    elif dd > th:
        s["lvl"] = 1
    elif -dd > th:
        s["lvl"] = 0
    lvl, k = s["lvl"], s["k"]
    if k == 0:
        if prev == 1 and lvl == 0:
            s["k"], s["t_q8"], s["shift"] = 1, 0, 0
        return
    s["t_q8"] += 256
    if s["t_q8"] < (k - 1) * s["bit"] + (s["bit"] >> 1):
        return
    if k == 1:
        s["k"] = 0 if lvl else 2
    elif k <= 6:
        s["shift"] |= lvl << (k - 2)
        s["k"] = k + 1
    else:
        if lvl:
            c = s["shift"]
            if c == LTRS:
                s["figs"] = 0
            elif c == FIGS:
                s["figs"] = 1
            else:
                b = int(tab[(s["figs"] * 32 + c) & 63])
                if b:
                    ring[s["count"] % len(ring)] = b
                    s["count"] += 1
                if p["usos"] and c == SPACE:
                    s["figs"] = 0
        else:
            s["ferr"] += 1
        s["k"] = 0


class FskDec:
    """the stage of `channels` channels"""

    def __init__(self, channels, mark, space, table=None, **par):
        assert not set(par) - set(DEFAULTS), par
        self.channels = channels
        p = dict(DEFAULTS, **par)
        self.par = {k: (F32(v) if k in FLOATS else int(v)) for k, v in p.items()}
        self.mark, self.space = np.array(mark, np.float32), np.array(space, np.float32)
        self.table = globals()["table"]() if table is None else np.array(table, np.uint8)
        self.reset()

    def reset(self):
        c = self.channels
        self.filt = np.zeros((c, 2, 4), np.float32)
        self.em, self.es, self.ew = (np.zeros(c, np.float32) for _ in range(3))
        self.k, self.t_q8, self.shift, self.figs, self.ferr = (np.zeros(c, np.uint32) for _ in range(5))
        self.lvl, self.bit = np.ones(c, np.uint32), np.full(c, self.par["bit_q8"], np.uint32)
        self.count = np.zeros(c, np.uint64)
        self.text = np.zeros((c, self.par["ring"]), np.uint8)

    def state(self):
        return {k: getattr(self, k).copy() for k in ROWS}

    def set_state(self, d):
        for k in d:
            setattr(self, k, np.array(d[k], dtype=ROWS[k]))

    def powers(self, x):
        """x [channels][ticks * T] -> pm, ps, pw f32 [channels][ticks] (before `reverse`); moves the filters"""
        x = np.asarray(x, np.float32)
        T = self.par["tick"]
        assert x.shape[0] == self.channels and x.shape[1] % T == 0, x.shape
        ym, ys = biquad(x, self.mark, self.filt[:, 0]), biquad(x, self.space, self.filt[:, 1])
        return tuple(mo.power(v.reshape(self.channels, -1, T)) for v in (ym, ys, x))

    def process_powers(self, pm, ps, pw):
        for c in range(self.channels):
            s = {k: int(getattr(self, k)[c]) for k in INTS}
            s.update({k: getattr(self, k)[c] for k in ("em", "es", "ew")})
            for t in range(pm.shape[1]):
                step(pm[c, t], ps[c, t], pw[c, t], s, self.par, self.table, self.text[c])
            for k, v in s.items():
                getattr(self, k)[c] = v

    def process(self, x):
        """x: the un-scaled audio [channels][ticks * T]; returns (pm, ps, pw)"""
        p = self.powers(x)
        self.process_powers(*p)
        return p

    def fsk_text(self, c):
        n, ring = int(self.count[c]), self.text[c]
        if n <= len(ring):
            return ring[:n].tobytes().decode("latin-1")
        at = n % len(ring)
        return (ring[at:].tobytes() + ring[:at].tobytes()).decode("latin-1")
