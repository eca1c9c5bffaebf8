"""numpy restatement of the signal-level meter and squelch (include/selenite_rx.h: selenite_rx_set_meter), every
operation one float32 operation, in the order the header states them:

    pw = arm_power_f32(x, n)          StatisticsFunctions/arm_power_f32.c:64-125: sum = +0.0f; sum = sum + in * in, n ascending
    ms = pw / (float)n
    ms <= FLT_MAX:  r = ms > level ? attack : decay;  d = ms - level;  level = level + r * d
    want_open / want_close by sense; open, hold (hang), opens, open_blocks

`power` is pinned to the reference's arm_power_f32 by tests/golden/meter.npz (tests/test_meter_oracle.py).  `step` is the law of one block on
float32 scalars; `Meter` runs it for every channel at once (arrays of float32, the same operations element by element) and keeps, for the
tests, the trace of the last call."""
import numpy as np

ABOVE, BELOW = 0, 1
F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def power(x):
    """arm_power_f32 over the last axis: sum = +0.0f; sum = sum + in * in, ascending (the product rounded, then the sum)"""
    x = np.asarray(x, np.float32)
    s = np.zeros(x.shape[:-1], np.float32)
    with np.errstate(all="ignore"):
        for i in range(x.shape[-1]):
            p = x[..., i] * x[..., i]
            s = s + p
    assert s.dtype == np.float32
    return s


def mean_square(x):
    """pw / (float)n of every block: x [...][n]"""
    with np.errstate(all="ignore"):
        return power(x) / F32(x.shape[-1])


def step(ms, level, is_open, hold, par):
    """one block on float32 scalars: returns (level, open, hold, opened, kept_by_hang)"""
    ms, level = F32(ms), F32(level)
    if ms <= FLT_MAX:                                    # (false for NaN)
        r = F32(par["attack"]) if ms > level else F32(par["decay"])
        d = F32(ms - level)
        level = F32(level + F32(r * d))
    v = level
    above = par["sense"] == ABOVE
    want_open = v > F32(par["open_level"]) if above else v < F32(par["open_level"])
    want_close = v < F32(par["close_level"]) if above else v > F32(par["close_level"])
    opened = kept = False
    if not is_open:
        if want_open:
            is_open, hold, opened = 1, int(par["hang"]), True
    elif want_close:
        if hold == 0:
            is_open = 0
        else:
            hold -= 1
            kept = True
    else:
        hold = int(par["hang"])
    return level, int(is_open), int(hold), opened, kept


class Meter:
    """the stage of `channels` channels with DSP blocks of n audio samples"""

    def __init__(self, channels, n, sense=ABOVE, gate=1, hang=0, attack=0.5, decay=0.125, open_level=1e-6, close_level=5e-7, level_init=0.0):
        self.channels, self.n = channels, n
        self.par = dict(sense=int(sense), gate=int(gate), hang=int(hang), attack=F32(attack), decay=F32(decay), open_level=F32(open_level),
                        close_level=F32(close_level), level_init=F32(level_init))
        self.reset()

    def reset(self):
        c = self.channels
        self.level = np.full(c, self.par["level_init"], np.float32)
        self.open, self.hold = np.zeros(c, np.uint32), np.zeros(c, np.uint32)
        self.opens, self.open_blocks = np.zeros(c, np.uint64), np.zeros(c, np.uint64)
        self.trace = None

    def state(self):
        return dict(level=self.level.copy(), open=self.open.copy(), hold=self.hold.copy(), opens=self.opens.copy(), open_blocks=self.open_blocks.copy())

    def set_state(self, d):
        for k in d:
            setattr(self, k, np.array(d[k], dtype=getattr(self, k).dtype))

    def process(self, x):
        """x: the un-scaled audio [channels][blocks * n]; returns the gate of every block, uint8 [channels][blocks] (open behind its update),
        and leaves self.trace = dict(open, kept, ms, level) [channels][blocks]"""
        p, n = self.par, self.n
        x = np.asarray(x, np.float32)
        assert x.shape[0] == self.channels and x.shape[1] % n == 0, x.shape
        nblk = x.shape[1] // n
        ms = mean_square(x.reshape(self.channels, nblk, n))
        bits = np.zeros((self.channels, nblk), np.uint8)
        kept = np.zeros((self.channels, nblk), bool)
        levels = np.zeros((self.channels, nblk), np.float32)
        level, is_open, hold = self.level.copy(), self.open.astype(bool), self.hold.astype(np.int64)
        above = p["sense"] == ABOVE
        with np.errstate(all="ignore"):
            for b in range(nblk):
                m = ms[:, b]
                r = np.where(m > level, p["attack"], p["decay"]).astype(np.float32)
                d = m - level
                s = r * d
                level = np.where(m <= FLT_MAX, level + s, level).astype(np.float32)
                want_open = level > p["open_level"] if above else level < p["open_level"]
                want_close = level < p["close_level"] if above else level > p["close_level"]
                opening = ~is_open & want_open
                closing = is_open & want_close
                holding = is_open & ~want_close
                kept[:, b] = closing & (hold > 0)
                new_open = opening | holding | (closing & (hold > 0))
                hold = np.where(opening | holding, p["hang"], np.where(closing & (hold > 0), hold - 1, hold))
                self.opens += opening.astype(np.uint64)
                is_open = new_open
                self.open_blocks += is_open.astype(np.uint64)
                bits[:, b] = is_open
                levels[:, b] = level
        self.level, self.open, self.hold = level, is_open.astype(np.uint32), hold.astype(np.uint32)
        self.trace = dict(open=bits.copy(), kept=kept, ms=ms, level=levels)
        return bits

    def gate_audio(self, y, bits):
        """the gate on the audio behind the AGC (f32 or int16 words), y [channels][blocks * n]: closed blocks become +0"""
        if not self.par["gate"]:
            return y
        out = y.copy().reshape(self.channels, -1, self.n)
        out[bits == 0] = 0
        return out.reshape(y.shape)
