"""numpy restatement of the tone-detector bank (selenite_rx_set_tones): K Goertzel recurrences
and the frame energy per channel on the un-scaled audio, one float32 operation per line, vectorised over channels and tones; the decision
law in integers.  tests/test_tones_oracle.py pins the recurrence, the energy, the powers and the maximum to the reference's own
arm_biquad_cascade_df1_f32, arm_power_f32, arm_cmplx_mag_squared_f32 and arm_max_f32 (tests/golden/tones.npz)."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
FLT_MAX = np.finfo(np.float32).max


def design(freq):
    """[K][3] {2 cos w, cos w, sin w}, w = 2 pi freq, in double, rounded once (selenite_rx_design_tones)"""
    w = 2.0 * np.pi * np.asarray(freq, np.float64).reshape(-1)
    return np.stack([2.0 * np.cos(w), np.cos(w), np.sin(w)], axis=1).astype(np.float32)


def arm_max(p):
    """arm_max_f32 over the last axis: out = p[0]; for i = 1 ..: if (out < p[i]) take -- the first index of the maximum, a NaN wins only at
    index 0.  p [..., K] -> (value [...], index [...])"""
    p = np.asarray(p, np.float32)
    out, idx = p[..., 0].copy(), np.zeros(p.shape[:-1], np.uint32)
    with np.errstate(invalid="ignore"):
        for i in range(1, p.shape[-1]):
            take = out < p[..., i]
            out = np.where(take, p[..., i], out)
            idx = np.where(take, np.uint32(i), idx)
    return out, idx


class Tones:
    """Tones(channels, n, coeffs, frame_blocks, confirm, release, ratio, min_power): n = audio samples per DSP block."""

    def __init__(self, channels, n, coeffs, frame_blocks=1, confirm=1, release=1, ratio=0.0, min_power=0.0):
        c = np.array(coeffs, np.float32)
        assert c.ndim == 2 and c.shape[1] == 3 and 1 <= c.shape[0] <= 64, c.shape
        self.channels, self.n, self.coeffs, self.K = channels, int(n), c, c.shape[0]
        self.frame_blocks, self.confirm, self.release = int(frame_blocks), int(confirm), int(release)
        self.ratio, self.min_power = F(ratio), F(min_power)
        self.N = self.frame_blocks * self.n
        self.reset()

    def reset(self):
        ch, K = self.channels, self.K
        self.s = np.zeros((ch, K, 2), np.float32)
        self.energy = np.zeros(ch, np.float32)
        self.power = np.zeros((ch, K), np.float32)
        self.frame_energy = np.zeros(ch, np.float32)
        self.last_best = np.zeros(ch, np.uint32)
        self.tone = np.full(ch, NONE, np.uint32)
        self.cand = np.full(ch, NONE, np.uint32)
        self.run = np.zeros(ch, np.uint32)
        self.changes = np.zeros(ch, np.uint64)
        self.position = 0              # DSP blocks
        self.done = 0                  # samples of the running frame

    def state(self):
        d = {k: getattr(self, k).copy() for k in ("s", "energy", "power", "frame_energy", "last_best", "tone", "cand", "run", "changes")}
        d["position"] = np.array([self.position], np.uint64)
        return d

    def decide(self, p_best, best, E):
        """the integer half of a frame's end, given arm_max_f32's result and the frame energy (each [channels])"""
        with np.errstate(all="ignore"):
            t = self.ratio * E
            t = t * F(self.N)
            hit = (p_best > t) & (p_best > self.min_power) & (p_best <= FLT_MAX)
        w = np.where(hit, best, np.uint32(NONE)).astype(np.uint32)
        same = w == self.cand
        self.run = np.where(same, np.minimum(self.run + np.uint32(1), np.uint32(65535)), np.uint32(1)).astype(np.uint32)
        self.cand = w
        need = np.where(self.cand == NONE, self.release, self.confirm)
        ch = (self.cand != self.tone) & (self.run >= need)
        self.tone = np.where(ch, self.cand, self.tone).astype(np.uint32)
        self.changes = self.changes + ch.astype(np.uint64)

    def frame_end(self):
        c, cw, sw = self.coeffs[:, 0], self.coeffs[:, 1], self.coeffs[:, 2]
        s1, s2 = self.s[:, :, 0], self.s[:, :, 1]
        with np.errstate(all="ignore"):
            u = cw * s2
            re = s1 - u
            im = sw * s2
            a = re * re
            b = im * im
            p = a + b
        p_best, best = arm_max(p)
        self.decide(p_best, best, self.energy)
        self.power, self.frame_energy, self.last_best = p.astype(np.float32), self.energy.copy(), best
        self.s = np.zeros_like(self.s)
        self.energy = np.zeros_like(self.energy)

    def process(self, x):
        """x [channels][whole DSP blocks] continues the stream; returns nothing (a tap)"""
        x = np.asarray(x, np.float32)
        assert x.ndim == 2 and x.shape[0] == self.channels and x.shape[1] % self.n == 0, x.shape
        c = self.coeffs[:, 0][None, :]
        with np.errstate(all="ignore"):
            for i in range(x.shape[1]):
                xn = x[:, i]
                s1, s2 = self.s[:, :, 0], self.s[:, :, 1]
                t = c * s1
                s0 = xn[:, None] + t
                s0 = s0 - s2
                self.s = np.stack([s0, s1], axis=2)
                e = xn * xn
                self.energy = self.energy + e
                self.done += 1
                if self.done == self.N:
                    self.frame_end()
                    self.done = 0
        assert self.s.dtype == np.float32 and self.energy.dtype == np.float32
        self.position += x.shape[1] // self.n


def same_bits(a, b):
    """bit for bit, but any NaN equals any NaN (the sign of a generated NaN is the implementation's)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and np.where(na, F(0), a).tobytes() == np.where(nb, F(0), b).tobytes()
