"""The impulse noise blanker restated in numpy, vectorised over channels: arm_cmplx_mag_squared_f32,
arm_mean_f32 (the summation an explicit loop over n: strictly sequential, as StatisticsFunctions/arm_mean_f32.c:67-120 has it), the level
recursion, the hit / burst / guard decisions and the copy.  Every float32 operation of the stage is one numpy float32 operation here, in
the stage's order; tests/test_nb_oracle.py pins power and mean bit for bit to tests/golden/nb.npz.

TEST INFRASTRUCTURE.  Nothing here is imported by the product."""
import numpy as np

F32 = np.float32


def q15_to_float(q):
    return np.divide(np.asarray(q).astype(F32), F32(32768.0))   # arm_q15_to_float


def power(x):
    """arm_cmplx_mag_squared_f32 on [..., 2]: two rounded products, then the rounded sum"""
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        re2, im2 = x[..., 0] * x[..., 0], x[..., 1] * x[..., 1]
        return re2 + im2


def mean(p):
    """arm_mean_f32 over the last axis: s = +0.0f; s = s + p[n], n ascending; s / (float)n"""
    p = np.asarray(p, F32)
    s = np.zeros(p.shape[:-1], F32)
    with np.errstate(all="ignore"):
        for n in range(p.shape[-1]):
            s = s + p[..., n]
        return s / F32(p.shape[-1])


def level_step(level, m, alpha, clamp):
    """the level behind a frame of mean m, elementwise; `level` and `m` are float32 arrays"""
    with np.errstate(all="ignore"):
        c = F32(clamp) * level
        mc = np.where(m < c, m, c)
        d = mc - level
        s = F32(alpha) * d
        return np.where(level > 0, level + s, m).astype(F32)


def spread(hit, guard):
    """[..., F] bool: True where a hit lies within `guard` samples, inside the frame"""
    out = hit.copy()
    for d in range(1, guard + 1):
        out[..., d:] |= hit[..., :-d]
        out[..., :-d] |= hit[..., d:]
    return out


class Blanker:
    """the stage of selenite_rx_set_nb; state as selenite_rx_nb_state_view has it"""

    def __init__(self, channels, frame=64, guard=2, max_hits=8, threshold=8.0, alpha=0.125, clamp=2.0):
        self.c, self.frame, self.guard, self.max_hits = channels, frame, guard, max_hits
        self.threshold, self.alpha, self.clamp = F32(threshold), F32(alpha), F32(clamp)
        self.reset()

    def reset(self):
        self.level = np.zeros(self.c, F32)
        self.blanked = np.zeros(self.c, np.uint64)
        self.bursts = np.zeros(self.c, np.uint64)

    def process(self, iq):
        """one call's input [channels][L][2], f32 or int16; returns the blanked copy in the same format"""
        iq = np.asarray(iq)
        q15 = iq.dtype == np.int16
        x = q15_to_float(iq) if q15 else np.asarray(iq, F32)
        ch, L = x.shape[0], x.shape[1]
        F = self.frame
        assert ch == self.c and L % F == 0, (x.shape, F)
        out = iq.copy()                                           # (the samples that are not blanked: the input's own bits)
        p = power(x).reshape(ch, L // F, F)
        m = mean(p)                                               # [C][frames]
        with np.errstate(all="ignore"):
            for f in range(L // F):
                primed = self.level > 0
                thr = self.threshold * self.level
                hit = (p[:, f] > thr[:, None]) & primed[:, None]
                k = hit.sum(axis=1)
                blank = spread(hit, self.guard) & ((k >= 1) & (k <= self.max_hits))[:, None]
                self.bursts += (k > self.max_hits).astype(np.uint64)
                self.blanked += blank.sum(axis=1).astype(np.uint64)
                out[:, f * F:(f + 1) * F][blank] = 0              # (+0.0f, +0.0f) | (0, 0)
                self.level = level_step(self.level, m[:, f], self.alpha, self.clamp)
        return out

    def state(self):
        return dict(level=self.level.copy(), blanked=self.blanked.copy(), bursts=self.bursts.copy())

    def set_state(self, d):
        self.level, self.blanked, self.bursts = d["level"].copy(), d["blanked"].copy(), d["bursts"].copy()
