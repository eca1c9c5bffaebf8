"""The I/Q correction stage restated in numpy, vectorised over channels: arm_mean_f32,
arm_power_f32 and arm_dot_prod_f32 (each summation an explicit loop over n: strictly sequential, one accumulator from +0.0f, as the CMSIS
sources have them), arm_offset_f32 / arm_scale_f32 / arm_sub_f32, the quotient, arm_sqrt_f32, the validity test, the clamps and the two
recursions.  Every float32 operation of the stage is one numpy float32 operation here, in the stage's order; tests/test_iqc_oracle.py pins
the primitives bit for bit to tests/golden/iqc.npz.

TEST INFRASTRUCTURE.  Nothing here is imported by the product."""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def q15_to_float(q):
    return np.divide(np.asarray(q).astype(F32), F32(32768.0))   # arm_q15_to_float


def mean(x):
    """arm_mean_f32 over the last axis: s = +0.0f; s = s + x[n], n ascending; s / (float)n"""
    x = np.asarray(x, F32)
    s = np.zeros(x.shape[:-1], F32)
    with np.errstate(all="ignore"):
        for n in range(x.shape[-1]):
            s = s + x[..., n]
        return s / F32(x.shape[-1])


def dot(a, b):
    """arm_dot_prod_f32 over the last axis (arm_power_f32 is dot(a, a)): sum = sum + (a[n] * b[n]), product rounded, then the sum"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    s = np.zeros(a.shape[:-1], F32)
    with np.errstate(all="ignore"):
        for n in range(a.shape[-1]):
            s = s + a[..., n] * b[..., n]
    return s


def power(a):
    return dot(a, a)


def offset(x, off):
    """arm_offset_f32: x[n] + off (the stage passes the negated dc: the bits of x[n] - dc)"""
    with np.errstate(all="ignore"):
        return (np.asarray(x, F32) + np.asarray(off, F32)).astype(F32)


def scale(x, k):
    with np.errstate(all="ignore"):
        return (np.asarray(x, F32) * np.asarray(k, F32)).astype(F32)


def sub(a, b):
    with np.errstate(all="ignore"):
        return (np.asarray(a, F32) - np.asarray(b, F32)).astype(F32)


def quotient(a, b):
    with np.errstate(all="ignore"):
        return np.divide(np.asarray(a, F32), np.asarray(b, F32)).astype(F32)


def sqrt(a):
    """arm_sqrt_f32 as the stage uses it: sqrtf, correctly rounded (the stage only uses the result where the argument is positive)"""
    with np.errstate(all="ignore"):
        return np.sqrt(np.asarray(a, F32)).astype(F32)


def follow(x, target, alpha):
    """x + alpha * (target - x): difference, product and sum each rounded"""
    with np.errstate(all="ignore"):
        d = target - x
        s = F32(alpha) * d
        return (x + s).astype(F32)


def estimate(i, q):
    """the raw imbalance estimate of DC-removed rails [..., F]: pii, pqq, piq, a, r, b"""
    pii, pqq, piq = power(i), power(q), dot(i, q)
    a = quotient(piq, pii)
    r = sub(pqq, scale(a, piq))
    b = sqrt(quotient(pii, r))
    return pii, pqq, piq, a, r, b


class Corrector:
    """the stage of selenite_rx_set_iqc; state as selenite_rx_iqc_state_view has it"""

    def __init__(self, channels, frame=64, alpha=1.0 / 64, dc_alpha=1.0 / 16, p_max=0.25, g_max=1.5, min_power=1e-12, p_init=0.0, g_init=1.0,
                 dc_i_init=0.0, dc_q_init=0.0):
        self.c, self.frame = channels, frame
        self.alpha, self.dc_alpha, self.p_max, self.g_max, self.min_power = F32(alpha), F32(dc_alpha), F32(p_max), F32(g_max), F32(min_power)
        self.g_min = F32(1.0) / self.g_max
        self.inits = dict(dc_i=F32(dc_i_init), dc_q=F32(dc_q_init), p=F32(p_init), g=F32(g_init))
        self.reset()

    def reset(self):
        for k, v in self.inits.items():
            setattr(self, k, np.full(self.c, v, F32))
        self.held = np.zeros(self.c, np.uint64)

    def process(self, data):
        """one call's input [channels][L][2], f32 or int16; returns the corrected copy, always f32"""
        data = np.asarray(data)
        x = q15_to_float(data) if data.dtype == np.int16 else np.asarray(data, F32)
        ch, L = x.shape[0], x.shape[1]
        F = self.frame
        assert ch == self.c and L % F == 0, (x.shape, F)
        out = np.empty((ch, L, 2), F32)
        with np.errstate(all="ignore"):
            for f in range(L // F):
                I, Q = x[:, f * F:(f + 1) * F, 0], x[:, f * F:(f + 1) * F, 1]
                i, q = sub(I, self.dc_i[:, None]), sub(Q, self.dc_q[:, None])
                out[:, f * F:(f + 1) * F, 0] = i
                out[:, f * F:(f + 1) * F, 1] = scale(sub(q, scale(i, self.p[:, None])), self.g[:, None])
                if self.dc_alpha > 0:
                    mi, mq = mean(I), mean(Q)
                    self.dc_i = np.where(np.isfinite(mi), follow(self.dc_i, mi, self.dc_alpha), self.dc_i).astype(F32)
                    self.dc_q = np.where(np.isfinite(mq), follow(self.dc_q, mq, self.dc_alpha), self.dc_q).astype(F32)
                if self.alpha > 0:
                    pii, _, _, a, r, b = estimate(i, q)
                    valid = (pii > self.min_power) & (pii <= FLT_MAX) & (r > self.min_power) & (r <= FLT_MAX)
                    a = np.where(a < -self.p_max, -self.p_max, np.where(a > self.p_max, self.p_max, a)).astype(F32)
                    b = np.where(b < self.g_min, self.g_min, np.where(b > self.g_max, self.g_max, b)).astype(F32)
                    self.p = np.where(valid, follow(self.p, a, self.alpha), self.p).astype(F32)
                    self.g = np.where(valid, follow(self.g, b, self.alpha), self.g).astype(F32)
                    self.held += (~valid).astype(np.uint64)
        return out

    def state(self):
        return dict(dc_i=self.dc_i.copy(), dc_q=self.dc_q.copy(), p=self.p.copy(), g=self.g.copy(), held=self.held.copy())

    def set_state(self, d):
        for k in d:
            setattr(self, k, np.array(d[k], np.uint64 if k == "held" else F32))
