"""numpy restatement of the audio biquad filter stage (selenite_rx_set_afilt): arm_biquad_cascade_df1_f32
(FilteringFunctions/arm_biquad_cascade_df1_f32.c:165-407) in place on the un-scaled audio of every channel, stage-outer, one float32
operation per line, vectorised over channels.  Coefficients {b0, b1, b2, a1, a2} in CMSIS sign (the a's are ADDED), state {x1, x2, y1, y2}
in pState order.  tests/test_afilt_oracle.py pins it to the reference's own function (tests/golden/afilt.npz)."""
import numpy as np

F = np.float32


class Afilt:
    """Afilt(channels, coeffs, per_channel): coeffs [n_stages][5], or with per_channel [channels][n_stages][5]."""

    def __init__(self, channels, coeffs, per_channel=False):
        c = np.array(coeffs, np.float32)
        if c.ndim == 1:
            c = c.reshape(-1, 5)
        self.channels, self.per_channel = channels, bool(per_channel)
        if self.per_channel:
            assert c.ndim == 3 and c.shape[0] == channels and c.shape[2] == 5, c.shape
            self.coeffs = c.copy()
        else:
            assert c.ndim == 2 and c.shape[1] == 5, c.shape
            self.coeffs = np.tile(c, (channels, 1, 1))
        self.n_stages = self.coeffs.shape[1]
        self.state = np.zeros((channels, self.n_stages, 4), np.float32)

    def set_coeffs(self, coeffs, first_channel=0):
        """replaces the rows of channels first_channel .. and keeps the state (selenite_rx_set_afilt_coeffs)"""
        c = np.array(coeffs, np.float32)
        if self.per_channel:
            assert c.ndim == 3 and c.shape[1:] == (self.n_stages, 5)
            self.coeffs[first_channel:first_channel + c.shape[0]] = c
        else:
            assert first_channel == 0
            self.coeffs[:] = c.reshape(1, self.n_stages, 5)

    def reset(self):
        self.state[...] = 0

    def process(self, x):
        """x [channels][n] -> y [channels][n]; continues the stream"""
        x = np.array(x, np.float32)
        assert x.ndim == 2 and x.shape[0] == self.channels
        n = x.shape[1]
        with np.errstate(all="ignore"):
            for s in range(self.n_stages):
                b0, b1, b2, a1, a2 = (self.coeffs[:, s, k].copy() for k in range(5))
                x1, x2, y1, y2 = (self.state[:, s, k].copy() for k in range(4))
                y = np.empty_like(x)
                for i in range(n):
                    xn = x[:, i]
                    p0 = b0 * xn
                    p1 = b1 * x1
                    p2 = b2 * x2
                    p3 = a1 * y1
                    p4 = a2 * y2
                    acc = p0 + p1
                    acc = acc + p2
                    acc = acc + p3
                    acc = acc + p4
                    x2 = x1
                    x1 = xn
                    y2 = y1
                    y1 = acc
                    y[:, i] = acc
                for k, v in enumerate((x1, x2, y1, y2)):
                    self.state[:, s, k] = v
                x = y
        assert x.dtype == np.float32
        return x


def same_bits(a, b):
    """bit for bit, but any NaN equals any NaN: IEEE 754 leaves the sign and payload of a generated NaN to the implementation (x86 SSE gives
    the negative quiet NaN for Inf - Inf, gfx950 the positive one)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and np.where(na, F(0), a).tobytes() == np.where(nb, F(0), b).tobytes()
