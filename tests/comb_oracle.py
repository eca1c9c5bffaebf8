"""The polyphase combiner (include/selenite_comb.h) restated in numpy, vectorised over bands and frames: per input
frame the inverse arm_cfft_f32 (imag negated, spectrum_oracle.cfft -- pinned to the reference by tests/test_spectrum_oracle.py -- then
re * invL and (-im) * invL), per output sample and rail arm_dot_prod_f32 over the Q = P * oversample frames that overlap in it (acc = +0.0f;
acc = acc + g * u, product rounded, then the sum, t ascending), and arm_float_to_q15 for the int16 output.  Every float32 operation of the
composition is one numpy float32 operation here, in its order; tests/test_comb_oracle.py pins it bit for bit to tests/golden/comb.npz.
direct64() is the float64 direct form (zero-stuff, filter, mix up, sum, / K) the composition is measured against.

TEST INFRASTRUCTURE.  Nothing here is imported by the product."""
import numpy as np

import spectrum_oracle as so

F32 = np.float32


def float_to_q15(x, rounding=0):
    """arm_float_to_q15 (SupportFunctions/arm_float_to_q15.c:117; :90-101 with ARM_MATH_ROUNDING): * 32768, [+- 0.5], truncate, saturate"""
    with np.errstate(all="ignore"):
        v = np.asarray(x, F32) * F32(32768.0)
        if rounding:
            v = v + np.where(v > 0, F32(0.5), F32(-0.5)).astype(F32)
        return np.clip(np.trunc(v), -32768, 32767).astype(np.int16)


class Combiner:
    """the object of selenite_comb_init; state as selenite_comb_state_view has it"""

    def __init__(self, bands, fft_len, oversample, taps_per_branch, coeffs, bins=None, q15_rounding=0):
        self.bands, self.k, self.ovs, self.p = bands, fft_len, oversample, taps_per_branch
        self.d, self.q = fft_len // oversample, taps_per_branch * oversample
        self.g = np.asarray(coeffs, F32).reshape(self.q, self.d)                    # g[t][i] = g[i + t D]
        self.bins = np.arange(fft_len) if bins is None else np.asarray(bins, np.int64)
        assert len(set(self.bins.tolist())) == len(self.bins)
        self.rows = bands * len(self.bins)
        self.rounding = q15_rounding
        self.tw = so.twiddles(fft_len)
        self.inv_l = F32(1.0) / F32(fft_len)
        self.reset()

    def reset(self):
        self.history = np.zeros((self.rows, self.q - 1, 2), F32)
        self.position = 0

    def out_len(self, block_size):
        return block_size * self.d

    def _u(self, rows):
        """the inverse transforms of the frames of rows [bands n_bins][F][2]: u [bands][F][K][2]"""
        nb, nf = len(self.bins), rows.shape[1]
        v = np.zeros((self.bands, nf, self.k, 2), F32)                              # bins nobody feeds: +0.0f
        v[:, :, self.bins] = np.transpose(rows.reshape(self.bands, nb, nf, 2), (0, 2, 1, 3))
        with np.errstate(all="ignore"):
            v[..., 1] = -v[..., 1]                                                  # arm_cfft_f32.c:571-580
            y = so.cfft(v, self.tw)
            re = y[..., 0] * self.inv_l                                             # :610
            im = (-y[..., 1]) * self.inv_l                                          # :611
        return np.stack([re, im], axis=-1)

    def process(self, x):
        """one call's input [bands * n_bins][nin][2] f32; returns [bands][nin * D][2] f32"""
        x = np.asarray(x, F32)
        k, d, q = self.k, self.d, self.q
        nin = x.shape[1]
        assert x.shape[0] == self.rows and nin > 0
        buf = np.concatenate([self.history, x], axis=1)                             # frame f of the call is buf[:, f + Q - 1]
        f0 = self.position // d
        out = np.empty((self.bands, nin, d, 2), F32)
        jr = d - 1 - np.arange(d)
        with np.errstate(all="ignore"):
            for m0 in range(0, nin, 64):                                            # (in pieces: bounded memory at K = 512)
                n = min(nin, m0 + 64) - m0
                u = self._u(buf[:, m0:m0 + n + q - 1])                              # [bands][n + Q - 1][K][2]
                fr = np.arange(n)
                pidx = (((f0 + m0 + fr) * d) % k)[:, None] + np.arange(d)[None, :]   # p = (f D + j) mod K
                acc = np.zeros((self.bands, n, d, 2), F32)
                for t in range(q):
                    ut = u[:, fr[:, None] + t, pidx]                                # u_{f - Q + 1 + t}[p]: [bands][n][D][2]
                    prod = self.g[t][jr][None, None, :, None] * ut
                    acc = acc + prod
                out[:, m0:m0 + n] = acc
        self.history = buf[:, nin:].copy()
        self.position += nin * d
        return out.reshape(self.bands, nin * d, 2)

    def process_q15(self, x):
        return float_to_q15(self.process(x), self.rounding)

    def state(self):
        return dict(history=self.history.copy(), position=np.array([self.position], np.uint64))

    def set_state(self, d):
        self.history, self.position = np.asarray(d["history"], F32).copy(), int(d["position"][0])


def direct64(rows, coeffs, fft_len, oversample, bins=None):
    """float64 direct form on whole channel streams rows [n_bins][F][2] (zeros in front): every channel zero-stuffed by D, filtered by h
    (coeffs[i] = h[K P - 1 - i]) and mixed up by e^(+2 pi i k n / K); the sum over the channels, / K.  Returns complex128 [F * D]."""
    k, d = fft_len, fft_len // oversample
    h = np.asarray(coeffs, np.float64)[::-1]
    c = np.asarray(rows, np.float64)
    c = c[..., 0] + 1j * c[..., 1]
    nf = c.shape[1]
    bins = np.arange(k) if bins is None else np.asarray(bins)
    n = np.arange(nf * d)
    out = np.zeros(nf * d, np.complex128)
    for i, b in enumerate(bins):
        up = np.zeros(nf * d, np.complex128)
        up[::d] = c[i]
        out += np.convolve(up, h)[:nf * d] * np.exp(2j * np.pi * ((b * n) % k) / k)
    return out / k
