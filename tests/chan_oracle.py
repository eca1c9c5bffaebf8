"""The polyphase channeliser (include/selenite_chan.h) restated in numpy, vectorised over bands and outputs: the
window of K P samples per output, arm_dot_prod_f32 per FFT position and rail (acc = +0.0f; acc = acc + g * s, product rounded, then the
sum, t ascending), the rotation by n0, and arm_cfft_f32 (spectrum_oracle.cfft, pinned to the reference by tests/test_spectrum_oracle.py).
Every float32 operation of the composition is one numpy float32 operation here, in its order; tests/test_chan_oracle.py pins it bit for bit
to tests/golden/chan.npz.  direct64() is the float64 direct form (mix, filter, decimate) the composition is measured against.

TEST INFRASTRUCTURE.  Nothing here is imported by the product."""
import numpy as np

import spectrum_oracle as so

F32 = np.float32


class Channelizer:
    """the object of selenite_chan_init; state as selenite_chan_state_view has it"""

    def __init__(self, bands, fft_len, oversample, taps_per_branch, coeffs, bins=None):
        self.bands, self.k, self.ovs, self.p = bands, fft_len, oversample, taps_per_branch
        self.d = fft_len // oversample
        self.hlen = fft_len * taps_per_branch - self.d
        self.g = np.asarray(coeffs, F32).reshape(taps_per_branch, fft_len)          # g[t][r] = g[r + t K]
        self.bins = np.arange(fft_len) if bins is None else np.asarray(bins, np.int64)
        self.tw = so.twiddles(fft_len)
        self.reset()

    def reset(self):
        self.history = np.zeros((self.bands, self.hlen, 2), F32)
        self.position = 0

    def out_len(self, block_size):
        return block_size // self.d

    def process(self, iq):
        """one call's input [bands][L][2], f32 or int16; returns [bands * n_bins][L / D][2]"""
        x = so.q15_to_float(iq) if np.asarray(iq).dtype == np.int16 else np.asarray(iq, F32)
        k, p, d = self.k, self.p, self.d
        L = x.shape[1]
        assert x.shape[0] == self.bands and L > 0 and L % d == 0
        nout = L // d
        buf = np.concatenate([self.history, x], axis=1)                             # window of output m: buf[:, m D : m D + K P]
        out = np.empty((self.bands, len(self.bins), nout, 2), F32)
        with np.errstate(all="ignore"):
            for m0 in range(0, nout, 64):                                           # (in pieces: bounded memory at K = 512)
                ms = np.arange(m0, min(nout, m0 + 64))
                idx = (ms[:, None] * d + np.arange(k * p)[None, :])                 # [m][r + t K]
                s = buf[:, idx].reshape(self.bands, len(ms), p, k, 2)
                acc = np.zeros((self.bands, len(ms), k, 2), F32)
                for t in range(p):
                    prod = self.g[t][None, None, :, None] * s[:, :, t]
                    acc = acc + prod
                v = np.empty_like(acc)
                for i, m in enumerate(ms):
                    n0 = (self.position + (int(m) + 1) * d) % k
                    v[:, i] = np.roll(acc[:, i], n0, axis=1)                        # v[(r + n0) mod K] = acc[r]
                y = so.cfft(v, self.tw)                                             # [bands][m][K][2]
                out[:, :, ms - 0] = np.transpose(y[:, :, self.bins], (0, 2, 1, 3))
        self.history = buf[:, L:].copy()
        self.position += L
        return out.reshape(self.bands * len(self.bins), nout, 2)

    def state(self):
        return dict(history=self.history.copy(), position=np.array([self.position], np.uint64))

    def set_state(self, d):
        self.history, self.position = np.asarray(d["history"], F32).copy(), int(d["position"][0])


def direct64(x, coeffs, fft_len, oversample, bins=None):
    """float64 direct form on a whole stream x [L][2] (zeros in front): channel k = x[n] e^(-2 pi i k n / K) filtered by h
    (coeffs[j] = h[K P - 1 - j]), every D-th output kept, the first at n = D - 1.  Returns complex128 [n_bins][L / D]."""
    k, d = fft_len, fft_len // oversample
    g = np.asarray(coeffs, np.float64)
    n_taps = len(g)
    z = np.asarray(x, np.float64)
    z = z[:, 0] + 1j * z[:, 1]
    L = len(z)
    zp = np.concatenate([np.zeros(n_taps - 1, np.complex128), z])
    n = np.arange(-(n_taps - 1), L)
    bins = np.arange(k) if bins is None else np.asarray(bins)
    ends = np.arange(d - 1, L, d)                                                   # stream index of the newest sample of each output
    out = np.empty((len(bins), len(ends)), np.complex128)
    for i, b in enumerate(bins):
        mixed = zp * np.exp(-2j * np.pi * ((b * n) % k) / k)
        win = np.lib.stride_tricks.sliding_window_view(mixed, n_taps)[ends]         # [m][j]: samples ends - (n_taps - 1) + j
        out[i] = win @ g
    return out
