"""The spectrum tap restated in numpy, vectorised over channels and frames: framing of the stream,
the pending frame, the stride, arm_cmplx_mult_real_f32, arm_cfft_f32 for the pure radix-8 lengths (arm_radix8_butterfly_f32 + the base-8 digit
reversal that arm_bitreversal_32 performs with armBitRevIndexTable64 / 512), arm_cmplx_mag_squared_f32, the averaging and the display order.
Every float32 operation of the reference is one numpy float32 operation here, in the reference's order; tests/test_spectrum_oracle.py pins
it bit for bit to tests/golden/spectrum.npz.

TEST INFRASTRUCTURE.  Nothing here is imported by the product."""
import numpy as np

F32 = np.float32
C81 = F32(0.70710678118)          # arm_cfft_radix8_f32.c:62


def twiddles(n):
    """twiddleCoef_n as CommonTables/arm_common_tables.c holds it: the float of the nine-decimal rendering of cos / sin(2 pi i / n)"""
    a = 2.0 * np.pi * np.arange(n) / n
    return np.array([[F32(float("%.9f" % np.cos(v))), F32(float("%.9f" % np.sin(v)))] for v in a], F32)


def digit_reversal(n):
    """perm[k] = the position that holds bin k behind the passes: k with its base-8 digits reversed"""
    nd = {64: 2, 512: 3}[n]
    k = np.arange(n)
    out = np.zeros(n, np.int64)
    for d in range(nd):
        out = out * 8 + (k >> (3 * d)) % 8
    return out


def _bfly8(xr, xi):
    """the sums of both butterfly forms (arm_cfft_radix8_f32.c:74-132 / :175-251); xr, xi: lists of the eight elements' parts"""
    r1, r5 = xr[0] + xr[4], xr[0] - xr[4]
    r2, r6 = xr[1] + xr[5], xr[1] - xr[5]
    r3, r7 = xr[2] + xr[6], xr[2] - xr[6]
    r4, r8 = xr[3] + xr[7], xr[3] - xr[7]
    t1 = r1 - r3
    r1 = r1 + r3
    r3 = r2 - r4
    r2 = r2 + r4
    s1, s5 = xi[0] + xi[4], xi[0] - xi[4]
    s2, s6 = xi[1] + xi[5], xi[1] - xi[5]
    s3, s7 = xi[2] + xi[6], xi[2] - xi[6]
    s4, s8 = xi[3] + xi[7], xi[3] - xi[7]
    t2 = s1 - s3
    s1 = s1 + s3
    s3 = s2 - s4
    s2 = s2 + s4
    yr, yi = [None] * 8, [None] * 8
    yr[0], yi[0] = r1 + r2, s1 + s2
    yr[4], yi[4] = r1 - r2, s1 - s2
    yr[2], yi[2] = t1 + s3, t2 - r3
    yr[6], yi[6] = t1 - s3, t2 + r3
    q1 = (r6 - r8) * C81
    r6 = (r6 + r8) * C81
    q2 = (s6 - s8) * C81
    s6 = (s6 + s8) * C81
    t1 = r5 - q1
    r5 = r5 + q1
    r8 = r7 - r6
    r7 = r7 + r6
    t2 = s5 - q2
    s5 = s5 + q2
    s8 = s7 - s6
    s7 = s7 + s6
    yr[1], yi[1] = r5 + s7, s5 - r7
    yr[7], yi[7] = r5 - s7, s5 + r7
    yr[5], yi[5] = t1 + s8, t2 - r8
    yr[3], yi[3] = t1 - s8, t2 + r8
    return yr, yi


def radix8(re, im, tw):
    """arm_radix8_butterfly_f32(p, n, tw, 1) on [..., n] arrays of the parts (returns new arrays, output digit-reversed)"""
    n = re.shape[-1]
    lead = re.shape[:-1]
    re, im = re.astype(F32).copy(), im.astype(F32).copy()
    n2, mod = n, 1
    with np.errstate(all="ignore"):
        while True:
            n1, n2 = n2, n2 >> 3
            vr, vi = re.reshape(lead + (n // n1, 8, n2)), im.reshape(lead + (n // n1, 8, n2))      # [.., i1 / n1, m, j]: element i1 + m * n2 + j
            yr, yi = _bfly8([vr[..., m, :] for m in range(8)], [vi[..., m, :] for m in range(8)])
            if n2 >= 8:
                # columns j >= 1: element m times (co, si)[m * j * mod] (:146-168, :214-275); column 0 keeps the sums (:72-135)
                j = np.arange(n2)
                for m in range(1, 8):
                    co, si = tw[m * j * mod, 0], tw[m * j * mod, 1]
                    p1, p2, p3, p4 = co * yr[m], si * yi[m], co * yi[m], si * yr[m]
                    tr, ti = p1 + p2, p3 - p4
                    tr[..., 0], ti[..., 0] = yr[m][..., 0], yi[m][..., 0]
                    yr[m], yi[m] = tr, ti
            re = np.stack(yr, axis=-2).reshape(lead + (n,))
            im = np.stack(yi, axis=-2).reshape(lead + (n,))
            if n2 < 8:
                return re, im
            mod <<= 3


def cfft(frames, tw=None):
    """arm_cfft_f32(&arm_cfft_sR_f32_lenN, frame, 0, 1) on [..., n, 2]: forward, natural-order output"""
    n = frames.shape[-2]
    re, im = radix8(frames[..., 0], frames[..., 1], twiddles(n) if tw is None else tw)
    perm = digit_reversal(n)
    return np.stack([re[..., perm], im[..., perm]], axis=-1)


def power(frames, window=None, tw=None):
    """window -> transform -> arm_cmplx_mag_squared_f32 on [..., n, 2]; returns (fft [..., n, 2], power [..., n]) in natural order"""
    x = np.asarray(frames, F32)
    with np.errstate(all="ignore"):
        if window is not None:
            x = x * np.asarray(window, F32)[:, None]            # arm_cmplx_mult_real_f32: re * w, im * w
        y = cfft(x, tw)
        re2, im2 = y[..., 0] * y[..., 0], y[..., 1] * y[..., 1]
        return y, re2 + im2


def q15_to_float(q):
    return np.divide(np.asarray(q).astype(F32), F32(32768.0))   # arm_q15_to_float


class Spectrum:
    """the stage of selenite_rx_set_spectrum; state as selenite_rx_spec_state_view has it"""

    def __init__(self, channels, fft_len, stride=1, average=0, alpha=1.0, window=None):
        self.c, self.n, self.stride, self.average, self.alpha = channels, fft_len, stride, average, F32(alpha)
        self.window = None if window is None else np.asarray(window, F32)
        self.tw = twiddles(fft_len)
        self.reset()

    def reset(self):
        self.rows = np.zeros((self.c, self.n), F32)
        self.pending = np.zeros((self.c, self.n, 2), F32)
        self.position = 0

    @property
    def frames(self):
        return (self.position // self.n + self.stride - 1) // self.stride

    def process(self, iq):
        """one call's input [channels][L][2], f32 or int16"""
        x = q15_to_float(iq) if np.asarray(iq).dtype == np.int16 else np.asarray(iq, F32)
        n, L = self.n, x.shape[1]
        off, f0 = self.position % n, self.position // n
        nfr = (off + L) // n
        todo = []
        for i in range(nfr):
            if (f0 + i) % self.stride:
                continue                                       # skipped frames are never read
            v0 = i * n - off
            todo.append(np.concatenate([self.pending[:, :off], x[:, :v0 + n]], axis=1) if v0 < 0 else x[:, v0:v0 + n])
        if todo:
            _, p = power(np.stack(todo, axis=1), self.window, self.tw)      # [C][F][n]
            half = n // 2
            with np.errstate(all="ignore"):
                for f in range(p.shape[1]):
                    pd = np.roll(p[:, f], half, axis=-1)       # display order: bin k at (k + n / 2) mod n
                    if self.average:
                        d = pd - self.rows
                        s = self.alpha * d
                        self.rows = self.rows + s
                    else:
                        self.rows = pd.copy()
        vt = nfr * n - off
        if vt < L and (f0 + nfr) % self.stride == 0:           # the frame the call ends in waits, when it will be transformed
            lo = max(vt, 0)
            self.pending[:, lo - vt:L - vt] = x[:, lo:L]
        self.position += L
        return self.rows

    def state(self):
        return dict(rows=self.rows.copy(), pending=self.pending.copy(), position=np.array([self.position], np.uint64))

    def set_state(self, d):
        self.rows, self.pending, self.position = d["rows"].copy(), d["pending"].copy(), int(d["position"][0])
