"""CPU restatement of the audio output stage (step 7 of DESIGN.md section 2): arm_fir_interpolate_f32 of CMSIS-DSP 1.5.3 per channel and DSP
block behind the audio of a chain oracle (rxcommon.CpuChain), then arm_float_to_q15 (nr_oracle.float_to_q15, both roundings) and the mono /
stereo frame format of DSP_Out_Buff_Read (Core/Src/dsp_if.c:213-214: each sample written twice, left then right).

Two forms of the interpolator, equal bit for bit (tests/test_out_oracle.py):
  "c"   oracle/tx_oracle.c orc_fir_interpolate_f32 with arith = 0 (librx_oracle.so; pinned to the real function by tests/test_tx_oracle.py), one
        call per channel and DSP block;
  "np"  the same order vectorised in numpy -- per output one accumulator from +0.0f, t ascending, np.float32 product, then np.float32 sum --
        for the checks at full size.

TEST INFRASTRUCTURE.  Nothing here is imported by the product.
"""
import ctypes as C

import numpy as np

import nr_oracle as nro
import rxcommon as rc

f32 = np.float32
OUT_MONO, OUT_STEREO = 0, 1


def _lib():
    L = rc.oracle_lib()
    L.orc_fir_interpolate_f32.argtypes = [rc.f32p, C.c_uint32, C.c_uint32, rc.f32p, rc.f32p, rc.f32p, C.c_uint32, C.c_int]
    L.orc_fir_interpolate_f32.restype = None
    return L


class OutStage:
    """`channels` arm_fir_interpolate_instance_f32 (L = interp, pCoeffs = coeffs; no coefficients with interp 1: the samples pass as they are)
    and the frame format behind them.  `state` is [channels][P - 1], oldest first."""

    def __init__(self, channels, interp=1, coeffs=None, frames=OUT_MONO):
        self.C, self.L, self.frames = channels, int(interp), int(frames)
        self.coeffs = np.ascontiguousarray(coeffs if coeffs is not None else [], f32)
        assert self.coeffs.size % self.L == 0 and (self.coeffs.size or self.L == 1)
        self.P = self.coeffs.size // self.L
        self.state = np.zeros((channels, max(self.P - 1, 0)), f32)

    # -- the interpolator, two forms ---------------------------------------------------------
    def interp_c(self, x, na):
        """orc_fir_interpolate_f32(arith = 0): one call per channel and DSP block of `na` samples"""
        x = np.ascontiguousarray(x, f32)
        c, n = x.shape
        assert c == self.C and n % na == 0
        if not self.P:
            return x.copy()
        L, y = _lib(), np.empty((c, n * self.L), f32)
        st = np.zeros(self.P - 1 + na, f32)
        for ch in range(c):
            st[:self.P - 1] = self.state[ch]
            for b0 in range(0, n, na):
                src, dst = np.ascontiguousarray(x[ch, b0:b0 + na]), np.empty(na * self.L, f32)
                L.orc_fir_interpolate_f32(rc.fptr(self.coeffs), self.coeffs.size, self.L, rc.fptr(st), rc.fptr(src), rc.fptr(dst), na, 0)
                y[ch, b0 * self.L:(b0 + na) * self.L] = dst
            self.state[ch] = st[:self.P - 1]
        return y

    def interp_np(self, x):
        """the same order, every channel and sample at once (arm_fir_interpolate_f32.c:389-440 per output)"""
        x = np.ascontiguousarray(x, f32)
        c, n = x.shape
        assert c == self.C
        if not self.P:
            return x.copy()
        full = np.concatenate([self.state, x], axis=1)
        y = np.empty((c, n, self.L), f32)
        for ph in range(self.L):                                      # phase j - 1 = ph reads pCoeffs[(L - j) + t * L]
            acc = np.zeros((c, n), f32)
            for t in range(self.P):
                acc = np.add(acc, np.multiply(full[:, t:t + n], self.coeffs[(self.L - 1 - ph) + t * self.L]))
            y[:, :, ph] = acc
        self.state = full[:, n:].copy()
        return y.reshape(c, n * self.L)

    # -- int16 slots and frames -----------------------------------------------------------------
    def format(self, y, q15=False, rounding=False):
        out = nro.float_to_q15(y, rounding) if q15 else np.asarray(y, f32)
        return np.repeat(out, 2, axis=1) if self.frames == OUT_STEREO else out.copy()

    def process(self, audio, na=None, q15=False, rounding=False, form="np"):
        """the stage on the chain's audio [channels][n]: interpolate, [arm_float_to_q15], frames"""
        y = self.interp_np(audio) if form == "np" else self.interp_c(audio, na if na else np.asarray(audio).shape[1])
        return self.format(y, q15, rounding)


class StagedChain:
    """rxcommon.CpuChain + OutStage: what an instance with selenite_rx_set_out returns.  int16 slots: arm_q15_to_float on the input, the
    float chain, the stage, arm_float_to_q15 (cfg.q15_rounding) on the interpolated samples."""

    def __init__(self, spec, interp=1, coeffs=None, frames=OUT_MONO, form="c"):
        self.spec, self.form = spec, form
        self.chain = rc.CpuChain(spec, "orc")
        self.stage = OutStage(spec.channels, interp, coeffs, frames)
        self.na = spec.block // spec.decim

    def set_mode(self, mode):
        return self.chain.set_mode(mode)

    def audio(self, iq):
        return self.chain.process(iq)

    def process(self, iq):
        return self.stage.process(self.chain.process(iq), self.na, form=self.form)

    def process_q15(self, iq16):
        iq = np.divide(np.ascontiguousarray(iq16, np.int16).astype(f32), f32(32768.0))      # arm_q15_to_float.c:87
        return self.stage.process(self.chain.process(iq), self.na, q15=True, rounding=self.spec.q15_rounding, form=self.form)
