"""numpy float32 restatement of the NLMS stage (step 4b of DESIGN.md section 2) and of what follows it: the delay line,
arm_lms_norm_f32 of CMSIS-DSP 1.5.3 (FilteringFunctions/arm_lms_norm_f32.c:196-348, the ARM_MATH_DSP branch that -DARM_MATH_CM4
selects; init arm_lms_norm_init_f32.c:60-89), the AGC law (DESIGN.md "AGC"; oracle/rx_oracle.c) and arm_float_to_q15 (truncating and
ARM_MATH_ROUNDING).  Vectorised over channels, sequential over samples and taps; every operation is one float32 ufunc, so the
rounding is the reference's (products, then sums in tap order, a correctly rounded division, nothing fused).

TEST INFRASTRUCTURE.  Nothing here is imported by the product.
"""
import numpy as np

f32 = np.float32
EPS = f32(0.000000119209289)          # arm_lms_norm_f32.c:258
NR_OFF, NR_DENOISE, NR_NOTCH = 0, 1, 2


class Nlms:
    """`channels` arm_lms_norm_instance_f32 (one per channel) behind a delay line of `delay` samples (0: no delay line)."""

    def __init__(self, channels, num_taps, mu, coeffs_init=None, delay=0):
        c, n = channels, num_taps
        self.N, self.D, self.mu = n, delay, f32(mu)
        init = np.zeros(n, f32) if coeffs_init is None else np.asarray(coeffs_init, f32)
        self.coeffs = np.tile(init, (c, 1))                 # init.c:72 pCoeffs (the caller's array)
        self.window = np.zeros((c, n - 1), f32)             # init.c:75 the state buffer is cleared
        self.energy = np.zeros(c, f32)                      # init.c:84
        self.x0 = np.zeros(c, f32)                          # init.c:87
        self.delay = np.zeros((c, delay), f32)

    def lms(self, src, ref):
        """arm_lms_norm_f32(S, pSrc = src, pRef = ref, pOut, pErr, n) per channel: returns (pOut, pErr)."""
        src, ref = np.asarray(src, f32), np.asarray(ref, f32)
        c, nsamp = src.shape
        y, err = np.empty((c, nsamp), f32), np.empty((c, nsamp), f32)
        w, energy, x0, mu = self.coeffs, self.energy, self.x0, self.mu
        px = np.concatenate([self.window, np.zeros((c, 1), f32)], axis=1)
        for i in range(nsamp):
            inp = src[:, i]
            px[:, self.N - 1] = inp                                        # :201 *pStateCurnt++ = *pSrc
            energy = np.subtract(energy, np.multiply(x0, x0))             # :213 energy -= x0 * x0
            energy = np.add(energy, np.multiply(inp, inp))                # :214 energy += in * in
            s = np.zeros(c, f32)                                           # :217 sum = 0.0f
            for k in range(self.N):                                        # :220-245 sum += (*px++) * (*pb++), tap order
                s = np.add(s, np.multiply(px[:, k], w[:, k]))
            y[:, i] = s                                                    # :248 *pOut++ = sum
            e = np.subtract(ref[:, i], s)                                  # :251-252 e = d - sum
            err[:, i] = e
            wf = np.divide(np.multiply(e, mu), np.add(energy, EPS))        # :258 w = (e * mu) / (energy + 0.000000119209289f)
            w = np.add(w, np.multiply(wf[:, None], px))                    # :267-297 *pb += w * (*px++), every tap independent
            x0 = px[:, 0].copy()                                           # :299 x0 = *pState
            px[:, :self.N - 1] = px[:, 1:].copy()                          # :302 pState + 1 (and :315-346 the copy-back)
        self.coeffs, self.energy, self.x0 = w, energy, x0
        self.window = px[:, :self.N - 1].copy()
        return y, err

    def process(self, x, kind):
        """The stage on un-scaled audio x [channels][n]: u[n] = x[n - D], arm_lms_norm_f32(u, x); DENOISE -> y, NOTCH -> e."""
        x = np.asarray(x, f32)
        full = np.concatenate([self.delay, x], axis=1)
        u = full[:, :x.shape[1]]
        self.delay = full[:, full.shape[1] - self.D:].copy()
        y, e = self.lms(u, x)
        return y if kind == NR_DENOISE else e

    def state(self):
        return dict(coeffs=self.coeffs.copy(), window=self.window.copy(), delay=self.delay.copy(),
                    energy=self.energy.copy(), x0=self.x0.copy())

    def set_state(self, d):
        for k, v in d.items():
            setattr(self, k, np.array(v, f32))


class Agc:
    """The AGC law per DSP block of `na` audio samples (oracle/rx_oracle.c, statement for statement; DESIGN.md "AGC"):
    env = max |a| (arm_abs_f32 + arm_max_f32), e = max(env, floor), d = target / e clamped to [gain_min, gain_max],
    gain += rate * (d - gain) with rate = attack when the gain falls, decay otherwise; the block is scaled by the new gain.
    agc_global: env = the maximum over all channels (orc_rx_process_f32_env); process(a, env=...) takes the blocks' maxima from the caller."""

    def __init__(self, channels, na, params, agc_global=False):
        self.na, self.agc_global = na, agc_global
        p = {k: f32(v) for k, v in params.items()}
        self.p = p
        self.gain = np.full(channels, p["gain_init"], f32)

    def process(self, a, env=None):
        a = np.asarray(a, f32)
        p, out = self.p, np.empty_like(a)
        g = self.gain
        for b0 in range(0, a.shape[1], self.na):
            blk = a[:, b0:b0 + self.na]
            m = np.max(np.abs(blk), axis=1)
            if self.agc_global:
                m = np.full_like(m, m.max())
            if env is not None:
                m = np.full_like(m, f32(env[b0 // self.na]))
            e = np.where(m < p["env_floor"], p["env_floor"], m)
            with np.errstate(divide="ignore"):
                d = np.divide(p["target"], e)          # (floor 0 and a silent block: +inf, clamped to gain_max below -- as the oracle)
            d = np.where(d > p["gain_max"], p["gain_max"], d)
            d = np.where(d < p["gain_min"], p["gain_min"], d)
            diff = np.subtract(d, g)
            rate = np.where(diff < f32(0), p["attack"], p["decay"])
            g = np.add(g, np.multiply(rate, diff))
            out[:, b0:b0 + self.na] = np.multiply(blk, g[:, None])
        self.gain = g
        return out


def float_to_q15(a, rounding=False):
    """arm_float_to_q15 (SupportFunctions/arm_float_to_q15.c:117 truncating; :90-101 the ARM_MATH_ROUNDING variant)."""
    v = np.multiply(np.asarray(a, f32), f32(32768.0))
    if rounding:
        v = np.add(v, np.where(v > f32(0), f32(0.5), f32(-0.5)))
    return np.clip(np.trunc(v), -32768, 32767).astype(np.int16)
