"""TEST ORACLE ONLY: numpy restatement of the keyed CW path of the TX chain (include/selenite_tx_cw.h, DESIGN.md section 2 "TX CW keyed").

One rounding per line, every float operation in f32 (numpy never contracts), denormals kept:

    e0[n] = key[n] ? 1.0f : +0.0f
    e[n]  = arm_fir_f32(shape, ns)(e0)         acc = +0.0f; acc = acc + w[n + k] * c[k], k ascending (w = the last ns - 1 key values, then e0)
    a[n]  = e[n] * amplitude
    u[m]  = arm_fir_interpolate_f32(a)         taken from the existing TX oracle (below)
    x = (float)(phase >> 8) * 0x1.921fb6p-22f;  out[m] = (arm_cos_f32(x) * u[m], arm_sin_f32(x) * u[m]);  phase += step_eff
    xs = (float)(side_phase >> 8) * 0x1.921fb6p-22f;  s = arm_sin_f32(xs);  g = e[n] * side_level;  y = s * g;  side_phase += side_step

tests/golden/txcw.npz (tests/golden/make_txcw_golden.py: the reference's own functions) pins it bit for bit (tests/test_txcw_oracle.py).
sin_f32 / cos_f32 / phase_arg / float_to_q15 are txfm_oracle's.

TxCwOracle follows an instance through keyed calls, audio calls in every mode (FM included), retunes, mode switches, reset and restored
state.  The keyed path shares the I rail of interp_state and nco_phase with the audio entries and leaves the front of the chain alone, so
the oracle keeps the chain in two parts.  The front (ALC, the arm_fir_f32 pair, the sideband select: fir_state, alc_gain) is one
rc.TxCpuChain with interp = 1 and no NCO, whose output is z = (I', +-Q') itself.  The interpolator is a second rc.TxCpuChain without ALC,
FIR pair and NCO, made afresh for every call and fed the rail's history in front of the new samples: arm_fir_interpolate_f32's pState
tail is the last P - 1 input samples verbatim, so this is the streaming filter on bits, and the history is an array the keyed path can
share.  tests/test_txcw_oracle.py pins this two-part oracle against TxFmOracle (one chain per rail) in every mode.
"""
import copy

import numpy as np

import rxcommon as rc
import txfm_oracle as fo
from txfm_oracle import cos_f32, float_to_q15, phase_arg, sin_f32

f32 = np.float32
M32 = np.uint64(0xFFFFFFFF)


def shape_env(window, coeffs):
    """arm_fir_f32: window = [ns - 1 of history | N new] e0 values (f32), coeffs [ns] CMSIS order -> e [N]"""
    window, coeffs = np.asarray(window, f32), np.asarray(coeffs, f32)
    ns = coeffs.size
    N = window.shape[-1] - (ns - 1)
    acc = np.zeros(window.shape[:-1] + (N,), f32)
    for k in range(ns):
        pr = window[..., k:k + N] * coeffs[k]
        acc = acc + pr
    return acc


def fma_f32(x, c, acc):
    """fmaf(x, c, acc) for f32 arrays: the product is exact in double (24 + 24 bits), the sum is rounded to odd in double (TwoSum gives
    the error) and then once to f32 -- 53 >= 2 * 24 + 2 bits make that the correctly rounded result"""
    p = np.asarray(x, f32).astype(np.float64) * np.asarray(c, f32).astype(np.float64)
    a = np.asarray(acc, f32).astype(np.float64)
    s = a + p
    bb = s - a
    err = (a - (s - bb)) + (p - bb)
    bits = s.view(np.int64).copy()
    odd = (bits & 1) == 1
    toward = (err > 0) == (s > 0)                                 # the exact sum lies further from zero than s
    fix = (err != 0) & ~odd
    bits = np.where(fix & toward, bits + 1, np.where(fix & ~toward, bits - 1, bits))
    return bits.view(np.float64).astype(f32)


def shape_env_fma(window, coeffs):
    """the same FIR with every tap fused (SELENITE_ARITH_FMA's loop): equal to shape_env on bits, because e0 is 0 or 1"""
    window, coeffs = np.asarray(window, f32), np.asarray(coeffs, f32)
    ns = coeffs.size
    N = window.shape[-1] - (ns - 1)
    acc = np.zeros(window.shape[:-1] + (N,), f32)
    for k in range(ns):
        acc = fma_f32(window[..., k:k + N], coeffs[k], acc)
    return acc


def sidetone(e, side_phase, side_step, side_level):
    """one channel: e [N] -> (y [N] f32, side_phase behind the last sample)"""
    e = np.asarray(e, f32)
    n = np.arange(e.size, dtype=np.uint64)
    sp = ((np.uint64(side_phase) + n * np.uint64(side_step)) & M32).astype(np.uint32)
    s = sin_f32(phase_arg(sp))
    g = e * f32(side_level)
    y = s * g
    return y, np.uint32((int(side_phase) + e.size * int(side_step)) & 0xFFFFFFFF)


def side_write(dst, y, mix, rounding=False):
    """the speaker mix: dst f32 (arm_add_f32) or int16 (arm_float_to_q15, arm_add_q15: saturating); returns the new buffer"""
    if dst.dtype == np.float32:
        return (dst + y) if mix else y.astype(f32)
    q = float_to_q15(y, rounding)
    if not mix:
        return q
    return np.clip(dst.astype(np.int32) + q.astype(np.int32), -32768, 32767).astype(np.int16)


def carrier(u, phase, step):
    """one channel: u [M] -> (out [M][2] f32, phase behind the last sample)"""
    u = np.asarray(u, f32)
    m = np.arange(u.size, dtype=np.uint64)
    ph = ((np.uint64(phase) + m * np.uint64(step)) & M32).astype(np.uint32)
    x = phase_arg(ph)
    out = np.stack([cos_f32(x) * u, sin_f32(x) * u], axis=-1)
    return out, np.uint32((int(phase) + u.size * int(step)) & 0xFFFFFFFF)


def breakin(keys, block, tx_on, hold, hang_blocks):
    """one channel: the KEY_TIMEOUT flag over the DSP blocks of a call"""
    tx_on, hold = int(tx_on), int(hold)
    for b in range(keys.size // block):
        if keys[b * block:(b + 1) * block].any():
            tx_on, hold = 1, int(hang_blocks)
        elif tx_on:
            if hold == 0:
                tx_on = 0
            else:
                hold -= 1
    return tx_on, hold


def keyed_sequential(keys, hist, coeffs, amplitude, side_phase, side_step, side_level):
    """One channel, sample by sample as the specification writes it (what the vectorised functions must equal; small N):
    -> (e, a, y, side_phase)."""
    coeffs = np.asarray(coeffs, f32)
    w = [f32(1.0) if v else f32(0.0) for v in hist]
    es, As, ys = [], [], []
    sp = int(side_phase)
    for kv in keys:
        w.append(f32(1.0) if kv else f32(0.0))
        acc = f32(0.0)
        for k in range(coeffs.size):
            acc = f32(acc + f32(w[len(w) - coeffs.size + k] * coeffs[k]))
        s = f32(sin_f32(phase_arg(np.uint32(sp))))
        g = f32(acc * f32(side_level))
        ys.append(f32(s * g))
        sp = (sp + int(side_step)) & 0xFFFFFFFF
        es.append(acc)
        As.append(f32(acc * f32(amplitude)))
    return np.array(es, f32), np.array(As, f32), np.array(ys, f32), np.uint32(sp)


def carrier_sequential(u, phase, step):
    out, phase = [], int(phase)
    for um in np.asarray(u, f32):
        x = phase_arg(np.uint32(phase))
        out.append((f32(cos_f32(x) * um), f32(sin_f32(x) * um)))
        phase = (phase + int(step)) & 0xFFFFFFFF
    return np.array(out, f32).reshape(-1, 2), np.uint32(phase)


def interpolate(spec, hist, x):
    """arm_fir_interpolate_f32 of the TX oracle on rails: hist [R][P - 1], x [R][N] -> (u [R][N * L], the new history).  cfg.arith of
    `spec` decides CMSIS / FMA (SPLIT16 runs as FMA)."""
    x = np.ascontiguousarray(x, f32)
    if not spec.ni_taps:
        return x.copy(), hist
    R, p1, L = x.shape[0], hist.shape[1], spec.interp
    s = rc.TxSpec(R, block=1, interp=L, ni_taps=spec.ni_taps, nh_taps=0, mode=rc.MODE_USB,
                  arith=rc.ARITH_CMSIS if spec.arith == rc.ARITH_CMSIS else rc.ARITH_FMA, nco=False, alc=False)
    s.ic = spec.ic
    ch = rc.TxCpuChain(s, "orc")
    assert ch.ok()
    full = np.ascontiguousarray(np.concatenate([hist, x], axis=1), f32)
    y = ch.process(full)
    return np.ascontiguousarray(y[:, p1 * L:, 0]), full[:, full.shape[1] - p1:].copy()


class TxCwOracle:
    """A TX instance followed through audio calls, keyed calls, mode switches, FM and CW settings, resets and restored state
    (module docstring).  spec: the rc.TxSpec of the instance (its taps are taken as they stand)."""

    def __init__(self, spec):
        self.spec = spec
        C_ = spec.channels
        self.mode = spec.mode
        self.p1 = (spec.ni_taps // spec.interp - 1) if spec.ni_taps else 0
        self.steps = np.zeros(C_, np.uint32)
        if spec.nco:
            self.steps[:] = spec.nco_steps if spec.nco_steps is not None else spec.nco_step_all
        self.fm_set = self.cw_set = False
        self.tone_phase = np.zeros(C_, np.uint32)
        self.reset()

    # ---- the front of the chain: one oracle instance with interp = 1 ----
    def _front(self):
        s = copy.copy(self.spec)
        s.interp, s.ni_taps, s.ic, s.nco = 1, 0, None, False
        s.mode = rc.MODE_USB
        self.front = rc.TxCpuChain(s, "orc")
        assert self.front.ok()
        self._front_mode()

    def _front_mode(self):
        assert self.front.set_mode(rc.MODE_USB if self.mode == rc.MODE_FM else self.mode) == 0

    def reset(self):
        """selenite_tx_reset: the mode and the FM / CW settings stay"""
        C_ = self.spec.channels
        self._front()
        self.ihist = np.zeros((C_, 2, self.p1), f32)
        self.phase = np.zeros(C_, np.uint32)
        self.tone_phase[:] = 0
        if self.cw_set:
            self._cw_clear(True)
        return 0

    def set_mode(self, mode):
        if mode == rc.MODE_FM and not self.fm_set:
            return rc.ARGUMENT_ERROR
        self.mode = mode
        self._front_mode()
        return 0

    def set_phase(self, phase):
        self.phase[:] = phase

    # ---- FM (as TxFmOracle) ----
    def set_fm(self, deviation, amplitude=1.0, tone_level=0.0, tone_steps=None):
        self.deviation, self.fm_amplitude, self.tone_level = deviation, amplitude, tone_level
        self.tone_on = tone_steps is not None
        self.tone_steps = np.zeros(self.spec.channels, np.uint32)
        if self.tone_on:
            self.tone_steps[:] = tone_steps
        if not self.fm_set:
            self.tone_phase[:] = 0
        self.fm_set = True
        return 0

    # ---- keyed CW ----
    def _cw_clear(self, everything):
        C_ = self.spec.channels
        self.key_state = np.zeros((C_, self.shape.size - 1), np.uint8)
        if everything:
            self.side_phase = np.zeros(C_, np.uint32)
            self.tx_on = np.zeros(C_, np.uint32)
            self.hold = np.zeros(C_, np.uint32)

    def set_cw(self, shape, amplitude=1.0, offset_step=0, side_level=0.0, side_step=0, side_mix=0, hang_blocks=0):
        """the first setting (or the first behind clear_cw) clears the CW state; a retune keeps it, a changed ns_taps clears key_state"""
        shape = np.ascontiguousarray(shape, f32).reshape(-1)
        new_len = not self.cw_set or shape.size != self.shape.size
        self.shape, self.amplitude, self.offset_step, self.side_level = shape, amplitude, int(offset_step), side_level
        self.side_steps = np.zeros(self.spec.channels, np.uint32)
        self.side_steps[:] = side_step
        self.side_mix, self.hang_blocks = int(side_mix), int(hang_blocks)
        if new_len:
            self._cw_clear(not self.cw_set)
        self.cw_set = True
        return 0

    def clear_cw(self):
        self.cw_set = False
        return 0

    def set_cw_state(self, a):
        for k in ("key_state", "side_phase", "tx_on", "hold"):
            if k in a:
                v = np.array(a[k], getattr(self, k).dtype)
                assert v.shape == getattr(self, k).shape
                setattr(self, k, (v != 0).astype(np.uint8) if k == "key_state" else v)

    def key_refused(self, block_size):
        """the status a keyed call of this length returns before it writes anything (the LDS budget is the kernel's, not restated)"""
        if not self.cw_set or self.mode not in (rc.MODE_CW, rc.MODE_CWR):
            return rc.ARGUMENT_ERROR
        if block_size == 0 or block_size % self.spec.block:
            return rc.LENGTH_ERROR
        return 0

    def process_key(self, keys, side=None, q15=False):
        """keys [channels][N] uint8 -> (I/Q [channels][N * L][2], sidetone buffer or None), f32 or (q15) int16.  `side` is the buffer the
        sidetone is stored or mixed into; it is not changed, the new one is returned."""
        keys = np.ascontiguousarray(keys, np.uint8)
        C_, N = keys.shape
        assert self.key_refused(N) == 0
        L = self.spec.interp
        window = np.concatenate([self.key_state, keys], axis=1) != 0
        e = shape_env(window.astype(f32), self.shape)
        self.last_e = e
        a = e * f32(self.amplitude)
        u, hi = interpolate(self.spec, self.ihist[:, 0], a)
        if self.p1:
            self.ihist = np.stack([hi, self._q_zero(N)], axis=1)
        off = self.offset_step if self.mode == rc.MODE_CW else (-self.offset_step) & 0xFFFFFFFF
        out = np.empty((C_, N * L, 2), f32)
        new_side = None if side is None else np.array(side)
        for c in range(C_):
            step = (int(self.steps[c]) + off) & 0xFFFFFFFF
            out[c], self.phase[c] = carrier(u[c], self.phase[c], step)
            y, self.side_phase[c] = sidetone(e[c], self.side_phase[c], self.side_steps[c], self.side_level)
            if side is not None:
                new_side[c] = side_write(new_side[c], y, self.side_mix, self.spec.q15_rounding)
            self.tx_on[c], self.hold[c] = breakin(keys[c], self.spec.block, self.tx_on[c], self.hold[c], self.hang_blocks)
        self.key_state = window[:, window.shape[1] - self.key_state.shape[1]:].astype(np.uint8)
        return (float_to_q15(out, self.spec.q15_rounding) if q15 else out), new_side

    def _q_zero(self, N):
        """the Q rail takes N samples of +0.0f"""
        q = np.concatenate([self.ihist[:, 1], np.zeros((self.spec.channels, N), f32)], axis=1)
        return q[:, q.shape[1] - self.p1:]

    # ---- the audio entries ----
    def process(self, audio):
        audio = np.ascontiguousarray(audio, f32)
        C_, N = audio.shape
        z = self.front.process(audio)                              # [C][N][2]: (I', +-Q'), AM (0.5 + 0.5 I', +0.0f)
        fm = self.mode == rc.MODE_FM
        if fm:
            u, hi = interpolate(self.spec, self.ihist[:, 0], z[:, :, 0])
            if self.p1:
                self.ihist = np.stack([hi, self._q_zero(N)], axis=1)
        else:
            rails = np.concatenate([z[:, :, 0], z[:, :, 1]], axis=0)
            u2, h2 = interpolate(self.spec, np.concatenate([self.ihist[:, 0], self.ihist[:, 1]], axis=0), rails)
            u, v = u2[:C_], u2[C_:]
            if self.p1:
                self.ihist = np.stack([h2[:C_], h2[C_:]], axis=1)
        M = u.shape[1]
        out = np.empty((C_, M, 2), f32)
        if fm:
            for c in range(C_):
                r = fo.fm_tail(u[c], self.phase[c], self.steps[c], self.deviation, self.fm_amplitude, self.tone_phase[c], self.tone_steps[c],
                               self.tone_on, self.tone_level)
                out[c] = r["out"]
                self.phase[c], self.tone_phase[c] = r["phase"][-1], r["tone_phase"]
        elif self.spec.nco:
            m = np.arange(M, dtype=np.uint64)
            for c in range(C_):
                ph = ((np.uint64(self.phase[c]) + m * np.uint64(self.steps[c])) & M32).astype(np.uint32)
                x = phase_arg(ph)
                lc, ls = cos_f32(x), sin_f32(x)
                a, b = u[c], v[c]
                ac, bd, ad, bc = a * lc, b * ls, a * ls, b * lc       # arm_cmplx_mult_cmplx_f32.c:186-187
                out[c, :, 0], out[c, :, 1] = ac - bd, ad + bc
                self.phase[c] = np.uint32((int(self.phase[c]) + M * int(self.steps[c])) & 0xFFFFFFFF)
        else:
            out[:, :, 0], out[:, :, 1] = u, v
        return out

    def process_q15(self, audio):
        a = np.ascontiguousarray(audio, np.int16).astype(f32) / f32(32768.0)             # arm_q15_to_float.c:87
        return float_to_q15(self.process(a), self.spec.q15_rounding)

    def state(self):
        sf = self.front.state()
        st = {"fir_state": sf["fir_state"], "interp_state": self.ihist.copy(), "alc_gain": sf["alc_gain"], "nco_phase": self.phase.copy(),
              "tone_phase": self.tone_phase.copy()}
        if self.cw_set:
            st.update(key_state=self.key_state.copy(), side_phase=self.side_phase.copy(), tx_on=self.tx_on.copy(), hold=self.hold.copy())
        return st
