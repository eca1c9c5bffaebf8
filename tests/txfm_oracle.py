"""TEST ORACLE ONLY: numpy restatement of the FM transmit mode of the TX chain (include/selenite_tx_fm.h, DESIGN.md section 2 "TX FM").

The FM tail, one rounding per line, every float operation in f32 (numpy never contracts), denormals kept:

    tone on:   xt = (float)(tone_phase >> 8) * 0x1.921fb6p-22f;  t = arm_sin_f32(xt) * tone_level;  w = u[n] + t;  tone_phase += tone_step
    tone off:  w = u[n]
    v = w * deviation;  d = arm_float_to_q31(v);  phase += (uint32_t)d
    x = (float)(phase >> 8) * 0x1.921fb6p-22f;  out[n] = (arm_cos_f32(x) * amplitude, arm_sin_f32(x) * amplitude);  phase += step

tests/golden/txfm.npz (tests/golden/make_txfm_golden.py: the reference's own arm_float_to_q31, arm_sin_f32, arm_cos_f32, arm_scale_f32 and
arm_add_f32) pins it bit for bit (tests/test_txfm_oracle.py).  The front of the chain -- ALC, arm_fir_f32 with the delay taps,
arm_fir_interpolate_f32 -- is the existing oracle's (rc.TxCpuChain over oracle/tx_oracle.c): a USB instance without NCO whose Hilbert taps
are all +0.0f has the FM instance's I rail and, bit for bit, its fir_state, interp_state and alc_gain.

TxFmOracle follows an instance through mode switches, FM settings (set_fm, clear_fm), reset() and a restored phase as well.  The two interpolator rails are independent filters, so two oracle instances
side by side give every rail of every mode: `b` (Hilbert taps +0.0f; AM while the mode is AM, else USB) the I rail, `a` (the instance's own
taps; AM while the mode is FM, so that its Q rail takes +0.0f) the Q rail.  The up-mix of the other modes is restated here too
(arm_cmplx_mult_cmplx_f32.c:186-187), because the phase accumulator is shared with FM.
"""
import copy
import os

import numpy as np

import rxcommon as rc

f32 = np.float32
K = f32(float.fromhex("0x1.921fb6p-22"))        # 2 pi / 2^24
INV2PI = f32(0.159154943092)                    # arm_sin_f32.c:88, arm_cos_f32.c:81
_table = None


def table():
    global _table
    if _table is None:
        _table = np.fromfile(os.path.join(rc.GOLDEN_DIR, "sintable_f32.bin"), f32)
        assert _table.shape == (513,)
    return _table


def _lookup(p):
    """arm_sin_f32.c:88-118 behind `in = x * 0.159154943092f` for in >= 0 (x comes from an unsigned phase)"""
    T = table()
    n = p.astype(np.int32)
    i = p - n.astype(f32)
    findex = f32(512.0) * i
    index = findex.astype(np.uint16).astype(np.uint32) & np.uint32(0x1FF)
    fract = findex - index.astype(f32)
    a, b = T[index], T[index + 1]
    w = f32(1.0) - fract
    return w * a + fract * b


def sin_f32(x):
    x = np.asarray(x, f32)
    assert (x >= 0).all()
    return _lookup(x * INV2PI)


def cos_f32(x):
    x = np.asarray(x, f32)
    assert (x >= 0).all()
    return _lookup(x * INV2PI + f32(0.25))


def phase_arg(phase):
    return (np.asarray(phase, np.uint32) >> np.uint32(8)).astype(f32) * K


def float_to_q31(v):
    """arm_float_to_q31.c:129 (ARM_MATH_ROUNDING off): clip_q63_to_q31((q63_t)(in * 2147483648.0f)); NaN -> 0 [build-defined]"""
    s = (np.asarray(v, f32) * f32(2147483648.0)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        t = np.clip(np.trunc(s), -2147483648.0, 2147483647.0)
    t = np.where(np.isnan(s), 0.0, t)
    return t.astype(np.int64).astype(np.int32)


def float_to_q15(x, rounding):
    """arm_float_to_q15.c:117 (truncating: the firmware's build) / :90-101 (ARM_MATH_ROUNDING)"""
    v = np.asarray(x, f32) * f32(32768.0)
    if rounding:
        v = v + np.where(v > 0, f32(0.5), f32(-0.5)).astype(f32)
    with np.errstate(invalid="ignore"):
        t = np.clip(np.trunc(v.astype(np.float64)), -32768.0, 32767.0)
    return np.where(np.isnan(v), 0.0, t).astype(np.int16)


def fm_tail(u, phase, step, deviation, amplitude, tone_phase=0, tone_step=0, tone_on=False, tone_level=0.0):
    """One channel: u [N] f32 -> dict(out [N][2] f32, d [N] int32, phase [N] uint32 behind every sample, tone_phase behind the last)."""
    u = np.asarray(u, f32)
    N = u.size
    n = np.arange(N, dtype=np.uint64)
    w = u
    if tone_on:
        tp = ((np.uint64(tone_phase) + n * np.uint64(tone_step)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        t = sin_f32(phase_arg(tp)) * f32(tone_level)
        w = u + t
        tone_phase = int((int(tone_phase) + N * int(tone_step)) & 0xFFFFFFFF)
    v = w * f32(deviation)
    d = float_to_q31(v)
    inc = d.astype(np.int64).astype(np.uint64) + np.uint64(step)         # two's complement: the sum is taken modulo 2^32 below
    after = (np.uint64(phase) + np.cumsum(inc, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    used = ((after - np.uint64(step)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    x = phase_arg(used)
    out = np.stack([cos_f32(x) * f32(amplitude), sin_f32(x) * f32(amplitude)], axis=-1)
    return {"out": out, "d": d, "phase": after.astype(np.uint32), "tone_phase": np.uint32(tone_phase)}


def fm_tail_sequential(u, phase, step, deviation, amplitude, tone_phase=0, tone_step=0, tone_on=False, tone_level=0.0):
    """The same, sample by sample as the specification writes it (what fm_tail's prefix sums must equal; small N)."""
    out, ds, phs = [], [], []
    phase, tone_phase = int(phase), int(tone_phase)
    for un in np.asarray(u, f32):
        w = f32(un)
        if tone_on:
            w = w + sin_f32(phase_arg(np.uint32(tone_phase))) * f32(tone_level)
            tone_phase = (tone_phase + int(tone_step)) & 0xFFFFFFFF
        d = int(float_to_q31(f32(w) * f32(deviation)))
        phase = (phase + d) & 0xFFFFFFFF
        x = phase_arg(np.uint32(phase))
        out.append((cos_f32(x) * f32(amplitude), sin_f32(x) * f32(amplitude)))
        phase = (phase + int(step)) & 0xFFFFFFFF
        ds.append(d)
        phs.append(phase)
    return {"out": np.array(out, f32).reshape(-1, 2), "d": np.array(ds, np.int32), "phase": np.array(phs, np.uint32),
            "tone_phase": np.uint32(tone_phase)}


class TxFmOracle:
    """A TX instance followed through calls, mode switches, FM settings and resets (module docstring).
    spec: the rc.TxSpec the instance was created from -- its taps (spec.delay, spec.hilb, spec.ic) are taken as they stand, so a test may
    overwrite them before it builds the instance and the oracle; deviation: None leaves FM unconfigured (set_mode(MODE_FM) is then refused
    as selenite_tx_set_mode refuses it); tone_steps: [channels], one value for all, or None (tone off)."""

    def __init__(self, spec, deviation=None, amplitude=1.0, tone_level=0.0, tone_steps=None):
        self.spec = spec
        C_ = spec.channels
        self.mode = spec.mode
        self._chains()
        self.steps = np.zeros(C_, np.uint32)
        if spec.nco:
            self.steps[:] = spec.nco_steps if spec.nco_steps is not None else spec.nco_step_all
        self.phase = np.zeros(C_, np.uint32)
        self.tone_phase = np.zeros(C_, np.uint32)
        self.fm_set = False
        if deviation is not None:
            self.set_fm(deviation, amplitude, tone_level, tone_steps)
        self.last_d = None

    def _chains(self):
        """both inner chains new (zero filter state, alc_gain = gain_init) in the current mode"""
        sa, sb = copy.copy(self.spec), copy.copy(self.spec)
        sa.nco = sb.nco = False
        sa.mode = sb.mode = rc.MODE_USB
        if self.spec.nh_taps:
            sb.hilb = np.zeros(self.spec.nh_taps, f32)
        self.a, self.b = rc.TxCpuChain(sa, "orc"), rc.TxCpuChain(sb, "orc")
        assert self.a.ok() and self.b.ok()
        self._inner_modes()

    def _inner_modes(self):
        assert self.a.set_mode(rc.MODE_AM if self.mode == rc.MODE_FM else self.mode) == 0
        assert self.b.set_mode(rc.MODE_AM if self.mode == rc.MODE_AM else rc.MODE_USB) == 0

    def set_fm(self, deviation, amplitude=1.0, tone_level=0.0, tone_steps=None):
        """a retune: tone_phase stays; the first setting (or the first behind clear_fm) starts the tone at phase 0"""
        self.deviation, self.amplitude, self.tone_level = deviation, amplitude, tone_level
        self.tone_on = tone_steps is not None
        self.tone_steps = np.zeros(self.spec.channels, np.uint32)
        if self.tone_on:
            self.tone_steps[:] = tone_steps
        if not self.fm_set:
            self.tone_phase[:] = 0
        self.fm_set = True
        return 0

    def clear_fm(self):
        """selenite_tx_set_fm(S, NULL): refused while the mode is FM"""
        if self.mode == rc.MODE_FM:
            return rc.ARGUMENT_ERROR
        self.fm_set = False
        return 0

    def reset(self):
        """selenite_tx_reset: filter states, gains and both phases as in a new instance; the mode and the FM setting stay"""
        self._chains()
        self.phase[:] = 0
        self.tone_phase[:] = 0
        return 0

    def set_phase(self, phase):
        """selenite_tx_set_state with nco_phase alone changed"""
        self.phase[:] = phase

    def set_mode(self, mode):
        if mode == rc.MODE_FM and not self.fm_set:
            return rc.ARGUMENT_ERROR
        self.mode = mode
        self._inner_modes()
        return 0

    def process(self, audio):
        audio = np.ascontiguousarray(audio, f32)
        ya, yb = self.a.process(audio), self.b.process(audio)
        C_, N = yb.shape[0], yb.shape[1]
        out = np.empty((C_, N, 2), f32)
        if self.mode == rc.MODE_FM:
            self.last_d = np.empty((C_, N), np.int32)
            for c in range(C_):
                r = fm_tail(yb[c, :, 0], self.phase[c], self.steps[c], self.deviation, self.amplitude, self.tone_phase[c], self.tone_steps[c],
                            self.tone_on, self.tone_level)
                out[c], self.last_d[c] = r["out"], r["d"]
                self.phase[c], self.tone_phase[c] = r["phase"][-1], r["tone_phase"]
        elif self.spec.nco:
            n = np.arange(N, dtype=np.uint64)
            for c in range(C_):
                ph = ((np.uint64(self.phase[c]) + n * np.uint64(self.steps[c])) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
                x = phase_arg(ph)
                lc, ls = cos_f32(x), sin_f32(x)
                a, b = yb[c, :, 0], ya[c, :, 1]
                ac, bd, ad, bc = a * lc, b * ls, a * ls, b * lc
                out[c, :, 0], out[c, :, 1] = ac - bd, ad + bc
                self.phase[c] = np.uint32((int(self.phase[c]) + N * int(self.steps[c])) & 0xFFFFFFFF)
        else:
            out[:, :, 0], out[:, :, 1] = yb[:, :, 0], ya[:, :, 1]
        return out

    def process_q15(self, audio):
        a = np.ascontiguousarray(audio, np.int16).astype(f32) / f32(32768.0)             # arm_q15_to_float.c:87
        return float_to_q15(self.process(a), self.spec.q15_rounding)

    def state(self):
        sa, sb = self.a.state(), self.b.state()
        assert rc.identical(sa["fir_state"], sb["fir_state"]) and rc.identical(sa["alc_gain"], sb["alc_gain"])
        ist = sb["interp_state"].copy()
        if ist.size:
            ist[:, 1] = sa["interp_state"][:, 1]
        return {"fir_state": sb["fir_state"], "interp_state": ist, "alc_gain": sb["alc_gain"], "nco_phase": self.phase.copy(),
                "tone_phase": self.tone_phase.copy()}
