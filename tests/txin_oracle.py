"""TEST ORACLE ONLY: numpy restatement of the audio input stage of the TX chain (include/selenite_tx_in.h, DESIGN.md section 2 "TX input"),
call by call, with state.  One rounding per line, every float operation in f32 (numpy never contracts), denormals kept:

    int16:  x = (float)w / 32768.0f                              arm_q15_to_float.c:87
    pick:   MONO s = x[i];  LEFT s = x[2i];  RIGHT s = x[2i + 1];  MIX t = x[2i] + x[2i + 1];  s = t * 0.5f     (arm_add_f32, arm_scale_f32)
    g = s * gain                                                 arm_scale_f32
    st = {the last nd_taps - 1 values of g before the call} ++ g
    a[n] = sum over k ascending of st[n M + k] * coeffs[k]       arm_fir_decimate_f32.c: acc = +0.0f; acc = acc + x * c (product rounded,
                                                                 then the sum); M == 1 and nd_taps == 0: a = g
    VOX per DSP block of `block` samples of a: tests/meter_oracle.py with sense ABOVE (arm_power_f32, the division, the law)
    gate == 1: a block whose open is 0 after its update becomes +0.0f
    int16 chain: q = arm_float_to_q15(a) under q15_rounding

tests/golden/txin.npz (tests/golden/make_txin_golden.py: the reference's own arm_q15_to_float, arm_add_f32, arm_scale_f32,
arm_fir_decimate_f32, arm_power_f32 and arm_float_to_q15) pins it bit for bit (tests/test_txin_oracle.py).  The rest of a frame call is the
audio entry on the stage's output: TxInOracle hands it to tests/txcw_oracle.py's TxCwOracle (which follows tx_oracle.c through modes, FM and
keyed calls), so that an instance can be followed through frame calls, audio calls, keyed calls, mode switches, settings and resets."""
import numpy as np

import meter_oracle as mo
import rxcommon as rc
import txcw_oracle as co
from txfm_oracle import float_to_q15

f32 = np.float32
MONO, LEFT, RIGHT, MIX = 0, 1, 2, 3
K_F32, K_Q15, K_Q15_F32 = 0, 1, 2                  # the three device entries: frame type -> I/Q type


def q15_to_float(w):
    return np.asarray(w, np.int16).astype(f32) / f32(32768.0)


def pick_frames(x, pick):
    """x [C][words] f32 -> s [C][samples]"""
    x = np.asarray(x, f32)
    if pick == MONO:
        return x
    l, r = x[:, 0::2], x[:, 1::2]
    if pick == LEFT:
        return np.ascontiguousarray(l)
    if pick == RIGHT:
        return np.ascontiguousarray(r)
    with np.errstate(all="ignore"):
        t = l + r
        return t * f32(0.5)


def fir_decimate(hist, g, coeffs, M):
    """arm_fir_decimate_f32 on rows: hist [C][nt - 1], g [C][N M] -> (a [C][N], the new history)"""
    g = np.asarray(g, f32)
    nt = len(coeffs)
    if nt == 0:
        assert M == 1
        return g.copy(), hist
    st = np.concatenate([hist, g], axis=1).astype(f32)
    n = g.shape[1] // M
    acc = np.zeros((g.shape[0], n), f32)
    with np.errstate(all="ignore"):
        for k in range(nt):
            p = st[:, k:k + n * M:M] * f32(coeffs[k])
            acc = acc + p
    assert acc.dtype == np.float32
    return acc, st[:, st.shape[1] - (nt - 1):].copy()


class TxInStage:
    """the stage alone, `channels` rows; block: the DSP block in audio samples; vox: None or a dict of meter fields"""

    def __init__(self, channels, block, M=1, coeffs=None, pick=MONO, gain=1.0, vox=None):
        self.channels, self.block = channels, block
        self.meter = None
        self.coeffs = np.zeros(0, f32)
        self.configure(M, coeffs, pick, gain, vox, first=True)

    def configure(self, M, coeffs, pick, gain, vox, first=False):
        """selenite_tx_set_in: the first setting clears everything; a retune keeps the state, a changed nd_taps clears the decimator's"""
        coeffs = np.zeros(0, f32) if coeffs is None else np.ascontiguousarray(coeffs, f32).reshape(-1)
        new_len = first or coeffs.size != self.coeffs.size
        self.M, self.coeffs, self.pick, self.gain = int(M), coeffs, int(pick), f32(gain)
        if new_len:
            self.hist = np.zeros((self.channels, max(coeffs.size - 1, 0)), f32)
        self.vox = None if vox is None else dict(vox)
        if first:
            self.level_init = f32(vox.get("level_init", 0.0)) if vox else f32(0.0)
            self.meter = self._new_meter(self.level_init)
        elif vox is not None:                       # a retune: the law's parameters change, level / open / hold / counters stay
            st = self.meter.state()
            self.level_init = f32(vox.get("level_init", 0.0))
            self.meter = self._new_meter(self.level_init)
            self.meter.set_state(st)

    def _new_meter(self, level_init):
        v = dict(gate=0, hang=0, attack=0.5, decay=0.125, open_level=1e-6, close_level=5e-7)
        v.update({k: x for k, x in (self.vox or {}).items() if k not in ("level_init", "sense")})
        return mo.Meter(self.channels, self.block, sense=mo.ABOVE, level_init=level_init, **v)

    def reset(self):
        self.hist[:] = 0
        self.meter = self._new_meter(self.level_init)

    def words(self, block_size):
        return block_size * self.M * (1 if self.pick == MONO else 2)

    def process(self, frames, out_q15, q15_rounding=False):
        """frames [C][words] f32 or int16 -> dict(a: in front of the gate, audio: what enters the chain (f32 or int16), bits or None)"""
        frames = np.asarray(frames)
        x = q15_to_float(frames) if frames.dtype == np.int16 else frames.astype(f32)
        with np.errstate(all="ignore"):
            g = pick_frames(x, self.pick) * self.gain
        a, self.hist = fir_decimate(self.hist, g, self.coeffs, self.M)
        assert a.shape[1] % self.block == 0 and a.shape[1] > 0
        bits, y = None, a
        if self.vox is not None:
            bits = self.meter.process(a)
            y = self.meter.gate_audio(a, bits)
        return dict(a=a, bits=bits, audio=float_to_q15(y, q15_rounding) if out_q15 else y)

    def state(self):
        st = self.meter.state()
        st["dec_state"] = self.hist.copy()
        return st

    def set_state(self, d):
        d = dict(d)
        if "dec_state" in d:
            h = np.array(d.pop("dec_state"), f32)
            assert h.shape == self.hist.shape
            self.hist = h
        self.meter.set_state(d)


class TxInOracle:
    """A TX instance with an input stage: `chain` is the co.TxCwOracle of the instance (audio calls, keyed calls, modes, FM, reset go
    through it as before), `stage` the TxInStage behind set_in."""

    def __init__(self, spec):
        self.spec = spec
        self.chain = co.TxCwOracle(spec)
        self.stage = None

    def set_in(self, M=1, coeffs=None, pick=MONO, gain=1.0, vox=None):
        if self.stage is None:
            self.stage = TxInStage(self.spec.channels, self.spec.block, M, coeffs, pick, gain, vox)
        else:
            self.stage.configure(M, coeffs, pick, gain, vox)
        return 0

    def clear_in(self):
        self.stage = None
        return 0

    def reset(self):
        self.chain.reset()
        if self.stage is not None:
            self.stage.reset()
        return 0

    def set_mode(self, mode):
        return self.chain.set_mode(mode)

    def frames_refused(self, block_size):
        if self.stage is None:
            return rc.ARGUMENT_ERROR
        if block_size == 0 or block_size % self.spec.block:
            return rc.LENGTH_ERROR
        return 0

    def process_frames(self, frames, kind=K_F32):
        """-> (the stage's audio as in_audio_device shows it, I/Q)"""
        r = self.stage.process(frames, kind == K_Q15, self.spec.q15_rounding)
        self.last = r
        iq = self.chain.process_q15(r["audio"]) if kind == K_Q15 else self.chain.process(r["audio"])
        return r["audio"], iq

    def state(self):
        st = self.chain.state()
        st.pop("tone_phase", None)
        for k in ("key_state", "side_phase", "tx_on", "hold"):
            st.pop(k, None)
        return st

    def in_state(self):
        return self.stage.state()
