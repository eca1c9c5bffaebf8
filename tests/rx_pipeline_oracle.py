"""The whole RX path as ONE composition of the per-stage restatements -- what an instance with any subset of the nine stages switched on must
return and leave behind, derived from DESIGN.md section 2 (steps 0b .. 7) and the setters' docstrings, not from the dispatcher:

    0b   spectrum_oracle.Spectrum     a tap on the caller's own input (int16 words or f32)
    0b2  iqc_oracle.Corrector         a corrected copy, always f32: an int16 call runs on as f32 in, int16 out
    0c   nb_oracle.Blanker            a blanked copy of whatever the correction left, in that format
    1-4  rxcommon.CpuChain            the chain with its AGC off: the un-scaled audio (or, in SELENITE_ARITH_SPLIT16 / _AUTO, audio from outside)
    4-t  tones_oracle.Tones           a tap on the un-scaled audio
    4-d  cwdec_oracle.CwDec           a tap on the same audio
    4a   afilt_oracle.Afilt           in place
    4b   nr_oracle.Nlms               in place, behind the filter
    4c   meter_oracle.Meter           reads what the listener hears; leaves the gate of every DSP block
    5    nr_oracle.Agc                per channel, or agc_global: the maximum over all channels per DSP block
    4c'  Meter.gate_audio             closed blocks of the SCALED audio become +0
    6    nr_oracle.float_to_q15       int16 slots (cfg.q15_rounding) -- behind the output stage when there is one
    7    out_oracle.OutStage          interpolator and frames

Nothing here is arithmetic of its own: every number comes out of one of those classes.  tests/test_rx_pipeline_oracle.py pins the composition
(one stage on equals that stage's oracle, no stage on equals CpuChain with its AGC on, cut invariance, the split call) and shows that the
order is observable on the fuzz signal: Pipeline.order and Pipeline.gate_first exist for that test alone.

TEST INFRASTRUCTURE.  Nothing here is imported by the product.
"""
import copy
import ctypes as C

import numpy as np

import afilt_oracle as ao
import cwdec_oracle as co
import iqc_oracle as io
import meter_oracle as mo
import nb_oracle as no
import nr_oracle as nro
import out_oracle as oo
import rxcommon as rc
import spectrum_oracle as so
import tones_oracle as to

f32 = np.float32
STAGES = ("spectrum", "iqc", "nb", "tones", "cwdec", "afilt", "nr", "meter", "out")
ORDER = ("tones", "cwdec", "afilt", "nr", "meter")          # in front of the AGC: two taps, two in-place stages, the meter
EXACT = (rc.ARITH_CMSIS, rc.ARITH_FMA)


def no_agc(spec):
    s = copy.copy(spec)
    s.agc, s.agc_global = False, False
    return s


def q15_to_float(q):
    return np.divide(np.asarray(q).astype(f32), f32(32768.0))       # arm_q15_to_float


class Pipeline:
    """Pipeline(spec, stages): spec an rc.ChainSpec, stages {name: keyword arguments of the matching Rx.set_*} over a subset of STAGES."""

    def __init__(self, spec, stages=None):
        self.spec, self.ch, self.na = spec, spec.channels, spec.block // spec.decim
        self.mode = spec.mode
        self.exact = spec.arith in EXACT
        self.order, self.gate_first = ORDER, False
        self.par, self.st = {}, {}
        self._new_chain()
        for name, p in (stages or {}).items():
            self.set_stage(name, p)
        self.held = None

    # ---- construction -------------------------------------------------------------------------------------------------------------------
    def _new_chain(self):
        self.chain = rc.CpuChain(no_agc(self.spec), "orc") if self.exact else None
        if self.chain is not None:
            assert self.chain.ok()
            if self.mode != self.spec.mode:
                assert self.chain.set_mode(self.mode) == 0
        self.agc = nro.Agc(self.ch, self.na, self.spec.agc_params, self.spec.agc_global) if self.spec.agc else None
        self.gain_idle = np.full(self.ch, f32(self.spec.agc_params["gain_init"]), f32)      # (AGC off: the row stays at gain_init)

    def _build(self, name, p):
        ch, na = self.ch, self.na
        if name == "spectrum":
            return so.Spectrum(ch, **p)
        if name == "iqc":
            return io.Corrector(ch, **p)
        if name == "nb":
            return no.Blanker(ch, **p)
        if name == "tones":
            return to.Tones(ch, na, **p)
        if name == "cwdec":
            return co.CwDec(ch, na, **p)
        if name == "afilt":
            return ao.Afilt(ch, p["coeffs"], p.get("per_channel", False))
        if name == "nr":
            return nro.Nlms(ch, p["num_taps"], p["mu"], p.get("coeffs_init"), p["delay"])
        if name == "meter":
            return mo.Meter(ch, na, **p)
        if name == "out":
            return oo.OutStage(ch, p.get("interp", 1), p.get("coeffs"), p.get("frames", oo.OUT_MONO))
        raise KeyError(name)

    def set_stage(self, name, params):
        """Rx.set_<name>(**params), or with None its removal; a stage set again starts fresh"""
        assert name in STAGES, name
        if params is None or (name == "nr" and params.get("kind", nro.NR_DENOISE) == nro.NR_OFF):
            self.par.pop(name, None)
            self.st.pop(name, None)
            return
        self.par[name] = dict(params)
        self.st[name] = self._build(name, self.par[name])

    def on(self, name):
        return name in self.st

    def reset(self):
        """selenite_rx_reset: the chain at its start (the mode stays), every stage where its setter left it"""
        self._new_chain()
        for name in list(self.par):
            self.st[name] = self._build(name, self.par[name])
        self.held = None

    def set_mode(self, mode):
        self.mode = mode
        return self.chain.set_mode(mode) if self.chain is not None else 0

    # ---- one call -------------------------------------------------------------------------------------------------------------------------
    def _front(self, data):
        """steps 0b .. 0c: the chain's f32 input"""
        data = np.asarray(data)
        if self.on("spectrum"):
            self.st["spectrum"].process(data)
        x = data
        if self.on("iqc"):
            x = self.st["iqc"].process(x)
        if self.on("nb"):
            x = self.st["nb"].process(x)
        return q15_to_float(x) if x.dtype == np.int16 else np.ascontiguousarray(x, f32)

    def _unscaled(self, pre, data):
        """everything in front of the AGC: returns the un-scaled audio the AGC sees and the gate of every block (None without a meter)"""
        x = self._front(data)
        if pre is None:
            assert self.chain is not None, "SELENITE_ARITH_SPLIT16 / _AUTO: the un-scaled audio comes from outside (process_audio)"
            a = self.chain.process(x)
        else:
            a = np.array(pre, f32)
        bits = None
        for name in self.order:
            if not self.on(name):
                continue
            s = self.st[name]
            if name in ("tones", "cwdec"):
                s.process(a)
            elif name == "afilt":
                a = s.process(a)
            elif name == "nr":
                a = s.process(a, self.par["nr"].get("kind", nro.NR_DENOISE))
            else:
                bits = s.process(a)
        return a, bits

    def _scale(self, a, bits, env=None):
        """step 5 and the gate behind it"""
        gate = bits is not None and self.st["meter"].par["gate"]
        if gate and self.gate_first:                                  # (a wrong order, for tests/test_rx_pipeline_oracle.py)
            a = self.st["meter"].gate_audio(a, bits)
        y = self.agc.process(a, env) if self.agc is not None else a
        if gate and not self.gate_first:
            y = self.st["meter"].gate_audio(y, bits)
        return y

    def _store(self, y, q15):
        if self.on("out"):
            return self.st["out"].process(y, self.na, q15=q15, rounding=self.spec.q15_rounding, form="np")
        return nro.float_to_q15(y, self.spec.q15_rounding) if q15 else np.ascontiguousarray(y, f32)

    def process_audio(self, pre, data):
        """one call whose un-scaled chain audio is `pre` (None: the oracle chain's); data: the caller's input, f32 or int16"""
        data = np.asarray(data)
        a, bits = self._unscaled(pre, data)
        return self._store(self._scale(a, bits), data.dtype == np.int16)

    def process(self, iq):
        return self.process_audio(None, np.ascontiguousarray(iq, f32))

    def process_q15(self, iq16):
        return self.process_audio(None, np.ascontiguousarray(iq16, np.int16))

    # ---- the split global-gain call -----------------------------------------------------------------------------------------------------
    def phase1(self, iq, pre=None):
        """everything up to and including the meter: returns the un-scaled audio and the envelope row (one maximum per DSP block)"""
        assert self.agc is not None and self.spec.agc_global and not self.on("out")
        a, bits = self._unscaled(pre, np.ascontiguousarray(iq, f32))
        self.held = (a, bits)
        env = np.max(np.abs(a).reshape(self.ch, -1, self.na), axis=(0, 2)).astype(f32)
        return a.copy(), env

    def phase2(self, env=None):
        """the gain and the gate, nothing else"""
        a, bits = self.held
        self.held = None
        return np.ascontiguousarray(self._scale(a, bits, env), f32)

    # ---- state --------------------------------------------------------------------------------------------------------------------------
    def state(self):
        """{stage: rows} as the library's *_state() getters return them, and "chain" (in _SPLIT16 / _AUTO: its agc_gain only)"""
        d = {}
        chain = self.chain.state() if self.chain is not None else {}
        chain["agc_gain"] = (self.agc.gain if self.agc is not None else self.gain_idle).copy()
        d["chain"] = chain
        for name, s in self.st.items():
            if name == "afilt":
                c = s.coeffs if s.per_channel else s.coeffs[0]
                d[name] = dict(state=s.state.copy(), coeffs=c.copy())
            elif name == "out":
                if s.P >= 2:
                    d[name] = s.state.copy()
            else:
                d[name] = s.state()
        return d

    def spectrum_frames(self):
        return self.st["spectrum"].frames

    def set_state(self, d):
        for name, rows in d.items():
            if name == "chain":
                if self.chain is not None:
                    arrs = {k: np.ascontiguousarray(v) for k, v in rows.items()}
                    assert self.chain.L.orc_rx_set_state(self.chain.h, C.byref(rc.state_view(arrs))) == 0
                if self.agc is not None:
                    self.agc.gain = np.array(rows["agc_gain"], f32)
                else:
                    self.gain_idle = np.array(rows["agc_gain"], f32)
                continue
            s = self.st[name]
            if name == "afilt":
                s.state = np.array(rows["state"], f32)
            elif name == "out":
                s.state = np.array(rows, f32)
            elif name == "tones":
                for k, v in rows.items():
                    if k == "position":
                        s.position = int(np.asarray(v).reshape(-1)[0])
                    else:
                        setattr(s, k, np.array(v, dtype=getattr(s, k).dtype))
                s.done = (s.position % s.frame_blocks) * s.n             # (calls are whole DSP blocks)
            else:
                s.set_state({k: np.array(v) for k, v in rows.items()})
