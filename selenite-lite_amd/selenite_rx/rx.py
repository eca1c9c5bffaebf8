"""Rx: one selenite_rx_instance (include/selenite_rx.h) and its stages."""
import ctypes as C

import numpy as np

from . import RxError, _fp, lib, ring_text
from ._state import channel_rows, dtypes, get_state, set_state
from . import (ARGUMENT_ERROR, CWDEC_DEFAULTS, FSKDEC_DEFAULTS, LENGTH_ERROR, NR_OFF, OUT_MONO, SQ_ABOVE, SUCCESS, AfiltConfig, AfiltStateView,
                  CwdecConfig, CwdecStateView, FskdecConfig, FskdecStateView, IqcConfig, IqcStateView, MeterConfig, MeterStateView, NbConfig, NbStateView, NrConfig,
                  NrStateView, OutConfig, SpecConfig, SpecStateView, StateView, TonesConfig, TonesStateView, i16p, u8p, u32p, u64p)


class Rx:
    """One selenite_rx_instance.  `cfg` is a filled Config whose coefficient arrays the caller keeps
    alive until construction returns (the library copies them)."""

    def __init__(self, cfg):
        self.L = lib()
        self.cfg = cfg
        self.h = C.c_void_p()
        # what Python remembers of each stage to size its state arrays (None: the stage is off); _set_stage keeps them
        self._nr = self._out = self._spec = self._nb = self._iqc = self._meter = self._afilt = self._tones = self._cwdec = self._fskdec = None
        rc = self.L.selenite_rx_init(C.byref(self.h), C.byref(cfg))
        if rc != SUCCESS:
            raise RxError(rc, self.L.selenite_rx_error_string(None).decode())

    # -- CMSIS-style calls ------------------------------------------------------------------
    def out_len(self, block_size):
        """values per channel a call of block_size writes: block_size / decim, or what the output stage makes of it (out_values)"""
        if self._out is not None:
            return self.out_values(block_size)
        return block_size // self.cfg.decim

    def process(self, iq, out=None):
        """selenite_rx_process_f32 on host arrays (pageable numpy memory, or page-locked `pinned_array`s)."""
        iq = np.ascontiguousarray(iq, np.float32)
        c, bs = iq.shape[0], iq.shape[1]
        if out is None:
            out = np.empty((c, self.out_len(bs)), np.float32)
        self.L.selenite_rx_process_f32(self.h, _fp(iq), _fp(out), bs)
        self.check()
        return out

    def process_q15(self, iq, out=None):
        iq = np.ascontiguousarray(iq, np.int16)
        c, bs = iq.shape[0], iq.shape[1]
        if out is None:
            out = np.empty((c, self.out_len(bs)), np.int16)
        self.L.selenite_rx_process_q15(self.h, iq.ctypes.data_as(i16p), out.ctypes.data_as(i16p), bs)
        self.check()
        return out

    def process_device(self, d_src, d_dst, block_size):
        self.L.selenite_rx_process_f32_device(self.h, d_src, d_dst, block_size)

    def process_q15_device(self, d_src, d_dst, block_size):
        self.L.selenite_rx_process_q15_device(self.h, d_src, d_dst, block_size)

    def global_phase1(self, d_src, d_dst, d_env, block_size):
        self.L.selenite_rx_global_phase1_device(self.h, d_src, d_dst, d_env, block_size)

    def global_phase2(self, d_dst, d_env, block_size):
        self.L.selenite_rx_global_phase2_device(self.h, d_dst, d_env, block_size)

    def set_mode(self, mode):
        return self.L.selenite_rx_set_mode(self.h, mode)

    def set_stream(self, stream_ptr):
        return self.L.selenite_rx_set_stream(self.h, stream_ptr)

    def sync(self):
        rc = self.L.selenite_rx_sync(self.h)
        if rc:
            raise RxError(rc, self.error())

    def reset(self):
        return self.L.selenite_rx_reset(self.h)

    def status(self):
        return self.L.selenite_rx_status(self.h)

    def error(self):
        return self.L.selenite_rx_error_string(self.h).decode()

    def check(self):
        rc = self.status()
        if rc:
            raise RxError(rc, self.error())

    def kernel_name(self):
        return self.L.selenite_rx_kernel_name(self.h).decode()

    # -- parity guard of the split-precision arithmetic ----------------------------------------
    def set_guard_ratio(self, ratio):
        rc = self.L.selenite_rx_set_guard_ratio(self.h, ratio)
        if rc:
            raise RxError(rc, "selenite_rx_set_guard_ratio")

    def guard_stats(self):
        """dict(blocks, channel_calls, rerun_channel_calls, handover_blocks) since init / the last guard_clear()."""
        b, c, r = C.c_uint64(), C.c_uint64(), C.c_uint64()
        rc = self.L.selenite_rx_guard_stats(self.h, C.byref(b), C.byref(c), C.byref(r))
        if rc:
            raise RxError(rc, self.error())
        h = C.c_uint64()
        rc = self.L.selenite_rx_guard_handover(self.h, C.byref(h))
        if rc:
            raise RxError(rc, self.error())
        return dict(blocks=int(b.value), channel_calls=int(c.value), rerun_channel_calls=int(r.value), handover_blocks=int(h.value))

    def set_handover_repair(self, on):
        return self.L.selenite_rx_set_handover_repair(self.h, int(bool(on)))

    def set_auto_launches(self, launches):
        """SELENITE_ARITH_AUTO: 1 (default) = the matrix kernel recomputes a channel it guarded itself where it can (k_hilb_split16: one launch
        per call), 3 = always k_hist_exact and the rerun pass behind it.  Same bits either way."""
        return self.L.selenite_rx_set_auto_launches(self.h, int(launches))

    def auto_launches_last(self):
        """1 / 3: the form the last SELENITE_ARITH_AUTO call on a matrix kernel took (0: none yet)."""
        return int(self.L.selenite_rx_auto_launches_last(self.h))

    def guard_channels(self):
        out = np.zeros(self.cfg.channels, np.uint32)
        rc = self.L.selenite_rx_guard_channels(self.h, out.ctypes.data_as(u32p))
        if rc:
            raise RxError(rc, self.error())
        return out

    def auto_words(self):
        """Diagnostic: the per-channel words of SELENITE_ARITH_AUTO (bit 0 rerun, bits 1-2 provenance, bit 5 held by the exact kernel, ...)."""
        out = np.zeros(self.cfg.channels, np.uint32)
        rc = self.L.selenite_rx_auto_words(self.h, out.ctypes.data_as(u32p))
        if rc:
            raise RxError(rc, self.error())
        return out

    def guard_clear(self):
        return self.L.selenite_rx_guard_clear(self.h)

    def nco_path(self):
        return self.L.selenite_rx_nco_path(self.h).decode()

    def time_process(self, d_src, d_dst, block_size, iters):
        ms = C.c_float()
        rc = self.L.selenite_rx_time_process_device(self.h, d_src, d_dst, block_size, iters, C.byref(ms))
        if rc:
            raise RxError(rc, self.error())
        return ms.value

    def time_process_q15(self, d_src, d_dst, block_size, iters):
        ms = C.c_float()
        rc = self.L.selenite_rx_time_process_q15_device(self.h, d_src, d_dst, block_size, iters, C.byref(ms))
        if rc:
            raise RxError(rc, self.error())
        return ms.value

    def time_process_each(self, d_src, d_dst, block_size, iters, q15=False):
        """per-call durations (ms) of `iters` back-to-back device calls, one HIP event between calls"""
        ms = np.zeros(iters, np.float32)
        rc = self.L.selenite_rx_time_process_each_device(self.h, d_src, d_dst, block_size, iters, _fp(ms), int(q15))
        if rc:
            raise RxError(rc, self.error())
        return ms

    def time_streaming_roof(self, d_src, d_dst, block_size, iters, q15=False):
        """per-launch durations (ms) of the no-arithmetic kernel that moves the algorithmic bytes of one call (d_dst is overwritten)"""
        ms = np.zeros(iters, np.float32)
        rc = self.L.selenite_rx_time_streaming_roof_device(self.h, d_src, d_dst, block_size, iters, _fp(ms), int(q15))
        if rc:
            raise RxError(rc, self.error())
        return ms

    def time_pattern_roof(self, d_src, d_dst, block_size, iters, q15=False, work=0):
        """per-launch durations (ms) of the no-DSP kernel with the fetch pattern and launch shape of the systolic CW kernel, `work` dependent
        vector instructions per chunk where its biquad steps are (d_dst is overwritten; CW shapes only)"""
        ms = np.zeros(iters, np.float32)
        rc = self.L.selenite_rx_time_pattern_roof_device(self.h, d_src, d_dst, block_size, iters, _fp(ms), int(q15), int(work))
        if rc:
            raise RxError(rc, self.error())
        return ms

    def synth_device(self, d_iq, first_channel, nch, first_sample, nsamp, seed):
        rc = self.L.selenite_rx_synth_iq_device(self.h, d_iq, first_channel, nch, first_sample, nsamp, seed)
        if rc:
            raise RxError(rc, self.error())

    def algorithmic_bytes(self, block_size):
        rd = C.c_uint64()
        tot = self.L.selenite_rx_algorithmic_bytes(C.byref(self.cfg), block_size, C.byref(rd))
        return int(tot), int(rd.value)

    # -- state ------------------------------------------------------------------------------
    def _state_shapes(self):
        g = self.cfg
        c = g.channels
        return dict(dec_state=(c, 2, max(g.nd_taps - 1, 0)), fir_state=(c, 2, max(g.nh_taps - 1, 0)), biq_state=(c, g.n_biquad, 4),
                    agc_gain=(c,), nco_phase=(c,))

    def state(self):
        return get_state(self.L.selenite_rx_get_state, self.h, StateView, self._state_shapes(), self.error)

    def set_state(self, arrs):
        set_state(self.L.selenite_rx_set_state, self.h, StateView, self._state_shapes(), arrs, self.error)

    # -- the stages: what every set_* and *_state below shares ----------------------------------
    def _set_stage(self, shadow, setter, cfg, new):
        """setter(h, cfg) -- cfg None: the stage off -- and `new` into the attribute `shadow` behind it.  A refused field (the two codes
        the library refuses with) leaves the old stage in place and the old shadow with it; any other failure, a failed allocation for
        one, leaves NO stage: the shadow is forgotten until a call succeeds."""
        old = getattr(self, shadow)
        setattr(self, shadow, None)
        rc = setter(self.h, None if cfg is None else C.byref(cfg))
        if rc in (ARGUMENT_ERROR, LENGTH_ERROR):
            setattr(self, shadow, old)
            raise RxError(rc, self.L.selenite_rx_error_string(None).decode())
        if rc:
            raise RxError(rc, self.error())
        setattr(self, shadow, new)

    def _on(self, shadow, what):
        """the shadow of a stage; RxError while the stage is off"""
        s = getattr(self, shadow)
        if s is None:
            raise RxError(ARGUMENT_ERROR, "the %s is off" % what)
        return s

    # -- NLMS noise reduction / automatic notch (selenite_rx_set_nr) --------------------------
    def set_nr(self, kind, num_taps=32, delay=16, mu=0.05, coeffs_init=None):
        """(Re)initialise the NLMS stage of every channel (NR_DENOISE / NR_NOTCH), or remove it (NR_OFF).  Raises RxError on a bad field;
        the instance is then left as it was."""
        g = NrConfig()
        g.struct_size = C.sizeof(NrConfig)
        g.kind, g.num_taps, g.delay, g.mu = int(kind), int(num_taps), int(delay), float(mu)
        w = None
        if coeffs_init is not None:
            w = np.ascontiguousarray(coeffs_init, np.float32)
            g.coeffs_init = _fp(w)
        self._set_stage("_nr", self.L.selenite_rx_set_nr, g, (int(num_taps), int(delay)) if kind != NR_OFF else None)

    def _nr_shapes(self):
        n, d = self._on("_nr", "NLMS stage")
        c = self.cfg.channels
        return dict(coeffs=(c, n), window=(c, n - 1), delay=(c, d), energy=(c,), x0=(c,))

    def nr_state(self):
        return get_state(self.L.selenite_rx_get_nr_state, self.h, NrStateView, self._nr_shapes())

    def set_nr_state(self, d):
        set_state(self.L.selenite_rx_set_nr_state, self.h, NrStateView, self._nr_shapes(), d)

    # -- audio output stage (selenite_rx_set_out) ---------------------------------------------
    def set_out(self, interp=1, coeffs=None, frames=OUT_MONO):
        """Put the output stage behind the AGC -- arm_fir_interpolate_f32 by `interp` with `coeffs` (pCoeffs order; None with interp 1: no
        FIR, frames only), mono or stereo frames -- or remove it (interp=None).  Clears the stage's state.  Raises RxError on a bad field;
        the instance is then left as it was."""
        if interp is None:
            return self._set_stage("_out", self.L.selenite_rx_set_out, None, None)
        g = OutConfig()
        g.struct_size = C.sizeof(OutConfig)
        w = np.ascontiguousarray(coeffs if coeffs is not None else [], np.float32)
        g.interp, g.ni_taps, g.frames = int(interp), int(w.size), int(frames)
        g.coeffs = _fp(w) if w.size else None
        # (interp, the phase length, frames; the library refuses interp 0)
        self._set_stage("_out", self.L.selenite_rx_set_out, g, (int(interp), int(w.size) // max(int(interp), 1), int(frames)))

    def out_values(self, block_size):
        """selenite_rx_out_values: values per channel a process call of block_size writes"""
        if not hasattr(self.L, "selenite_rx_out_values"):      # (an older build named by SELENITE_RX_LIB: no stage)
            return block_size // self.cfg.decim
        return int(self.L.selenite_rx_out_values(self.h, block_size))

    def _out_state_array(self):
        if self._out is None or self._out[1] < 2:
            raise RxError(ARGUMENT_ERROR, "the output stage is off or keeps no state (phase length <= 1)")
        return np.zeros((self.cfg.channels, self._out[1] - 1), np.float32)

    def out_state(self):
        """[channels][P - 1]: the interpolator's history, oldest first"""
        a = self._out_state_array()
        rc = self.L.selenite_rx_get_out_state(self.h, _fp(a))
        if rc:
            raise RxError(rc, "selenite_rx_get_out_state")
        return a

    def set_out_state(self, state):
        a = np.ascontiguousarray(state, np.float32)
        assert a.shape == self._out_state_array().shape, a.shape
        rc = self.L.selenite_rx_set_out_state(self.h, _fp(a))
        if rc:
            raise RxError(rc, "selenite_rx_set_out_state")

    # -- spectrum tap (selenite_rx_set_spectrum) ------------------------------------------------
    def set_spectrum(self, fft_len=512, stride=1, average=0, alpha=1.0, window=None):
        """Put the spectrum tap on the raw input of every channel, or remove it (fft_len=None).  Clears the tap's state.  Raises RxError on a
        bad field; the instance is then left as it was."""
        if fft_len is None:
            return self._set_stage("_spec", self.L.selenite_rx_set_spectrum, None, None)
        g = SpecConfig()
        g.struct_size = C.sizeof(SpecConfig)
        g.fft_len, g.stride, g.average, g.alpha = int(fft_len), int(stride), int(average), float(alpha)
        w = None
        if window is not None:
            w = np.ascontiguousarray(window, np.float32)
            assert w.shape == (int(fft_len),), w.shape
            g.window = _fp(w)
        self._set_stage("_spec", self.L.selenite_rx_set_spectrum, g, int(fft_len))

    def _spec_shapes(self):
        n, c = self._on("_spec", "spectrum tap"), self.cfg.channels
        return dict(rows=(c, n), pending=(c, n, 2), position=(1,))

    def spectrum(self):
        """(rows [channels][fft_len] display order, frames transformed so far); drains the stream"""
        rows = np.zeros(self._spec_shapes()["rows"], np.float32)
        n = C.c_uint64(0)
        rc = self.L.selenite_rx_get_spectrum(self.h, _fp(rows), C.byref(n))
        if rc:
            raise RxError(rc, "selenite_rx_get_spectrum")
        return rows, int(n.value)

    def spectrum_device(self):
        """device address of the row buffer (None while the tap is off)"""
        return self.L.selenite_rx_spectrum_device(self.h)

    def spectrum_state(self):
        return get_state(self.L.selenite_rx_get_spectrum_state, self.h, SpecStateView, self._spec_shapes())

    def set_spectrum_state(self, d):
        set_state(self.L.selenite_rx_set_spectrum_state, self.h, SpecStateView, self._spec_shapes(), d)

    # -- impulse noise blanker (selenite_rx_set_nb) ---------------------------------------------
    def set_nb(self, frame=64, guard=2, max_hits=8, threshold=8.0, alpha=0.125, clamp=2.0):
        """Put the noise blanker on the raw input of every channel, in front of the NCO, or remove it (frame=None).  Clears the blanker's
        state.  Raises RxError on a bad field; the instance is then left as it was."""
        if frame is None:
            return self._set_stage("_nb", self.L.selenite_rx_set_nb, None, None)
        g = NbConfig()
        g.struct_size = C.sizeof(NbConfig)
        g.frame, g.guard, g.max_hits = int(frame), int(guard), int(max_hits)
        g.threshold, g.alpha, g.clamp = float(threshold), float(alpha), float(clamp)
        self._set_stage("_nb", self.L.selenite_rx_set_nb, g, int(frame))

    def _nb_shapes(self):
        self._on("_nb", "noise blanker")
        return channel_rows(NbStateView, self.cfg.channels)

    def nb_state(self):
        """dict(level [channels] f32, blanked [channels] u64, bursts [channels] u64); drains the stream"""
        return get_state(self.L.selenite_rx_get_nb_state, self.h, NbStateView, self._nb_shapes())

    def set_nb_state(self, d):
        set_state(self.L.selenite_rx_set_nb_state, self.h, NbStateView, self._nb_shapes(), d)

    # -- I/Q correction (selenite_rx_set_iqc) ----------------------------------------------------
    def set_iqc(self, frame=64, alpha=1.0 / 64, dc_alpha=1.0 / 16, p_max=0.25, g_max=1.5, min_power=1e-12, p_init=0.0, g_init=1.0,
                dc_i_init=0.0, dc_q_init=0.0):
        """Put the I/Q correction (DC offset, gain and phase imbalance) on the raw input of every channel, in front of the noise blanker, or
        remove it (frame=None).  Sets the stage's state to the inits.  Raises RxError on a bad field; the instance is then left as it was."""
        if frame is None:
            return self._set_stage("_iqc", self.L.selenite_rx_set_iqc, None, None)
        g = IqcConfig()
        g.struct_size, g.frame = C.sizeof(IqcConfig), int(frame)
        g.alpha, g.dc_alpha, g.p_max, g.g_max, g.min_power = float(alpha), float(dc_alpha), float(p_max), float(g_max), float(min_power)
        g.p_init, g.g_init, g.dc_i_init, g.dc_q_init = float(p_init), float(g_init), float(dc_i_init), float(dc_q_init)
        self._set_stage("_iqc", self.L.selenite_rx_set_iqc, g, int(frame))

    def _iqc_shapes(self):
        self._on("_iqc", "I/Q correction")
        return channel_rows(IqcStateView, self.cfg.channels)

    def iqc_state(self):
        """dict(dc_i, dc_q, p, g [channels] f32, held [channels] u64); drains the stream"""
        return get_state(self.L.selenite_rx_get_iqc_state, self.h, IqcStateView, self._iqc_shapes())

    def set_iqc_state(self, d):
        set_state(self.L.selenite_rx_set_iqc_state, self.h, IqcStateView, self._iqc_shapes(), d)

    # -- signal-level meter and squelch (selenite_rx_set_meter) -----------------------------------
    METER_TYPES = dtypes(MeterStateView)

    def set_meter(self, sense=SQ_ABOVE, gate=1, hang=0, attack=0.5, decay=0.125, open_level=1e-6, close_level=5e-7, level_init=0.0):
        """Put the level meter / squelch on the un-scaled audio of every channel, in front of the AGC (gate=1: closed DSP blocks leave as
        zeros, behind the AGC), or remove it (sense=None).  Sets the stage's state to level_init, closed, counters zero.  Raises RxError on
        a bad field; the instance is then left as it was."""
        if sense is None:
            return self._set_stage("_meter", self.L.selenite_rx_set_meter, None, None)
        g = MeterConfig()
        g.struct_size, g.sense, g.gate, g.hang = C.sizeof(MeterConfig), int(sense), int(gate), int(hang)
        g.attack, g.decay, g.open_level, g.close_level, g.level_init = float(attack), float(decay), float(open_level), float(close_level), float(level_init)
        self._set_stage("_meter", self.L.selenite_rx_set_meter, g, True)

    def _meter_shapes(self):
        self._on("_meter", "level meter")
        return channel_rows(MeterStateView, self.cfg.channels)

    def meter_state(self):
        """dict(level f32, open u32, hold u32, opens u64, open_blocks u64, each [channels]); drains the stream"""
        return get_state(self.L.selenite_rx_get_meter_state, self.h, MeterStateView, self._meter_shapes())

    def set_meter_state(self, d):
        set_state(self.L.selenite_rx_set_meter_state, self.h, MeterStateView, self._meter_shapes(), d)

    def meter_level_device(self):
        """device address of the level row (None while the stage is off)"""
        return self.L.selenite_rx_meter_level_device(self.h)

    def meter_open_device(self):
        """device address of the open row (None while the stage is off)"""
        return self.L.selenite_rx_meter_open_device(self.h)

    # -- audio biquad filter (selenite_rx_set_afilt) -----------------------------------------------
    def set_afilt(self, coeffs, per_channel=False):
        """Put a biquad cascade (arm_biquad_cascade_df1_f32) on the un-scaled audio of every channel, in front of NLMS, the meter and the
        AGC, or remove it (coeffs=None).  coeffs: [n_stages][5] for all channels, or with per_channel [channels][n_stages][5]; CMSIS order
        and sign.  Clears the stage's state.  Raises RxError on a bad field; the instance is then left as it was."""
        if coeffs is None:
            return self._set_stage("_afilt", self.L.selenite_rx_set_afilt, None, None)
        a = np.ascontiguousarray(coeffs, np.float32)
        want = 3 if per_channel else 2
        if a.ndim == 1 and not per_channel and a.size == 5:
            a = a.reshape(1, 5)
        if a.ndim != want or a.shape[-1] != 5 or (per_channel and a.shape[0] != self.cfg.channels):
            raise RxError(ARGUMENT_ERROR, "set_afilt: coeffs is not [n_stages][5] / [channels][n_stages][5]")
        g = AfiltConfig()
        g.struct_size, g.n_stages, g.per_channel, g.reserved, g.coeffs = C.sizeof(AfiltConfig), a.shape[-2], int(bool(per_channel)), 0, _fp(a)
        self._set_stage("_afilt", self.L.selenite_rx_set_afilt, g, (int(a.shape[-2]), bool(per_channel)))

    def set_afilt_coeffs(self, coeffs, first_channel=0):
        """Replace the coefficient rows of channels first_channel .. (coeffs [n][n_stages][5]; one shared set: [n_stages][5]) and keep the
        state; ordered on the instance's stream."""
        a = np.ascontiguousarray(coeffs, np.float32)
        n = a.shape[0] if a.ndim == 3 else 1
        rc = self.L.selenite_rx_set_afilt_coeffs(self.h, int(first_channel), int(n), _fp(a))
        if rc:
            raise RxError(rc, self.L.selenite_rx_error_string(None).decode() if rc == ARGUMENT_ERROR else self.error())

    def _afilt_shapes(self):
        ns, per = self._on("_afilt", "audio filter")
        return dict(state=(self.cfg.channels, ns, 4), coeffs=(self.cfg.channels, ns, 5) if per else (ns, 5))

    def afilt_state(self):
        """dict(state f32 [channels][n_stages][4] {x1, x2, y1, y2}, coeffs f32 as configured); drains the stream"""
        return get_state(self.L.selenite_rx_get_afilt_state, self.h, AfiltStateView, self._afilt_shapes())

    def set_afilt_state(self, state):
        """state: the array, or a dict with it under "state" (the coefficients are not state: set_afilt_coeffs)"""
        a = dict(state=state["state"] if isinstance(state, dict) else state)
        set_state(self.L.selenite_rx_set_afilt_state, self.h, AfiltStateView, self._afilt_shapes(), a)

    # -- tone-detector bank (selenite_rx_set_tones) --------------------------------------------------
    TONES_TYPES = dtypes(TonesStateView)

    def set_tones(self, coeffs, frame_blocks=1, confirm=1, release=1, ratio=0.0, min_power=0.0):
        """Put the tone-detector bank on the un-scaled audio of every channel (a tap in front of the audio filter, NLMS, the meter and the
        AGC), or remove it (coeffs=None).  coeffs: [K][3] {2 cos w, cos w, sin w} (design_tones).  Puts the stage's state at its start.
        Raises RxError on a bad field; the instance is then left as it was."""
        if coeffs is None:
            return self._set_stage("_tones", self.L.selenite_rx_set_tones, None, None)
        a = np.ascontiguousarray(coeffs, np.float32)
        if a.ndim != 2 or a.shape[1] != 3:
            raise RxError(ARGUMENT_ERROR, "set_tones: coeffs is not [n_tones][3]")
        g = TonesConfig()
        g.struct_size, g.n_tones, g.frame_blocks, g.confirm, g.release, g.reserved = C.sizeof(TonesConfig), a.shape[0], int(frame_blocks), int(confirm), int(release), 0
        g.ratio, g.min_power, g.coeffs = float(ratio), float(min_power), _fp(a)
        self._set_stage("_tones", self.L.selenite_rx_set_tones, g, int(a.shape[0]))

    def _tones_shapes(self):
        ch, k = self.cfg.channels, self._on("_tones", "tone detector")
        return dict(channel_rows(TonesStateView, self.cfg.channels), s=(ch, k, 2), power=(ch, k), position=(1,))

    def tones_state(self):
        """dict(s f32 [channels][K][2], energy, frame_energy f32 [channels], power f32 [channels][K], last_best, tone, cand, run u32
        [channels], changes u64 [channels], position u64 [1]); drains the stream"""
        return get_state(self.L.selenite_rx_get_tones_state, self.h, TonesStateView, self._tones_shapes())

    def set_tones_state(self, d):
        set_state(self.L.selenite_rx_set_tones_state, self.h, TonesStateView, self._tones_shapes(), d)

    def tones(self):
        """(tone u32 [channels], power f32 [channels][K] of the last whole frame, whole frames since set_tones / reset); drains the stream"""
        sh = self._tones_shapes()
        tone, power, frames = np.zeros(sh["tone"], np.uint32), np.zeros(sh["power"], np.float32), C.c_uint64(0)
        rc = self.L.selenite_rx_get_tones(self.h, tone.ctypes.data_as(u32p), _fp(power), C.byref(frames))
        if rc:
            raise RxError(rc, "selenite_rx_get_tones")
        return tone, power, int(frames.value)

    def tones_tone_device(self):
        """device address of the tone row (None while the stage is off)"""
        return self.L.selenite_rx_tones_tone_device(self.h)

    def tones_power_device(self):
        """device address of the power rows (None while the stage is off)"""
        return self.L.selenite_rx_tones_power_device(self.h)

    # -- Morse decoder (selenite_rx_set_cwdec) ----------------------------------------------------------
    CWDEC_TYPES = dtypes(CwdecStateView)

    def set_cwdec(self, on=True, table=None, **par):
        """Put the Morse decoder on the un-scaled audio of every channel (a tap at the tone bank's place: it changes no audio), or remove
        it (set_cwdec(None)).  par: the fields of selenite_rx_cwdec_config; the defaults are CWDEC_DEFAULTS: peak_attack 0.5, peak_decay
        0.002, floor_attack 0.25, floor_decay 0.002, on_frac 0.4, off_frac 0.25, snr 4, min_power 1e-8, debounce 2, adapt 1, track 2,
        unit_min 2 * 256, unit_init 10 * 256, unit_max 64 * 256 (Q8 DSP blocks), ring 256.  table: uint8 [256] (None: morse_table()).
        Puts the stage's state at its start.  Raises RxError on a bad field; the instance is then left as it was."""
        if on is None or on is False:
            return self._set_stage("_cwdec", self.L.selenite_rx_set_cwdec, None, None)
        unknown = set(par) - set(CWDEC_DEFAULTS)
        if unknown:
            raise TypeError("set_cwdec: unknown fields %s" % sorted(unknown))
        p = dict(CWDEC_DEFAULTS, **par)
        g = CwdecConfig()
        g.struct_size = C.sizeof(CwdecConfig)
        for k, v in p.items():
            setattr(g, k, float(v) if isinstance(CWDEC_DEFAULTS[k], float) else int(v))
        t = None
        if table is not None:
            t = np.ascontiguousarray(table, np.uint8)
            if t.shape != (256,):
                raise RxError(ARGUMENT_ERROR, "set_cwdec: table is not [256]")
            g.table = t.ctypes.data_as(u8p)
        self._set_stage("_cwdec", self.L.selenite_rx_set_cwdec, g, int(p["ring"]))

    def _cwdec_shapes(self):
        ch, ring = self.cfg.channels, self._on("_cwdec", "Morse decoder")
        return dict(channel_rows(CwdecStateView, self.cfg.channels), text=(ch, ring))

    def cwdec_state(self):
        """dict(peak, floor f32; primed, key, flip, run, unit, code, word u32; count u64, each [channels]; text u8 [channels][ring]); drains
        the stream"""
        return get_state(self.L.selenite_rx_get_cwdec_state, self.h, CwdecStateView, self._cwdec_shapes())

    def set_cwdec_state(self, d):
        set_state(self.L.selenite_rx_set_cwdec_state, self.h, CwdecStateView, self._cwdec_shapes(), d)

    def cwdec(self):
        """(text u8 [channels][ring], count u64, unit u32, key u32 [channels]): selenite_rx_get_cwdec; drains the stream"""
        sh = self._cwdec_shapes()
        text, count = np.zeros(sh["text"], np.uint8), np.zeros(sh["count"], np.uint64)
        unit, key = np.zeros(sh["unit"], np.uint32), np.zeros(sh["key"], np.uint32)
        rc = self.L.selenite_rx_get_cwdec(self.h, text.ctypes.data_as(u8p), count.ctypes.data_as(u64p), unit.ctypes.data_as(u32p),
                                          key.ctypes.data_as(u32p))
        if rc:
            raise RxError(rc, "selenite_rx_get_cwdec")
        return text, count, unit, key

    def cw_text(self, channel=None):
        """the last min(count, ring) characters of a channel in order, as str; channel=None: a list for all channels.  Drains the stream."""
        text, count, _, _ = self.cwdec()
        out = [ring_text(text[c], int(count[c])) for c in (range(self.cfg.channels) if channel is None else [channel])]
        return out if channel is None else out[0]

    def cw_unit(self):
        """the dit length of every channel in DSP blocks (unit / 256), float64 [channels]; drains the stream"""
        return self.cwdec()[2].astype(np.float64) / 256.0

    def cwdec_text_device(self):
        """device address of the rings, u8 [channels][ring] (None while the stage is off)"""
        return self.L.selenite_rx_cwdec_text_device(self.h)

    def cwdec_count_device(self):
        """device address of the count row, u64 [channels] (None while the stage is off)"""
        return self.L.selenite_rx_cwdec_count_device(self.h)

    def cwdec_unit_device(self):
        """device address of the unit row, u32 [channels] (None while the stage is off)"""
        return self.L.selenite_rx_cwdec_unit_device(self.h)

    # -- FSK teleprinter decoder (selenite_rx_set_fskdec) ------------------------------------------------
    FSKDEC_TYPES = dtypes(FskdecStateView)

    def set_fskdec(self, mark=None, space=None, table=None, **par):
        """Put the FSK teleprinter decoder on the un-scaled audio of every channel (a tap at the tone bank's place: it changes no audio), or
        remove it (set_fskdec(None)).  mark, space: float32 [5] each (fsk_bandpass).  par: the fields of selenite_rx_fskdec_config; the
        defaults are FSKDEC_DEFAULTS: tick 16, bit_q8 4224 (16.5 ticks: 45.45 baud at 12 kHz), reverse 0, usos 1, ring 256, alpha 0.25,
        hyst 0.1, frac 0.35, min_power 1e-6.  table: uint8 [64] (None: ita2_table()).  Puts the stage's state at its start.  Raises
        RxError on a bad field; the instance is then left as it was."""
        if mark is None or mark is False:
            return self._set_stage("_fskdec", self.L.selenite_rx_set_fskdec, None, None)
        unknown = set(par) - set(FSKDEC_DEFAULTS)
        if unknown:
            raise TypeError("set_fskdec: unknown fields %s" % sorted(unknown))
        m, s = np.ascontiguousarray(mark, np.float32), np.ascontiguousarray(space, np.float32)
        if m.shape != (5,) or s.shape != (5,):
            raise RxError(ARGUMENT_ERROR, "set_fskdec: mark / space is not [5]")
        p = dict(FSKDEC_DEFAULTS, **par)
        g = FskdecConfig()
        g.struct_size = C.sizeof(FskdecConfig)
        for k, v in p.items():
            setattr(g, k, float(v) if isinstance(FSKDEC_DEFAULTS[k], float) else int(v))
        g.mark[:], g.space[:] = m.tolist(), s.tolist()
        t = None
        if table is not None:
            t = np.ascontiguousarray(table, np.uint8)
            if t.shape != (64,):
                raise RxError(ARGUMENT_ERROR, "set_fskdec: table is not [64]")
            g.table = t.ctypes.data_as(u8p)
        self._set_stage("_fskdec", self.L.selenite_rx_set_fskdec, g, int(p["ring"]))

    def _fskdec_shapes(self):
        ch, ring = self.cfg.channels, self._on("_fskdec", "FSK decoder")
        return dict(channel_rows(FskdecStateView, ch), filt=(ch, 2, 4), text=(ch, ring))

    def fskdec_state(self):
        """dict(filt f32 [channels][2][4]; em, es, ew f32; lvl, k, t_q8, shift, figs, ferr, bit u32; count u64, each [channels]; text u8
        [channels][ring]); drains the stream"""
        return get_state(self.L.selenite_rx_get_fskdec_state, self.h, FskdecStateView, self._fskdec_shapes())

    def set_fskdec_state(self, d):
        set_state(self.L.selenite_rx_set_fskdec_state, self.h, FskdecStateView, self._fskdec_shapes(), d)

    def fskdec(self):
        """(text u8 [channels][ring], count u64, ferr u32, lvl u32 [channels]): selenite_rx_get_fskdec; drains the stream"""
        sh = self._fskdec_shapes()
        text, count = np.zeros(sh["text"], np.uint8), np.zeros(sh["count"], np.uint64)
        ferr, lvl = np.zeros(sh["ferr"], np.uint32), np.zeros(sh["lvl"], np.uint32)
        rc = self.L.selenite_rx_get_fskdec(self.h, text.ctypes.data_as(u8p), count.ctypes.data_as(u64p), ferr.ctypes.data_as(u32p),
                                           lvl.ctypes.data_as(u32p))
        if rc:
            raise RxError(rc, "selenite_rx_get_fskdec")
        return text, count, ferr, lvl

    def fsk_text(self, channel=None):
        """the last min(count, ring) characters of a channel in order, as str; channel=None: a list for all channels.  Drains the stream."""
        text, count, _, _ = self.fskdec()
        out = [ring_text(text[c], int(count[c])) for c in (range(self.cfg.channels) if channel is None else [channel])]
        return out if channel is None else out[0]

    def fsk_lvl(self):
        """the level of every channel behind the last tick, uint32 [channels]: 1 = mark (idle), 0 = space; drains the stream"""
        return self.fskdec()[3]

    def fskdec_text_device(self):
        """device address of the rings, u8 [channels][ring] (None while the stage is off)"""
        return self.L.selenite_rx_fskdec_text_device(self.h)

    def fskdec_count_device(self):
        """device address of the count row, u64 [channels] (None while the stage is off)"""
        return self.L.selenite_rx_fskdec_count_device(self.h)

    def fskdec_lvl_device(self):
        """device address of the lvl row, u32 [channels] (None while the stage is off)"""
        return self.L.selenite_rx_fskdec_lvl_device(self.h)

    def close(self):
        if self.h:
            self.L.selenite_rx_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
