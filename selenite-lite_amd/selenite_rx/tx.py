"""Tx: one batched TX chain instance (include/selenite_tx.h) and its stages.  Unlike Rx's, the set_* calls here return the status code."""
import ctypes as C

import numpy as np

from . import RxError, lib
from ._state import channel_rows, get_state, set_state
from . import (IN_F32, IN_MONO, KEYER_IAMBIC_B, SQ_ABOVE, MeterConfig, TxCwConfig, TxCwStateView, TxFmConfig, TxFmStateView,
                  TxInConfig, TxInStateView, TxKeyerConfig, TxKeyerStateView, TxStateView, f32p, u8p, u32p)


class Tx:
    """One batched TX chain instance (include/selenite_tx.h); mirror of Rx."""

    def __init__(self, cfg):
        self.L = lib()
        self.cfg = cfg
        self.h = C.c_void_p()
        # what Python remembers of the stages to size their state arrays and host buffers, as they are before the stage's set_* call
        self._cw_ns, self._in_nt, self._in_M, self._in_fw, self._keyer_ring = 1, 0, 1, 1, 1
        rc = self.L.selenite_tx_init(C.byref(self.h), C.byref(cfg))
        if rc:
            raise RxError(rc, "selenite_tx_init failed")

    def error(self):
        return self.L.selenite_tx_error_string(self.h).decode()

    def check(self):
        rc = self.L.selenite_tx_status(self.h)
        if rc:
            raise RxError(rc, self.error())

    def process(self, audio):
        audio = np.ascontiguousarray(audio, np.float32)
        c, bs = audio.shape
        out = np.empty((c, bs * self.cfg.interp, 2), np.float32)
        self.L.selenite_tx_process_f32(self.h, audio.ctypes.data, out.ctypes.data, bs)
        self.check()
        return out

    def process_q15(self, audio):
        audio = np.ascontiguousarray(audio, np.int16)
        c, bs = audio.shape
        out = np.empty((c, bs * self.cfg.interp, 2), np.int16)
        self.L.selenite_tx_process_q15(self.h, audio.ctypes.data, out.ctypes.data, bs)
        self.check()
        return out

    def process_device(self, d_src, d_dst, block_size):
        self.L.selenite_tx_process_f32_device(self.h, d_src, d_dst, block_size)

    def kernel_name(self):
        return self.L.selenite_tx_kernel_name(self.h).decode()

    def set_mode(self, mode):
        return self.L.selenite_tx_set_mode(self.h, mode)

    def sync(self):
        return self.L.selenite_tx_sync(self.h)

    def reset(self):
        return self.L.selenite_tx_reset(self.h)

    def _state_shapes(self):
        g = self.cfg
        return dict(channel_rows(TxStateView, self.cfg.channels), fir_state=(g.channels, 2, max(g.nh_taps - 1, 0)),
                    interp_state=(g.channels, 2, max(g.ni_taps // g.interp - 1, 0) if g.ni_taps else 0))

    def state(self):
        return get_state(self.L.selenite_tx_get_state, self.h, TxStateView, self._state_shapes(), self.error)

    def set_state(self, a):
        set_state(self.L.selenite_tx_set_state, self.h, TxStateView, self._state_shapes(), a, self.error)

    def set_fm(self, deviation=0.25, amplitude=1.0, tone_level=0.0, tone_step=None, tone_enable=None):
        """FM transmit mode (selenite_tx_set_fm; then set_mode(MODE_FM)).  tone_step: None (no tone), one phase increment per output
        sample for every channel, or an array [channels]; tone_enable defaults to `tone_step is not None`.  Returns the status code."""
        g = TxFmConfig()
        g.struct_size, g.deviation, g.amplitude, g.tone_level, g.reserved = C.sizeof(TxFmConfig), deviation, amplitude, tone_level, 0
        g.tone_enable = int(tone_step is not None) if tone_enable is None else int(tone_enable)
        steps = None
        if tone_step is not None and np.ndim(tone_step):
            steps = np.ascontiguousarray(tone_step, np.uint32)
            if steps.shape != (self.cfg.channels,):
                raise ValueError("tone_step: one value or [channels]")
            g.tone_step = steps.ctypes.data_as(u32p)
        elif tone_step is not None:
            g.tone_step_all = int(tone_step)
        return self.L.selenite_tx_set_fm(self.h, C.byref(g))

    def clear_fm(self):
        """selenite_tx_set_fm(S, NULL): FM off again (ARGUMENT_ERROR while the mode is FM)"""
        return self.L.selenite_tx_set_fm(self.h, None)

    def fm_state(self):
        return get_state(self.L.selenite_tx_get_fm_state, self.h, TxFmStateView, channel_rows(TxFmStateView, self.cfg.channels),
                         "selenite_tx_get_fm_state: FM is not configured (set_fm)")

    def set_fm_state(self, a):
        set_state(self.L.selenite_tx_set_fm_state, self.h, TxFmStateView, channel_rows(TxFmStateView, self.cfg.channels), a,
                  "selenite_tx_set_fm_state: FM is not configured (set_fm)")

    def set_cw(self, shape, amplitude=1.0, offset_step=0, side_level=0.0, side_step=0, side_mix=0, hang_blocks=0):
        """the keyed CW path (selenite_tx_set_cw; valid while the mode is MODE_CW or MODE_CWR).  shape: the keying taps (sr.keyshape);
        offset_step: the pitch as a phase increment per OUTPUT sample; side_step: per AUDIO sample, one value or [channels].
        Returns the status code."""
        g = TxCwConfig()
        taps = np.ascontiguousarray(shape, np.float32).reshape(-1)
        g.struct_size, g.ns_taps, g.shape_coeffs = C.sizeof(TxCwConfig), taps.size, taps.ctypes.data_as(f32p)
        g.amplitude, g.offset_step, g.side_level, g.side_mix, g.hang_blocks, g.reserved = amplitude, int(offset_step), side_level, int(side_mix), int(hang_blocks), 0
        steps = None
        if np.ndim(side_step):
            steps = np.ascontiguousarray(side_step, np.uint32)
            if steps.shape != (self.cfg.channels,):
                raise ValueError("side_step: one value or [channels]")
            g.side_step = steps.ctypes.data_as(u32p)
        else:
            g.side_step_all = int(side_step)
        rc = self.L.selenite_tx_set_cw(self.h, C.byref(g))
        if rc == 0:
            self._cw_ns = taps.size
        return rc

    def clear_cw(self):
        """selenite_tx_set_cw(S, NULL): keyed CW off again"""
        return self.L.selenite_tx_set_cw(self.h, None)

    def process_key(self, d_key, d_iq, d_side, block_size, q15=False):
        """key states [channels][block_size] uint8 -> I/Q [channels][block_size * interp][2] and, unless d_side is None, the sidetone
        [channels][block_size]; device pointers (f32, or int16 with q15=True), asynchronous.  Returns the status code."""
        f = self.L.selenite_tx_process_key_q15_device if q15 else self.L.selenite_tx_process_key_f32_device
        return f(self.h, d_key, d_iq, d_side, block_size)

    def process_key_host(self, key, side=None, q15=False):
        """the host entries: key [channels][n] uint8 -> (status, I/Q, sidetone or None); `side` is the buffer the sidetone is written or
        mixed into (a copy is returned)"""
        key = np.ascontiguousarray(key, np.uint8)
        c, bs = key.shape
        dt = np.int16 if q15 else np.float32
        out = np.zeros((c, bs * self.cfg.interp, 2), dt)
        sd = None if side is None else np.array(side, dt, order="C")
        f = self.L.selenite_tx_process_key_q15 if q15 else self.L.selenite_tx_process_key_f32
        rc = f(self.h, key.ctypes.data, out.ctypes.data, None if sd is None else sd.ctypes.data, bs)
        return rc, out, sd

    def _cw_shapes(self):
        return dict(channel_rows(TxCwStateView, self.cfg.channels), key_state=(self.cfg.channels, self._cw_ns - 1))

    def cw_state(self):
        return get_state(self.L.selenite_tx_get_cw_state, self.h, TxCwStateView, self._cw_shapes(),
                         "selenite_tx_get_cw_state: keyed CW is not configured (set_cw)")

    def set_cw_state(self, a):
        """members that are missing from `a` are left as they are"""
        set_state(self.L.selenite_tx_set_cw_state, self.h, TxCwStateView, self._cw_shapes(), a,
                  "selenite_tx_set_cw_state: keyed CW is not configured (set_cw)")

    def cw_txon(self):
        """device pointer of the break-in flags, uint32 [channels] (None before set_cw)"""
        return self.L.selenite_tx_cw_txon_device(self.h)

    def time_process_key(self, d_key, d_iq, d_side, block_size, iters):
        ms = C.c_float()
        rc = self.L.selenite_tx_time_process_key_device(self.h, d_key, d_iq, d_side, block_size, iters, C.byref(ms))
        if rc:
            raise RxError(rc, self.error())
        return ms.value

    def set_in(self, M=1, coeffs=None, pick=IN_MONO, gain=1.0, vox=None):
        """the audio input stage (selenite_tx_set_in): slot-rate frames -> pick -> gain -> arm_fir_decimate_f32 by M -> VOX -> the chain.
        coeffs: the decimator's taps in CMSIS order (None or empty: no FIR, M = 1 only); vox: None (off) or a dict of
        selenite_rx_meter_config fields (gate, hang, attack, decay, open_level, close_level, level_init; sense defaults to SQ_ABOVE).
        Returns the status code."""
        g = TxInConfig()
        taps = np.zeros(0, np.float32) if coeffs is None else np.ascontiguousarray(coeffs, np.float32).reshape(-1)
        g.struct_size, g.M, g.nd_taps, g.pick, g.gain, g.reserved = C.sizeof(TxInConfig), int(M), taps.size, int(pick), gain, 0
        g.coeffs = taps.ctypes.data_as(f32p) if taps.size else None
        if vox is not None:
            v = dict(sense=SQ_ABOVE, gate=0, hang=0, attack=0.5, decay=0.125, open_level=1e-6, close_level=5e-7, level_init=0.0)
            v.update(vox)
            g.vox = 1
            g.meter.struct_size = C.sizeof(MeterConfig)
            for k, x in v.items():
                setattr(g.meter, k, x)
        rc = self.L.selenite_tx_set_in(self.h, C.byref(g))
        if rc == 0:
            self._in_nt, self._in_M, self._in_fw = taps.size, int(M), 1 if int(pick) == IN_MONO else 2
        return rc

    def clear_in(self):
        """selenite_tx_set_in(S, NULL): the input stage off again"""
        return self.L.selenite_tx_set_in(self.h, None)

    def process_frames(self, d_frames, d_iq, block_size, kind=IN_F32):
        """frames [channels][block_size * M * (1 or 2)] -> I/Q [channels][block_size * interp][2]; device pointers, asynchronous.
        kind: IN_F32 (f32 frames, f32 I/Q), IN_Q15 (int16, int16) or IN_Q15_F32 (int16 frames, f32 I/Q).  Returns the status code."""
        f = (self.L.selenite_tx_process_frames_f32_device, self.L.selenite_tx_process_frames_q15_device,
             self.L.selenite_tx_process_frames_q15_f32_device)[kind]
        return f(self.h, d_frames, d_iq, block_size)

    def process_frames_host(self, frames, q15=False):
        """the host entries: frames [channels][n * M * (1 or 2)] -> (status, I/Q)"""
        dt = np.int16 if q15 else np.float32
        frames = np.ascontiguousarray(frames, dt)
        c = frames.shape[0]
        bs = frames[0].size // (self._in_M * self._in_fw)
        out = np.zeros((c, bs * self.cfg.interp, 2), dt)
        f = self.L.selenite_tx_process_frames_q15 if q15 else self.L.selenite_tx_process_frames_f32
        rc = f(self.h, frames.ctypes.data, out.ctypes.data, bs)
        return rc, out

    def _in_shapes(self):
        return dict(channel_rows(TxInStateView, self.cfg.channels), dec_state=(self.cfg.channels, max(self._in_nt - 1, 0)))

    def in_state(self):
        return get_state(self.L.selenite_tx_get_in_state, self.h, TxInStateView, self._in_shapes(),
                         "selenite_tx_get_in_state: the input stage is not configured (set_in)")

    def set_in_state(self, a):
        """members that are missing from `a` are left as they are"""
        set_state(self.L.selenite_tx_set_in_state, self.h, TxInStateView, self._in_shapes(), a,
                  "selenite_tx_set_in_state: the input stage is not configured (set_in)")

    def in_vox(self):
        """device pointer of the VOX flags, uint32 [channels] (None before set_in)"""
        return self.L.selenite_tx_in_vox_device(self.h)

    def in_audio_device(self):
        """device pointer of the stage's output of the last frame call, [channels][block_size] in the entry's audio type (None before it)"""
        return self.L.selenite_tx_in_audio_device(self.h)

    def time_in_stage(self, d_frames, block_size, iters, kind=IN_F32):
        """mean ms of the stage kernel alone over `iters` launches"""
        ms = C.c_float()
        rc = self.L.selenite_tx_time_in_stage_device(self.h, d_frames, kind, block_size, iters, C.byref(ms))
        if rc:
            raise RxError(rc, self.error())
        return ms.value

    def set_keyer(self, mode=KEYER_IAMBIC_B, unit=720, ring=256, codes=None, reserved=0):
        """the keyer stage in front of the keyed CW path (selenite_tx_set_keyer; needs set_cw).  unit: audio samples per dit, one value
        or [channels]; ring: text bytes per channel; codes: morse_codes() of another table, None = the built-in one.  Returns the status code."""
        g = TxKeyerConfig()
        g.struct_size, g.mode, g.ring, g.reserved = C.sizeof(TxKeyerConfig), int(mode), int(ring), int(reserved)
        units = table = None
        if np.ndim(unit):
            units = np.ascontiguousarray(unit, np.uint32)
            if units.shape != (self.cfg.channels,):
                raise ValueError("unit: one value or [channels]")
            g.unit = units.ctypes.data_as(u32p)
        else:
            g.unit_all = int(unit)
        if codes is not None:
            table = np.ascontiguousarray(codes, np.uint8)
            if table.shape != (256,):
                raise ValueError("codes: uint8 [256]")
            g.codes = table.ctypes.data_as(u8p)
        rc = self.L.selenite_tx_set_keyer(self.h, C.byref(g))
        if rc == 0:
            self._keyer_ring = int(ring)
        return rc

    def clear_keyer(self):
        """selenite_tx_set_keyer(S, NULL): the keyer off again"""
        return self.L.selenite_tx_set_keyer(self.h, None)

    def keyer_send(self, text, first_channel=0, n_channels=None):
        """queue text: one str / bytes for every channel of the range, or a list of n_channels texts of one length.  Returns the status
        code (LENGTH_ERROR: a channel lacks room; nothing was written)."""
        n = self.cfg.channels - first_channel if n_channels is None else int(n_channels)
        enc = lambda x: x.encode("latin-1") if isinstance(x, str) else bytes(x)
        if isinstance(text, (str, bytes, bytearray)):
            buf, per = np.frombuffer(enc(text), np.uint8), 0
            ln = buf.size
        else:
            rows = [enc(x) for x in text]
            if len(rows) != n or any(len(r) != len(rows[0]) for r in rows):
                raise ValueError("keyer_send: n_channels texts of one length")
            buf, per, ln = np.frombuffer(b"".join(rows), np.uint8), 1, len(rows[0])
        return self.L.selenite_tx_keyer_send(self.h, int(first_channel), n, buf.ctypes.data if buf.size else None, ln, per)

    def keyer_pending(self):
        """characters queued and not yet begun, uint32 [channels]"""
        a = np.zeros(self.cfg.channels, np.uint32)
        rc = self.L.selenite_tx_keyer_pending(self.h, a.ctypes.data_as(u32p))
        if rc:
            raise RxError(rc, "selenite_tx_keyer_pending: the keyer is not configured (set_keyer)")
        return a

    def process_paddles(self, d_paddles, d_iq, d_side, block_size, q15=False):
        """paddle bytes [channels][block_size] uint8 (bit 0 dit, bit 1 dah, bit 2 straight key; None: the text memory alone) -> the keyer
        -> the keyed CW path: I/Q and sidetone as process_key writes them; device pointers, asynchronous.  Returns the status code."""
        f = self.L.selenite_tx_process_paddles_q15_device if q15 else self.L.selenite_tx_process_paddles_f32_device
        return f(self.h, d_paddles, d_iq, d_side, block_size)

    def process_paddles_host(self, paddles, block_size=None, side=None, q15=False):
        """the host entries: paddles [channels][n] uint8, or None with block_size -> (status, I/Q, sidetone or None)"""
        if paddles is not None:
            paddles = np.ascontiguousarray(paddles, np.uint8)
            block_size = paddles.shape[1]
        c, bs = self.cfg.channels, int(block_size)
        dt = np.int16 if q15 else np.float32
        out = np.zeros((c, bs * self.cfg.interp, 2), dt)
        sd = None if side is None else np.array(side, dt, order="C")
        f = self.L.selenite_tx_process_paddles_q15 if q15 else self.L.selenite_tx_process_paddles_f32
        rc = f(self.h, None if paddles is None else paddles.ctypes.data, out.ctypes.data, None if sd is None else sd.ctypes.data, bs)
        return rc, out, sd

    def keyer_run(self, d_paddles, d_key, block_size):
        """the stage alone: key bytes [channels][block_size] into d_key; device pointers, asynchronous.  Returns the status code."""
        return self.L.selenite_tx_keyer_run_device(self.h, d_paddles, d_key, block_size)

    def keyer_key_device(self):
        """device pointer of the key bytes of the last paddle call, uint8 [channels][block_size] (None before it)"""
        return self.L.selenite_tx_keyer_key_device(self.h)

    def _keyer_shapes(self):
        return dict(channel_rows(TxKeyerStateView, self.cfg.channels), text=(self.cfg.channels, self._keyer_ring))

    def keyer_state(self):
        return get_state(self.L.selenite_tx_get_keyer_state, self.h, TxKeyerStateView, self._keyer_shapes(),
                         "selenite_tx_get_keyer_state: the keyer is not configured (set_keyer)")

    def set_keyer_state(self, a):
        """members that are missing from `a` are left as they are"""
        set_state(self.L.selenite_tx_set_keyer_state, self.h, TxKeyerStateView, self._keyer_shapes(), a,
                  "selenite_tx_set_keyer_state: the keyer is not configured (set_keyer)")

    def time_keyer_stage(self, d_paddles, block_size, iters):
        """mean ms of the stage kernel alone over `iters` launches behind one untimed launch; the state moves"""
        ms = C.c_float()
        rc = self.L.selenite_tx_time_keyer_stage_device(self.h, d_paddles, block_size, iters, C.byref(ms))
        if rc:
            raise RxError(rc, self.error())
        return ms.value

    def time_process(self, d_src, d_dst, block_size, iters):
        ms = C.c_float()
        rc = self.L.selenite_tx_time_process_device(self.h, d_src, d_dst, block_size, iters, C.byref(ms))
        if rc:
            raise RxError(rc, self.error())
        return ms.value

    def close(self):
        if self.h:
            self.L.selenite_tx_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
