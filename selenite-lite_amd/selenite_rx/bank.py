"""The polyphase filter banks: Channelizer (include/selenite_chan.h), Combiner (include/selenite_comb.h) and their prototype designers."""
import ctypes as C

import numpy as np

from . import RxError, _fp, lib
from ._state import get_state, set_state
from . import ChanConfig, ChanStateView, CombConfig, CombStateView, u32p


def design_chan_prototype(fft_len, taps_per_branch, width=1.0):
    """the channeliser's prototype g[K P] in CMSIS order: design_lowpass(K P, 0.5 * width / K), width in channel spacings (0 < width <= 2)"""
    g = np.empty(fft_len * taps_per_branch, np.float32)
    rc = lib().selenite_chan_design_prototype(_fp(g), fft_len, taps_per_branch, float(width))
    if rc:
        raise ValueError("selenite_chan_design_prototype: %d" % rc)
    return g


class _FilterBank:
    """What Channelizer and Combiner share: one object of the C prefix `_prefix` (selenite_chan_ / selenite_comb_) whose state is a history
    of shape _hist_shape() and a position.  Device pointers only (DeviceBuffer.ptr)."""
    _prefix = None
    _config = None
    _state_view = None

    def _init(self, bands, fft_len, oversample, taps_per_branch, coeffs, bins, *own_fields):
        self.L = lib()
        coeffs = np.ascontiguousarray(coeffs, np.float32)
        assert coeffs.size == fft_len * taps_per_branch, coeffs.shape
        b = None if bins is None else np.ascontiguousarray(bins, np.uint32)
        self.bands, self.fft_len, self.oversample, self.taps_per_branch = int(bands), int(fft_len), int(oversample), int(taps_per_branch)
        self.n_bins = self.fft_len if b is None else int(b.size)
        cfg = self._config(C.sizeof(self._config), self.bands, self.fft_len, self.oversample, self.taps_per_branch, self.n_bins, *own_fields, 0,
                           _fp(coeffs), None if b is None else b.ctypes.data_as(u32p))
        self.h = C.c_void_p()
        rc = self._c("init")(C.byref(self.h), C.byref(cfg))
        if rc:
            raise RxError(rc, "%sinit failed (no GPU, or a bad configuration)" % self._prefix)

    def _c(self, name):
        return getattr(self.L, self._prefix + name)

    def error(self):
        return self._c("error_string")(self.h).decode()

    def _raise(self, rc):
        if rc:
            raise RxError(rc, self.error())

    def status(self):
        return self._c("status")(self.h)

    def check(self):
        self._raise(self.status())

    def out_len(self, block_size):
        return self._c("out_len")(self.h, block_size)

    def process_device(self, d_src, d_dst, block_size):
        """f32 in, f32 out, asynchronous; a refused call raises"""
        self._c("process_f32_device")(self.h, d_src, d_dst, block_size)
        self.check()

    def process_q15_device(self, d_src, d_dst, block_size):
        """the int16 side of the object (Channelizer: the input; Combiner: the output)"""
        self._c("process_q15_device")(self.h, d_src, d_dst, block_size)
        self.check()

    def set_stream(self, stream_ptr):
        return self._c("set_stream")(self.h, stream_ptr)

    def sync(self):
        self._raise(self._c("sync")(self.h))

    def reset(self):
        return self._c("reset")(self.h)

    def _shapes(self):
        return dict(history=self._hist_shape(), position=(1,))

    def state(self):
        return get_state(self._c("get_state"), self.h, self._state_view, self._shapes(), self.error)

    def set_state(self, a):
        set_state(self._c("set_state"), self.h, self._state_view, self._shapes(), a, self.error)

    def close(self):
        if self.h:
            self._c("free")(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Channelizer(_FilterBank):
    """One selenite_chan object (include/selenite_chan.h): `bands` wideband I/Q streams in, bands * n_bins channels out, in the layout
    Rx.process_device reads: d_src [bands][block_size][2] f32 (process_q15_device: int16, arm_q15_to_float) -> d_dst
    [bands * n_bins][block_size / D][2] f32."""
    _prefix, _config, _state_view = "selenite_chan_", ChanConfig, ChanStateView

    def __init__(self, bands, fft_len, oversample, taps_per_branch, coeffs, bins=None):
        self._init(bands, fft_len, oversample, taps_per_branch, coeffs, bins)
        self.decim = self.fft_len // self.oversample
        self.hist_len = self.fft_len * self.taps_per_branch - self.decim

    def _hist_shape(self):
        return (self.bands, self.hist_len, 2)

    def out_channels(self):
        return self._c("out_channels")(self.h)


def design_comb_prototype(fft_len, taps_per_branch, width=1.0, oversample=1):
    """the combiner's prototype g[K P] in CMSIS order: design_chan_prototype(K, P, width) times K * D, D = K / oversample, so that a constant
    on channel 0 leaves as that constant (the 1 / K is arm_cfft_f32's own)"""
    g = np.empty(fft_len * taps_per_branch, np.float32)
    rc = lib().selenite_comb_design_prototype(_fp(g), fft_len, taps_per_branch, float(width), oversample)
    if rc:
        raise ValueError("selenite_comb_design_prototype: %d" % rc)
    return g


class Combiner(_FilterBank):
    """One selenite_comb object (include/selenite_comb.h): bands * n_bins TX channel rows in, in the layout Tx.process_device writes, `bands`
    wideband I/Q streams out: d_src [bands * n_bins][block_size][2] f32 -> d_dst [bands][block_size * D][2] f32 (process_q15_device: int16,
    arm_float_to_q15, saturating)."""
    _prefix, _config, _state_view = "selenite_comb_", CombConfig, CombStateView

    def __init__(self, bands, fft_len, oversample, taps_per_branch, coeffs, bins=None, q15_rounding=0):
        self._init(bands, fft_len, oversample, taps_per_branch, coeffs, bins, int(q15_rounding))
        self.interp = self.fft_len // self.oversample
        self.hist_len = self.taps_per_branch * self.oversample - 1

    def _hist_shape(self):
        return (self.bands * self.n_bins, self.hist_len, 2)

    def in_channels(self):
        return self._c("in_channels")(self.h)
