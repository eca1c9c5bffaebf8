"""Ring: the slot ring buffers either side of the DSP (include/selenite_ring.h)."""
import ctypes as C

import numpy as np

from . import RxError, lib
from ._state import get_state, set_state
from . import RingStateView


class Ring:
    """`channels` reference DSP_Buff_TypeDef rings in HBM (include/selenite_ring.h; dsp_if.c:83-340).
    Method names and size units follow the reference functions they replace."""

    def __init__(self, channels, frames=384):
        self.L = lib()
        self.channels, self.frames = int(channels), int(frames)
        self.h = C.c_void_p()
        rc = self.L.selenite_ring_init(C.byref(self.h), self.channels, self.frames)
        if rc:
            raise RxError(rc, "selenite_ring_init failed (no GPU, or bad channels/frames)")

    def error(self):
        return self.L.selenite_ring_error_string(self.h).decode()

    def check(self):
        rc = self.L.selenite_ring_status(self.h)
        if rc:
            raise RxError(rc, self.error())

    def _packet(self, arr, words):
        arr = np.ascontiguousarray(arr, np.int16)
        assert arr.shape == (self.channels, words), arr.shape
        return arr

    def in_write(self, pkt):                       # DSP_In_Buff_Write (words)
        pkt = np.ascontiguousarray(pkt, np.int16)
        self.L.selenite_ring_in_write(self.h, self._packet(pkt, pkt.shape[1]).ctypes.data, pkt.shape[1])
        self.check()

    def out_write(self, pkt):                      # DSP_Out_Buff_Write (bytes)
        pkt = np.ascontiguousarray(pkt, np.int16)
        self.L.selenite_ring_out_write(self.h, self._packet(pkt, pkt.shape[1]).ctypes.data, 2 * pkt.shape[1])
        self.check()

    def in_read(self, size_bytes):                 # DSP_In_Buff_Read (bytes)
        out = np.empty((self.channels, size_bytes // 2), np.int16)
        self.L.selenite_ring_in_read(self.h, out.ctypes.data, size_bytes)
        self.check()
        return out

    def out_read(self, size_words):                # DSP_Out_Buff_Read (words)
        out = np.empty((self.channels, size_words), np.int16)
        self.L.selenite_ring_out_read(self.h, out.ctypes.data, size_words)
        self.check()
        return out

    def mute(self):
        self.L.selenite_ring_mute(self.h)
        self.L.selenite_ring_sync(self.h)
        self.check()

    def _shapes(self):
        c = self.channels
        return dict(i=(c, self.frames), q=(c, self.frames), buff_enable=(c,), rd_ptr=(c,), wr_ptr=(c,))

    def state(self):
        return get_state(self.L.selenite_ring_get_state, self.h, RingStateView, self._shapes(), self.error)

    def set_state(self, a):
        set_state(self.L.selenite_ring_set_state, self.h, RingStateView, self._shapes(), a, self.error)

    def time_pair(self, d_src, d_dst, size_words, iters):
        ms = C.c_float()
        rc = self.L.selenite_ring_time_device(self.h, d_src, d_dst, size_words, iters, C.byref(ms))
        if rc:
            raise RxError(rc, self.error())
        return ms.value

    def close(self):
        if self.h:
            self.L.selenite_ring_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
