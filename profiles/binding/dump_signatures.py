"""Print `symbol [restype, [argtypes]]`, one line each, of every declared symbol the loaded library exports, as lib() leaves it with nothing constructed.

Run with the selenite_rx package to examine first on sys.path.  A package from before the signature table (no selenite_rx.SIGNATURES)
bound part of the ABI elsewhere; those assignments are repeated here, as the issue asks, so that the two dumps compare like with like:
Tx.__init__ (16 symbols), Tx.kernel_name (1), and the two places the issue does not name, Ring.__init__ (18) and Rx.time_process_q15 (1).
"""
import ctypes as C
import json

import selenite_rx as sr

L = sr.lib()
if not hasattr(sr, "SIGNATURES"):
    vp = C.c_void_p
    L.selenite_tx_init.argtypes = [C.POINTER(vp), C.POINTER(sr.TxConfig)]
    L.selenite_tx_free.argtypes = [vp]
    L.selenite_tx_set_mode.argtypes = [vp, C.c_uint8]
    L.selenite_tx_status.argtypes = [vp]
    L.selenite_tx_error_string.argtypes = [vp]
    L.selenite_tx_error_string.restype = C.c_char_p
    for n in ("process_f32", "process_q15", "process_f32_device", "process_q15_device"):
        getattr(L, "selenite_tx_" + n).argtypes = [vp, vp, vp, C.c_uint32]
        getattr(L, "selenite_tx_" + n).restype = None
    L.selenite_tx_set_stream.argtypes = [vp, vp]
    L.selenite_tx_sync.argtypes = [vp]
    L.selenite_tx_get_state.argtypes = [vp, C.POINTER(sr.TxStateView)]
    L.selenite_tx_set_state.argtypes = [vp, C.POINTER(sr.TxStateView)]
    L.selenite_tx_reset.argtypes = [vp]
    L.selenite_tx_time_process_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    L.selenite_tx_kernel_name.argtypes = [vp]
    L.selenite_tx_kernel_name.restype = C.c_char_p
    L.selenite_ring_init.argtypes = [C.POINTER(vp), C.c_uint32, C.c_uint32]
    L.selenite_ring_free.argtypes = [vp]
    L.selenite_ring_status.argtypes = [vp]
    L.selenite_ring_error_string.argtypes = [vp]
    L.selenite_ring_error_string.restype = C.c_char_p
    L.selenite_ring_set_stream.argtypes = [vp, vp]
    L.selenite_ring_sync.argtypes = [vp]
    for n, a in (("in_write", C.c_uint16), ("in_read", C.c_uint32), ("out_write", C.c_uint32), ("out_read", C.c_uint16)):
        for f in (getattr(L, "selenite_ring_%s" % n), getattr(L, "selenite_ring_%s_device" % n)):
            f.argtypes, f.restype = [vp, vp, a], None
    L.selenite_ring_mute.argtypes = [vp]
    L.selenite_ring_mute.restype = None
    L.selenite_ring_get_state.argtypes = [vp, C.POINTER(sr.RingStateView)]
    L.selenite_ring_set_state.argtypes = [vp, C.POINTER(sr.RingStateView)]
    L.selenite_ring_time_device.argtypes = [vp, vp, vp, C.c_uint16, C.c_uint32, C.POINTER(C.c_float)]
    L.selenite_rx_time_process_q15_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]


def name(t):
    return None if t is None else t.__name__


out = {}
for key in sorted(k for k in dir(sr) if k.endswith("ABI_SYMBOLS")):
    for sym in getattr(sr, key):
        if hasattr(L, sym):
            f = getattr(L, sym)
            out[sym] = [name(f.restype), None if f.argtypes is None else [name(a) for a in f.argtypes]]
for sym in sorted(out):
    print(sym, json.dumps(out[sym]))
