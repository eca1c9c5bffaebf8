"""CPU: the C-ABI of the keyed CW path of the TX chain (include/selenite_tx_cw.h, which include/selenite_tx.h includes) is exported and bound,
the ctypes structs lay out as the C compiler does, the entry points refuse a NULL instance without touching a GPU, and selenite_tx.h
itself still declares its 16 functions.  (That every bad field and call is refused with nothing written needs an instance:
tests/test_gpu_txcw.py.)"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

import rxcommon as rc
import selenite_rx as sr

NAMES = {"selenite_tx_set_cw": 2, "selenite_tx_get_cw_state": 2, "selenite_tx_set_cw_state": 2,
         "selenite_tx_process_key_f32_device": 5, "selenite_tx_process_key_q15_device": 5, "selenite_tx_process_key_f32": 5,
         "selenite_tx_process_key_q15": 5, "selenite_tx_cw_txon_device": 1, "selenite_tx_time_process_key_device": 7,
         "selenite_tx_design_keyshape": 2}
CONFIG_FIELDS = ("struct_size", "ns_taps", "shape_coeffs", "amplitude", "offset_step", "side_level", "side_step_all", "side_step", "side_mix",
                 "hang_blocks", "reserved")
VIEW_FIELDS = ("key_state", "side_phase", "tx_on", "hold")


def declared(header):
    text = open(os.path.join(rc.ROOT, "include", header)).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(selenite_tx_[a-z0-9_]+)\s*\(", code)))


def test_symbols_exported_and_bound():
    L = sr.lib()
    assert declared("selenite_tx_cw.h") == sorted(NAMES) == sorted(sr.TXCW_ABI_SYMBOLS)
    for n, nargs in NAMES.items():
        assert hasattr(L, n), n
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == nargs, n
    assert '#include "selenite_tx_cw.h"' in open(os.path.join(rc.ROOT, "include", "selenite_tx.h")).read()      # one header to include
    for m in ("set_cw", "process_key", "cw_state", "set_cw_state", "cw_txon"):
        assert callable(getattr(sr.Tx, m))
    assert callable(sr.keyshape)


def test_selenite_tx_h_still_declares_its_16_functions():
    names = declared("selenite_tx.h")
    assert len(names) == 16 and names == sorted(sr.TX_ABI_SYMBOLS)
    assert not set(names) & set(NAMES) and not set(sr.TXFM_ABI_SYMBOLS) & set(NAMES)


C_SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "selenite_tx.h"
#define O(f) offsetof(selenite_tx_cw_config, f)
#define V(f) offsetof(selenite_tx_cw_state_view, f)
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_tx_cw_config), O(struct_size), O(ns_taps), O(shape_coeffs),
           O(amplitude), O(offset_step), O(side_level), O(side_step_all), O(side_step), O(side_mix), O(hang_blocks), O(reserved));
    printf("%zu %zu %zu %zu %zu\n", sizeof(selenite_tx_cw_state_view), V(key_state), V(side_phase), V(tx_on), V(hold));
    printf("%zu %zu\n", sizeof(selenite_tx_config), sizeof(selenite_tx_fm_config));
    return 0;
}
"""


def test_ctypes_layout_equals_offsetof():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write(C_SNIPPET)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(rc.ROOT, "include"), "-o", exe, src], check=True)
        lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    assert [int(v) for v in lines[0].split()] == [C.sizeof(sr.TxCwConfig)] + [getattr(sr.TxCwConfig, f).offset for f in CONFIG_FIELDS]
    assert [int(v) for v in lines[1].split()] == [C.sizeof(sr.TxCwStateView)] + [getattr(sr.TxCwStateView, f).offset for f in VIEW_FIELDS]
    assert C.sizeof(sr.TxCwConfig) == 56 and sr.TxCwConfig.side_step.offset == 32 and C.sizeof(sr.TxCwStateView) == 32
    assert [f for f, _ in sr.TxCwConfig._fields_] == list(CONFIG_FIELDS) and [f for f, _ in sr.TxCwStateView._fields_] == list(VIEW_FIELDS)
    assert [int(v) for v in lines[2].split()] == [C.sizeof(sr.TxConfig), C.sizeof(sr.TxFmConfig)] == [104, 40]      # the older structs do not change


def test_null_instance_is_an_argument_error():
    L = sr.lib()
    taps = sr.keyshape(8)
    g = sr.TxCwConfig()
    g.struct_size, g.ns_taps, g.shape_coeffs, g.amplitude = C.sizeof(sr.TxCwConfig), 8, taps.ctypes.data_as(sr.f32p), 1.0
    assert L.selenite_tx_set_cw(None, C.byref(g)) == sr.ARGUMENT_ERROR
    assert L.selenite_tx_set_cw(None, None) == sr.ARGUMENT_ERROR
    sp = np.full(4, 7, np.uint32)
    v = sr.TxCwStateView()
    v.side_phase = sp.ctypes.data_as(sr.u32p)
    assert L.selenite_tx_get_cw_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_tx_set_cw_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_tx_get_cw_state(None, None) == sr.ARGUMENT_ERROR
    assert (sp == 7).all()
    key, iq, side = np.ones(64, np.uint8), np.full((64, 2), 3, np.float32), np.full(64, 3, np.float32)
    for n in ("f32_device", "q15_device", "f32", "q15"):
        assert getattr(L, "selenite_tx_process_key_" + n)(None, key.ctypes.data, iq.ctypes.data, side.ctypes.data, 64) == sr.ARGUMENT_ERROR
    ms = C.c_float(-1.0)
    assert L.selenite_tx_time_process_key_device(None, key.ctypes.data, iq.ctypes.data, None, 64, 1, C.byref(ms)) == sr.ARGUMENT_ERROR
    assert (iq == 3).all() and (side == 3).all() and ms.value == -1.0
    assert L.selenite_tx_cw_txon_device(None) is None
    assert L.selenite_tx_design_keyshape(0, taps.ctypes.data_as(sr.f32p)) == sr.ARGUMENT_ERROR
    assert L.selenite_tx_design_keyshape(8, None) == sr.ARGUMENT_ERROR
