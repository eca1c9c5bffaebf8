"""CPU: the C-ABI of the audio input stage of the TX chain (include/selenite_tx_in.h, which include/selenite_tx.h includes) is exported and
bound, the ctypes structs lay out as the C compiler does, the entry points refuse a NULL instance without touching a GPU, and the older
headers still declare what they declared.  (That every bad field and call is refused with nothing written needs an instance:
tests/test_gpu_txin.py.)"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

import rxcommon as rc
import selenite_rx as sr

NAMES = {"selenite_tx_set_in": 2, "selenite_tx_get_in_state": 2, "selenite_tx_set_in_state": 2,
         "selenite_tx_process_frames_f32_device": 4, "selenite_tx_process_frames_q15_device": 4, "selenite_tx_process_frames_q15_f32_device": 4,
         "selenite_tx_process_frames_f32": 4, "selenite_tx_process_frames_q15": 4, "selenite_tx_in_vox_device": 1,
         "selenite_tx_in_audio_device": 1, "selenite_tx_time_in_stage_device": 6}
CONFIG_FIELDS = ("struct_size", "M", "nd_taps", "pick", "coeffs", "gain", "vox", "meter", "reserved")
VIEW_FIELDS = ("dec_state", "level", "open", "hold", "opens", "open_blocks")


def declared(header):
    text = open(os.path.join(rc.ROOT, "include", header)).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(selenite_tx_[a-z0-9_]+)\s*\(", code)))


def test_symbols_exported_and_bound():
    L = sr.lib()
    assert declared("selenite_tx_in.h") == sorted(NAMES) == sorted(sr.TXIN_ABI_SYMBOLS)
    for n, nargs in NAMES.items():
        assert hasattr(L, n), n
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == nargs, n
    assert '#include "selenite_tx_in.h"' in open(os.path.join(rc.ROOT, "include", "selenite_tx.h")).read()      # one header to include
    for m in ("set_in", "clear_in", "process_frames", "process_frames_host", "in_state", "set_in_state", "in_vox", "in_audio_device",
              "time_in_stage"):
        assert callable(getattr(sr.Tx, m))
    assert (sr.IN_MONO, sr.IN_LEFT, sr.IN_RIGHT, sr.IN_MIX) == (0, 1, 2, 3) and (sr.IN_F32, sr.IN_Q15, sr.IN_Q15_F32) == (0, 1, 2)


def test_the_older_headers_declare_what_they_declared():
    assert declared("selenite_tx.h") == sorted(sr.TX_ABI_SYMBOLS) and len(sr.TX_ABI_SYMBOLS) == 16
    assert declared("selenite_tx_cw.h") == sorted(sr.TXCW_ABI_SYMBOLS) and declared("selenite_tx_fm.h") == sorted(sr.TXFM_ABI_SYMBOLS)
    assert not set(NAMES) & (set(sr.TX_ABI_SYMBOLS) | set(sr.TXFM_ABI_SYMBOLS) | set(sr.TXCW_ABI_SYMBOLS))


C_SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "selenite_tx.h"
#define O(f) offsetof(selenite_tx_in_config, f)
#define V(f) offsetof(selenite_tx_in_state_view, f)
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_tx_in_config), O(struct_size), O(M), O(nd_taps), O(pick), O(coeffs),
           O(gain), O(vox), O(meter), O(reserved));
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_tx_in_state_view), V(dec_state), V(level), V(open), V(hold), V(opens), V(open_blocks));
    printf("%zu %zu %zu %zu\n", sizeof(selenite_tx_config), sizeof(selenite_tx_fm_config), sizeof(selenite_tx_cw_config),
           sizeof(selenite_rx_meter_config));
    printf("%d %d %d %d %d %d %d\n", SELENITE_TX_IN_MONO, SELENITE_TX_IN_LEFT, SELENITE_TX_IN_RIGHT, SELENITE_TX_IN_MIX, SELENITE_TX_IN_F32,
           SELENITE_TX_IN_Q15, SELENITE_TX_IN_Q15_F32);
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
    assert [int(v) for v in lines[0].split()] == [C.sizeof(sr.TxInConfig)] + [getattr(sr.TxInConfig, f).offset for f in CONFIG_FIELDS]
    assert [int(v) for v in lines[1].split()] == [C.sizeof(sr.TxInStateView)] + [getattr(sr.TxInStateView, f).offset for f in VIEW_FIELDS]
    assert C.sizeof(sr.TxInConfig) == 72 and sr.TxInConfig.coeffs.offset == 16 and sr.TxInConfig.meter.offset == 32
    assert C.sizeof(sr.TxInStateView) == 48
    assert [f for f, _ in sr.TxInConfig._fields_] == list(CONFIG_FIELDS) and [f for f, _ in sr.TxInStateView._fields_] == list(VIEW_FIELDS)
    assert [int(v) for v in lines[2].split()] == [C.sizeof(sr.TxConfig), C.sizeof(sr.TxFmConfig), C.sizeof(sr.TxCwConfig),
                                                  C.sizeof(sr.MeterConfig)] == [104, 40, 56, 36]      # the older structs do not change
    assert [int(v) for v in lines[3].split()] == [sr.IN_MONO, sr.IN_LEFT, sr.IN_RIGHT, sr.IN_MIX, sr.IN_F32, sr.IN_Q15, sr.IN_Q15_F32]


def test_null_instance_is_an_argument_error():
    L = sr.lib()
    taps = sr.design_lowpass(8, 0.2)
    g = sr.TxInConfig()
    g.struct_size, g.M, g.nd_taps, g.coeffs, g.gain = C.sizeof(sr.TxInConfig), 2, 8, taps.ctypes.data_as(sr.f32p), 1.0
    assert L.selenite_tx_set_in(None, C.byref(g)) == sr.ARGUMENT_ERROR
    assert L.selenite_tx_set_in(None, None) == sr.ARGUMENT_ERROR
    lv = np.full(4, 7, np.float32)
    v = sr.TxInStateView()
    v.level = lv.ctypes.data_as(sr.f32p)
    assert L.selenite_tx_get_in_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_tx_set_in_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_tx_get_in_state(None, None) == sr.ARGUMENT_ERROR
    assert (lv == 7).all()
    fr, iq = np.ones(128, np.float32), np.full((64, 2), 3, np.float32)
    for n in ("f32_device", "q15_device", "q15_f32_device", "f32", "q15"):
        assert getattr(L, "selenite_tx_process_frames_" + n)(None, fr.ctypes.data, iq.ctypes.data, 64) == sr.ARGUMENT_ERROR
    ms = C.c_float(-1.0)
    assert L.selenite_tx_time_in_stage_device(None, fr.ctypes.data, 0, 64, 1, C.byref(ms)) == sr.ARGUMENT_ERROR
    assert (iq == 3).all() and ms.value == -1.0
    assert L.selenite_tx_in_vox_device(None) is None and L.selenite_tx_in_audio_device(None) is None
