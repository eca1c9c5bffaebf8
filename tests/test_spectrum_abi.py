"""CPU: the spectrum tap's C-ABI (include/selenite_rx.h: selenite_rx_set_spectrum, selenite_rx_get_spectrum, selenite_rx_spectrum_device,
selenite_rx_get_spectrum_state, selenite_rx_set_spectrum_state, selenite_rx_spectrum_twiddles, selenite_rx_design_window) is exported and
bound, the ctypes structs lay out as the C compiler does, and the entry points refuse a NULL instance without touching a GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import rxcommon as rc
import selenite_rx as sr

NAMES = ["selenite_rx_set_spectrum", "selenite_rx_get_spectrum", "selenite_rx_spectrum_device", "selenite_rx_get_spectrum_state",
         "selenite_rx_set_spectrum_state", "selenite_rx_spectrum_twiddles", "selenite_rx_design_window"]


def test_symbols_exported_and_bound():
    L = sr.lib()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in sr.ABI_SYMBOLS
    assert (sr.WINDOW_HANN, sr.WINDOW_BLACKMAN_HARRIS) == (0, 1)
    text = open(os.path.join(rc.ROOT, "include", "selenite_rx.h")).read()
    assert "#define SELENITE_RX_WINDOW_HANN            0" in text and "#define SELENITE_RX_WINDOW_BLACKMAN_HARRIS 1" in text
    assert "#define SELENITE_RX_ABI_VERSION 2" in text and L.selenite_rx_abi_version() == 2
    for m in ("set_spectrum", "spectrum", "spectrum_device", "spectrum_state", "set_spectrum_state"):
        assert callable(getattr(sr.Rx, m))


C_SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "selenite_rx.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_rx_spec_config), offsetof(selenite_rx_spec_config, struct_size),
           offsetof(selenite_rx_spec_config, fft_len), offsetof(selenite_rx_spec_config, stride), offsetof(selenite_rx_spec_config, average),
           offsetof(selenite_rx_spec_config, alpha), offsetof(selenite_rx_spec_config, window));
    printf("%zu %zu %zu %zu\n", sizeof(selenite_rx_spec_state_view), offsetof(selenite_rx_spec_state_view, rows),
           offsetof(selenite_rx_spec_state_view, pending), offsetof(selenite_rx_spec_state_view, position));
    return 0;
}
"""


def test_ctypes_layout_equals_offsetof():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write(C_SNIPPET)
        subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(rc.ROOT, "include"), "-o", exe, src], check=True)
        lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    assert [int(v) for v in lines[0].split()] == [C.sizeof(sr.SpecConfig)] + [
        getattr(sr.SpecConfig, f).offset for f in ("struct_size", "fft_len", "stride", "average", "alpha", "window")]
    assert [int(v) for v in lines[1].split()] == [C.sizeof(sr.SpecStateView)] + [
        getattr(sr.SpecStateView, f).offset for f in ("rows", "pending", "position")]


def test_null_instance_is_an_argument_error():
    L = sr.lib()
    g = sr.SpecConfig()
    g.struct_size, g.fft_len, g.stride, g.average, g.alpha = C.sizeof(sr.SpecConfig), 512, 1, 0, 1.0
    assert L.selenite_rx_set_spectrum(None, C.byref(g)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_spectrum(None, None) == sr.ARGUMENT_ERROR
    rows, n = np.zeros(512, np.float32), C.c_uint64(7)
    assert L.selenite_rx_get_spectrum(None, rows.ctypes.data_as(sr.f32p), C.byref(n)) == sr.ARGUMENT_ERROR
    assert n.value == 7 and not rows.any()
    assert L.selenite_rx_spectrum_device(None) is None
    v = sr.SpecStateView(rows.ctypes.data_as(sr.f32p), None, None)
    assert L.selenite_rx_get_spectrum_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_spectrum_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_get_spectrum_state(None, None) == sr.ARGUMENT_ERROR
