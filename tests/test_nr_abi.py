"""CPU: the NLMS stage's C-ABI (include/selenite_rx.h: selenite_rx_set_nr, selenite_rx_get_nr_state, selenite_rx_set_nr_state) is
exported, the ctypes structs lay out as the C compiler does, and the entry points refuse a NULL instance without touching a GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

import rxcommon as rc
import selenite_rx as sr

NAMES = ["selenite_rx_set_nr", "selenite_rx_get_nr_state", "selenite_rx_set_nr_state"]


def test_symbols_exported_and_bound():
    L = sr.lib()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in sr.ABI_SYMBOLS
    assert (sr.NR_OFF, sr.NR_DENOISE, sr.NR_NOTCH) == (0, 1, 2)
    text = open(os.path.join(rc.ROOT, "include", "selenite_rx.h")).read()
    for k, v in (("OFF", 0), ("DENOISE", 1), ("NOTCH", 2)):
        assert "#define SELENITE_RX_NR_%-7s %d" % (k, v) in text


C_SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "selenite_rx.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_rx_nr_config), offsetof(selenite_rx_nr_config, struct_size),
           offsetof(selenite_rx_nr_config, kind), offsetof(selenite_rx_nr_config, num_taps), offsetof(selenite_rx_nr_config, delay),
           offsetof(selenite_rx_nr_config, mu), offsetof(selenite_rx_nr_config, coeffs_init));
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(selenite_rx_nr_state_view), offsetof(selenite_rx_nr_state_view, coeffs),
           offsetof(selenite_rx_nr_state_view, window), offsetof(selenite_rx_nr_state_view, delay),
           offsetof(selenite_rx_nr_state_view, energy), offsetof(selenite_rx_nr_state_view, x0));
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
    cfg = [int(v) for v in lines[0].split()]
    view = [int(v) for v in lines[1].split()]
    assert cfg == [C.sizeof(sr.NrConfig)] + [getattr(sr.NrConfig, f).offset
                                             for f in ("struct_size", "kind", "num_taps", "delay", "mu", "coeffs_init")]
    assert view == [C.sizeof(sr.NrStateView)] + [getattr(sr.NrStateView, f).offset for f in ("coeffs", "window", "delay", "energy", "x0")]


def test_null_instance_is_an_argument_error():
    L = sr.lib()
    g = sr.NrConfig()
    g.struct_size, g.kind, g.num_taps, g.delay, g.mu = C.sizeof(sr.NrConfig), sr.NR_DENOISE, 32, 16, 0.05
    assert L.selenite_rx_set_nr(None, C.byref(g)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_nr(None, None) == sr.ARGUMENT_ERROR
    v = sr.NrStateView()
    assert L.selenite_rx_get_nr_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_nr_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_get_nr_state(None, None) == sr.ARGUMENT_ERROR
