"""CPU: the I/Q correction's C-ABI (include/selenite_rx.h: selenite_rx_set_iqc, selenite_rx_get_iqc_state, selenite_rx_set_iqc_state) is
exported and bound, the ctypes structs lay out as the C compiler does, and the entry points refuse a NULL instance without touching a GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import rxcommon as rc
import selenite_rx as sr

NAMES = ["selenite_rx_set_iqc", "selenite_rx_get_iqc_state", "selenite_rx_set_iqc_state"]
CONFIG_FIELDS = ("struct_size", "frame", "alpha", "dc_alpha", "p_max", "g_max", "min_power", "p_init", "g_init", "dc_i_init", "dc_q_init")
VIEW_FIELDS = ("dc_i", "dc_q", "p", "g", "held")


def test_symbols_exported_and_bound():
    L = sr.lib()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in sr.ABI_SYMBOLS
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == 2
    text = open(os.path.join(rc.ROOT, "include", "selenite_rx.h")).read()
    for n in NAMES:
        assert "int %s(selenite_rx_instance *S, const selenite_rx_iqc_" % n in text
    assert "#define SELENITE_RX_ABI_VERSION 2" in text and L.selenite_rx_abi_version() == 2      # (a new stage, not a new version)
    for m in ("set_iqc", "iqc_state", "set_iqc_state"):
        assert callable(getattr(sr.Rx, m))


C_SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "selenite_rx.h"
#define O(f) offsetof(selenite_rx_iqc_config, f)
#define V(f) offsetof(selenite_rx_iqc_state_view, f)
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_rx_iqc_config), O(struct_size), O(frame), O(alpha), O(dc_alpha),
           O(p_max), O(g_max), O(min_power), O(p_init), O(g_init), O(dc_i_init), O(dc_q_init));
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(selenite_rx_iqc_state_view), V(dc_i), V(dc_q), V(p), V(g), V(held));
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
    assert [int(v) for v in lines[0].split()] == [C.sizeof(sr.IqcConfig)] + [getattr(sr.IqcConfig, f).offset for f in CONFIG_FIELDS]
    assert [int(v) for v in lines[1].split()] == [C.sizeof(sr.IqcStateView)] + [getattr(sr.IqcStateView, f).offset for f in VIEW_FIELDS]
    assert C.sizeof(sr.IqcConfig) == 44 and C.sizeof(sr.IqcStateView) == 40
    assert [f for f, _ in sr.IqcConfig._fields_] == list(CONFIG_FIELDS) and [f for f, _ in sr.IqcStateView._fields_] == list(VIEW_FIELDS)


def test_null_instance_is_an_argument_error():
    L = sr.lib()
    g = sr.IqcConfig()
    g.struct_size, g.frame, g.alpha, g.dc_alpha, g.p_max, g.g_max, g.min_power = C.sizeof(sr.IqcConfig), 64, 1.0 / 64, 1.0 / 16, 0.25, 1.5, 1e-12
    g.p_init, g.g_init = 0.0, 1.0
    assert L.selenite_rx_set_iqc(None, C.byref(g)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_iqc(None, None) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_error_string(None)
    f, n = np.full(4, 3.0, np.float32), np.full(4, 7, np.uint64)
    v = sr.IqcStateView(f.ctypes.data_as(sr.f32p), None, f.ctypes.data_as(sr.f32p), None, n.ctypes.data_as(sr.u64p))
    assert L.selenite_rx_get_iqc_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_iqc_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_get_iqc_state(None, None) == sr.ARGUMENT_ERROR
    assert (f == 3.0).all() and (n == 7).all()
