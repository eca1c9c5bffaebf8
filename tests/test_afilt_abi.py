"""CPU: the audio filter's C-ABI (include/selenite_rx.h: selenite_rx_set_afilt, selenite_rx_set_afilt_coeffs, selenite_rx_get_afilt_state,
selenite_rx_set_afilt_state, selenite_rx_design_biquad, selenite_rx_design_deemphasis) is exported and bound, the ctypes structs lay out as
the C compiler does, and the entry points refuse a NULL instance without touching a GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import rxcommon as rc
import selenite_rx as sr

NAMES = {"selenite_rx_set_afilt": 2, "selenite_rx_set_afilt_coeffs": 4, "selenite_rx_get_afilt_state": 2, "selenite_rx_set_afilt_state": 2,
         "selenite_rx_design_biquad": 5, "selenite_rx_design_deemphasis": 2}
CONFIG_FIELDS = ("struct_size", "n_stages", "per_channel", "reserved", "coeffs")
VIEW_FIELDS = ("state", "coeffs")


def test_symbols_exported_and_bound():
    L = sr.lib()
    for n, nargs in NAMES.items():
        assert hasattr(L, n), n
        assert n in sr.ABI_SYMBOLS
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == nargs
    text = open(os.path.join(rc.ROOT, "include", "selenite_rx.h")).read()
    for decl in ("int selenite_rx_set_afilt(selenite_rx_instance *S, const selenite_rx_afilt_config *f);",
                 "int selenite_rx_set_afilt_coeffs(selenite_rx_instance *S, uint32_t first_channel, uint32_t n_channels, const float *coeffs);",
                 "int selenite_rx_get_afilt_state(selenite_rx_instance *S, const selenite_rx_afilt_state_view *dst);",
                 "int selenite_rx_set_afilt_state(selenite_rx_instance *S, const selenite_rx_afilt_state_view *src);",
                 "int selenite_rx_design_biquad(float coeffs[5], int kind, double f0, double q, double gain_db);",
                 "int selenite_rx_design_deemphasis(float coeffs[5], double tau_samples);"):
        assert decl in text, decl
    for k, name in enumerate(("NOTCH", "PEAKING", "LOWPASS", "HIGHPASS")):
        assert "#define SELENITE_RX_BIQUAD_%s" % name in text and getattr(sr, "BIQUAD_" + name) == k
        assert ("#define SELENITE_RX_BIQUAD_%-8s %d" % (name, k)) in text
    assert "#define SELENITE_RX_ABI_VERSION 2" in text and L.selenite_rx_abi_version() == 2      # (a new stage, not a new version)
    for m in ("set_afilt", "set_afilt_coeffs", "afilt_state", "set_afilt_state"):
        assert callable(getattr(sr.Rx, m))
    assert callable(sr.design_biquad) and callable(sr.design_deemphasis)


C_SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "selenite_rx.h"
#define O(f) offsetof(selenite_rx_afilt_config, f)
#define V(f) offsetof(selenite_rx_afilt_state_view, f)
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(selenite_rx_afilt_config), O(struct_size), O(n_stages), O(per_channel), O(reserved), O(coeffs));
    printf("%zu %zu %zu\n", sizeof(selenite_rx_afilt_state_view), V(state), V(coeffs));
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
    assert [int(v) for v in lines[0].split()] == [C.sizeof(sr.AfiltConfig)] + [getattr(sr.AfiltConfig, f).offset for f in CONFIG_FIELDS]
    assert [int(v) for v in lines[1].split()] == [C.sizeof(sr.AfiltStateView)] + [getattr(sr.AfiltStateView, f).offset for f in VIEW_FIELDS]
    assert C.sizeof(sr.AfiltConfig) == 24 and C.sizeof(sr.AfiltStateView) == 16
    assert [f for f, _ in sr.AfiltConfig._fields_] == list(CONFIG_FIELDS) and [f for f, _ in sr.AfiltStateView._fields_] == list(VIEW_FIELDS)


def test_null_instance_is_an_argument_error():
    L = sr.lib()
    k5 = np.array([1, 0, 0, 0, 0], np.float32)
    g = sr.AfiltConfig()
    g.struct_size, g.n_stages, g.per_channel, g.reserved, g.coeffs = C.sizeof(sr.AfiltConfig), 1, 0, 0, k5.ctypes.data_as(sr.f32p)
    assert L.selenite_rx_set_afilt(None, C.byref(g)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_afilt(None, None) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_error_string(None)
    assert L.selenite_rx_set_afilt_coeffs(None, 0, 1, k5.ctypes.data_as(sr.f32p)) == sr.ARGUMENT_ERROR
    s, c = np.full(4, 3.0, np.float32), np.full(5, 5.0, np.float32)
    v = sr.AfiltStateView(s.ctypes.data_as(sr.f32p), c.ctypes.data_as(sr.f32p))
    assert L.selenite_rx_get_afilt_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_afilt_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_get_afilt_state(None, None) == sr.ARGUMENT_ERROR
    assert (s == 3.0).all() and (c == 5.0).all() and (k5 == np.array([1, 0, 0, 0, 0], np.float32)).all()
