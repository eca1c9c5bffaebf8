"""CPU: the noise blanker's C-ABI (include/selenite_rx.h: selenite_rx_set_nb, selenite_rx_get_nb_state, selenite_rx_set_nb_state) is exported
and bound, the ctypes structs lay out as the C compiler does, and the entry points refuse a NULL instance without touching a GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import rxcommon as rc
import selenite_rx as sr

NAMES = ["selenite_rx_set_nb", "selenite_rx_get_nb_state", "selenite_rx_set_nb_state"]


def test_symbols_exported_and_bound():
    L = sr.lib()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in sr.ABI_SYMBOLS
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == 2
    text = open(os.path.join(rc.ROOT, "include", "selenite_rx.h")).read()
    for n in NAMES:
        assert "int %s(selenite_rx_instance *S, const selenite_rx_nb_" % n in text
    assert "#define SELENITE_RX_ABI_VERSION 2" in text and L.selenite_rx_abi_version() == 2      # (a new stage, not a new version)
    for m in ("set_nb", "nb_state", "set_nb_state"):
        assert callable(getattr(sr.Rx, m))


C_SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "selenite_rx.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_rx_nb_config), offsetof(selenite_rx_nb_config, struct_size),
           offsetof(selenite_rx_nb_config, frame), offsetof(selenite_rx_nb_config, guard), offsetof(selenite_rx_nb_config, max_hits),
           offsetof(selenite_rx_nb_config, threshold), offsetof(selenite_rx_nb_config, alpha), offsetof(selenite_rx_nb_config, clamp));
    printf("%zu %zu %zu %zu\n", sizeof(selenite_rx_nb_state_view), offsetof(selenite_rx_nb_state_view, level),
           offsetof(selenite_rx_nb_state_view, blanked), offsetof(selenite_rx_nb_state_view, bursts));
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
    assert [int(v) for v in lines[0].split()] == [C.sizeof(sr.NbConfig)] + [
        getattr(sr.NbConfig, f).offset for f in ("struct_size", "frame", "guard", "max_hits", "threshold", "alpha", "clamp")]
    assert [int(v) for v in lines[1].split()] == [C.sizeof(sr.NbStateView)] + [
        getattr(sr.NbStateView, f).offset for f in ("level", "blanked", "bursts")]
    assert C.sizeof(sr.NbConfig) == 28 and C.sizeof(sr.NbStateView) == 24


def test_null_instance_is_an_argument_error():
    L = sr.lib()
    g = sr.NbConfig()
    g.struct_size, g.frame, g.guard, g.max_hits, g.threshold, g.alpha, g.clamp = C.sizeof(sr.NbConfig), 64, 2, 8, 8.0, 0.125, 2.0
    assert L.selenite_rx_set_nb(None, C.byref(g)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_nb(None, None) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_error_string(None)
    level, n = np.full(4, 3.0, np.float32), np.full(4, 7, np.uint64)
    v = sr.NbStateView(level.ctypes.data_as(sr.f32p), n.ctypes.data_as(sr.u64p), None)
    assert L.selenite_rx_get_nb_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_nb_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_get_nb_state(None, None) == sr.ARGUMENT_ERROR
    assert (level == 3.0).all() and (n == 7).all()
