"""CPU: the level meter's C-ABI (include/selenite_rx.h: selenite_rx_set_meter, selenite_rx_get_meter_state, selenite_rx_set_meter_state,
selenite_rx_meter_level_device, selenite_rx_meter_open_device) is exported and bound, the ctypes structs lay out as the C compiler does, and
the entry points refuse a NULL instance without touching a GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import rxcommon as rc
import selenite_rx as sr

NAMES = ["selenite_rx_set_meter", "selenite_rx_get_meter_state", "selenite_rx_set_meter_state"]
DEVICE_NAMES = ["selenite_rx_meter_level_device", "selenite_rx_meter_open_device"]
CONFIG_FIELDS = ("struct_size", "sense", "gate", "hang", "attack", "decay", "open_level", "close_level", "level_init")
VIEW_FIELDS = ("level", "open", "hold", "opens", "open_blocks")


def test_symbols_exported_and_bound():
    L = sr.lib()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in sr.ABI_SYMBOLS
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == 2
    for n in DEVICE_NAMES:
        assert hasattr(L, n) and n in sr.ABI_SYMBOLS
        assert len(getattr(L, n).argtypes) == 1 and getattr(L, n).restype is C.c_void_p
    text = open(os.path.join(rc.ROOT, "include", "selenite_rx.h")).read()
    for n in NAMES:
        assert "int %s(selenite_rx_instance *S, const selenite_rx_meter_" % n in text
    assert "const float *selenite_rx_meter_level_device(const selenite_rx_instance *S);" in text
    assert "const uint32_t *selenite_rx_meter_open_device(const selenite_rx_instance *S);" in text
    assert "#define SELENITE_RX_SQ_ABOVE 0" in text and "#define SELENITE_RX_SQ_BELOW 1" in text
    assert (sr.SQ_ABOVE, sr.SQ_BELOW) == (0, 1)
    assert "#define SELENITE_RX_ABI_VERSION 2" in text and L.selenite_rx_abi_version() == 2      # (a new stage, not a new version)
    for m in ("set_meter", "meter_state", "set_meter_state"):
        assert callable(getattr(sr.Rx, m))


C_SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "selenite_rx.h"
#define O(f) offsetof(selenite_rx_meter_config, f)
#define V(f) offsetof(selenite_rx_meter_state_view, f)
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_rx_meter_config), O(struct_size), O(sense), O(gate), O(hang), O(attack),
           O(decay), O(open_level), O(close_level), O(level_init));
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(selenite_rx_meter_state_view), V(level), V(open), V(hold), V(opens), V(open_blocks));
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
    assert [int(v) for v in lines[0].split()] == [C.sizeof(sr.MeterConfig)] + [getattr(sr.MeterConfig, f).offset for f in CONFIG_FIELDS]
    assert [int(v) for v in lines[1].split()] == [C.sizeof(sr.MeterStateView)] + [getattr(sr.MeterStateView, f).offset for f in VIEW_FIELDS]
    assert C.sizeof(sr.MeterConfig) == 36 and C.sizeof(sr.MeterStateView) == 40
    assert [f for f, _ in sr.MeterConfig._fields_] == list(CONFIG_FIELDS) and [f for f, _ in sr.MeterStateView._fields_] == list(VIEW_FIELDS)


def test_null_instance_is_an_argument_error():
    L = sr.lib()
    g = sr.MeterConfig()
    g.struct_size, g.sense, g.gate, g.hang = C.sizeof(sr.MeterConfig), sr.SQ_ABOVE, 1, 2
    g.attack, g.decay, g.open_level, g.close_level, g.level_init = 0.5, 0.125, 1e-6, 5e-7, 0.0
    assert L.selenite_rx_set_meter(None, C.byref(g)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_meter(None, None) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_error_string(None)
    f, u, n = np.full(4, 3.0, np.float32), np.full(4, 5, np.uint32), np.full(4, 7, np.uint64)
    v = sr.MeterStateView(f.ctypes.data_as(sr.f32p), u.ctypes.data_as(sr.u32p), None, n.ctypes.data_as(sr.u64p), None)
    assert L.selenite_rx_get_meter_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_meter_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_get_meter_state(None, None) == sr.ARGUMENT_ERROR
    assert (f == 3.0).all() and (u == 5).all() and (n == 7).all()
    assert L.selenite_rx_meter_level_device(None) is None and L.selenite_rx_meter_open_device(None) is None
