"""CPU: the tone detector's C-ABI (include/selenite_rx.h: selenite_rx_set_tones, selenite_rx_get_tones_state, selenite_rx_set_tones_state,
selenite_rx_get_tones, selenite_rx_tones_tone_device, selenite_rx_tones_power_device, selenite_rx_design_tones, selenite_rx_ctcss_hz) is
exported and bound, the ctypes structs lay out as the C compiler does, and the entry points refuse a NULL instance and bad arguments without
touching a GPU.  (That every bad field of the config is refused with a working stage left in place needs an instance:
tests/test_gpu_tones.py.)"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import rxcommon as rc
import selenite_rx as sr

NAMES = {"selenite_rx_set_tones": 2, "selenite_rx_get_tones_state": 2, "selenite_rx_set_tones_state": 2, "selenite_rx_get_tones": 4,
         "selenite_rx_tones_tone_device": 1, "selenite_rx_tones_power_device": 1, "selenite_rx_design_tones": 3, "selenite_rx_ctcss_hz": 1}
CONFIG_FIELDS = ("struct_size", "n_tones", "frame_blocks", "confirm", "release", "reserved", "ratio", "min_power", "coeffs")
VIEW_FIELDS = ("s", "energy", "power", "frame_energy", "last_best", "tone", "cand", "run", "changes", "position")


def test_symbols_exported_and_bound():
    L = sr.lib()
    for n, nargs in NAMES.items():
        assert hasattr(L, n), n
        assert n in sr.ABI_SYMBOLS
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == nargs
    text = open(os.path.join(rc.ROOT, "include", "selenite_rx.h")).read()
    for decl in ("int selenite_rx_set_tones(selenite_rx_instance *S, const selenite_rx_tones_config *f);",
                 "int selenite_rx_get_tones_state(selenite_rx_instance *S, const selenite_rx_tones_state_view *dst);",
                 "int selenite_rx_set_tones_state(selenite_rx_instance *S, const selenite_rx_tones_state_view *src);",
                 "int selenite_rx_get_tones(selenite_rx_instance *S, uint32_t *tone, float *power, uint64_t *frames);",
                 "const uint32_t *selenite_rx_tones_tone_device(const selenite_rx_instance *S);",
                 "const float *selenite_rx_tones_power_device(const selenite_rx_instance *S);",
                 "int selenite_rx_design_tones(float *coeffs, const double *freq, uint32_t n_tones);",
                 "uint32_t selenite_rx_ctcss_hz(double hz[50]);"):
        assert decl in text, decl
    assert "#define SELENITE_RX_TONES_MAX  64" in text and sr.TONES_MAX == 64
    assert "#define SELENITE_RX_TONE_NONE  0xFFFFFFFFu" in text and sr.TONE_NONE == 0xFFFFFFFF
    assert "#define SELENITE_RX_ABI_VERSION 2" in text and L.selenite_rx_abi_version() == 2      # (a new stage, not a new version)
    for m in ("set_tones", "tones_state", "set_tones_state", "tones", "tones_tone_device", "tones_power_device"):
        assert callable(getattr(sr.Rx, m))
    assert callable(sr.design_tones) and callable(sr.ctcss_hz)


C_SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "selenite_rx.h"
#define O(f) offsetof(selenite_rx_tones_config, f)
#define V(f) offsetof(selenite_rx_tones_state_view, f)
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_rx_tones_config), O(struct_size), O(n_tones), O(frame_blocks), O(confirm),
           O(release), O(reserved), O(ratio), O(min_power), O(coeffs));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_rx_tones_state_view), V(s), V(energy), V(power), V(frame_energy),
           V(last_best), V(tone), V(cand), V(run), V(changes), V(position));
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
    assert [int(v) for v in lines[0].split()] == [C.sizeof(sr.TonesConfig)] + [getattr(sr.TonesConfig, f).offset for f in CONFIG_FIELDS]
    assert [int(v) for v in lines[1].split()] == [C.sizeof(sr.TonesStateView)] + [getattr(sr.TonesStateView, f).offset for f in VIEW_FIELDS]
    assert C.sizeof(sr.TonesConfig) == 40 and C.sizeof(sr.TonesStateView) == 80
    assert [f for f, _ in sr.TonesConfig._fields_] == list(CONFIG_FIELDS) and [f for f, _ in sr.TonesStateView._fields_] == list(VIEW_FIELDS)


def test_null_instance_is_an_argument_error():
    L = sr.lib()
    k3 = sr.design_tones([0.1, 0.2])
    keep = k3.copy()
    g = sr.TonesConfig()
    g.struct_size, g.n_tones, g.frame_blocks, g.confirm, g.release, g.reserved = C.sizeof(sr.TonesConfig), 2, 1, 1, 1, 0
    g.ratio, g.min_power, g.coeffs = 0.02, 0.0, k3.ctypes.data_as(sr.f32p)
    assert L.selenite_rx_set_tones(None, C.byref(g)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_tones(None, None) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_error_string(None)
    tone, power, pos = np.full(4, 7, np.uint32), np.full(8, 3.0, np.float32), np.full(1, 9, np.uint64)
    v = sr.TonesStateView()
    v.tone, v.power, v.position = tone.ctypes.data_as(sr.u32p), power.ctypes.data_as(sr.f32p), pos.ctypes.data_as(sr.u64p)
    assert L.selenite_rx_get_tones_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_tones_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_get_tones_state(None, None) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_get_tones(None, tone.ctypes.data_as(sr.u32p), power.ctypes.data_as(sr.f32p), pos.ctypes.data_as(sr.u64p)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_tones_tone_device(None) is None and L.selenite_rx_tones_power_device(None) is None
    assert (tone == 7).all() and (power == 3.0).all() and pos[0] == 9 and k3.tobytes() == keep.tobytes()


def test_design_helpers_refuse_bad_arguments_and_leave_the_output_alone():
    L = sr.lib()
    dp = C.POINTER(C.c_double)
    out = np.full(6, 5.0, np.float32)
    f = np.array([0.1, 0.2])
    assert L.selenite_rx_design_tones(None, f.ctypes.data_as(dp), 2) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_design_tones(out.ctypes.data_as(sr.f32p), None, 2) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_design_tones(out.ctypes.data_as(sr.f32p), f.ctypes.data_as(dp), 0) == sr.ARGUMENT_ERROR
    for bad in (0.0, 0.5, -0.25, np.nan, np.inf):
        fb = np.array([0.1, bad])
        assert L.selenite_rx_design_tones(out.ctypes.data_as(sr.f32p), fb.ctypes.data_as(dp), 2) == sr.ARGUMENT_ERROR
        assert (out == 5.0).all()
    assert L.selenite_rx_design_tones(out.ctypes.data_as(sr.f32p), f.ctypes.data_as(dp), 2) == 0 and (out != 5.0).all()
    assert L.selenite_rx_ctcss_hz(None) == 50
