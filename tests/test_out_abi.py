"""CPU: the audio output stage's C-ABI (include/selenite_rx.h: selenite_rx_set_out, selenite_rx_out_values, selenite_rx_get_out_state,
selenite_rx_set_out_state, selenite_rx_design_interp) is exported and bound, the ctypes struct lays out as the C compiler does, and the
entry points refuse a NULL instance without touching a GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import rxcommon as rc
import selenite_rx as sr

NAMES = ["selenite_rx_set_out", "selenite_rx_out_values", "selenite_rx_get_out_state", "selenite_rx_set_out_state",
         "selenite_rx_design_interp"]


def test_symbols_exported_and_bound():
    L = sr.lib()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in sr.ABI_SYMBOLS
    assert (sr.OUT_MONO, sr.OUT_STEREO) == (0, 1)
    text = open(os.path.join(rc.ROOT, "include", "selenite_rx.h")).read()
    for k, v in (("MONO", 0), ("STEREO", 1)):
        assert "#define SELENITE_RX_OUT_%-6s %d" % (k, v) in text
    assert "#define SELENITE_RX_ABI_VERSION 2" in text and L.selenite_rx_abi_version() == 2
    for m in ("set_out", "out_values", "out_state", "set_out_state"):
        assert callable(getattr(sr.Rx, m))


C_SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "selenite_rx.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(selenite_rx_out_config), offsetof(selenite_rx_out_config, struct_size),
           offsetof(selenite_rx_out_config, interp), offsetof(selenite_rx_out_config, ni_taps), offsetof(selenite_rx_out_config, frames),
           offsetof(selenite_rx_out_config, coeffs));
    return 0;
}
"""


def test_ctypes_layout_equals_offsetof():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write(C_SNIPPET)
        subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(rc.ROOT, "include"), "-o", exe, src], check=True)
        line = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")[0]
    assert [int(v) for v in line.split()] == [C.sizeof(sr.OutConfig)] + [getattr(sr.OutConfig, f).offset
                                                                         for f in ("struct_size", "interp", "ni_taps", "frames", "coeffs")]


def test_null_instance_is_an_argument_error():
    L = sr.lib()
    taps = np.ones(8, np.float32)
    g = sr.OutConfig()
    g.struct_size, g.interp, g.ni_taps, g.frames, g.coeffs = C.sizeof(sr.OutConfig), 4, 8, sr.OUT_STEREO, taps.ctypes.data_as(sr.f32p)
    assert L.selenite_rx_set_out(None, C.byref(g)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_out(None, None) == sr.ARGUMENT_ERROR
    buf = np.zeros(8, np.float32)
    assert L.selenite_rx_get_out_state(None, buf.ctypes.data_as(sr.f32p)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_out_state(None, buf.ctypes.data_as(sr.f32p)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_get_out_state(None, None) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_out_values(None, 96) == 0          # (returns a count, not a status: nothing to write)


def test_design_interp_is_the_lowpass_times_l():
    for interp in (1, 2, 4, 8):
        for plen in (2, 8, 13, 64):
            n = interp * plen
            if n < 2:
                continue
            cut = 0.4 / max(interp, 2)
            want = sr.design_lowpass(n, cut) * np.float32(interp)
            got = sr.design_interp(n, interp, cut)
            assert got.dtype == np.float32 and got.tobytes() == want.astype(np.float32).tobytes(), (interp, plen)
    # unity pass-band level behind the zero stuffing: every phase sums to about 1
    h = sr.design_interp(64, 4, 0.1)
    assert np.allclose(h.reshape(16, 4).sum(axis=0), 1.0, atol=2e-2)


def test_design_interp_argument_errors():
    L = sr.lib()
    h = np.zeros(64, np.float32)
    p = h.ctypes.data_as(sr.f32p)
    assert L.selenite_rx_design_interp(p, 30, 4, 0.1) == sr.LENGTH_ERROR        # arm_fir_interpolate_init_f32.c:91-96
    for interp in (0, 3, 5, 16):
        assert L.selenite_rx_design_interp(p, 48, interp, 0.1) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_design_interp(None, 32, 4, 0.1) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_design_interp(p, 32, 4, 0.0) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_design_interp(p, 32, 4, 0.5) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_design_interp(p, 0, 1, 0.1) == sr.ARGUMENT_ERROR       # (the low-pass helper wants two taps)


def test_host_example_builds_with_gcc_and_runs():
    """host/dsp_if_codec_slot.c: plain C over the ABI; exit 77 without a GPU (as dsp_if_slot.c), 0 with one"""
    src = os.path.join(rc.PKG_DIR, "host", "dsp_if_codec_slot.c")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "dsp_if_codec_slot")
        subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I" + os.path.join(rc.ROOT, "include"), src, "-L" + rc.PKG_DIR, "-lselenite_rx",
                        "-Wl,-rpath," + rc.PKG_DIR, "-lm", "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 77), (r.returncode, r.stdout, r.stderr)
    assert ("L/R frames per channel" in r.stdout) if r.returncode == 0 else ("DSP_Init failed" in r.stderr)
