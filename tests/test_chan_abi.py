"""CPU: the polyphase channeliser's C-ABI (include/selenite_chan.h) is exported and bound, the ctypes structs lay out as the C compiler
does, selenite_chan_init validates every field before it touches a device, and the entry points refuse a NULL object without a GPU."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import rxcommon as rc
import selenite_rx as sr


def header_names():
    text = open(os.path.join(rc.ROOT, "include", "selenite_chan.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(selenite_chan_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    names = header_names()
    assert len(names) == 14
    L = sr.lib()
    for n in names:
        assert hasattr(L, n), "libselenite_rx.so does not export %s" % n
        assert getattr(L, n).argtypes is not None, "%s is not bound" % n
    assert sorted(sr.CHAN_ABI_SYMBOLS) == names
    for m in ("process_device", "process_q15_device", "state", "set_state", "reset", "sync", "set_stream", "out_channels", "out_len"):
        assert callable(getattr(sr.Channelizer, m))
    # nothing of it went into selenite_rx.h
    assert "selenite_chan" not in open(os.path.join(rc.ROOT, "include", "selenite_rx.h")).read() and L.selenite_rx_abi_version() == sr.ABI_VERSION


C_SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "selenite_chan.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_chan_config), offsetof(selenite_chan_config, struct_size),
           offsetof(selenite_chan_config, bands), offsetof(selenite_chan_config, fft_len), offsetof(selenite_chan_config, oversample),
           offsetof(selenite_chan_config, taps_per_branch), offsetof(selenite_chan_config, n_bins), offsetof(selenite_chan_config, reserved),
           offsetof(selenite_chan_config, coeffs), offsetof(selenite_chan_config, bins));
    printf("%zu %zu %zu\n", sizeof(selenite_chan_state_view), offsetof(selenite_chan_state_view, history),
           offsetof(selenite_chan_state_view, position));
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
    assert [int(v) for v in lines[0].split()] == [C.sizeof(sr.ChanConfig)] + [
        getattr(sr.ChanConfig, f).offset for f in ("struct_size", "bands", "fft_len", "oversample", "taps_per_branch", "n_bins", "reserved",
                                                   "coeffs", "bins")]
    assert [int(v) for v in lines[1].split()] == [C.sizeof(sr.ChanStateView)] + [
        getattr(sr.ChanStateView, f).offset for f in ("history", "position")]


def good(k=64, p=4):
    g = np.full(k * p, 1.0 / (k * p), np.float32)
    bins = np.array([3, 1, 3], np.uint32)
    cfg = sr.ChanConfig(C.sizeof(sr.ChanConfig), 2, k, 2, p, 3, 0, g.ctypes.data_as(sr.f32p), bins.ctypes.data_as(sr.u32p))
    return cfg, (g, bins)


def init(cfg):
    h = C.c_void_p(1)
    rc_ = sr.lib().selenite_chan_init(C.byref(h), C.byref(cfg) if cfg is not None else None)
    return rc_, h


BAD = [("struct_size", 8, sr.ARGUMENT_ERROR), ("bands", 0, sr.ARGUMENT_ERROR),
       ("bands", 1 << 26, sr.ARGUMENT_ERROR),                    # SELENITE_CHAN_MAX_BANDS + 1 (bands * n_bins = 3 * 2^26 is still below 2^32)
       ("fft_len", 128, sr.LENGTH_ERROR), ("fft_len", 0, sr.LENGTH_ERROR),
       ("oversample", 0, sr.ARGUMENT_ERROR), ("oversample", 4, sr.ARGUMENT_ERROR), ("taps_per_branch", 6, sr.ARGUMENT_ERROR),
       ("taps_per_branch", 20, sr.ARGUMENT_ERROR), ("n_bins", 0, sr.ARGUMENT_ERROR), ("reserved", 1, sr.ARGUMENT_ERROR)]


@pytest.mark.parametrize("field,value,code", BAD)
def test_each_bad_field_returns_its_code(field, value, code):
    cfg, keep = good()
    setattr(cfg, field, value)
    rc_, h = init(cfg)
    assert rc_ == code and h.value is None


def apply_faults(cfg, keep, faults):
    """a field name sets that field; the other names damage what the pointers lead to"""
    for name, value in faults:
        if name == "tap":
            keep[0][-1] = value
        elif name == "bin":
            keep[1][1] = value
        elif name in ("coeffs", "bins"):
            setattr(cfg, name, None)
        else:
            setattr(cfg, name, value)


# Two faults at once: which return code wins.  The codes are those the build before the shared filter-bank host code (pfb.h) returned, recorded
# by running this table against it; none of them is a device error, with or without a GPU.
PRECEDENCE = [((("fft_len", 128), ("bands", 0)), sr.LENGTH_ERROR),
              ((("fft_len", 0), ("struct_size", 8)), sr.ARGUMENT_ERROR),
              ((("tap", np.nan), ("bin", 64)), sr.ARGUMENT_ERROR),
              ((("reserved", 1), ("coeffs", None)), sr.ARGUMENT_ERROR),
              ((("bands", 1 << 26), ("n_bins", 0)), sr.ARGUMENT_ERROR),
              ((("fft_len", 128), ("reserved", 1)), sr.LENGTH_ERROR),
              ((("fft_len", 128), ("coeffs", None)), sr.LENGTH_ERROR),
              ((("fft_len", 100), ("oversample", 3)), sr.LENGTH_ERROR),
              ((("fft_len", 128), ("taps_per_branch", 5)), sr.LENGTH_ERROR),
              ((("fft_len", 128), ("bins", None)), sr.LENGTH_ERROR),
              ((("fft_len", 128), ("bands", 1 << 26)), sr.LENGTH_ERROR),
              ((("struct_size", 0), ("coeffs", None)), sr.ARGUMENT_ERROR),
              ((("oversample", 0), ("bin", 64)), sr.ARGUMENT_ERROR),
              ((("bins", None), ("tap", np.inf)), sr.ARGUMENT_ERROR)]


@pytest.mark.parametrize("faults,code", PRECEDENCE, ids=["+".join(n for n, _ in f) for f, _ in PRECEDENCE])
def test_return_code_precedence_of_two_faults(faults, code):
    cfg, keep = good()
    apply_faults(cfg, keep, faults)
    rc_, h = init(cfg)
    assert rc_ == code and h.value is None


def test_bad_pointers_taps_and_bins_are_argument_errors():
    assert sr.lib().selenite_chan_init(None, None) == sr.ARGUMENT_ERROR
    rc_, h = init(None)
    assert rc_ == sr.ARGUMENT_ERROR and h.value is None
    cfg, keep = good()
    cfg.coeffs = None
    assert init(cfg)[0] == sr.ARGUMENT_ERROR
    for bad in (np.nan, np.inf):
        cfg, keep = good()
        keep[0][-1] = bad
        assert init(cfg)[0] == sr.ARGUMENT_ERROR
    cfg, keep = good()
    keep[1][1] = 64                                              # a bin that is not < K
    assert init(cfg)[0] == sr.ARGUMENT_ERROR
    cfg, keep = good()
    cfg.bins = None                                              # all bins: n_bins must be K
    assert init(cfg)[0] == sr.ARGUMENT_ERROR


def test_good_config_is_a_device_error_without_a_gpu():
    """(with a GPU the same configurations build an object: there is no third outcome)"""
    L = sr.lib()
    gpu = L.selenite_rx_device_count() > 0
    for k, p in ((64, 4), (512, 16)):
        cfg, keep = good(k, p)
        rc_, h = init(cfg)
        if gpu:
            assert rc_ == sr.SUCCESS and h.value and L.selenite_chan_out_channels(h) == 6 and L.selenite_chan_out_len(h, 3 * k // 2) == 3
            L.selenite_chan_free(h)
        else:
            assert rc_ == sr.DEVICE_ERROR and h.value is None
    if not gpu:
        with pytest.raises(sr.RxError) as e:
            sr.Channelizer(1, 64, 1, 4, np.zeros(256, np.float32))
        assert e.value.code == sr.DEVICE_ERROR


def test_null_object_is_refused():
    L = sr.lib()
    assert L.selenite_chan_status(None) == sr.ARGUMENT_ERROR
    assert L.selenite_chan_error_string(None) == b"null channeliser"
    assert L.selenite_chan_set_stream(None, None) == sr.ARGUMENT_ERROR
    assert L.selenite_chan_sync(None) == sr.ARGUMENT_ERROR
    assert L.selenite_chan_reset(None) == sr.ARGUMENT_ERROR
    pos = np.array([7], np.uint64)
    v = sr.ChanStateView(None, pos.ctypes.data_as(sr.u64p))
    assert L.selenite_chan_get_state(None, C.byref(v)) == sr.ARGUMENT_ERROR and pos[0] == 7
    assert L.selenite_chan_set_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_chan_out_channels(None) == 0 and L.selenite_chan_out_len(None, 64) == 0
    L.selenite_chan_process_f32_device(None, None, None, 64)     # ignored: there is no object to hold a status
    L.selenite_chan_process_q15_device(None, None, None, 64)
    L.selenite_chan_free(None)


def test_design_chan_prototype_is_the_lowpass_design():
    for k, p, w in ((64, 4, 1.0), (64, 16, 2.0), (512, 8, 0.8), (512, 12, 2.0)):
        assert np.array_equal(sr.design_chan_prototype(k, p, w).view(np.uint32), sr.design_lowpass(k * p, 0.5 * w / k).view(np.uint32))
    L, g = sr.lib(), np.zeros(64 * 16, np.float32)
    fp = g.ctypes.data_as(sr.f32p)
    assert L.selenite_chan_design_prototype(fp, 128, 4, 1.0) == sr.LENGTH_ERROR
    assert L.selenite_chan_design_prototype(fp, 64, 5, 1.0) == sr.ARGUMENT_ERROR
    for w in (0.0, -1.0, 2.5, float("nan")):
        assert L.selenite_chan_design_prototype(fp, 64, 4, w) == sr.ARGUMENT_ERROR
    assert L.selenite_chan_design_prototype(None, 64, 4, 1.0) == sr.ARGUMENT_ERROR and not g.any()
