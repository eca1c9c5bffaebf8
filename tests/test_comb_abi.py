"""CPU: the polyphase combiner's C-ABI (include/selenite_comb.h) is exported and bound, the ctypes structs lay out as the C compiler does,
selenite_comb_init validates every field before it touches a device, and the entry points refuse a NULL object without a GPU."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import rxcommon as rc
import selenite_rx as sr

CONFIG_FIELDS = ("struct_size", "bands", "fft_len", "oversample", "taps_per_branch", "n_bins", "q15_rounding", "reserved", "coeffs", "bins")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(rc.ROOT, "include", "selenite_comb.h")).read(), flags=re.S)


def header_names():
    return sorted(set(re.findall(r"\b(selenite_comb_[a-z0-9_]+)\s*\(", header_text())))


def test_header_symbols_are_exported_and_bound():
    names = header_names()
    assert len(names) == 14
    L = sr.lib()
    for n in names:
        assert hasattr(L, n), "libselenite_rx.so does not export %s" % n
        assert getattr(L, n).argtypes is not None, "%s is not bound" % n
    assert sorted(sr.COMB_ABI_SYMBOLS) == names
    for m in ("process_device", "process_q15_device", "state", "set_state", "reset", "sync", "set_stream", "in_channels", "out_len"):
        assert callable(getattr(sr.Combiner, m))
    # nothing of it went into the other headers
    for h in ("selenite_rx.h", "selenite_tx.h", "selenite_chan.h"):
        assert "selenite_comb" not in open(os.path.join(rc.ROOT, "include", h)).read()
    assert L.selenite_rx_abi_version() == sr.ABI_VERSION
    m = re.search(r"#define\s+SELENITE_COMB_MAX_BANDS\s+0x([0-9A-Fa-f]+)u", header_text())
    assert m and int(m.group(1), 16) == (1 << 26) - 1           # 64 threads per band in the grid's x, under 2^32


C_SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "selenite_comb.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_comb_config), offsetof(selenite_comb_config, struct_size),
           offsetof(selenite_comb_config, bands), offsetof(selenite_comb_config, fft_len), offsetof(selenite_comb_config, oversample),
           offsetof(selenite_comb_config, taps_per_branch), offsetof(selenite_comb_config, n_bins), offsetof(selenite_comb_config, q15_rounding),
           offsetof(selenite_comb_config, reserved), offsetof(selenite_comb_config, coeffs), offsetof(selenite_comb_config, bins));
    printf("%zu %zu %zu\n", sizeof(selenite_comb_state_view), offsetof(selenite_comb_state_view, history),
           offsetof(selenite_comb_state_view, position));
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
    assert [int(v) for v in lines[0].split()] == [C.sizeof(sr.CombConfig)] + [getattr(sr.CombConfig, f).offset for f in CONFIG_FIELDS]
    assert [name for name, _ in sr.CombConfig._fields_] == list(CONFIG_FIELDS)
    assert [int(v) for v in lines[1].split()] == [C.sizeof(sr.CombStateView)] + [
        getattr(sr.CombStateView, f).offset for f in ("history", "position")]


def good(k=64, p=4, ovs=2):
    g = np.full(k * p, 1.0 / (k * p), np.float32)
    bins = np.array([3, 1, 63], np.uint32)
    cfg = sr.CombConfig(C.sizeof(sr.CombConfig), 2, k, ovs, p, 3, 0, 0, g.ctypes.data_as(sr.f32p), bins.ctypes.data_as(sr.u32p))
    return cfg, (g, bins)


def init(cfg):
    h = C.c_void_p(1)
    rc_ = sr.lib().selenite_comb_init(C.byref(h), C.byref(cfg) if cfg is not None else None)
    return rc_, h


BAD = [("struct_size", 8, sr.ARGUMENT_ERROR), ("struct_size", 56, sr.ARGUMENT_ERROR), ("bands", 0, sr.ARGUMENT_ERROR),
       ("bands", 1 << 26, sr.ARGUMENT_ERROR),                    # SELENITE_COMB_MAX_BANDS + 1 (bands * n_bins = 3 * 2^26 is still below 2^32)
       ("fft_len", 128, sr.LENGTH_ERROR), ("fft_len", 0, sr.LENGTH_ERROR),
       ("oversample", 0, sr.ARGUMENT_ERROR), ("oversample", 4, sr.ARGUMENT_ERROR), ("taps_per_branch", 6, sr.ARGUMENT_ERROR),
       ("taps_per_branch", 12, sr.ARGUMENT_ERROR), ("taps_per_branch", 16, sr.ARGUMENT_ERROR),      # with oversample 2: Q = 24, 32 > 16
       ("taps_per_branch", 20, sr.ARGUMENT_ERROR), ("n_bins", 0, sr.ARGUMENT_ERROR), ("q15_rounding", 2, sr.ARGUMENT_ERROR),
       ("reserved", 1, sr.ARGUMENT_ERROR)]


@pytest.mark.parametrize("field,value,code", BAD)
def test_each_bad_field_returns_its_code(field, value, code):
    cfg, keep = good(p=16 if field == "taps_per_branch" else 4)  # (the taps array is long enough for every P tried)
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
              ((("bins", None), ("tap", np.inf)), sr.ARGUMENT_ERROR),
              ((("bin", 3), ("q15_rounding", 2)), sr.ARGUMENT_ERROR),                  # (bins 3, 3, 63: two rows on one bin)
              ((("fft_len", 128), ("q15_rounding", 2)), sr.LENGTH_ERROR),
              ((("fft_len", 0), ("n_bins", 65)), sr.LENGTH_ERROR),
              ((("fft_len", 128), ("taps_per_branch", 12)), sr.LENGTH_ERROR),          # with oversample 2: Q = 24 > 16
              ((("n_bins", 65), ("tap", np.nan)), sr.ARGUMENT_ERROR)]


@pytest.mark.parametrize("faults,code", PRECEDENCE, ids=["+".join(n for n, _ in f) for f, _ in PRECEDENCE])
def test_return_code_precedence_of_two_faults(faults, code):
    cfg, keep = good()
    apply_faults(cfg, keep, faults)
    rc_, h = init(cfg)
    assert rc_ == code and h.value is None


def test_bad_pointers_taps_and_bins_are_argument_errors():
    assert sr.lib().selenite_comb_init(None, None) == sr.ARGUMENT_ERROR
    rc_, h = init(None)
    assert rc_ == sr.ARGUMENT_ERROR and h.value is None
    cfg, keep = good()
    cfg.coeffs = None
    assert init(cfg)[0] == sr.ARGUMENT_ERROR
    for bad in (np.nan, np.inf, -np.inf):
        cfg, keep = good()
        keep[0][-1] = bad
        assert init(cfg)[0] == sr.ARGUMENT_ERROR
    cfg, keep = good()
    keep[1][1] = 64                                              # a bin that is not < K
    assert init(cfg)[0] == sr.ARGUMENT_ERROR
    cfg, keep = good()
    keep[1][2] = 3                                               # two rows on one bin
    assert init(cfg)[0] == sr.ARGUMENT_ERROR
    cfg, keep = good()
    cfg.bins = None                                              # all bins: n_bins must be K
    assert init(cfg)[0] == sr.ARGUMENT_ERROR


def test_good_config_is_a_device_error_without_a_gpu():
    """(with a GPU the same configurations build an object: there is no third outcome)"""
    L = sr.lib()
    gpu = L.selenite_rx_device_count() > 0
    for k, p, ovs in ((64, 4, 2), (64, 8, 2), (512, 16, 1), (512, 12, 1)):
        cfg, keep = good(k, p, ovs)
        rc_, h = init(cfg)
        if gpu:
            assert rc_ == sr.SUCCESS and h.value and L.selenite_comb_in_channels(h) == 6 and L.selenite_comb_out_len(h, 3) == 3 * k // ovs
            assert L.selenite_comb_out_len(h, 0) == 0
            L.selenite_comb_free(h)
        else:
            assert rc_ == sr.DEVICE_ERROR and h.value is None
    if not gpu:
        with pytest.raises(sr.RxError) as e:
            sr.Combiner(1, 64, 1, 4, np.zeros(256, np.float32))
        assert e.value.code == sr.DEVICE_ERROR


def test_null_object_is_refused():
    L = sr.lib()
    assert L.selenite_comb_status(None) == sr.ARGUMENT_ERROR
    assert L.selenite_comb_error_string(None) == b"null combiner"
    assert L.selenite_comb_set_stream(None, None) == sr.ARGUMENT_ERROR
    assert L.selenite_comb_sync(None) == sr.ARGUMENT_ERROR
    assert L.selenite_comb_reset(None) == sr.ARGUMENT_ERROR
    pos = np.array([7], np.uint64)
    v = sr.CombStateView(None, pos.ctypes.data_as(sr.u64p))
    assert L.selenite_comb_get_state(None, C.byref(v)) == sr.ARGUMENT_ERROR and pos[0] == 7
    assert L.selenite_comb_set_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_comb_in_channels(None) == 0 and L.selenite_comb_out_len(None, 64) == 0
    L.selenite_comb_process_f32_device(None, None, None, 64)     # ignored: there is no object to hold a status
    L.selenite_comb_process_q15_device(None, None, None, 64)
    L.selenite_comb_free(None)


def test_design_comb_prototype_is_the_channelisers_times_k_d():
    for k, p, w, ovs in ((64, 4, 1.0, 1), (64, 8, 2.0, 2), (512, 8, 0.8, 2), (512, 12, 2.0, 1), (64, 16, 1.0, 1)):
        want = (sr.design_chan_prototype(k, p, w).astype(np.float64) * (k * (k // ovs))).astype(np.float32)
        got = sr.design_comb_prototype(k, p, w, ovs)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        # unity gain from channel 0 to the stream: every output phase's taps sum to about K (the 1 / K is arm_cfft_f32's own)
        assert abs(got.astype(np.float64).sum() / (k * (k // ovs)) - 1.0) < 1e-6
    L, g = sr.lib(), np.zeros(64 * 16, np.float32)
    fp = g.ctypes.data_as(sr.f32p)
    assert L.selenite_comb_design_prototype(fp, 128, 4, 1.0, 1) == sr.LENGTH_ERROR
    assert L.selenite_comb_design_prototype(fp, 64, 5, 1.0, 1) == sr.ARGUMENT_ERROR
    assert L.selenite_comb_design_prototype(fp, 64, 12, 1.0, 2) == sr.ARGUMENT_ERROR
    assert L.selenite_comb_design_prototype(fp, 64, 4, 1.0, 3) == sr.ARGUMENT_ERROR
    for w in (0.0, -1.0, 2.5, float("nan")):
        assert L.selenite_comb_design_prototype(fp, 64, 4, w, 1) == sr.ARGUMENT_ERROR
    assert L.selenite_comb_design_prototype(None, 64, 4, 1.0, 1) == sr.ARGUMENT_ERROR and not g.any()
