"""CPU: the Morse decoder's C-ABI (include/selenite_rx.h: selenite_rx_set_cwdec, selenite_rx_get_cwdec_state, selenite_rx_set_cwdec_state,
selenite_rx_get_cwdec, selenite_rx_cwdec_text_device, selenite_rx_cwdec_count_device, selenite_rx_cwdec_unit_device,
selenite_rx_design_morse) is exported and bound, the ctypes structs lay out as the C compiler does, the entry points refuse a NULL instance
and bad arguments without touching a GPU, and the built-in table is the one the restatement and the key generator use.  (That every bad
field of the config is refused with a working stage left in place needs an instance: tests/test_gpu_cwdec.py.)"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cwdec_oracle as co
import rxcommon as rc
import selenite_rx as sr

NAMES = {"selenite_rx_set_cwdec": 2, "selenite_rx_get_cwdec_state": 2, "selenite_rx_set_cwdec_state": 2, "selenite_rx_get_cwdec": 5,
         "selenite_rx_cwdec_text_device": 1, "selenite_rx_cwdec_count_device": 1, "selenite_rx_cwdec_unit_device": 1,
         "selenite_rx_design_morse": 2}
CONFIG_FIELDS = ("struct_size", "peak_attack", "peak_decay", "floor_attack", "floor_decay", "on_frac", "off_frac", "snr", "min_power",
                 "debounce", "adapt", "track", "unit_min", "unit_init", "unit_max", "ring", "table")
VIEW_FIELDS = ("peak", "floor", "primed", "key", "flip", "run", "unit", "code", "word", "count", "text")


def test_symbols_exported_and_bound():
    L = sr.lib()
    for n, nargs in NAMES.items():
        assert hasattr(L, n), n
        assert n in sr.ABI_SYMBOLS
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == nargs
    text = open(os.path.join(rc.ROOT, "include", "selenite_rx.h")).read()
    for decl in ("int selenite_rx_set_cwdec(selenite_rx_instance *S, const selenite_rx_cwdec_config *f);",
                 "int selenite_rx_get_cwdec_state(selenite_rx_instance *S, const selenite_rx_cwdec_state_view *dst);",
                 "int selenite_rx_set_cwdec_state(selenite_rx_instance *S, const selenite_rx_cwdec_state_view *src);",
                 "int selenite_rx_get_cwdec(selenite_rx_instance *S, uint8_t *text, uint64_t *count, uint32_t *unit, uint32_t *key);",
                 "const uint8_t *selenite_rx_cwdec_text_device(const selenite_rx_instance *S);",
                 "const uint64_t *selenite_rx_cwdec_count_device(const selenite_rx_instance *S);",
                 "const uint32_t *selenite_rx_cwdec_unit_device(const selenite_rx_instance *S);",
                 "int selenite_rx_design_morse(uint8_t table[256], uint8_t unknown);"):
        assert decl in text, decl
    assert "#define SELENITE_RX_ABI_VERSION 2" in text and L.selenite_rx_abi_version() == 2 and sr.ABI_VERSION == 2      # (a new stage, not a new version)
    for m in ("set_cwdec", "cwdec_state", "set_cwdec_state", "cwdec", "cw_text", "cw_unit", "cwdec_text_device", "cwdec_count_device",
              "cwdec_unit_device"):
        assert callable(getattr(sr.Rx, m))
    assert callable(sr.morse_table) and callable(sr.morse_key)


def test_the_law_stands_word_for_word_in_the_header_the_kernel_file_and_the_design():
    """every line of the law between `pw = arm_power_f32` and `emit(c):`, less the comment leaders"""
    def law(path, lead):
        lines = [ln.strip() for ln in open(os.path.join(rc.ROOT, path)).read().split("\n")]
        lines = [ln[len(lead):].strip() if ln.startswith(lead) else ln for ln in lines]
        a = next(i for i, ln in enumerate(lines) if ln.startswith("pw = arm_power_f32(x, n);"))
        b = next(i for i, ln in enumerate(lines) if ln.startswith("emit(c):"))
        return [" ".join(ln.split()) for ln in lines[a:b + 1]]
    h = law("include/selenite_rx.h", "*")
    assert len(h) == 28
    assert h == law("selenite-lite_amd/csrc/rx_cwdec.hip", "//")
    assert h == law("DESIGN.md", "")


C_SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "selenite_rx.h"
#define O(f) offsetof(selenite_rx_cwdec_config, f)
#define V(f) offsetof(selenite_rx_cwdec_state_view, f)
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_rx_cwdec_config), O(struct_size),
           O(peak_attack), O(peak_decay), O(floor_attack), O(floor_decay), O(on_frac), O(off_frac), O(snr), O(min_power), O(debounce), O(adapt),
           O(track), O(unit_min), O(unit_init), O(unit_max), O(ring), O(table));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(selenite_rx_cwdec_state_view), V(peak), V(floor), V(primed), V(key),
           V(flip), V(run), V(unit), V(code), V(word), V(count), V(text));
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
    assert [int(v) for v in lines[0].split()] == [C.sizeof(sr.CwdecConfig)] + [getattr(sr.CwdecConfig, f).offset for f in CONFIG_FIELDS]
    assert [int(v) for v in lines[1].split()] == [C.sizeof(sr.CwdecStateView)] + [getattr(sr.CwdecStateView, f).offset for f in VIEW_FIELDS]
    assert C.sizeof(sr.CwdecConfig) == 72 and C.sizeof(sr.CwdecStateView) == 88
    assert [f for f, _ in sr.CwdecConfig._fields_] == list(CONFIG_FIELDS) and [f for f, _ in sr.CwdecStateView._fields_] == list(VIEW_FIELDS)
    assert sr.Rx.CWDEC_TYPES.keys() == set(VIEW_FIELDS) and list(sr.Rx.CWDEC_TYPES) == list(VIEW_FIELDS) == list(co.ROWS)


def config(**over):
    g = sr.CwdecConfig()
    g.struct_size = C.sizeof(sr.CwdecConfig)
    for k, v in dict(sr.CWDEC_DEFAULTS, **over).items():
        setattr(g, k, v)
    return g


def test_null_instance_is_an_argument_error():
    L = sr.lib()
    assert L.selenite_rx_set_cwdec(None, C.byref(config())) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_cwdec(None, None) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_error_string(None)
    text, count, unit, key = np.full(64, 7, np.uint8), np.full(4, 9, np.uint64), np.full(4, 5, np.uint32), np.full(4, 3, np.uint32)
    v = sr.CwdecStateView()
    v.text, v.count, v.unit, v.key = text.ctypes.data_as(sr.u8p), count.ctypes.data_as(sr.u64p), unit.ctypes.data_as(sr.u32p), key.ctypes.data_as(sr.u32p)
    assert L.selenite_rx_get_cwdec_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_set_cwdec_state(None, C.byref(v)) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_get_cwdec_state(None, None) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_get_cwdec(None, v.text, v.count, v.unit, v.key) == sr.ARGUMENT_ERROR
    assert L.selenite_rx_cwdec_text_device(None) is None and L.selenite_rx_cwdec_count_device(None) is None
    assert L.selenite_rx_cwdec_unit_device(None) is None
    assert (text == 7).all() and (count == 9).all() and (unit == 5).all() and (key == 3).all()


def test_the_defaults_are_the_documented_ones():
    assert sr.CWDEC_DEFAULTS == dict(peak_attack=0.5, peak_decay=0.002, floor_attack=0.25, floor_decay=0.002, on_frac=0.4, off_frac=0.25, snr=4.0,
                                     min_power=1e-8, debounce=2, adapt=1, track=2, unit_min=2 * 256, unit_init=10 * 256, unit_max=64 * 256,
                                     ring=256)
    assert co.DEFAULTS == sr.CWDEC_DEFAULTS
    for k in sr.CWDEC_DEFAULTS:
        assert k in sr.Rx.set_cwdec.__doc__, k


def test_design_morse_against_morse_table_and_the_key_generators_patterns():
    L = sr.lib()
    assert L.selenite_rx_design_morse(None, ord("#")) == sr.ARGUMENT_ERROR
    t = np.full(256, 1, np.uint8)
    assert L.selenite_rx_design_morse(t.ctypes.data_as(sr.u8p), ord("~")) == 0
    assert t.tobytes() == sr.morse_table("~").tobytes() == co.table("~").tobytes()
    assert sr.morse_table().tobytes() == co.table("#").tobytes()
    # A-Z, 0-9 and the eight punctuation marks, nothing else; index 0 (overflow) and 1 (no element) are `unknown`
    known = {chr(c): i for i, c in enumerate(t) if c != ord("~")}
    assert sorted(known) == sorted("ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789.,?/=+-@") and len(known) == 44
    assert t[0] == ord("~") and t[1] == ord("~") and t[0b101] == ord("A")
    for ch, pat in {".": ".-.-.-", ",": "--..--", "?": "..--..", "/": "-..-.", "=": "-...-", "+": ".-.-.", "-": "-....-", "@": ".--.-."}.items():
        assert known[ch] == co.code_of(pat), ch
    # morse_key keys what the table decodes: every character's runs read back as its index, with 1 / 3 / 7 unit gaps
    for u in (1, 5):
        for ch, code in known.items():
            k = sr.morse_key(ch, u)
            assert k.dtype == np.uint8 and k[0] == 1 and k[-1] == 1
            runs = np.diff(np.flatnonzero(np.diff(np.concatenate([[0], k, [0]])))) // u          # down, up, down ... in units
            els, gaps = runs[0::2], runs[1::2]
            assert set(els) <= {1, 3} and (gaps == 1).all()
            assert co.code_of("".join("-" if e == 3 else "." for e in els)) == code, ch
        text = "CQ DE K1ABC = 73"
        assert sr.morse_key(text, u).tobytes() == co.key_of(text, u).tobytes() == sr.morse_key(" " + text.lower() + "  ", u).tobytes()
        k = sr.morse_key("E E  T", u)
        assert k.tolist() == [1] * u + [0] * 7 * u + [1] * u + [0] * 7 * u + [1] * 3 * u
        assert sr.morse_key("ET", u).tolist() == [1] * u + [0] * 3 * u + [1] * 3 * u
    assert sr.morse_key("", 3).size == 0
    for bad in ("#", "~", "\n", "É"):
        with pytest.raises(ValueError):
            sr.morse_key(bad, 3)
    with pytest.raises(ValueError):
        sr.morse_key("E", 0)
